"""numpy float64 statement of imdbn_unit_moments (the same skip rules) and an INDEPENDENT statement of the statistics
imdbn.utils.unit_tuning derives from the moments: least squares on the raw design matrix, ANOVA and curves from per-class arrays --
not the moment formulas again."""
import numpy as np

KEYS = ("cls_sum", "cls_sumsq", "cls_count", "xa", "aa", "xx", "rows")


def used_rows(B, cls=None, n_classes=0, x=None):
    """Boolean [B]: the class lies in [0, K) (every row without cls) and every regressor is finite."""
    ok = np.ones(B, dtype=bool)
    if cls is not None:
        c = np.asarray(cls).astype(np.int64)
        ok &= (c >= 0) & (c < n_classes)
    if x is not None and np.asarray(x).size:
        ok &= np.isfinite(np.asarray(x, dtype=np.float64).reshape(B, -1)).all(1)
    return ok


def unit_moments(act, cls=None, n_classes=0, x=None):
    """The seven accumulators of one call from zero: float64 sums of products formed in float64 from the fp32 inputs."""
    a = np.asarray(act, dtype=np.float32).astype(np.float64)
    B, H = a.shape
    K = int(n_classes) if cls is not None else 0
    xs = None if x is None else np.asarray(x, dtype=np.float32).astype(np.float64).reshape(B, -1)
    R = 0 if xs is None else xs.shape[1]
    ok = used_rows(B, cls, K, xs)
    au = a[ok]
    z = np.concatenate([np.ones((au.shape[0], 1)), xs[ok] if R else np.zeros((au.shape[0], 0))], 1)
    o = {"cls_sum": np.zeros((K, H)), "cls_sumsq": np.zeros((K, H)), "cls_count": np.zeros(K, dtype=np.int64)}
    if K:
        c = np.asarray(cls).astype(np.int64)[ok]
        for k in range(K):
            rows = au[c == k]
            o["cls_sum"][k], o["cls_sumsq"][k], o["cls_count"][k] = rows.sum(0), (rows * rows).sum(0), rows.shape[0]
    with np.errstate(invalid="ignore"):
        o["xa"] = np.stack([(z[:, q:q + 1] * au).sum(0) for q in range(R + 1)])
        o["aa"] = (au * au).sum(0)
    o["xx"] = np.array([[(z[:, p] * z[:, q]).sum() for q in range(R + 1)] for p in range(R + 1)], dtype=np.float64).reshape(R + 1, R + 1)
    o["rows"] = np.array([int(ok.sum()), int(B - ok.sum())], dtype=np.int64)
    return o


def abs_moments(act, cls=None, n_classes=0, x=None):
    """Per accumulator entry the float64 sum of the absolute values of its terms (the same rows skipped)."""
    return unit_moments(np.abs(np.asarray(act, dtype=np.float32)), cls, n_classes, None if x is None else np.abs(np.asarray(x, dtype=np.float32)))


def term_counts(mom):
    """Per accumulator entry the number of its terms: the class count for the class sums, the used rows for the others."""
    n = int(mom["rows"][0])
    return {"cls_sum": mom["cls_count"][:, None].astype(np.float64), "cls_sumsq": mom["cls_count"][:, None].astype(np.float64),
            "xa": float(n), "aa": float(n), "xx": float(n)}


def add(a, b):
    return {k: a[k] + b[k] for k in KEYS}


def statistics(act, cls, n_classes, x=None, class_values=None, numerosity=0, r2_min=0.1, beta_min=0.1, beta_max=0.1):
    """The derived statistics straight from the rows: numpy.linalg.lstsq on [1, x], per-class arrays, residuals.  Also
    ``cond`` = cond(C_xx) of the centred regressors (1 without regressors), which the tolerances of the tests scale with."""
    a = np.asarray(act, dtype=np.float32).astype(np.float64)
    B, H = a.shape
    K = int(n_classes)
    xs = np.zeros((B, 0)) if x is None else np.asarray(x, dtype=np.float32).astype(np.float64).reshape(B, -1)
    R = xs.shape[1]
    ok = used_rows(B, cls, K, xs)
    a, X, c = a[ok], xs[ok], np.asarray(cls).astype(np.int64)[ok]
    n = a.shape[0]
    grand = a.mean(0)
    ss_tot = ((a - grand) ** 2).sum(0)
    with np.errstate(invalid="ignore"):
        degenerate = ~(ss_tot > 1e-12 * (a * a).sum(0)) | ~np.isfinite(a).all(0)
    count = np.array([(c == k).sum() for k in range(K)], dtype=np.int64)
    mean = np.full((K, H), np.nan)
    var = np.full((K, H), np.nan)
    for k in range(K):
        if count[k]:
            mean[k], var[k] = a[c == k].mean(0), a[c == k].var(0)
    full = count > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        eta2 = sum(count[k] * (mean[k] - grand) ** 2 for k in range(K) if full[k]) / ss_tot
        hi = np.where(full[:, None], mean, -np.inf)
        preferred = hi.argmax(0)
        low = np.where(full[:, None], mean, np.inf).min(0)
        depth = hi.max(0) - low
        v = np.log(np.arange(1, K + 1, dtype=np.float64)) if class_values is None else np.asarray(class_values, dtype=np.float64)
        w = np.where(full[:, None], mean - low, 0.0)
        vv = np.where(full, v, 0.0)
        centre = (w * vv[:, None]).sum(0) / w.sum(0)
        width = np.sqrt((w * np.where(full[:, None], (vv[:, None] - centre) ** 2, 0.0)).sum(0) / w.sum(0))
    D = np.concatenate([np.ones((n, 1)), X], 1)
    beta = np.linalg.lstsq(D, a, rcond=None)[0]
    res = a - D @ beta
    with np.errstate(invalid="ignore", divide="ignore"):
        r2 = 1.0 - (res * res).sum(0) / ss_tot
        beta_std = beta[1:] * X.std(0)[:, None] / a.std(0)[None, :]
    Xc = X - X.mean(0)
    rank = int(np.linalg.matrix_rank(Xc)) if R else 0
    cond = float(np.linalg.cond(Xc.T @ Xc)) if R else 1.0
    nanv = np.full(H, np.nan)
    eta2, r2, centre, width = (np.where(degenerate, nanv, t) for t in (eta2, r2, centre, width))
    beta_std = np.where(degenerate[None, :], np.nan, beta_std)
    if R:
        b = np.abs(beta_std)
        others = np.ones(R, dtype=bool); others[numerosity] = False
        with np.errstate(invalid="ignore"):
            selective = (r2 >= r2_min) & (b[numerosity] >= beta_min) & (b[others] < beta_max).all(0)
    else:
        selective = np.zeros(H, dtype=bool)
    return {"count": count, "mean": mean, "var": var, "eta2": eta2, "preferred": preferred, "depth": depth, "centre": centre,
            "width": width, "beta": beta, "beta_std": beta_std, "r2": r2, "rank": rank, "degenerate": degenerate,
            "selective": selective, "n": n, "n_skipped": B - n, "cond": cond}
