"""Per-unit tuning curves and feature regressions of a layer.

Which hidden units are tuned to number, to which number, and how much of each unit's response is explained by number rather than by
the continuous visual features: the per-unit regression on log numerosity and log cumulative area that finds the "number-sensitive"
units of Stoianov & Zorzi (2012), next to tuning curves, preferred numerosity, tuning width and a one-way ANOVA per unit.

Everything here is a closed form of one family of sufficient statistics of the activation matrix, accumulated by
``engine.unit_moments`` (imdbn_unit_moments) in one fused pass over the validation embeddings, which stay on the device:

    cls_sum, cls_sumsq [K, H], cls_count [K]   per (class, unit) sum a, sum a^2 and the rows of the class
    xa [R + 1, H], aa [H], xx [R + 1, R + 1]   sum z a, sum a^2, sum z z^T with z = [1, x_1 .. x_R]
    rows [2]                                   rows used, rows skipped

``tuning_from_moments`` turns such a dict into the statistics (float64, on the dict's device, one ``.cpu()`` at the end);
``evaluate_unit_tuning`` builds the classes and regressors from ``model.features`` and runs the whole analysis;
``log_unit_tuning`` logs its scalars; ``population_curve`` is the table behind the population-code figure.  Figures stay out of
scope, as everywhere in this package.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from .. import engine as _E
from . import probe_utils as _PU

_EPS = 2.0 ** -52


def _pinv_solve(C: torch.Tensor, c: torch.Tensor, scale: torch.Tensor):
    """Minimum-norm least-squares solution of the symmetric system ``C b = c`` and the rank of ``C``, by an eigendecomposition
    (what ``torch.linalg.lstsq`` gives with a rank-revealing driver; the device drivers of lstsq assume full rank, a collinear
    regressor pair does not have it).  Eigenvalues at or below ``64 eps scale`` count as zero: ``scale`` is the largest
    un-centred second moment, the magnitude at which the centred matrix was rounded."""
    lam, V = torch.linalg.eigh(C)
    keep = lam > 64.0 * _EPS * scale
    inv = torch.where(keep, 1.0 / torch.where(keep, lam, torch.ones_like(lam)), torch.zeros_like(lam))
    return V @ (inv[:, None] * (V.T @ c)), keep.sum()


@torch.no_grad()
def tuning_from_moments(acc: Dict[str, torch.Tensor], class_values: Optional[torch.Tensor] = None, names: Optional[Sequence[str]] = None,
                        numerosity: int = 0, r2_min: float = 0.1, beta_min: float = 0.1, beta_max: float = 0.1) -> dict:
    """The per-unit statistics of an accumulator dict of ``engine.unit_moments`` (a pure function of it; any device).

    With n = rows used, abar = xa[0] / n and SS_tot = aa - xa[0]^2 / n:

    * curves: ``count`` [K], ``mean`` [K, H] (NaN for an empty class), ``var`` [K, H] (population variance, clamped at 0);
    * ANOVA: ``eta2`` [H] = sum_k count_k (mean_k - abar)^2 / SS_tot;
    * tuning: ``preferred`` [H] (the first maximum of the curve over non-empty classes), ``depth`` [H] (max - min), ``centre`` and
      ``width`` [H] (mean and standard deviation of ``class_values`` -- default log(k + 1) -- under the weights mean_k - min_k mean);
    * regression on [1, x_1 .. x_R], from the centred forms C_xx = xx[1:, 1:] - n xbar xbar^T and c_xa = xa[1:] - n xbar abar so that
      a large feature mean costs no digits: ``beta`` [R + 1, H] (intercept first), ``beta_std`` [R, H] = beta_r sd(x_r) / sd(a),
      ``r2`` [H] = 1 - SS_res / SS_tot with SS_res the full quadratic form, ``rank`` of C_xx (a deficient C_xx gets the
      minimum-norm slopes);
    * flags: ``degenerate`` [H] (SS_tot <= 1e-12 aa or a non-finite moment: a constant or poisoned unit; its eta2, r2, beta_std,
      centre and width are NaN -- the threshold guards a division by rounding noise, it is no tolerance), ``selective`` [H]
      (Stoianov & Zorzi 2012: r2 >= r2_min, |beta_std[numerosity]| >= beta_min and |beta_std[r]| < beta_max for every other r);
    * ``n``, ``n_skipped``, ``names``.

    Without classes (K = 0) the curve statistics are empty or NaN and ``preferred`` is -1; without regressors ``r2`` is 0 and no
    unit is selective."""
    f64 = torch.float64
    cs, cq, cc = acc["cls_sum"].to(f64), acc["cls_sumsq"].to(f64), acc["cls_count"].to(f64)
    xa, aa, xx = acc["xa"].to(f64), acc["aa"].to(f64), acc["xx"].to(f64)
    dev = xa.device
    K, H, R = cs.size(0), xa.size(1), xa.size(0) - 1
    n = acc["rows"][0].to(f64)
    nan = torch.full((H,), float("nan"), dtype=f64, device=dev)
    abar = xa[0] / n
    ss_tot = aa - xa[0] * xa[0] / n
    finite = torch.isfinite(aa) & torch.isfinite(xa).all(0)
    if K:
        finite &= torch.isfinite(cs).all(0) & torch.isfinite(cq).all(0)
    degenerate = ~finite | ~(ss_tot > 1e-12 * aa)
    ss_safe = torch.where(degenerate, torch.ones_like(ss_tot), ss_tot)

    # ---- curves, ANOVA, tuning
    full = cc > 0
    mean = cs / cc[:, None]                                            # 0 / 0: NaN for an empty class
    var = (cq / cc[:, None] - mean * mean).clamp(min=0.0)
    if K:
        fk = full[:, None]
        zero = torch.zeros((), dtype=f64, device=dev)
        eta2 = torch.where(fk, cc[:, None] * (mean - abar) ** 2, zero).sum(0) / ss_safe
        hi = torch.where(fk, mean, torch.full_like(mean, float("-inf")))
        lo = torch.where(fk, mean, torch.full_like(mean, float("inf")))
        preferred = hi.argmax(0)
        top, low = hi.max(0).values, lo.min(0).values
        depth = top - low
        v = (torch.log(torch.arange(1, K + 1, dtype=f64, device=dev)) if class_values is None
             else torch.as_tensor(class_values).to(device=dev, dtype=f64).reshape(K))
        w = torch.where(fk, mean - low, zero)
        wv = torch.where(fk, w * v[:, None], zero)                     # an empty class may carry any class value
        sw = w.sum(0)
        centre = wv.sum(0) / sw
        width = (torch.where(fk, w * (v[:, None] - centre) ** 2, zero).sum(0) / sw).clamp(min=0.0).sqrt()
    else:
        eta2, depth, centre, width = nan, nan, nan, nan
        preferred = torch.full((H,), -1, dtype=torch.long, device=dev)

    # ---- regression
    if R:
        xbar = xx[0, 1:] / n
        Cxx = xx[1:, 1:] - n * xbar[:, None] * xbar[None, :]
        cxa = xa[1:] - n * xbar[:, None] * abar[None, :]
        cxa_safe = torch.where(finite[None, :], cxa, torch.zeros_like(cxa))
        slopes, rank = _pinv_solve(Cxx, cxa_safe, xx[1:, 1:].diagonal().abs().max())
        slopes = torch.where(finite[None, :], slopes, nan[None, :])
        beta = torch.cat([(abar - (slopes * xbar[:, None]).sum(0))[None, :], slopes], 0)
        ss_res = ss_tot - 2.0 * (slopes * cxa).sum(0) + (slopes * (Cxx @ slopes)).sum(0)
        r2 = 1.0 - ss_res / ss_safe
        beta_std = slopes * (Cxx.diagonal().clamp(min=0.0)[:, None] / ss_safe[None, :]).sqrt()
    else:
        rank = torch.zeros((), dtype=torch.long, device=dev)
        beta, beta_std, r2 = abar[None, :], torch.zeros((0, H), dtype=f64, device=dev), torch.zeros(H, dtype=f64, device=dev)
    eta2, r2, centre, width = (torch.where(degenerate, nan, t) for t in (eta2, r2, centre, width))
    beta_std = torch.where(degenerate[None, :], nan[None, :], beta_std)
    if R and 0 <= int(numerosity) < R:
        b = beta_std.abs()
        others = torch.ones(R, dtype=torch.bool, device=dev)
        others[int(numerosity)] = False
        selective = (r2 >= r2_min) & (b[int(numerosity)] >= beta_min) & (b[others] < beta_max).all(0)
    else:
        selective = torch.zeros(H, dtype=torch.bool, device=dev)

    # ---- one host copy: everything goes over as one float64 vector (the integers and flags are exact in it)
    out = {"count": (cc, torch.long), "mean": (mean, f64), "var": (var, f64), "eta2": (eta2, f64), "preferred": (preferred, torch.long),
           "depth": (depth, f64), "centre": (centre, f64), "width": (width, f64), "beta": (beta, f64), "beta_std": (beta_std, f64),
           "r2": (r2, f64), "rank": (rank, torch.long), "degenerate": (degenerate, torch.bool), "selective": (selective, torch.bool),
           "n": (acc["rows"][0], torch.long), "n_skipped": (acc["rows"][1], torch.long)}
    flat = torch.cat([t.to(f64).reshape(-1) for t, _ in out.values()]).cpu()
    res, at = {}, 0
    for k, (t, dt) in out.items():
        res[k] = flat[at:at + t.numel()].reshape(t.shape).to(dt)
        at += t.numel()
    res["rank"], res["n"], res["n_skipped"] = int(res["rank"]), int(res["n"]), int(res["n_skipped"])
    res["names"] = list(names) if names is not None else [f"x{r + 1}" for r in range(R)]
    return res


def _regressor(feats: dict, name: str) -> torch.Tensor:
    by_norm = {_PU._norm(k): k for k in feats}
    key = by_norm.get(_PU._norm(name))
    if key is None:
        raise ValueError(f"unit tuning: the model's features have no '{name}' (they have {sorted(feats)})")
    return feats[key]


@torch.no_grad()
def evaluate_unit_tuning(model, upto_layer: Optional[int] = None, joint: bool = False, regressors: Sequence[str] = ("labels", "cum_area"),
                         log: bool = True, n_classes: Optional[int] = None, chunk: Optional[int] = None, **thresholds) -> dict:
    """The whole analysis for every unit of one layer over the validation split: the embeddings ``model.represent(...)`` (the joint
    layer's with ``joint``) stay on the device and go through ``engine.unit_moments`` in chunks of ``chunk`` rows (default: all at
    once); the result is ``tuning_from_moments`` of the accumulators plus ``class_labels``.

    The class of a row is its ``labels`` feature as an integer, offset so that the smallest label is class 0 (``class_labels[k]``
    is the label of class k; ``class_values`` = log of it).  The regressors are ``model.features`` entries by the normalised names
    of ``probe_utils`` (``labels``, ``cum_area``, ``convex_hull``, ``density``), taken as log with ``log``; a non-positive value
    then gives a non-finite regressor and its row is skipped and counted, from the curves as from the regression.  ``n_classes``
    defaults to the span of the labels; rows of a class beyond a smaller one are skipped.  The host reads two scalars (the
    smallest and largest label) and the result.
    ``thresholds``: ``r2_min``, ``beta_min``, ``beta_max``, ``numerosity`` of ``tuning_from_moments`` (``numerosity`` defaults to
    the position of ``labels`` among the regressors)."""
    if getattr(model, "features", None) is None:
        raise ValueError("unit tuning needs model.features (a validation loader over a dataset that carries the per-stimulus "
                         "feature lists); this model has none")
    if joint:
        E, feats = _PU.compute_joint_embeddings_and_features(model)
    else:
        E, feats = _PU.compute_val_embeddings_and_features(model, upto_layer=upto_layer)
    if "labels" not in feats:
        raise ValueError("unit tuning needs the 'labels' feature (the numerosity of every stimulus)")
    names = [_PU._norm(r) for r in regressors]
    lab = feats["labels"].round().long()
    low, high = torch.stack([lab.min(), lab.max()]).tolist()          # two scalars: the only host read before the result
    cls = (lab - low).to(torch.int32)
    K = int(n_classes) if n_classes is not None else high - low + 1
    class_labels = low + torch.arange(K)
    x = None
    if regressors:
        x = torch.stack([_regressor(feats, r).to(torch.float32) for r in regressors], 1)
        x = torch.log(x) if log else x
    eng = _E.get_engine(E)
    N = E.size(0)
    step = N if not chunk else int(chunk)
    acc = None
    for i in range(0, N, step):
        acc = eng.unit_moments(E[i:i + step], cls[i:i + step], K, None if x is None else x[i:i + step], acc)
    if "numerosity" not in thresholds:
        thresholds["numerosity"] = names.index("labels") if "labels" in names else 0
    res = tuning_from_moments(acc, class_values=torch.log(class_labels.to(torch.float64)), names=list(regressors), **thresholds)
    res["class_labels"] = class_labels
    return res


def population_curve(result: dict) -> torch.Tensor:
    """``[K, K]`` float64: row p is the mean tuning curve of the selective units whose preferred class is p (NaN where there is
    none) -- the table behind the population-code figure."""
    mean, pref, sel = result["mean"], result["preferred"], result["selective"]
    K = mean.size(0)
    out = torch.full((K, K), float("nan"), dtype=torch.float64)
    for p in range(K):
        m = sel & (pref == p)
        if bool(m.any()):
            out[p] = mean[:, m].mean(1)
    return out


def log_unit_tuning(model, epoch: int, upto_layer: Optional[int] = None, joint: bool = False, layer_tag: Optional[str] = None,
                    wandb_run=None, **kw) -> dict:
    """Run ``evaluate_unit_tuning`` and log its scalars (no figures), in the manner of ``log_linear_probe``: the number and fraction
    of selective units, mean and median r2 and mean eta2 over the non-degenerate units, and the histogram of ``preferred`` over the
    selective units as one count per class.  Returns the result with the logged payload under ``"scalars"``."""
    res = evaluate_unit_tuning(model, upto_layer=upto_layer, joint=joint, **kw)
    tag = layer_tag or ("joint" if joint else ("top" if upto_layer is None else f"layer{upto_layer}"))
    ok = ~res["degenerate"]
    sel = res["selective"]
    r2, eta2 = res["r2"][ok], res["eta2"][ok]
    nanf = float("nan")
    payload = {f"tuning/{tag}/n_selective": int(sel.sum()), f"tuning/{tag}/frac_selective": float(sel.double().mean()),
               f"tuning/{tag}/r2_mean": float(r2.mean()) if r2.numel() else nanf,
               f"tuning/{tag}/r2_median": float(r2.median()) if r2.numel() else nanf,
               f"tuning/{tag}/eta2_mean": float(eta2.mean()) if eta2.numel() else nanf, "epoch": epoch}
    hist = torch.bincount(res["preferred"][sel], minlength=res["mean"].size(0))
    for lab, c in zip(res["class_labels"].tolist(), hist.tolist()):
        payload[f"tuning/{tag}/preferred/{lab}"] = int(c)
    _PU._log(wandb_run if wandb_run is not None else getattr(model, "wandb_run", None), payload)
    res["scalars"] = payload
    return res
