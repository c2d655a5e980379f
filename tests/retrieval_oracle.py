"""float64 numpy twin of imdbn_rbm_pair_scores and imdbn.utils.retrieval: pair scores, both rank vectors, top-k lists, metrics,
and the rank interval a score tolerance allows.  The *definition*, written for clarity, fed the same fp32 parameters.

TEST INFRASTRUCTURE ONLY."""
import numpy as np


def f64(a):
    return np.asarray(a, dtype=np.float64)


def softplus(x):
    return np.logaddexp(0.0, x)


def scores(W, hid_bias, vis_bias, D1, z1, z2):
    """S[q, n] = -F([z1_q | z2_n]) = z1_q . b[:D1] + z2_n . b[D1:] + sum_j softplus(c_j + (z1_q W[:D1])_j + (z2_n W[D1:])_j)"""
    W, c, b, z1, z2 = f64(W), f64(hid_bias), f64(vis_bias), f64(z1), f64(z2)
    a = c[None, :] + z1 @ W[:D1]
    bb = z2 @ W[D1:]
    return (z1 @ b[:D1])[:, None] + (z2 @ b[D1:])[None, :] + softplus(a[:, None, :] + bb[None, :, :]).sum(-1)


def scores_loops(W, hid_bias, vis_bias, D1, z1, z2):
    """The same by a triple loop over (q, n, j) on the concatenated visible row: nothing shared with `scores` but the formula."""
    W, c, b = f64(W), f64(hid_bias), f64(vis_bias)
    Q, N = len(z1), len(z2)
    S = np.zeros((Q, N))
    for q in range(Q):
        for n in range(N):
            v = np.concatenate([f64(z1[q]), f64(z2[n])])
            s = float(v @ b)
            for j in range(W.shape[1]):
                x = c[j] + float(v @ W[:, j])
                s += max(x, 0.0) + np.log1p(np.exp(-abs(x)))
            S[q, n] = s
    return S


def ranks_rows(S, gt):
    """rank[q] = #{n : S[q, n] > S[q, g]} + #{n < g : S[q, n] == S[q, g]}, g = gt[q]; -1 (score NaN) for g outside [0, N).
    Returns (rank int64 [Q], matched score [Q])."""
    S = np.asarray(S)
    Q, N = S.shape
    rank = np.full(Q, -1, dtype=np.int64)
    ref = np.full(Q, np.nan, dtype=S.dtype)
    for q in range(Q):
        g = int(gt[q])
        if 0 <= g < N:
            r = S[q, g]
            ref[q] = r
            with np.errstate(invalid="ignore"):
                rank[q] = int((S[q] > r).sum() + (S[q, :g] == r).sum())
    return rank, ref


def ranks_cols(S, gt):
    return ranks_rows(np.asarray(S).T, gt)


def topk(S, k):
    """Per row the first k columns in rank order (score descending, lower index on ties, NaN never): (idx int32, score), -1 / -inf padded."""
    S = np.asarray(S)
    Q, N = S.shape
    idx = np.full((Q, k), -1, dtype=np.int32)
    sc = np.full((Q, k), -np.inf, dtype=S.dtype)
    for q in range(Q):
        cand = [n for n in range(N) if S[q, n] == S[q, n]]
        cand.sort(key=lambda n: (-S[q, n], n))
        for e, n in enumerate(cand[:k]):
            idx[q, e] = n
            sc[q, e] = S[q, n]
    return idx, sc


def rank_interval(S64, gt, tau):
    """What a score matrix within tau of S64 can give as the row ranks: lo = #{n != g : S[n] > S[g] + 2 tau},
    hi = #{n != g : S[n] >= S[g] - 2 tau}.  Rows with an invalid gt: (-1, -1)."""
    S64 = f64(S64)
    Q, N = S64.shape
    lo = np.full(Q, -1, dtype=np.int64)
    hi = np.full(Q, -1, dtype=np.int64)
    for q in range(Q):
        g = int(gt[q])
        if 0 <= g < N:
            others = np.delete(S64[q], g)
            lo[q] = int((others > S64[q, g] + 2 * tau).sum())
            hi[q] = int((others >= S64[q, g] - 2 * tau).sum())
    return lo, hi


def metrics(ranks, ks=(1, 5, 10)):
    """imdbn.utils.retrieval.retrieval_metrics, restated."""
    r = np.asarray(ranks, dtype=np.int64).reshape(-1)
    ok = np.sort(r[r >= 0]).astype(np.float64)
    n = ok.size
    nan = float("nan")
    out = {f"recall@{int(k)}": float((ok < k).mean()) if n else nan for k in ks}
    out["median_rank"] = float(ok[(n - 1) // 2]) if n else nan
    out["mean_rank"] = float(ok.mean()) if n else nan
    out["mrr"] = float((1.0 / (ok + 1.0)).mean()) if n else nan
    out["n"] = int(n)
    out["skipped"] = int(r.size - n)
    return out
