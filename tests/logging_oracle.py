"""numpy (fp64) restatement of the numeric core of imdbn/utils/imdbn_logging.py (reference :646-965): the latent scores, the
deduplicated / excluding top-k walk with its tie rule, the TXT->IMG trajectory with given draws, PCA with sklearn's sign
convention, and the joint auto-reconstruction metrics."""
from __future__ import annotations

import numpy as np

from trace_oracle import h_probs, sigmoid, v_probs


def metric_id(metric) -> int:
    """0 cosine, 1 inner, 2 l2, 3 "cosine_l1" (the cosine of log_vecdb_neighbors_for_traj: F.normalize(x, 1) is p = 1)."""
    if isinstance(metric, (int, np.integer)):
        return int(metric)
    return {"cosine": 0, "ip": 1, "inner": 1, "cosine_l1": 3}.get(metric, 2)


def scores(bank, q, metric):
    """[Q, N] fp64 scores: cosine (F.normalize eps 1e-12), inner, or l2 = -(|q|^2 + |b|^2 - 2 <q, b>)."""
    Z, q = np.asarray(bank, np.float64), np.atleast_2d(np.asarray(q, np.float64))
    m = metric_id(metric)
    if m == 0:
        Zn = Z / np.maximum(np.linalg.norm(Z, axis=1, keepdims=True), 1e-12)
        qn = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
        return qn @ Zn.T
    if m == 1:
        return q @ Z.T
    if m == 3:
        return (q / np.maximum(np.abs(q).sum(1, keepdims=True), 1e-12)) @ (Z / np.maximum(np.abs(Z).sum(1, keepdims=True), 1e-12)).T
    return -((q ** 2).sum(1, keepdims=True) + (Z ** 2).sum(1)[None, :] - 2 * q @ Z.T)


def topk_row(s, k, exclude=-1, key=None):
    """The reference's walk over one score row sorted descending (ties: the lower index first): skip ``exclude``, with a key
    skip every row whose key was seen.  Returns (ids, vals, margin): margin = the smallest score gap that decides the answer
    (between consecutive candidates up to the (k+1)-th, and between each picked row and the best other row of its key;
    exact ties do not count)."""
    s = np.asarray(s, np.float64)
    order = np.lexsort((np.arange(s.size), -s))
    ids, vals, seen, best_of = [], [], set(), {}
    for i in order:
        i = int(i)
        if i == exclude:
            continue
        if key is not None:
            kk = (float(key[i, 0]), float(key[i, 1]))
            if kk in seen:
                if kk not in best_of:
                    best_of[kk] = s[i]
                continue
            seen.add(kk)
        ids.append(i)
        vals.append(s[i])
        if len(ids) > k:
            break
    gaps = [vals[j] - vals[j + 1] for j in range(len(vals) - 1)]
    if key is not None:
        for i in ids[:k]:
            kk = (float(key[i, 0]), float(key[i, 1]))
            if kk in best_of:
                gaps.append(s[i] - best_of[kk])
    gaps = [x for x in gaps if x != 0]        # exact ties (identical rows) are decided by the index rule on both sides
    margin = min(gaps) if gaps else np.inf
    return np.asarray(ids[:k], np.int64), np.asarray(vals[:k]), margin


def topk(bank, q, metric, k, exclude=None, key=None):
    """Per query row: (ids [Q, k] padded with -1, vals [Q, k] padded with -inf, margins [Q])."""
    S = scores(bank, q, metric)
    Q = S.shape[0]
    ids, vals, margin = np.full((Q, k), -1, np.int64), np.full((Q, k), -np.inf), np.zeros(Q)
    for r in range(Q):
        i, v, m = topk_row(S[r], k, -1 if exclude is None else int(exclude[r]), key)
        ids[r, :len(i)], vals[r, :len(v)], margin[r] = i, v, m
    return ids, vals, margin


def row_keys(X):
    X = np.asarray(X, np.float64).reshape(len(X), -1)
    return np.stack([X.sum(1), (X ** 2).sum(1)], 1)


def trajectory(W, hb, vb, groups, z0, y, u):
    """TXT->IMG trajectory: z0 [B, Dz], y [B, K], u [T, B, H] uniforms; h = (p(h|v) > u), v = p(v|h) re-clamped.
    Returns (Z_traj [T+1, B, Dz], smallest |p - u|)."""
    z0, y = np.asarray(z0, np.float64), np.asarray(y, np.float64)
    Dz = z0.shape[1]
    v = np.concatenate([z0, y], 1)
    out, margin = [z0], np.inf
    for t in range(len(u)):
        p = h_probs(W, hb, v)
        margin = min(margin, float(np.abs(p - u[t]).min()))
        h = (p > u[t]).astype(np.float64)
        v = v_probs(W, vb, h, groups)
        v[:, Dz:] = y
        out.append(v[:, :Dz].copy())
    return np.stack(out), margin


def pca(Z, n):
    """(mean, components [n, D]) of the rows of Z, signs as sklearn's svd_flip(u_based_decision=False)."""
    Z = np.asarray(Z, np.float64)
    mean = Z.mean(0)
    w, V = np.linalg.eigh((Z - mean).T @ (Z - mean))
    comp = V[:, np.argsort(w)[::-1][:n]].T.copy()
    j = np.argmax(np.abs(comp), axis=1)
    comp *= np.sign(comp[np.arange(n), j])[:, None]
    return mean, comp


def auto_recon(small, x, y):
    """(text top-1, text BCE, image MSE) of the joint auto-reconstruction (reference :919-965); ``small`` a SmallOracle."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    z = small.represent(x)
    v = v_probs(small.W, small.vb, h_probs(small.W, small.hb, np.concatenate([z, y], 1)), small.groups)
    Dz = z.shape[1]
    yh = v[:, Dz:]
    z_dec = v[:, :Dz]
    for W, vb in reversed(small.decode_layers()):
        z_dec = sigmoid(z_dec @ W.T + vb)
    rec = np.clip(z_dec, 0, 1)
    top1 = float((yh.argmax(1) == y.argmax(1)).mean())
    p = np.clip(yh, 1e-6, 1 - 1e-6)
    bce = float(-(y * np.log(p) + (1 - y) * np.log(1 - p)).mean())
    return top1, bce, float(((x - rec) ** 2).mean())
