"""Numpy twin of imdbn_rbm_ais (include/imdbn_engine.h) and the exact partition function of a small RBM.

TEST INFRASTRUCTURE ONLY.  ``ais_logw`` restates the estimator in float64: the logits x = c + v W are formed in fp32 (as the
engine's up propagation forms them) and widened; both sums of the weight increment, the softplus and the sigmoid run in double.
Every Bernoulli decision 1[p > u] records its margin |p - u|; the smallest one is returned, so a test can insist that no decision
of the case sits within rounding distance of its draw before it asks the device for the same decisions.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.draws import PhiloxStream  # noqa: F401  (the draw source of the Philox cases)
from oracle_engine import OracleEngine, _Src, _np

F32, F64 = np.float32, np.float64


def softplus(t):
    t = np.asarray(t, F64)
    return np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))


def sigmoid(t):
    t = np.asarray(t, F64)
    return 1.0 / (1.0 + np.exp(-t))


def log_z_base(V, H, b_A):
    """log Z of the base-rate model: H log 2 + sum_i softplus(b_A,i); no b_A = zeros = V log 2."""
    return H * np.log(2.0) + float(softplus(np.zeros(V, F32) if b_A is None else np.asarray(b_A, F32)).sum())


def logmeanexp(x):
    x = np.asarray(x, F64)
    m = x.max()
    return float(m + np.log(np.exp(x - m).mean()))


def weight_stats(logw):
    """(logmeanexp, se, ess) as imdbn/utils/likelihood.py defines them: on weights shifted by their maximum."""
    x = np.asarray(logw, F64)
    w = np.exp(x - x.max())
    se = float(w.std(ddof=1) / (w.mean() * np.sqrt(w.size))) if w.size > 1 else 0.0
    return logmeanexp(x), se, float(w.sum() ** 2 / (w * w).sum())


def ais_logw(W, b, c, b_A, betas, M, draws):
    """-> (logw [M] float64, v_K [M, V] float32, smallest |p - u| over every Bernoulli decision made)."""
    W, b, c = np.asarray(W, F32), np.asarray(b, F32), np.asarray(c, F32)
    V, H = W.shape
    bA = np.zeros(V, F32) if b_A is None else np.asarray(b_A, F32)
    betas = np.asarray(betas, F32)
    K = betas.size - 1
    assert K >= 1 and betas[0] == 0 and betas[K] == 1 and (np.diff(betas) > 0).all()
    bt = betas.astype(F64)
    margin = np.inf

    def decide(p, u):
        nonlocal margin
        margin = min(margin, float(np.abs(p - u.astype(F64)).min()))
        return (p > u).astype(F32)

    v = decide(np.broadcast_to(sigmoid(bA), (M, V)), draws.uniform((M, V)))
    logw = np.zeros(M, F64)
    db = b.astype(F64) - bA.astype(F64)
    for k in range(1, K + 1):
        x = (v @ W + c).astype(F32).astype(F64)
        logw += (bt[k] - bt[k - 1]) * (v.astype(F64) @ db) + (softplus(bt[k] * x) - softplus(bt[k - 1] * x)).sum(1)
        if k < K:
            h = decide(sigmoid(bt[k] * x), draws.uniform((M, H)))
            vl = (h @ W.T).astype(F32).astype(F64) + b.astype(F64)
            v = decide(sigmoid(bt[k] * vl + (1.0 - bt[k]) * bA.astype(F64)), draws.uniform((M, V)))
    return logw, v, margin


def exact_log_z(W, b, c):
    """log sum_{v, h} exp(-E) by enumerating the 2^H hidden states (H <= 16), in double."""
    W, b, c = np.asarray(W, F64), np.asarray(b, F64), np.asarray(c, F64)
    V, H = W.shape
    assert H <= 16
    hs = ((np.arange(1 << H)[:, None] >> np.arange(H)[None, :]) & 1).astype(F64)        # [2^H, H]
    t = hs @ c + softplus(hs @ W.T + b).sum(1)
    m = t.max()
    return float(m + np.log(np.exp(t - m).sum()))


class AisOracleEngine(OracleEngine):
    """The CPU test double with ``ais``: what HipEngine.ais returns, from the twin; ``last_log`` = the draws it consumed."""

    def ais(self, rbm, betas, n_chains, rng, base_vis_bias=None, return_state=False):
        s = _Src(rng)
        n0 = len(s.p.log)
        bA = None if base_vis_bias is None else _np(base_vis_bias)
        b = betas.tolist() if hasattr(betas, "tolist") else list(betas)
        logw, v, self.last_margin = ais_logw(_np(rbm.W.data), _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), bA, np.asarray(b, F32),
                                             int(n_chains), s)
        self.last_log = [(k, int(shape[1])) for k, shape in s.p.log[n0:]]
        s.done()
        lw = torch.from_numpy(logw)
        return (lw, self._t(v)) if return_state else lw
