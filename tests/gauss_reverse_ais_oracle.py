"""Numpy twin of imdbn_rbm_gauss_reverse_ais (include/imdbn_engine.h): reverse annealed importance sampling over Gaussian
visibles, and the exact log-density of a small Gaussian-visible RBM by enumerating its 2^H hidden states.

TEST INFRASTRUCTURE ONLY.  ``gauss_reverse_ais_logw(..., dt)`` walks the ladder downwards in the dtype ``dt``, under the rules of
tests/gauss_ais_oracle.py:

float64 (the reference)   the state, u = v e^{-z}, the sigmoid and the visible expression run in float64; the two matrix products are
                          fp32 numbers (each row summed on its own in float64 and rounded once: gauss_ais_oracle.rows_times) that are
                          then WIDENED; every sum of a weight term and the softplus run in double.
float32 (the restatement) every fp32 quantity of the device in fp32: the state, u, e^{-z}, e^{z/2}, the sigmoid of the h draw and
                          v = ((1 - beta) b_A + beta m) + e^{z/2} n in the engine's order.  The sums stay in double, as on the device.

Draw schedule (imdbn.engine.rng.sched_gauss_reverse_ais): K x [("u", H), ("n", V)].
"""
from __future__ import annotations

import itertools

import numpy as np

from gauss_ais_oracle import log_z_base, rows_times, softplus  # noqa: F401  (log_z_base: for the callers)

F32, F64 = np.float32, np.float64


def gauss_reverse_ais_logw(W, b, c, z, b_A, betas, x, draws, dt=F64, record=None):
    """-> (logw [R] float64, u_1 [R, V] in dt, the smallest Bernoulli margin |sigmoid(beta x) - U|).  ``x`` [R, V]: the caller's
    rows; ``b_A`` None: b.  ``record`` (a list) receives every h sample, T_K's first.  A row with a non-finite element gets NaN."""
    W, b, c, z = (np.asarray(t, F32) for t in (W, b, c, z))
    x = np.asarray(x, F32)
    R, (V, H) = x.shape[0], W.shape
    bA = b if b_A is None else np.asarray(b_A, F32)
    betas = np.asarray(betas, F32)
    K = betas.size - 1
    assert K >= 1 and betas[0] == 0 and betas[K] == 1 and (np.diff(betas) > 0).all()
    bt = betas.astype(F64)
    # the weight terms' constants, in double on both sides
    b64, bA64, z64 = b.astype(F64), bA.astype(F64), z.astype(F64)
    coef = (b64 - bA64) * np.exp(-z64)
    mid = 0.5 * (b64 + bA64)
    # the state's constants in dt
    zt = z.astype(dt)
    sd, iv = np.exp(dt(0.5) * zt).astype(dt), np.exp(-zt).astype(dt)
    bAt = bA.astype(dt)
    margin = np.inf

    def logits(v):
        u = (v * iv[None, :]).astype(dt)
        x32 = (rows_times(u.astype(F32), W) + c[None, :]).astype(F32)
        return x32, x32.astype(F64)

    with np.errstate(invalid="ignore", over="ignore"):
        v = x.astype(dt)
        d = v.astype(F64) - b64[None, :]
        x32, xl = logits(v)
        logw = -((d * d) * (0.5 * np.exp(-z64))[None, :]).sum(1) + softplus(xl).sum(1)          # -F(x)
        for k in range(K, 0, -1):
            # T_k: h at beta_k from the current state, then the visible state from h
            if dt is F32:
                p = (F32(1.0) / (F32(1.0) + np.exp(-(betas[k] * x32)).astype(F32))).astype(F32)
            else:
                p = 1.0 / (1.0 + np.exp(-(bt[k] * xl)))
            uu = np.asarray(draws.uniform((R, H)), F32)
            gap = np.abs(p.astype(F64) - uu.astype(F64))
            margin = min(margin, float(np.nanmin(gap)) if np.isfinite(gap).any() else np.inf)
            h = (p > uu.astype(p.dtype)).astype(F32)
            if record is not None:
                record.append(h)
            m = (rows_times(h, W.T) + b[None, :]).astype(F32)
            n = np.asarray(draws.normal((R, V)), F32).astype(dt)
            v = (((dt(1.0) - dt(betas[k])) * bAt[None, :] + dt(betas[k]) * m.astype(dt)) + sd[None, :] * n).astype(dt)
            x32, xl = logits(v)
            tv = (coef[None, :] * (v.astype(F64) - mid[None, :])).sum(1)
            logw -= (bt[k] - bt[k - 1]) * tv + (softplus(bt[k] * xl) - softplus(bt[k - 1] * xl)).sum(1)
    logw[~np.isfinite(x).all(1)] = np.nan
    return logw, v, margin


def exact_log_p(W, b, c, z, v):
    """log p(v) = log sum_h exp(-E(v, h)) - log Z per row, float64 throughout, H <= 16: the joint over all 2^H hidden states,
    log N(v; b + W h, e^z) + log p(h) with p(h) from the marginal weights of gauss_ais_oracle.exact_log_z."""
    W, b, c, z, v = (np.asarray(t, F64) for t in (W, b, c, z, v))
    H = W.shape[1]
    assert H <= 16
    hs = np.array(list(itertools.product((0.0, 1.0), repeat=H)), F64)
    a = hs @ W.T                                                                                  # [n, V]
    t = hs @ c + ((b[None, :] * a + 0.5 * a * a) * np.exp(-z)[None, :]).sum(1)                    # log of h's unnormalised mass / sqrt-term
    log_ph = t - (t.max() + np.log(np.exp(t - t.max()).sum()))
    d = v[:, None, :] - (b[None, None, :] + a[None, :, :])
    ln = -(d * d * np.exp(-z) / 2.0 + z / 2.0).sum(2) - 0.5 * v.shape[1] * np.log(2.0 * np.pi)
    g = ln + log_ph[None, :]
    mx = g.max(1, keepdims=True)
    return (mx + np.log(np.exp(g - mx).sum(1, keepdims=True)))[:, 0]
