"""Numpy twin of imdbn_rbm_gauss_ais (include/imdbn_engine.h): annealed importance sampling over Gaussian visibles, and
the exact log Z of a small Gaussian-visible RBM by enumerating its 2^H hidden states.

TEST INFRASTRUCTURE ONLY.  ``gauss_ais_logw(..., dt)`` walks the ladder in the dtype ``dt``:

float64 (the reference)   the state v, u = v e^{-z}, the sigmoid and the visible expression run in float64.  The two matrix products
                          are what the engine's propagations produce: fp32 numbers -- the fp32 operand (u, or the 0/1 h) times the
                          fp32 weights, every row summed on its own (in float64, rounded once to fp32, so the value does not depend
                          on a summation order) -- which are then WIDENED.  Both sums of the weight increment and the softplus
                          run in double, each row on its own.
float32 (the restatement) the same walk with every fp32 quantity of the device in fp32: the state, u, e^{-z}, e^{z/2}, the sigmoid
                          of the h draw and the visible expression  v = ((1 - beta) b_A + beta m) + e^{z/2} n  in the engine's
                          order.  The sums of the weight increment stay in double, as on the device.  A continuous state carries
                          its rounding into the next logits, which a binary state does not: what fp32 alone costs is measured as
                          restatement against reference (tests/gauss_ais_cases.fp32_errors) and the device is gated at 8 x that.

Draw schedule (imdbn.engine.rng.sched_gauss_ais): ("n", V), then (K - 1) x [("u", H), ("n", V)].
"""
from __future__ import annotations

import itertools

import numpy as np

F32, F64 = np.float32, np.float64


def softplus(t):
    t = np.asarray(t, F64)
    return np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))


def rows_times(a, Wm):
    """The fp32 product a [R, n] @ Wm [n, m] of fp32 operands: each row on its own, summed in float64 and rounded once."""
    return (np.asarray(a, F32).astype(F64) @ np.asarray(Wm, F32).astype(F64)).astype(F32)


def log_z_base(V, H, z):
    """log Z_A = H log 2 + (V / 2) log 2 pi + sum z / 2, whatever b_A."""
    return H * np.log(2.0) + 0.5 * V * np.log(2.0 * np.pi) + 0.5 * float(np.asarray(z, F32).astype(F64).sum())


def exact_log_z(W, b, c, z):
    """log Z = log sum_h e^{c.h} prod_i sqrt(2 pi sigma_i^2) exp((b_i a_i + a_i^2 / 2) / sigma_i^2), a = W h; float64, H <= 16."""
    W, b, c, z = (np.asarray(x, F64) for x in (W, b, c, z))
    H = W.shape[1]
    assert H <= 16
    hs = np.array(list(itertools.product((0.0, 1.0), repeat=H)), F64)
    a = hs @ W.T
    t = hs @ c + ((b[None, :] * a + 0.5 * a * a) * np.exp(-z)[None, :]).sum(1)
    return float(0.5 * (np.log(2 * np.pi) + z).sum() + t.max() + np.log(np.exp(t - t.max()).sum()))


def gauss_ais_logw(W, b, c, z, b_A, betas, M, draws, dt=F64, record=None):
    """-> (logw [M] float64, v_K [M, V] in dt, the smallest Bernoulli margin |sigmoid(beta x) - U|).  ``b_A`` None: b.  ``record``
    (a list) receives every h sample."""
    W, b, c, z = (np.asarray(x, F32) for x in (W, b, c, z))
    V, H = W.shape
    bA = b if b_A is None else np.asarray(b_A, F32)
    betas = np.asarray(betas, F32)
    K = betas.size - 1
    assert K >= 1 and betas[0] == 0 and betas[K] == 1 and (np.diff(betas) > 0).all()
    bt = betas.astype(F64)
    M = int(M)
    # the weight term's constants, in double on both sides
    b64, bA64, z64 = b.astype(F64), bA.astype(F64), z.astype(F64)
    coef = (b64 - bA64) * np.exp(-z64)
    mid = 0.5 * (b64 + bA64)
    # the state's constants in dt
    zt = z.astype(dt)
    sd, iv = np.exp(dt(0.5) * zt).astype(dt), np.exp(-zt).astype(dt)
    bAt = bA.astype(dt)
    margin = np.inf

    def visible(beta, m):
        n = np.asarray(draws.normal((M, V)), F32).astype(dt)
        t = (dt(1.0) - dt(beta)) * bAt[None, :]
        if m is not None:
            t = t + dt(beta) * m.astype(dt)
        else:
            t = t + dt(0.0)
        return (t + sd[None, :] * n).astype(dt)

    v = visible(F32(0.0), None)
    logw = np.zeros(M, F64)
    for k in range(1, K + 1):
        u = (v * iv[None, :]).astype(dt)
        x32 = (rows_times(u.astype(F32), W) + c[None, :]).astype(F32)
        x = x32.astype(F64)
        tv = (coef[None, :] * (v.astype(F64) - mid[None, :])).sum(1)
        logw += (bt[k] - bt[k - 1]) * tv + (softplus(bt[k] * x) - softplus(bt[k - 1] * x)).sum(1)
        if k == K:
            break
        if dt is F32:
            p = (F32(1.0) / (F32(1.0) + np.exp(-(betas[k] * x32)).astype(F32))).astype(F32)
        else:
            p = 1.0 / (1.0 + np.exp(-(bt[k] * x)))
        uu = np.asarray(draws.uniform((M, H)), F32)
        margin = min(margin, float(np.abs(p.astype(F64) - uu.astype(F64)).min()))
        h = (p > uu.astype(p.dtype)).astype(F32)
        if record is not None:
            record.append(h)
        m = (rows_times(h, W.T) + b[None, :]).astype(F32)
        v = visible(betas[k], m)
    return logw, v, margin
