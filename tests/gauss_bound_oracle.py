"""Numpy twin of imdbn_rbm_gauss_bound_step (include/imdbn_engine.h): the bottom bracket of the DBN lower bound under a
Gaussian visible layer, the sample values of a whole stack above it, and the exact log-density and variational bound of a small
such stack by enumeration of every hidden layer.

TEST INFRASTRUCTURE ONLY.  ``gauss_bound_step(..., dt)`` forms one bracket in the dtype ``dt``:

float64 (the reference)   u = v e^{-z} and the sigmoid of the h draw run in float64.  The two matrix products are what the engine's
                          propagations produce: fp32 numbers -- the fp32 operand (u, or the 0/1 h) times the fp32 weights, every
                          row summed on its own (in float64, rounded once to fp32, so the value does not depend on a summation
                          order; gauss_ais_oracle.rows_times) -- which are then WIDENED.  E and log N are summed in double.
float32 (the restatement) the same with every fp32 quantity of the device in fp32: e^{-z}, u and the sigmoid of the h draw.  E (from
                          the fp32 logits) and log N (from the fp32 v, m, z, the subtraction done on the widened values) are formed
                          in double, as on the device.  What fp32 alone costs is measured as restatement against reference
                          (tests/gauss_bound_cases.fp32_error) and the device is gated at 8 x that.

A stack is ``(z, [(W_1, b_1, c_1), (W_2, b_2, c_2), ...])``: layer 1 Gaussian-visible with log-variances z, the others Bernoulli
(tests/bound_oracle.py twins them).  Draw schedule of one bracket (imdbn.engine.rng.sched_bound): ("u", H).
"""
from __future__ import annotations

import numpy as np

import anneal_oracle as A
import bound_oracle as B
from gauss_ais_oracle import rows_times, softplus

F32, F64 = np.float32, np.float64
MODES = ("entropy", "logq")
LOG_2PI = float(np.log(2.0 * np.pi))


def log_normal(v, m, z):
    """log N(v; m, e^z) per row, every element in double from the widened fp32 values, in the kernel's expression."""
    v, m, z = np.asarray(v, F32).astype(F64), np.asarray(m, F32).astype(F64), np.asarray(z, F32).astype(F64)
    d = v - m
    return (-((d * d) * np.exp(-z)[None, :] / 2.0 + z[None, :] / 2.0)).sum(1) + (-(v.shape[1] / 2.0) * LOG_2PI)


def gauss_bound_step(W, b, c, z, v, mode, draws, dt=F64):
    """-> (acc [M] float64, h [M, H] float32, smallest |sigmoid(x) - U| over the Bernoulli decisions, E [M], log N [M])."""
    assert mode in MODES
    W, b, c, z, v = (np.asarray(x, F32) for x in (W, b, c, z, v))
    M, H = v.shape[0], W.shape[1]
    iv = np.exp(-z.astype(dt)).astype(dt)
    u = (v.astype(dt) * iv[None, :]).astype(dt)
    x32 = (rows_times(u.astype(F32), W) + c[None, :]).astype(F32)
    x = x32.astype(F64)
    if dt is F32:
        p = (F32(1.0) / (F32(1.0) + np.exp(-x32).astype(F32))).astype(F32)
    else:
        p = 1.0 / (1.0 + np.exp(-x))
    uu = np.asarray(draws.uniform((M, H)), F32)
    margin = float(np.abs(p.astype(F64) - uu.astype(F64)).min())
    h = (p > uu.astype(p.dtype)).astype(F32)
    sp = softplus(x)
    e = (sp - x / (1.0 + np.exp(-x))).sum(1) if mode == "entropy" else (sp - h.astype(F64) * x).sum(1)
    m = (rows_times(h, W.T) + b[None, :]).astype(F32)
    ln = log_normal(v, m, z)
    return (e + ln), h, margin, e, ln


def gauss_dbn_values(z, layers, v, S, mode, draws, log_z_top=0.0, dt=F64):
    """-> (w [B, S] float64, smallest margin, magnitude of the top free energy's terms [B, S], the h of the bottom bracket): row b's
    samples are the S consecutive rows b S .. b S + S - 1 of the replicated batch; one draw tensor per directed layer.  Two layers
    and more (a stack of one draws nothing and is -F - log Z of the Gaussian RBM: tests/gauss_oracle.py)."""
    assert len(layers) >= 2
    cur = np.repeat(np.asarray(v, F32), int(S), axis=0)
    Bn = np.asarray(v).shape[0]
    acc, h1, margin, _, _ = gauss_bound_step(*layers[0], z, cur, mode, draws, dt)
    cur = h1
    for W, b, c in layers[1:-1]:
        a, cur, m = B.bound_step(W, b, c, cur, mode, draws)
        acc = acc + a
        margin = min(margin, m)
    F, mag = B.free_energy(*layers[-1], cur)
    return (acc + (-F - log_z_top)).reshape(Bn, S), margin, mag.reshape(Bn, S), h1


# ---- enumeration (H_l <= 12 per layer), parameters in float64 throughout --------------------------------------------------------------
def _bottom_tables(z, bottom, v):
    """(states of h_1 [n, H], log N(v_r; b + h_s W^T, e^z) [rows, n], log q(h_s | v_r) [rows, n], entropy of q(. | v_r) [rows])."""
    W, b, c = (np.asarray(x, F64) for x in bottom)
    z, v = np.asarray(z, F64), np.asarray(v, F64)
    hs = A._states(W.shape[1])
    m = hs @ W.T + b[None, :]                                                          # [n, V]
    d = v[:, None, :] - m[None, :, :]
    ln = -(d * d * np.exp(-z) / 2.0 + z / 2.0).sum(2) - 0.5 * v.shape[1] * LOG_2PI
    x = (v * np.exp(-z)[None, :]) @ W + c[None, :]
    return hs, ln, x @ hs.T - softplus(x).sum(1)[:, None], (softplus(x) - x * A.sigmoid(x)).sum(1)


def exact_log_p(z, layers, v):
    """log p_DBN(v) = log sum_{h_1} p(h_1) N(v; b_1 + h_1 W_1^T, e^z) per row; p(h_1) is the marginal of the Bernoulli stack above
    (bound_oracle.exact_dbn_log_p over every state of h_1)."""
    hs, ln, _, _ = _bottom_tables(z, layers[0], v)
    return A._lse(ln + B.exact_dbn_log_p(layers[1:], hs)[None, :], 1)


def exact_bound(z, layers, v):
    """The variational lower bound per row with the expectation under q taken exactly:
    E_q[log N(v; b_1 + h_1 W_1^T, e^z)] + H(q(. | v)) + E_q[bound of the Bernoulli stack above at h_1]."""
    hs, ln, lq, ent = _bottom_tables(z, layers[0], v)
    q = np.exp(lq)
    return (q * ln).sum(1) + ent + q @ B.exact_dbn_bound(layers[1:], hs)
