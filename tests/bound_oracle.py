"""Numpy twin of imdbn_rbm_bound_step (include/imdbn_engine.h), of the sample values of a whole stack, and the exact
likelihood and variational bound of a small DBN by enumeration.

TEST INFRASTRUCTURE ONLY.  ``bound_step`` restates one directed layer in float64: the logits x = c + v W and a = b + h W^T are formed
in fp32 (as the engine's propagations form them) and widened; softplus, sigmoid and every sum run in double.  Every Bernoulli
decision 1[p > u] records its margin |p - u|; the smallest one is returned, so a test can insist that no decision of the case sits
within rounding distance of its draw before it asks the device for the same decisions.

A stack is a list of ``(W [V_l, H_l], b [V_l], c [H_l])``, bottom first; its generative model is the top RBM with the directed
layers p(h_{l-1} | h_l) = Bernoulli(sigmoid(b_l + h_l W_l^T)) below it.  The enumerations use the parameters in float64 throughout.
"""
from __future__ import annotations

import numpy as np
import torch

from ais_oracle import AisOracleEngine, exact_log_z, sigmoid, softplus
from oracle_engine import _Src, _np

F32, F64 = np.float32, np.float64
MODES = ("entropy", "logq")


def bound_step(W, b, c, v, mode, draws):
    """-> (acc [M] float64, h [M, H] float32, smallest |p - u| over every Bernoulli decision made)."""
    assert mode in MODES
    W, b, c, v = np.asarray(W, F32), np.asarray(b, F32), np.asarray(c, F32), np.asarray(v, F32)
    M, H = v.shape[0], W.shape[1]
    x = (v @ W + c).astype(F32).astype(F64)
    p, u = sigmoid(x), draws.uniform((M, H))
    margin = float(np.abs(p - u.astype(F64)).min())
    h = (p > u).astype(F32)
    e = (softplus(x) - x * p).sum(1) if mode == "entropy" else (softplus(x) - h.astype(F64) * x).sum(1)
    a = (h @ W.T + b).astype(F32).astype(F64)
    return (v.astype(F64) * a - softplus(a)).sum(1) + e, h, margin


def free_energy(W, b, c, v):
    """-> (F [M] float64 from fp32 logits, sum of the magnitudes of its terms: what an fp32 sum of them works at)."""
    W, b, c, v = np.asarray(W, F32), np.asarray(b, F32), np.asarray(c, F32), np.asarray(v, F32)
    x = (v @ W + c).astype(F32).astype(F64)
    vb = v.astype(F64) * b.astype(F64)
    return -vb.sum(1) - softplus(x).sum(1), np.abs(vb).sum(1) + softplus(x).sum(1)


def dbn_values(layers, v, S, mode, draws, log_z_top=0.0):
    """-> (w [B, S] float64, smallest margin, magnitude of the top free energy's terms [B, S]): row b's samples are the S
    consecutive rows b S .. b S + S - 1 of the replicated batch, one draw tensor per directed layer."""
    cur = np.repeat(np.asarray(v, F32), int(S), axis=0)
    B = np.asarray(v).shape[0]
    acc, margin = None, np.inf
    for W, b, c in layers[:-1]:
        a, cur, m = bound_step(W, b, c, cur, mode, draws)
        acc = a if acc is None else acc + a
        margin = min(margin, m)
    F, mag = free_energy(*layers[-1], cur)
    w = -F - log_z_top
    if acc is not None:
        w = acc + w
    return w.reshape(B, S), margin, mag.reshape(B, S)


# ---- enumeration (H_l <= 12 per layer) ----------------------------------------------------------------------------------
def _states(n):
    assert n <= 12
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(F64)


def _lse(t, axis):
    m = t.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(t - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def _log_p_down(W, b, lower, upper):
    """log p(lower_r | upper_s) under the directed layer (W, b): [n_lower, n_upper]."""
    a = upper @ np.asarray(W, F64).T + np.asarray(b, F64)                 # [n_upper, V]
    return lower @ a.T - softplus(a).sum(1)[None, :]


def _log_q_up(W, c, lower, upper):
    """(log q(upper_s | lower_r) [n_lower, n_upper], entropy of q(. | lower_r) [n_lower])."""
    x = lower @ np.asarray(W, F64) + np.asarray(c, F64)                   # [n_lower, H]
    return x @ upper.T - softplus(x).sum(1)[:, None], (softplus(x) - x * sigmoid(x)).sum(1)


def _top_neg_free_energy(W, b, c, s):
    W, b, c = np.asarray(W, F64), np.asarray(b, F64), np.asarray(c, F64)
    return s @ b + softplus(s @ W + c).sum(1)


def exact_dbn_log_p(layers, v):
    """log p_DBN(v) per row: the sum over all hidden states of every directed layer; the top Z from ais_oracle.exact_log_z."""
    st = [np.asarray(v, F64)] + [_states(W.shape[1]) for W, _, _ in layers[:-1]]
    g = _top_neg_free_energy(*layers[-1], st[-1]) - exact_log_z(*layers[-1])
    for l in range(len(layers) - 2, -1, -1):
        W, b, _ = layers[l]
        g = _lse(_log_p_down(W, b, st[l], st[l + 1]) + g[None, :], 1)
    return g


def exact_dbn_bound(layers, v):
    """The variational lower bound per row, the expectation under q taken exactly:
    sum_l E_q[log p(h_{l-1} | h_l) + H(q(h_l | h_{l-1}))] - E_q[F_top(h_{L-1})] - log Z_top."""
    st = [np.asarray(v, F64)] + [_states(W.shape[1]) for W, _, _ in layers[:-1]]
    B = st[0].shape[0]
    out = np.zeros(B, F64)
    dist = np.eye(B, dtype=F64)                                           # dist[row, state of layer l - 1]
    for l, (W, b, c) in enumerate(layers[:-1]):
        lq, ent = _log_q_up(W, c, st[l], st[l + 1])
        joint = dist[:, :, None] * np.exp(lq)[None, :, :]                 # [row, lower, upper]
        out += (joint * _log_p_down(W, b, st[l], st[l + 1])[None, :, :]).sum((1, 2)) + dist @ ent
        dist = joint.sum(1)
    return out + dist @ _top_neg_free_energy(*layers[-1], st[-1]) - exact_log_z(*layers[-1])


class BoundOracleEngine(AisOracleEngine):
    """The CPU test double with ``bound_step``: what HipEngine.bound_step returns, from the twin."""

    def bound_step(self, rbm, v, rng, acc=None, mode="entropy"):
        s = _Src(rng)
        n0 = len(s.p.log)
        a, h, self.last_margin = bound_step(_np(rbm.W.data), _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), _np(v), mode, s)
        self.last_log = [(k, int(shape[1])) for k, shape in s.p.log[n0:]]
        s.done()
        a = torch.from_numpy(a)
        if acc is None:
            acc = a
        else:
            acc += a
        return acc, self._t(h)
