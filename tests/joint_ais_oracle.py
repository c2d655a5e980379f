"""Numpy twins of imdbn_rbm_ais_groups and imdbn_rbm_label_loglik (include/imdbn_engine.h), of the sample values of an
iMDBN, and the exact quantities of small models by enumeration.

TEST INFRASTRUCTURE ONLY.  ``ais_groups_logw`` restates the estimator in float64 with the fp32 logits widened, as
ais_oracle.ais_logw does; the visible transition uses the oracle's own arithmetic for a softmax group (oracle.rbm_oracle
``_softmax_rows`` in fp32 on the group's fp32 logits, clip to [1e-8, 1], ``PhiloxStream.categorical``).  Two margins come back: the
smallest |p - u| over the Bernoulli decisions of the columns OUTSIDE the groups (the draws of group columns decide nothing), and the
smallest categorical-CDF margin (oracle.draws.CATEGORICAL_MARGIN), so a test can insist that no decision of a case sits within
rounding distance of its draw before it asks the device for the same decisions.
"""
from __future__ import annotations

import numpy as np
import torch

import oracle.rbm_oracle as O
from oracle.draws import CATEGORICAL_MARGIN
from ais_oracle import exact_log_z, logmeanexp, sigmoid, softplus, weight_stats  # noqa: F401
from bound_oracle import BoundOracleEngine, _log_p_down, _log_q_up, _lse, _states, bound_step
from oracle_engine import _Src, _np

F32, F64 = np.float32, np.float64


def _free_mask(V, groups):
    m = np.ones(V, bool)
    for s, e in groups:
        m[s:e] = False
    return m


def log_z_base(V, H, b_A, groups):
    """H log 2 + sum_{i outside groups} softplus(b_A,i) + sum_g logsumexp(b_A[g]); no b_A = zeros."""
    bA = np.zeros(V, F64) if b_A is None else np.asarray(b_A, F32).astype(F64)
    out = H * np.log(2.0) + float(softplus(bA[_free_mask(V, groups)]).sum())
    for s, e in groups:
        out += float(_lse(bA[s:e], 0))
    return out


def ais_groups_logw(W, b, c, b_A, groups, betas, M, draws):
    """-> (logw [M] float64, v_K [M, V] float32, smallest Bernoulli margin outside the groups, smallest categorical margin)."""
    W, b, c = np.asarray(W, F32), np.asarray(b, F32), np.asarray(c, F32)
    V, H = W.shape
    groups = [(int(s), int(e)) for s, e in groups]
    free = _free_mask(V, groups)
    bA = np.zeros(V, F32) if b_A is None else np.asarray(b_A, F32)
    betas = np.asarray(betas, F32)
    K = betas.size - 1
    assert K >= 1 and betas[0] == 0 and betas[K] == 1 and (np.diff(betas) > 0).all()
    bt = betas.astype(F64)
    margin = np.inf
    CATEGORICAL_MARGIN["min"] = float("inf")

    def decide(p, u, cols=None):
        nonlocal margin
        d = np.abs(p - u.astype(F64))
        d = d if cols is None else d[:, cols]
        if d.size:
            margin = min(margin, float(d.min()))
        return (p > u).astype(F32)

    def sample_visible(p64, logits32):
        """Bernoulli over all columns, then one category per group from softmax(logits32[group]) (oracle.rbm_oracle.sample_visible)."""
        v = decide(p64, draws.uniform((M, V)), free)
        for s, e in groups:
            probs = np.clip(O._softmax_rows(logits32[:, s:e]), F32(1e-8), F32(1.0)).astype(F32)
            idx = np.asarray(draws.categorical(probs))
            v[:, s:e] = 0.0
            v[np.arange(M), s + idx] = 1.0
        return v

    v = sample_visible(np.broadcast_to(sigmoid(bA), (M, V)), np.broadcast_to(bA, (M, V)))
    logw = np.zeros(M, F64)
    db = b.astype(F64) - bA.astype(F64)
    for k in range(1, K + 1):
        x = (v @ W + c).astype(F32).astype(F64)
        logw += (bt[k] - bt[k - 1]) * (v.astype(F64) @ db) + (softplus(bt[k] * x) - softplus(bt[k - 1] * x)).sum(1)
        if k < K:
            h = decide(sigmoid(bt[k] * x), draws.uniform((M, H)))
            hw = (h @ W.T).astype(F32)
            p = sigmoid(bt[k] * (hw.astype(F64) + b.astype(F64)) + (1.0 - bt[k]) * bA.astype(F64))
            # the group's logits as the down propagation forms them: fp32, effective bias b + ((1 - beta) / beta) b_A, divided by T = 1 / beta
            eff = b if b_A is None else (b + F32((F32(1.0) - betas[k]) / betas[k]) * bA).astype(F32)
            logits = ((hw + eff) / F32(F32(1.0) / betas[k])).astype(F32)
            v = sample_visible(p, logits)
    return logw, v, margin, CATEGORICAL_MARGIN["min"]


def exact_log_z_groups(W, b, c, groups):
    """log Z by enumerating the 2^H hidden states (H <= 16): sum_h exp(c.h) prod_{i outside groups}(1 + e^{a_i}) prod_g sum_{k in g} e^{a_k}."""
    W, b, c = np.asarray(W, F64), np.asarray(b, F64), np.asarray(c, F64)
    V, H = W.shape
    assert H <= 16
    hs = ((np.arange(1 << H)[:, None] >> np.arange(H)[None, :]) & 1).astype(F64)
    a = hs @ W.T + b
    t = hs @ c + softplus(a[:, _free_mask(V, groups)]).sum(1)
    for s, e in groups:
        t = t + _lse(a[:, s:e], 1)
    return float(_lse(t, 0))


def visible_states(V, groups):
    """Every state of a visible layer with one-hot groups: [n, V] float64 (V small)."""
    free = np.nonzero(_free_mask(V, groups))[0]
    out = np.zeros((1 << free.size, V), F64)
    out[:, free] = ((np.arange(1 << free.size)[:, None] >> np.arange(free.size)[None, :]) & 1)
    for s, e in groups:
        rep = []
        for k in range(s, e):
            o = out.copy()
            o[:, k] = 1.0
            rep.append(o)
        out = np.concatenate(rep, 0)
    return out


def neg_free_energy(W, b, c, v):
    """-F(v) in float64 throughout."""
    W, b, c, v = np.asarray(W, F64), np.asarray(b, F64), np.asarray(c, F64), np.asarray(v, F64)
    return v @ b + softplus(v @ W + c).sum(1)


# ---- imdbn_rbm_label_loglik ---------------------------------------------------------------------------------------------------
def label_loglik(W, b, c, z, Dz, K, gt):
    """-> (joint [N], marg [N]) float64: base = c + z W[:Dz] in fp32, widened; everything else in double."""
    W, b, c, z = np.asarray(W, F32), np.asarray(b, F32), np.asarray(c, F32), np.asarray(z, F32)
    base = (z @ W[:Dz] + c).astype(F32).astype(F64)
    zb = z.astype(F64) @ b[:Dz].astype(F64)
    a = np.stack([zb + F64(b[Dz + k]) + softplus(base + W[Dz + k].astype(F64)).sum(1) for k in range(K)], 1)        # [N, K]
    gt = np.asarray(gt).astype(np.int64)
    ok = (gt >= 0) & (gt < K)
    joint = np.where(ok, a[np.arange(a.shape[0]), np.where(ok, gt, 0)], np.nan)
    return joint, _lse(a, 1)


def imdbn_values(layers, joint, K, img, gt, S, mode, draws, log_z=0.0):
    """-> (w_joint [B, S], w_image [B, S], smallest margin, z [B S, Dz]): one bound_step per image layer (ALL directed), then
    label_loglik; row b's samples are the rows b S .. b S + S - 1 of the replicated batch."""
    cur = np.repeat(np.asarray(img, F32), int(S), axis=0)
    g = np.repeat(np.asarray(gt), int(S), axis=0)
    B = np.asarray(img).shape[0]
    acc, margin = 0.0, np.inf
    for W, b, c in layers:
        a, cur, m = bound_step(W, b, c, cur, mode, draws)
        acc = acc + a
        margin = min(margin, m)
    Wj, bj, cj = joint
    j, mg = label_loglik(Wj, bj, cj, cur, Wj.shape[0] - K, K, g)
    return (acc + j - log_z).reshape(B, S), (acc + mg - log_z).reshape(B, S), margin, cur


# ---- enumeration of a small iMDBN: image layers all directed, the joint RBM over (z, y) on top -----------------------------------
def joint_top_values(joint, K):
    """(log p(z, y) [2^Dz, K], log p(z) [2^Dz]) under the joint RBM, over every binary z."""
    Wj, bj, cj = joint
    Dz = Wj.shape[0] - K
    zs = _states(Dz)
    lz = exact_log_z_groups(Wj, bj, cj, [(Dz, Dz + K)])
    a = np.stack([neg_free_energy(Wj, bj, cj, np.concatenate([zs, np.tile(np.eye(K)[k], (zs.shape[0], 1))], 1)) for k in range(K)], 1)
    return a - lz, _lse(a, 1) - lz


def exact_log_p(layers, v, top):
    """log sum over every directed layer's hidden states of prod p(h_{l-1} | h_l) exp(top[z]), per row of v."""
    st = [np.asarray(v, F64)] + [_states(W.shape[1]) for W, _, _ in layers]
    g = np.asarray(top, F64)
    for l in range(len(layers) - 1, -1, -1):
        W, b, _ = layers[l]
        g = _lse(_log_p_down(W, b, st[l], st[l + 1]) + g[None, :], 1)
    return g


def exact_bound(layers, v, top):
    """sum_l E_q[log p(h_{l-1} | h_l) + H(q(h_l | h_{l-1}))] + E_q[top[z]], the expectation under q taken exactly, per row of v."""
    st = [np.asarray(v, F64)] + [_states(W.shape[1]) for W, _, _ in layers]
    B = st[0].shape[0]
    out = np.zeros(B, F64)
    dist = np.eye(B, dtype=F64)
    for l, (W, b, c) in enumerate(layers):
        lq, ent = _log_q_up(W, c, st[l], st[l + 1])
        jt = dist[:, :, None] * np.exp(lq)[None, :, :]
        out += (jt * _log_p_down(W, b, st[l], st[l + 1])[None, :, :]).sum((1, 2)) + dist @ ent
        dist = jt.sum(1)
    return out + dist @ np.asarray(top, F64)


class JointOracleEngine(BoundOracleEngine):
    """The CPU test double with ``ais_groups`` and ``label_loglik``: what the HipEngine methods return, from the twins."""

    def ais_groups(self, rbm, betas, n_chains, rng, base_vis_bias=None, return_state=False):
        s = _Src(rng)
        n0 = len(s.p.log)
        bA = None if base_vis_bias is None else _np(base_vis_bias)
        b = betas.tolist() if hasattr(betas, "tolist") else list(betas)
        groups = [(int(x), int(y)) for x, y in (getattr(rbm, "softmax_groups", None) or [])]
        logw, v, self.last_margin, self.last_cat_margin = ais_groups_logw(
            _np(rbm.W.data), _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), bA, groups, np.asarray(b, F32), int(n_chains), s)
        self.last_log = [(k, int(shape[1]) if len(shape) > 1 else None) for k, shape in s.p.log[n0:]]
        s.done()
        lw = torch.from_numpy(logw)
        return (lw, self._t(v)) if return_state else lw

    def label_loglik(self, rbm, z, K, gt):
        W = _np(rbm.W.data)
        j, m = label_loglik(W, _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), _np(z), W.shape[0] - int(K), int(K), gt.cpu().numpy())
        return torch.from_numpy(j), torch.from_numpy(m)
