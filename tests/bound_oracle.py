"""Numpy twins of imdbn_rbm_bound_step and imdbn_rbm_label_loglik (include/imdbn_engine.h), of the sample values
of a whole stack and of an iMDBN, the exact likelihood and variational bound of a small DBN and a small iMDBN by enumeration, and the
engine's test double for every likelihood call (the annealing twins are tests/anneal_oracle.py).

TEST INFRASTRUCTURE ONLY.  ``bound_step`` restates one directed layer in float64: the logits x = c + v W and a = b + h W^T are formed
in fp32 (as the engine's propagations form them) and widened; softplus, sigmoid and every sum run in double.  Every Bernoulli
decision 1[p > u] records its margin |p - u|; the smallest one is returned, so a test can insist that no decision of the case sits
within rounding distance of its draw before it asks the device for the same decisions.

A stack is a list of ``(W [V_l, H_l], b [V_l], c [H_l])``, bottom first; its generative model is the top RBM with the directed
layers p(h_{l-1} | h_l) = Bernoulli(sigmoid(b_l + h_l W_l^T)) below it.  The enumerations use the parameters in float64 throughout.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import anneal_oracle as A
from anneal_oracle import _lse, _states, exact_log_z, neg_free_energy, sigmoid, softplus
from oracle_engine import OracleEngine, _Src, _np

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
def _log_p_down(W, b, lower, upper):
    """log p(lower_r | upper_s) under the directed layer (W, b): [n_lower, n_upper]."""
    a = upper @ np.asarray(W, F64).T + np.asarray(b, F64)                 # [n_upper, V]
    return lower @ a.T - softplus(a).sum(1)[None, :]


def _log_q_up(W, c, lower, upper):
    """(log q(upper_s | lower_r) [n_lower, n_upper], entropy of q(. | lower_r) [n_lower])."""
    x = lower @ np.asarray(W, F64) + np.asarray(c, F64)                   # [n_lower, H]
    return x @ upper.T - softplus(x).sum(1)[:, None], (softplus(x) - x * sigmoid(x)).sum(1)


def exact_dbn_log_p(layers, v):
    """log p_DBN(v) per row: the sum over all hidden states of every directed layer; the top Z from anneal_oracle.exact_log_z."""
    st = [np.asarray(v, F64)] + [_states(W.shape[1]) for W, _, _ in layers[:-1]]
    g = neg_free_energy(*layers[-1], st[-1]) - exact_log_z(*layers[-1])
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
    return out + dist @ neg_free_energy(*layers[-1], st[-1]) - exact_log_z(*layers[-1])


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
    lz = exact_log_z(Wj, bj, cj, [(Dz, Dz + K)])
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


# ---- the test double --------------------------------------------------------------------------------------------------------------
class LikelihoodOracleEngine(OracleEngine):
    """The CPU test double with the likelihood calls: what the HipEngine methods return, from the twins.  ``last_margin`` and
    ``last_cat_margin`` are the twin's; ``last_log`` = the draws the call consumed, as (kind, width or None)."""

    def _twin(self, rng, call):
        """call(draw source) -> (float64 values as a tensor, state as a tensor): the draws logged, the Philox counter advanced."""
        s = _Src(rng)
        n0 = len(s.p.log)
        vals, state, self.last_margin, *cat = call(s)
        self.last_cat_margin = cat[0] if cat else float("inf")
        self.last_log = [(k, int(shape[1]) if len(shape) > 1 else None) for k, shape in s.p.log[n0:]]
        s.done()
        return torch.from_numpy(vals), self._t(state)

    def _anneal(self, rbm, betas, rng, base_vis_bias, return_state, call):
        """call(W, b, c, b_A, betas, draw source) is one of the annealing twins."""
        bA = None if base_vis_bias is None else _np(base_vis_bias)
        b = np.asarray(betas.tolist() if hasattr(betas, "tolist") else list(betas), F32)
        lw, v = self._twin(rng, lambda s: call(_np(rbm.W.data), _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), bA, b, s))
        return (lw, v) if return_state else lw

    @staticmethod
    def _groups(rbm):
        return [(int(x), int(y)) for x, y in (getattr(rbm, "softmax_groups", None) or [])]

    def _forward(self, groups, rbm, betas, n_chains, rng, base_vis_bias=None, return_state=False):
        return self._anneal(rbm, betas, rng, base_vis_bias, return_state,
                            lambda W, b, c, bA, bt, s: A.ais_logw(W, b, c, bA, bt, int(n_chains), s, groups))

    def ais(self, rbm, *args, **kw):
        return self._forward((), rbm, *args, **kw)

    def ais_groups(self, rbm, *args, **kw):
        return self._forward(self._groups(rbm), rbm, *args, **kw)

    def reverse_ais(self, rbm, v_rows, betas, rng, base_vis_bias=None, return_state=False):
        self.calls.append(("reverse_ais", int(v_rows.shape[0])))
        return self._anneal(rbm, betas, rng, base_vis_bias, return_state,
                            lambda W, b, c, bA, bt, s: A.reverse_ais_logw(W, b, c, bA, self._groups(rbm), bt, _np(v_rows), s))

    def rows_logmeanexp(self, logw, n_chains):
        lme, ess = A.rows_logmeanexp(logw.numpy(), n_chains)
        return torch.from_numpy(lme), torch.from_numpy(ess)

    def label_loglik(self, rbm, z, K, gt):
        W = _np(rbm.W.data)
        j, m = label_loglik(W, _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), _np(z), W.shape[0] - int(K), int(K), gt.cpu().numpy())
        return torch.from_numpy(j), torch.from_numpy(m)

    def bound_step(self, rbm, v, rng, acc=None, mode="entropy"):
        a, h = self._twin(rng, lambda s: bound_step(_np(rbm.W.data), _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), _np(v), mode, s))
        if acc is None:
            acc = a
        else:
            acc += a
        return acc, h


def host_rbm(c, groups=None):
    """The RBM of a case dict, or of (W, b, c) arrays, on the CPU, with copies of the arrays; `groups`: None = the case's."""
    from imdbn.models import RBM
    if not isinstance(c, dict):
        c = dict(zip("Wbc", c))
    r = RBM(*c["W"].shape, 0.1, 0.0, 0.5, softmax_groups=(c.get("groups") if groups is None else groups) or None).to("cpu")
    r.W.data = torch.from_numpy(c["W"].copy())
    r.vis_bias.data = torch.from_numpy(c["b"].copy())
    r.hid_bias.data = torch.from_numpy(c["c"].copy())
    return r


@pytest.fixture()
def double():
    """The test double installed as the engine for one test (a test module imports the fixture by name)."""
    from imdbn import engine as E
    eng = LikelihoodOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)
