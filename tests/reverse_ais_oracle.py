"""Numpy twin of imdbn_rbm_reverse_ais and imdbn_rows_logmeanexp (include/imdbn_engine.h), and the annealing model of a
small RBM by enumeration.

TEST INFRASTRUCTURE ONLY.  ``reverse_ais_logw`` restates the estimator in float64 with the logits formed in fp32 and widened, as
ais_oracle.ais_logw does; the transitions are those of joint_ais_oracle.ais_groups_logw (a softmax group: the oracle's fp32 softmax on
the group's fp32 logits, clip to [1e-8, 1], ``categorical`` of the draw source).  The fp32 products are summed one row at a time in
column order, so a row's logits do not depend on how many rows ride along (the chunk-invariance tests compare bits).  Two margins
come back: the smallest |p - u| over the Bernoulli decisions of the columns outside the groups, and the smallest categorical-CDF
margin (oracle.draws.CATEGORICAL_MARGIN).

``annealing_model`` enumerates p_ann for V <= 10 without groups: p_A times the K transition matrices over all 2^V states, parameters
in float64 throughout.
"""
from __future__ import annotations

import numpy as np
import torch

import oracle.rbm_oracle as O
from oracle.draws import CATEGORICAL_MARGIN
from ais_oracle import logmeanexp, sigmoid, softplus, weight_stats  # noqa: F401
from joint_ais_oracle import JointOracleEngine, _free_mask, log_z_base  # noqa: F401
from oracle_engine import _Src, _np

F32, F64 = np.float32, np.float64


def _rows_times(a, Wm):
    """a [R, n] @ Wm [n, m] in fp32, every row summed over n in ascending order on its own."""
    return (np.asarray(a, F32)[:, :, None] * np.asarray(Wm, F32)[None, :, :]).sum(1, dtype=F32)


def valid_rows(x, groups):
    """True per row: every element exactly 0 or 1 and exactly one 1 in every group."""
    x = np.asarray(x, F32)
    ok = ((x == 0) | (x == 1)).all(1)
    for s, e in groups:
        ok &= (x[:, s:e] == 1).sum(1) == 1
    return ok


def reverse_ais_logw(W, b, c, b_A, groups, betas, x, draws):
    """-> (logw [R] float64, u_1 [R, V] float32, smallest Bernoulli margin outside the groups, smallest categorical margin)."""
    W, b, c = np.asarray(W, F32), np.asarray(b, F32), np.asarray(c, F32)
    V, H = W.shape
    groups = [(int(s), int(e)) for s, e in (groups or [])]
    free = _free_mask(V, groups)
    bA = np.zeros(V, F32) if b_A is None else np.asarray(b_A, F32)
    betas = np.asarray(betas, F32)
    K = betas.size - 1
    assert K >= 1 and betas[0] == 0 and betas[K] == 1 and (np.diff(betas) > 0).all()
    bt = betas.astype(F64)
    x = np.asarray(x, F32)
    R = x.shape[0]
    margin = np.inf
    CATEGORICAL_MARGIN["min"] = float("inf")

    def decide(p, u, cols=None):
        nonlocal margin
        d = np.abs(p - u.astype(F64))
        d = d if cols is None else d[:, cols]
        if d.size:
            margin = min(margin, float(d.min()))
        return (p > u).astype(F32)

    def logits(v):
        return (_rows_times(v, W) + c).astype(F32).astype(F64)

    def transition(v, k):
        """T_k: h at beta_k from v, then the visible state at beta_k from h."""
        h = decide(sigmoid(bt[k] * logits(v)), draws.uniform((R, H)))
        hw = _rows_times(h, W.T)
        p = sigmoid(bt[k] * (hw.astype(F64) + b.astype(F64)) + (1.0 - bt[k]) * bA.astype(F64))
        out = decide(p, draws.uniform((R, V)), free)
        if groups:
            # the group's logits as the down propagation forms them: fp32, effective bias b + ((1 - beta) / beta) b_A, divided by T = 1 / beta
            eff = b if b_A is None else (b + F32((F32(1.0) - betas[k]) / betas[k]) * bA).astype(F32)
            lg = ((hw + eff) / F32(F32(1.0) / betas[k])).astype(F32)
            for s, e in groups:
                probs = np.clip(O._softmax_rows(lg[:, s:e]), F32(1e-8), F32(1.0)).astype(F32)
                idx = np.asarray(draws.categorical(probs))
                out[:, s:e] = 0.0
                out[np.arange(R), s + idx] = 1.0
        return out

    u = (x == 1).astype(F32)
    logw = u.astype(F64) @ b.astype(F64) + softplus(logits(u)).sum(1)          # -F(x)
    db = b.astype(F64) - bA.astype(F64)
    for k in range(K, 0, -1):
        u = transition(u, k)
        xl = logits(u)
        logw -= (bt[k] - bt[k - 1]) * (u.astype(F64) @ db) + (softplus(bt[k] * xl) - softplus(bt[k - 1] * xl)).sum(1)
    logw[~valid_rows(x, groups)] = np.nan
    return logw, u, margin, CATEGORICAL_MARGIN["min"]


def rows_logmeanexp(logw, M):
    """-> (log mean exp [N], ess [N]) of the rows of logw viewed [N, M]; a NaN stays in its row."""
    x = np.asarray(logw, F64).reshape(-1, int(M))
    with np.errstate(invalid="ignore"):
        m = x.max(1, keepdims=True)
        w = np.exp(x - m)
        return (m[:, 0] + np.log(w.mean(1))), w.sum(1) ** 2 / (w * w).sum(1)


def row_stats(logw, M):
    """-> (log mean exp [N], se [N], ess [N]): se = std(w) / (mean(w) sqrt(M)) on the weights shifted by the row's maximum."""
    x = np.asarray(logw, F64).reshape(-1, int(M))
    w = np.exp(x - x.max(1, keepdims=True))
    lme, ess = rows_logmeanexp(x, M)
    se = w.std(1, ddof=1) / (w.mean(1) * np.sqrt(M)) if M > 1 else np.zeros(x.shape[0])
    return lme, se, ess


# ---- the annealing model by enumeration (V <= 10, H <= 12, no groups) ---------------------------------------------------------
def _states(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(F64)


def _bernoulli_table(logit, states):
    """[n_cond, n_states]: prod_i sigmoid(logit)^s_i (1 - sigmoid(logit))^(1 - s_i), from log-probabilities."""
    return np.exp(logit @ states.T - softplus(logit).sum(1)[:, None])


def annealing_model(W, b, c, b_A, betas):
    """log p_ann over all 2^V states (state i = the bits of i, column 0 lowest), and the states [2^V, V]."""
    W, b, c = np.asarray(W, F64), np.asarray(b, F64), np.asarray(c, F64)
    V, H = W.shape
    assert V <= 10 and H <= 12
    bA = np.zeros(V, F64) if b_A is None else np.asarray(b_A, F64)
    bt = np.asarray(betas, F32).astype(F64)
    vs, hs = _states(V), _states(H)
    p = _bernoulli_table(bA[None, :], vs)[0]                                   # v_1 ~ p_A
    for k in range(1, bt.size):
        ph = _bernoulli_table(bt[k] * (vs @ W + c), hs)                        # [2^V, 2^H]
        pv = _bernoulli_table(bt[k] * (hs @ W.T + b) + (1.0 - bt[k]) * bA, vs)   # [2^H, 2^V]
        p = (p @ ph) @ pv
    assert abs(p.sum() - 1.0) < 1e-10
    return np.log(p), vs.astype(F32)


class ReverseAisOracleEngine(JointOracleEngine):
    """The CPU test double with ``reverse_ais`` and ``rows_logmeanexp``: what the HipEngine methods return, from the twins."""

    def reverse_ais(self, rbm, v_rows, betas, rng, base_vis_bias=None, return_state=False):
        s = _Src(rng)
        n0 = len(s.p.log)
        bA = None if base_vis_bias is None else _np(base_vis_bias)
        b = betas.tolist() if hasattr(betas, "tolist") else list(betas)
        groups = [(int(x), int(y)) for x, y in (getattr(rbm, "softmax_groups", None) or [])]
        logw, u, self.last_margin, self.last_cat_margin = reverse_ais_logw(
            _np(rbm.W.data), _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), bA, groups, np.asarray(b, F32), _np(v_rows), s)
        self.last_log = [(k, int(shape[1]) if len(shape) > 1 else None) for k, shape in s.p.log[n0:]]
        self.calls.append(("reverse_ais", int(v_rows.shape[0])))
        s.done()
        lw = torch.from_numpy(logw)
        return (lw, self._t(u)) if return_state else lw

    def rows_logmeanexp(self, logw, n_chains):
        lme, ess = rows_logmeanexp(logw.numpy(), n_chains)
        return torch.from_numpy(lme), torch.from_numpy(ess)
