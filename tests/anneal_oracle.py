"""Numpy twin of the annealing path (imdbn_rbm_ais, imdbn_rbm_ais_groups, imdbn_rbm_reverse_ais and imdbn_rows_logmeanexp of
include/imdbn_engine.h), and the exact quantities of small RBMs by enumeration.

TEST INFRASTRUCTURE ONLY.  ``ais_logw`` and ``reverse_ais_logw`` walk one transition (``_Anneal``) up or down the temperature ladder
in float64: the logits x = c + v W are formed in fp32 (as the engine's up propagation forms them) and widened; both sums of the weight
increment, the softplus and the sigmoid run in double.  A softmax group is sampled with the oracle's own arithmetic
(oracle.rbm_oracle ``_softmax_rows`` in fp32 on the group's fp32 logits, clip to [1e-8, 1], ``categorical`` of the draw source).  Two
margins come back: the smallest |p - u| over the Bernoulli decisions of the columns OUTSIDE the groups (the draws of group columns
decide nothing), and the smallest categorical-CDF margin (oracle.draws.CATEGORICAL_MARGIN, inf without groups), so a test can insist
that no decision of a case sits within rounding distance of its draw before it asks the device for the same decisions.

``annealing_model`` enumerates p_ann for V <= 10 without groups: p_A times the K transition matrices over all 2^V states, parameters
in float64 throughout.
"""
from __future__ import annotations

import numpy as np

import oracle.rbm_oracle as O
from oracle.draws import CATEGORICAL_MARGIN

F32, F64 = np.float32, np.float64


def softplus(t):
    t = np.asarray(t, F64)
    return np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))


def sigmoid(t):
    t = np.asarray(t, F64)
    return 1.0 / (1.0 + np.exp(-t))


def _lse(t, axis):
    m = t.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(t - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def _states(n, most=12):
    """Every state of n binary units: [2^n, n] float64, state i = the bits of i, column 0 lowest."""
    assert n <= most
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(F64)


def _free_mask(V, groups):
    m = np.ones(V, bool)
    for s, e in groups:
        m[s:e] = False
    return m


def valid_rows(x, groups):
    """True per row: every element exactly 0 or 1 and exactly one 1 in every group."""
    x = np.asarray(x, F32)
    ok = ((x == 0) | (x == 1)).all(1)
    for s, e in groups:
        ok &= (x[:, s:e] == 1).sum(1) == 1
    return ok


# ---- statistics of log weights ------------------------------------------------------------------------------------------------
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


# ---- the transition both directions share -------------------------------------------------------------------------------------
def _rows_times(a, Wm):
    """a [R, n] @ Wm [n, m] in fp32, every row summed over n in ascending order on its own."""
    return (np.asarray(a, F32)[:, :, None] * np.asarray(Wm, F32)[None, :, :]).sum(1, dtype=F32)


class _Anneal:
    """The intermediate models of one ladder over n rows.  ``times(a, Wm)`` is the fp32 product of the logits."""

    def __init__(self, W, b, c, b_A, groups, betas, n, draws, times):
        self.W, self.b, self.c = np.asarray(W, F32), np.asarray(b, F32), np.asarray(c, F32)
        self.V, self.H = self.W.shape
        self.groups = [(int(s), int(e)) for s, e in (groups or ())]
        self.free = _free_mask(self.V, self.groups)
        self.has_bA = b_A is not None
        self.bA = np.zeros(self.V, F32) if b_A is None else np.asarray(b_A, F32)
        self.betas = np.asarray(betas, F32)
        self.K = self.betas.size - 1
        assert self.K >= 1 and self.betas[0] == 0 and self.betas[self.K] == 1 and (np.diff(self.betas) > 0).all()
        self.bt = self.betas.astype(F64)
        self.db = self.b.astype(F64) - self.bA.astype(F64)
        self.n, self.draws, self.times = int(n), draws, times
        self.margin = np.inf
        CATEGORICAL_MARGIN["min"] = float("inf")

    def decide(self, p, u, cols=None):
        d = np.abs(p - u.astype(F64))
        d = d if cols is None else d[:, cols]
        if d.size:
            self.margin = min(self.margin, float(d.min()))
        return (p > u).astype(F32)

    def logits(self, v):
        return (self.times(v, self.W) + self.c).astype(F32).astype(F64)

    def delta_k(self, v, x, k):
        """log p*_k(v) - log p*_{k-1}(v), x the logits of v."""
        bt = self.bt
        return (bt[k] - bt[k - 1]) * (v.astype(F64) @ self.db) + (softplus(bt[k] * x) - softplus(bt[k - 1] * x)).sum(1)

    def sample_h(self, x, k):
        return self.decide(sigmoid(self.bt[k] * x), self.draws.uniform((self.n, self.H)))

    def sample_visible(self, p64, logits32):
        """Bernoulli over all columns, then one category per group from softmax(logits32[group]) (oracle.rbm_oracle.sample_visible)."""
        v = self.decide(p64, self.draws.uniform((self.n, self.V)), self.free)
        for s, e in self.groups:
            probs = np.clip(O._softmax_rows(logits32[:, s:e]), F32(1e-8), F32(1.0)).astype(F32)
            idx = np.asarray(self.draws.categorical(probs))
            v[:, s:e] = 0.0
            v[np.arange(self.n), s + idx] = 1.0
        return v

    def sample_base(self):
        """v ~ p_A."""
        shape = (self.n, self.V)
        return self.sample_visible(np.broadcast_to(sigmoid(self.bA), shape), np.broadcast_to(self.bA, shape))

    def sample_v(self, h, k):
        """v | h at beta_k."""
        b, bA, bt, betas = self.b, self.bA, self.bt, self.betas
        hw = self.times(h, self.W.T).astype(F32)
        p = sigmoid(bt[k] * (hw.astype(F64) + b.astype(F64)) + (1.0 - bt[k]) * bA.astype(F64))
        # the group's logits as the down propagation forms them: fp32, effective bias b + ((1 - beta) / beta) b_A, divided by T = 1 / beta
        eff = (b + F32((F32(1.0) - betas[k]) / betas[k]) * bA).astype(F32) if self.has_bA else b
        return self.sample_visible(p, ((hw + eff) / F32(F32(1.0) / betas[k])).astype(F32))


# Two fp32 products: the forward pins come from numpy's matmul; reverse needs row-ordered sums (chunk invariance is compared bit for bit).
def ais_logw(W, b, c, b_A, betas, M, draws, groups=()):
    """-> (logw [M] float64, v_K [M, V] float32, smallest Bernoulli margin outside the groups, smallest categorical margin)."""
    a = _Anneal(W, b, c, b_A, groups, betas, M, draws, np.matmul)
    v = a.sample_base()
    logw = np.zeros(a.n, F64)
    for k in range(1, a.K + 1):
        x = a.logits(v)
        logw += a.delta_k(v, x, k)
        if k < a.K:
            v = a.sample_v(a.sample_h(x, k), k)
    return logw, v, a.margin, CATEGORICAL_MARGIN["min"]


def reverse_ais_logw(W, b, c, b_A, groups, betas, x, draws):
    """-> (logw [R] float64, u_1 [R, V] float32, smallest Bernoulli margin outside the groups, smallest categorical margin)."""
    x = np.asarray(x, F32)
    a = _Anneal(W, b, c, b_A, groups, betas, x.shape[0], draws, _rows_times)
    u = (x == 1).astype(F32)
    xl = a.logits(u)
    logw = u.astype(F64) @ a.b.astype(F64) + softplus(xl).sum(1)          # -F(x)
    for k in range(a.K, 0, -1):
        u = a.sample_v(a.sample_h(xl, k), k)                                # T_k: h at beta_k from u, then the visible state from h
        xl = a.logits(u)
        logw -= a.delta_k(u, xl, k)
    logw[~valid_rows(x, a.groups)] = np.nan
    return logw, u, a.margin, CATEGORICAL_MARGIN["min"]


# ---- partition functions --------------------------------------------------------------------------------------------------------
def log_z_base(V, H, b_A, groups=()):
    """H log 2 + sum_{i outside groups} softplus(b_A,i) + sum_g logsumexp(b_A[g]); no b_A = zeros."""
    bA = np.zeros(V, F64) if b_A is None else np.asarray(b_A, F32).astype(F64)
    out = H * np.log(2.0) + float(softplus(bA[_free_mask(V, groups)]).sum())
    for s, e in groups:
        out += float(_lse(bA[s:e], 0))
    return out


def exact_log_z(W, b, c, groups=()):
    """log Z by enumerating the 2^H hidden states (H <= 16): sum_h exp(c.h) prod_{i outside groups}(1 + e^{a_i}) prod_g sum_{k in g} e^{a_k}."""
    W, b, c = np.asarray(W, F64), np.asarray(b, F64), np.asarray(c, F64)
    V, H = W.shape
    hs = _states(H, 16)
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


# ---- the annealing model by enumeration (V <= 10, H <= 12, no groups) ---------------------------------------------------------
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
