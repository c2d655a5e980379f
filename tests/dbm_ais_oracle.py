"""Float64 reference and fp32 numpy twin of the DBM density arithmetic (imdbn_dbm_rowsum_layer, imdbn_dbm_ais, HipEngine.dbm_bound,
kernels_dbm_ais.hpp), on top of tests/dbm_oracle.py, and the error bounds of the device's results, derived here
and not tuned.

A layer call takes the operands of ``dbm_oracle.pre`` with ``s_lo = s_hi = 1``.  The twin computes ``pre`` in the dtype ``dt`` it is
given (fp32: the device's pre-activation up to ``dbm_oracle.pre_bound``) and, as the device does, every row sum in float64 FROM that
``pre``.

Bounds.  ``dpre = dbm_oracle.pre_bound`` is how far the device's fp32 ``pre`` may be from the float64 one.
  WEIGH   |d softplus| <= 1, so a unit's ``sp(e(beta)) - sp(e(beta_prev))`` moves by at most ``(beta + beta_prev) dpre``; the double
          arithmetic (two softplus, their difference, the butterfly and the tile sums) adds ``2^-50`` of the terms' magnitudes.
  SAMPLE  the fp32 effective input ``fl(fl(beta pre) + fl(fl(1 - beta) base))`` is four roundings of values no larger than
          ``|beta pre| + |(1 - beta) base|``: ``de <= beta dpre + 4 u (|beta pre| + |(1 - beta) base|)``; a sigmoid has slope <= 1/4 and
          its fp32 evaluation adds EPS_P (dbm_oracle): ``dp <= de / 4 + EPS_P``.  A draw whose ``|p - U|`` exceeds that has the same
          bit on the device and in float64; the bias dot of equal states is a double sum of fp32 values: ``2^-50 sum |b_n| s_n``.
  BOUND   ``|mu| dpre`` per unit, ``2^-50`` of the magnitudes of ``mu pre`` and of the entropy, and of the ``b_0 v`` products.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import dbm_oracle as Dt

F32, F64 = np.float32, np.float64
U = Dt.U
EPS_D = 2.0 ** -50


def softplus(t):
    t = np.asarray(t, F64)
    return np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))


def _sides(Ws, states, l):
    """The operands of layer l of a stack: (W_lo, x_lo, W_hi, x_hi)."""
    L = len(Ws)
    lo = (Ws[l - 1], states[l - 1]) if l > 0 else (None, None)
    hi = (Ws[l], states[l + 1]) if l < L else (None, None)
    return lo[0], lo[1], hi[0], hi[1]


def pre(W_lo, x_lo, W_hi, x_hi, bias, dt):
    return Dt.pre(W_lo, x_lo, 1.0, W_hi, x_hi, 1.0, bias, dt)


def dpre(W_lo, x_lo, W_hi, x_hi, bias):
    return Dt.pre_bound(W_lo, x_lo, 1.0, W_hi, x_hi, 1.0, bias)


# ---- the three epilogues ------------------------------------------------------------------------------------------------------------
def _e64(beta, p, base):
    e = F64(F32(beta)) * p.astype(F64)
    return e if base is None else e + (1.0 - F64(F32(beta))) * np.asarray(base, F64)


def weigh(W_lo, x_lo, W_hi, x_hi, bias, beta, beta_prev, base, dt):
    """Row sums of sp(e(beta)) - sp(e(beta_prev)), float64 [B]."""
    p = pre(W_lo, x_lo, W_hi, x_hi, bias, dt)
    return (softplus(_e64(beta, p, base)) - softplus(_e64(beta_prev, p, base))).sum(1)


def weigh_bound(W_lo, x_lo, W_hi, x_hi, bias, beta, beta_prev, base):
    p = pre(W_lo, x_lo, W_hi, x_hi, bias, F64)
    mag = np.abs(softplus(_e64(beta, p, base))) + np.abs(softplus(_e64(beta_prev, p, base)))
    return ((float(beta) + float(beta_prev)) * dpre(W_lo, x_lo, W_hi, x_hi, bias) + EPS_D * mag).sum(1)


def sample_p(W_lo, x_lo, W_hi, x_hi, bias, beta, base, dt):
    """p of the draw at beta in ``dt``; fp32: the device's roundings, one per operation."""
    p = pre(W_lo, x_lo, W_hi, x_hi, bias, dt)
    if dt is F64:
        return Dt.sigmoid(_e64(beta, p, base))
    e = F32(beta) * p
    if base is not None:
        e = e + (F32(1) - F32(beta)) * np.asarray(base, F32)
    return Dt.sigmoid(e.astype(F32))


def sample_p_bound(W_lo, x_lo, W_hi, x_hi, bias, beta, base):
    p = pre(W_lo, x_lo, W_hi, x_hi, bias, F64)
    mag = np.abs(float(beta) * p) + (0.0 if base is None else np.abs((1.0 - float(beta)) * np.asarray(base, F64)))
    return (float(beta) * dpre(W_lo, x_lo, W_hi, x_hi, bias) + 4 * U * mag) / 4 + Dt.EPS_P


def bias_dot(bias, s):
    return np.asarray(s, F64) @ np.asarray(bias, F64)


def bias_dot_bound(bias, s):
    return EPS_D * (np.abs(np.asarray(s, F64)) @ np.abs(np.asarray(bias, F64)))


def bound_layer(W_lo, x_lo, bias, mu, dt, bias_lo=None):
    """Row sums of mu pre + h(mu) (and of bias_lo x_lo), float64 [B]."""
    p = pre(W_lo, x_lo, None, None, bias, dt).astype(F64)
    m = np.asarray(mu, F64)
    out = np.zeros(m.shape[0]) if bias_lo is None else bias_dot(bias_lo, x_lo)
    return out + (m * p + Dt.entropy(m)).sum(1)


def bound_layer_bound(W_lo, x_lo, bias, mu, bias_lo=None):
    p = pre(W_lo, x_lo, None, None, bias, F64)
    m = np.asarray(mu, F64)
    out = (np.abs(m) * dpre(W_lo, x_lo, None, None, bias) + EPS_D * (np.abs(m * p) + Dt.entropy(m))).sum(1)
    return out if bias_lo is None else out + bias_dot_bound(bias_lo, x_lo)


# ---- the variational figure ---------------------------------------------------------------------------------------------------------
def bound_rows(Ws, bs, v, mus, dt=F64):
    """HipEngine.dbm_bound: the bound without - log Z, layer by layer."""
    s = [np.asarray(v, dt)] + [np.asarray(m, dt) for m in mus]
    out = np.zeros(s[0].shape[0])
    for l in range(1, len(s)):
        out = out + bound_layer(Ws[l - 1], s[l - 1], bs[l], s[l], dt, bias_lo=bs[0] if l == 1 else None)
    return out


def bound_rows_bound(Ws, bs, v, mus):
    s = [np.asarray(v, F64)] + [np.asarray(m, F64) for m in mus]
    return sum(bound_layer_bound(Ws[l - 1], s[l - 1], bs[l], s[l], bias_lo=bs[0] if l == 1 else None) for l in range(1, len(s)))


# ---- annealed importance sampling -----------------------------------------------------------------------------------------------------
def log_z_base(sizes, base=None):
    return sum(sizes[1:]) * np.log(2.0) + (sizes[0] * np.log(2.0) if base is None else float(softplus(base).sum()))


def ais(Ws, bs, betas, M, src, base=None, dt=F64, margins=None, bound=None):
    """imdbn_dbm_ais: ``(logw float64 [M], states)`` -- ``states`` the L + 1 layer states at the end (the odd ones are the chain).  Draws
    from ``src.uniform((M, N_l))`` in the order of ``rng.sched_dbm_ais``.  ``margins``: a list that receives, per draw, min(|p - U| - bound
    of p) in float64 terms; ``bound``: a one-element list that receives how far the device's logw may be from this run's when every
    state agrees (float64 [M])."""
    L = len(Ws)
    sizes = [np.asarray(b).size for b in bs]
    b = np.asarray(betas, F32)
    K = b.size - 1
    s = [np.zeros((M, n), dt) for n in sizes]
    logw, lb = np.zeros(M), np.zeros(M)

    def draw(l, p, pb):
        u = np.asarray(src.uniform(p.shape), dt)
        if margins is not None:
            margins.append(float((np.abs(p.astype(F64) - u.astype(F64)) - pb).min()))
        s[l] = (p > u).astype(dt)

    def odd_bias(d):
        nonlocal logw, lb
        for l in range(1, L + 1, 2):
            logw = logw + d * bias_dot(bs[l], s[l])
            lb = lb + abs(d) * bias_dot_bound(bs[l], s[l])

    for l in range(1, L + 1, 2):
        draw(l, np.full((M, sizes[l]), 0.5, dt), 0.0)
    odd_bias(F64(b[1]) - F64(b[0]))
    for k in range(1, K + 1):
        for l in range(0, L + 1, 2):
            ops = _sides(Ws, s, l)
            a = base if l == 0 else None
            logw = logw + weigh(*ops, bs[l], b[k], b[k - 1], a, dt)
            lb = lb + weigh_bound(*ops, bs[l], b[k], b[k - 1], a)
            if k < K:
                draw(l, sample_p(*ops, bs[l], b[k], a, dt), sample_p_bound(*ops, bs[l], b[k], a))
        if k < K:
            for l in range(1, L + 1, 2):
                ops = _sides(Ws, s, l)
                draw(l, sample_p(*ops, bs[l], b[k], None, dt), sample_p_bound(*ops, bs[l], b[k], None))
            odd_bias(F64(b[k + 1]) - F64(b[k]))
    if bound is not None:
        bound.append(lb + EPS_D * np.abs(logw))
    return logw, s


def weight_stats(logw, lzb):
    """(log Z estimate, its standard error): imdbn.utils.likelihood._weight_stats_device."""
    logw = np.asarray(logw, F64)
    w = np.exp(logw - logw.max())
    se = w.std(ddof=1) / (w.mean() * np.sqrt(w.size)) if w.size > 1 else 0.0
    return float(lzb + logw.max() + np.log(w.mean())), float(se)
