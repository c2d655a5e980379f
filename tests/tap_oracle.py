"""Float64 reference and fp32 numpy twin of the extended mean-field (TAP) arithmetic (imdbn_rbm_tap_iterate / imdbn_rbm_tap_step,
kernels_tap.hpp), plus the error bound of the device's magnetisations, derived here and not tuned.

Everything works in the dtype ``dt`` it is given.  ``W2 = fl32(W W)`` in both: the float64 reference squares the fp32 weights in fp32
and widens, so reference and twin state the same number.  Order 1 drops every W2 term.

Bound (GPU test 1).  With u = 2^-24 and K the reduction length, the device's pre-activation of one unit differs from the float64 one
of the SAME inputs by at most ``(K + 8) u (|bias| + |m||W| + |m_out - 1/2| (c W2)) + u |m_out - 1/2| (c W2)`` (fp32 sums of K
products in any order, the bias and correction operations, and the rounding of W2 itself, which the reference shares only up to u).
Inputs that already differ by dm_in / dm_out move it by ``dm_in (|W| + |m_out - 1/2| |1 - 2 m_in| W2) + dm_out (c W2)`` more.  A
sigmoid has slope <= 1/4, its fp32 evaluation and the damping arithmetic add 2^-23 per half-step:
``dm_new = damp dm_old + (1 - damp) dx / 4 + 2^-23``.  ``iterate_bounded`` carries dm through the iterations.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import oracle.rbm_oracle as O

F32, F64 = np.float32, np.float64
U = 2.0 ** -24


def w2_of(W, dt):
    W = np.asarray(W, F32)
    return (W * W).astype(F32).astype(dt)


def sigmoid(x):
    with np.errstate(over="ignore"):
        return (x.dtype.type(1) / (x.dtype.type(1) + np.exp(-x))).astype(x.dtype)


def var(m):
    return (m - (m * m).astype(m.dtype)).astype(m.dtype)


def half(Wk, W2k, bias, m_in, m_out, damp, order, dt):
    """One half-step.  Wk / W2k [K, N] (W for the hidden form, W^T for the visible one).  Returns (new m_out, sigmoid, x)."""
    half_ = dt(0.5)
    x = (bias + m_in @ Wk).astype(dt)
    if order == 2:
        x = (x - (m_out - half_) * (var(m_in) @ W2k)).astype(dt)
    s = sigmoid(x)
    return (dt(damp) * m_out + (dt(1) - dt(damp)) * s).astype(dt), s, x


def iterate(W, a, c, mv, mh, n_iters, damp=0.5, order=2, dt=F64):
    """(mv, mh, residual [B]) after n_iters iterations; the residual of the last one (zeros for none)."""
    Wd, W2 = np.asarray(W, F32).astype(dt), w2_of(W, dt)
    a, c = np.asarray(a, dt), np.asarray(c, dt)
    mv, mh = np.asarray(mv, dt).copy(), np.asarray(mh, dt).copy()
    res = np.zeros(mv.shape[0], dt)
    for _ in range(int(n_iters)):
        mh2, sh, _ = half(Wd, W2, c, mv, mh, damp, order, dt)
        r1 = np.abs(sh - mh).max(1)
        mh = mh2
        mv2, sv, _ = half(Wd.T, W2.T, a, mh, mv, damp, order, dt)
        res = np.maximum(r1, np.abs(sv - mv).max(1))
        mv = mv2
    return mv, mh, res


def _half_bound(Wk, W2k, bias, m_in, m_out, dm_in, dm_out, damp, order):
    K = Wk.shape[0]
    aW = np.abs(Wk)
    corr = var(m_in) @ W2k if order == 2 else 0.0
    lever = np.abs(m_out - 0.5)
    T = np.abs(bias) + np.abs(m_in) @ aW + lever * corr
    dx = (K + 8) * U * T + U * lever * corr + dm_in @ aW
    if order == 2:
        dx = dx + lever * ((dm_in * np.abs(1.0 - 2.0 * m_in)) @ W2k) + dm_out * corr
    return dx


def iterate_bounded(W, a, c, mv, mh, n_iters, damp=0.5, order=2):
    """The float64 iteration with the bound of the module docstring: (mv, mh, res, dmv, dmh, res_bound [B]).  ``res_bound``: how far
    an fp32 evaluation's residual may be from the float64 one (the largest dx / 4 + 2^-23 + dm_old of the last iteration)."""
    Wd, W2 = np.asarray(W, F32).astype(F64), w2_of(W, F64)
    a, c = np.asarray(a, F64), np.asarray(c, F64)
    mv, mh = np.asarray(mv, F64).copy(), np.asarray(mh, F64).copy()
    dmv, dmh = np.zeros_like(mv), np.zeros_like(mh)
    res, rb = np.zeros(mv.shape[0]), np.zeros(mv.shape[0])
    for _ in range(int(n_iters)):
        dx = _half_bound(Wd, W2, c, mv, mh, dmv, dmh, damp, order)
        mh2, sh, _ = half(Wd, W2, c, mv, mh, damp, order, F64)
        r1, b1 = np.abs(sh - mh).max(1), (dx / 4 + 2.0 ** -23 + dmh).max(1)
        dmh = damp * dmh + (1 - damp) * dx / 4 + 2.0 ** -23
        mh = mh2
        dx = _half_bound(Wd.T, W2.T, a, mh, mv, dmh, dmv, damp, order)
        mv2, sv, _ = half(Wd.T, W2.T, a, mh, mv, damp, order, F64)
        res, rb = np.maximum(r1, np.abs(sv - mv).max(1)), np.maximum(b1, (dx / 4 + 2.0 ** -23 + dmv).max(1))
        dmv = damp * dmv + (1 - damp) * dx / 4 + 2.0 ** -23
        mv = mv2
    return mv, mh, res, dmv, dmh, rb


def entropy(m):
    m = np.asarray(m, F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(m > 0, m * np.log(m), 0.0) + np.where(m < 1, (1 - m) * np.log(1 - m), 0.0)
    return t


def gamma(W, a, c, mv, mh, order=2):
    """Gamma per row in float64 of the magnetisations as given (cv / ch and W2 as the contract rounds them when mv is fp32)."""
    Wd, W2 = np.asarray(W, F32).astype(F64), w2_of(W, F64)
    mv, mh = np.asarray(mv, F64), np.asarray(mh, F64)
    g = entropy(mv).sum(1) + entropy(mh).sum(1) - mv @ np.asarray(a, F64) - mh @ np.asarray(c, F64) - ((mv @ Wd) * mh).sum(1)
    if order == 2:
        g = g - 0.5 * (((mv - mv * mv) @ W2) * (mh - mh * mh)).sum(1)
    return g


def gamma_bound(W, a, c, mv, mh, order=2):
    """How far the device's Gamma may be from ``gamma`` of the same magnetisations: the fp32 sums A1 = mv W, A2 = cv W2 (V products
    each) enter as mh A1 and ch A2 / 2, cv and ch carry one fp32 rounding each; the rest is double."""
    Wd, W2 = np.abs(np.asarray(W, F32).astype(F64)), w2_of(W, F64)
    mv, mh = np.asarray(mv, F64), np.asarray(mh, F64)
    V = Wd.shape[0]
    b = (V + 8) * U * ((mv @ Wd) * mh).sum(1)
    if order == 2:
        b = b + 0.5 * (V + 8 + 3) * U * (((mv - mv * mv) @ W2) * (mh - mh * mh)).sum(1)
    return b + 1e-13 * (np.abs(gamma(W, a, c, mv, mh, order)) + 1.0)


def free_energy_fixed_point(W, a, c, mv0, n_iters, damp=0.5, order=2):
    """(-Gamma* per start, residual per start) in float64 from the starts mv0 with mh0 = sigmoid(c + mv0 W)."""
    Wd = np.asarray(W, F32).astype(F64)
    mv0 = np.asarray(mv0, F64)
    mh0 = sigmoid(np.asarray(c, F64) + mv0 @ Wd)
    mv, mh, res = iterate(W, a, c, mv0, mh0, n_iters, damp, order, F64)
    return -gamma(W, a, c, mv, mh, order), res, mv, mh


def log_z_enumerated(W, a, c):
    import exact_oracle as X
    return float(X.reference(np.asarray(W, F64), np.asarray(a, F64), np.asarray(c, F64))["log_z"])


# ---- the update ---------------------------------------------------------------------------------------------------------------------
def state_as(st, dt):
    """A copy of the oracle state `st` with every array in `dt`."""
    s = st.copy()
    for k in ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m"):
        setattr(s, k, np.asarray(getattr(st, k), dt).copy())
    return s


def tap_step(st, data, mv, mh, lr, mom, n_iters, damp=0.5, order=2):
    """imdbn_rbm_tap_step in the dtype of st.W: updates `st` in place; returns (loss, mv, mh) -- the magnetisations after the
    negative phase.  The momentum / decay / sparsity rule is O.apply_cd_update's, operation for operation."""
    dt = st.W.dtype.type
    data = np.asarray(data, dt)
    W0 = st.W.copy()
    pos_h = sigmoid((data @ W0 + st.hid_bias).astype(dt))
    v_rec = sigmoid((pos_h @ W0.T + st.vis_bias).astype(dt))
    loss = dt(((data - v_rec) ** 2).astype(dt).mean(dtype=dt))
    Wf = W0.astype(F32) if dt is F32 else W0          # (the float64 reference squares fp32 weights: they are exactly representable)
    mv, mh, _ = iterate(Wf, st.vis_bias, st.hid_bias, mv, mh, n_iters, damp, order, dt)
    n = dt(data.shape[0])
    stat = (data.T @ pos_h - mv.T @ mh).astype(dt)
    if order == 2:
        stat = (stat - W0 * (var(mv).T @ var(mh)).astype(dt)).astype(dt)
    lr_, mom_ = dt(lr), dt(mom)
    st.W_m *= mom_
    st.W_m += lr_ * (stat / n - dt(st.weight_decay) * st.W)
    st.W += st.W_m
    st.hb_m *= mom_
    st.hb_m += lr_ * (pos_h.sum(0, dtype=dt) - mh.sum(0, dtype=dt)) / n
    if st.sparsity:
        st.hb_m += dt(-lr) * ((pos_h.sum(0, dtype=dt) / n).astype(dt) - dt(st.sparsity_factor))
    st.hid_bias += st.hb_m
    st.vb_m *= mom_
    st.vb_m += lr_ * (data.sum(0, dtype=dt) - mv.sum(0, dtype=dt)) / n
    st.vis_bias += st.vb_m
    return loss, mv, mh


def rel_frobenius(x, ref):
    x, ref = np.asarray(x, F64), np.asarray(ref, F64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))
