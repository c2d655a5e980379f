"""numpy twin of backprop fine-tuning through a Gaussian bottom layer (imdbn_rbm_gauss_backprop_step, HipEngine.gauss_autoencoder_step;
DESIGN section 35).

Gaussian layers are ``gauss_oracle.GState`` objects (W, b, c, z and their momenta), Bernoulli layers anything with the arrays of
``backprop_oracle.KEYS``.  Every function takes ``dt``: float64 is the reference the tests compare with -- all arithmetic in float64 on
the direct formulas, the update rounded once into the arrays' own dtype, as ``backprop_oracle`` does it -- and float32 restates the
kernels' formulas in their own precision (the statistics S of both pairs in one array, r_i = sum_j W_ij S_ij, the share t_i of the
down pair taken out of it), which measures what fp32 alone costs (tests/gauss_backprop_cases.fp32_errors).  No draws.

With z the log-variance of the layer, n rows, u = v e^{-z}, m = b + x_h W^T, e_0 = (v - m) e^{-z}:
    J    = (1/n) sum_b sum_i (v_bi - m_bi)^2 e^{-z_i} / 2 + z_i / 2
    down pair:  gW = e_0^T x_h / n,  gb = colsum(e_0) / n,  gzeta_i = e^{-z_i} sum_b (v_bi - m_bi)^2 / (2 n) - 1/2,
                err_h = (e_0 W) x_h (1 - x_h)
    up pair:    gW = u^T e_h / n,    gc = colsum(e_h) / n,  gz_i = -(1/n) sum_j W_ij (u^T e_h)_ij

TEST INFRASTRUCTURE ONLY."""
from types import SimpleNamespace

import numpy as np

import backprop_oracle as Bp

F32, F64 = np.float32, np.float64


def _sigmoid(a):
    return (1 / (1 + np.exp(-a))).astype(a.dtype)


def _put(dst, val):
    dst[...] = np.asarray(val).astype(dst.dtype)


def gauss_backprop_step(st, v, up=None, down=None, lr=0.0, mom=0.0, lr_z=0.0, z_lo=-np.inf, z_hi=np.inf, apply=True, dt=F64):
    """imdbn_rbm_gauss_backprop_step on the ``GState`` `st`, in place with ``apply``.  ``up`` = e_h, ``down`` = x_h.  Returns
    dict(m, e0, err_h, mag_h, nll, mse) in `dt` (None without the down pair): mag_h = (|e_0| |W|) x_h (1 - x_h), the magnitude sum the
    error bound of err_h is stated in."""
    W, b, z = np.asarray(st.W, dt), np.asarray(st.b, dt), np.asarray(st.z, dt)
    v = np.asarray(v, dt)
    n = dt(v.shape[0])
    iv = np.exp(-z)
    out = dict(m=None, e0=None, err_h=None, mag_h=None, nll=None, mse=None)
    S = np.zeros_like(W)
    g_z = np.zeros_like(z)
    t = None
    if down is not None:
        xh = np.asarray(down, dt)
        m = (xh @ W.T + b).astype(dt)
        dl = v - m
        e0 = dl * iv
        d = xh * (1 - xh)
        q = (dl * dl).sum(0)
        out.update(m=m, e0=e0, err_h=(e0 @ W) * d, mag_h=(np.abs(e0) @ np.abs(W)) * d,
                   nll=float(F64(dt(0.5)) * F64((q * iv).sum()) / F64(n) + 0.5 * F64(z.astype(F64).sum())),
                   mse=float(F64(q.sum()) / (F64(n) * v.shape[1])))
        S += e0.T @ xh
        g_z += (iv * q) / (dt(2) * n) - dt(0.5)
        t = (e0 * (m - b)).sum(0)
    if up is not None:
        eh = np.asarray(up, dt)
        u = v * iv
        Su = u.T @ eh
        S += Su
        if dt is F64:
            g_z += -(W * Su).sum(1) / n
        else:                                  # the kernels' route: r over both pairs' statistics, the down pair's share taken out
            r = (W * S).sum(1)
            g_z += -((r - t) if t is not None else r) / n
    if not apply:
        return out
    lr_, mom_ = dt(lr), dt(mom)
    _put(st.W_m, np.asarray(st.W_m, dt) * mom_ + lr_ * (S / n - dt(st.weight_decay) * W))
    _put(st.W, W + np.asarray(st.W_m, dt))
    if up is not None:
        _put(st.hb_m, np.asarray(st.hb_m, dt) * mom_ + lr_ * eh.sum(0) / n)
        _put(st.c, np.asarray(st.c, dt) + np.asarray(st.hb_m, dt))
    if down is not None:
        _put(st.vb_m, np.asarray(st.vb_m, dt) * mom_ + lr_ * e0.sum(0) / n)
        _put(st.b, b + np.asarray(st.vb_m, dt))
    if lr_z != 0:
        _put(st.z_m, np.asarray(st.z_m, dt) * mom_ + dt(lr_z) * g_z)
        _put(st.z, np.minimum(np.maximum(z + np.asarray(st.z_m, dt), dt(z_lo)), dt(z_hi)))
    return out


def backprop_step(st, up=None, down=None, lr=0.0, mom=0.0, apply=True, dt=F64):
    """``backprop_oracle.backprop_step`` (the float64 reference itself), or its restatement in float32."""
    if dt is F64:
        return Bp.backprop_step(st, up, down, lr, mom, apply)
    W = np.asarray(st.W, dt)
    out = dict(err_v=None, err_h=None)
    g = np.zeros_like(W)
    if up is not None:
        xv, eh = np.asarray(up[0], dt), np.asarray(up[1], dt)
        out["err_v"] = (eh @ W.T) * (xv * (1 - xv))
        g += xv.T @ eh
        n = dt(xv.shape[0])
    if down is not None:
        xh, ev = np.asarray(down[0], dt), np.asarray(down[1], dt)
        out["err_h"] = (ev @ W) * (xh * (1 - xh))
        g += ev.T @ xh
        n = dt(xh.shape[0])
    if not apply:
        return out
    lr_, mom_ = dt(lr), dt(mom)
    _put(st.W_m, np.asarray(st.W_m, dt) * mom_ + lr_ * (g / n - dt(st.weight_decay) * W))
    _put(st.W, W + np.asarray(st.W_m, dt))
    if up is not None:
        _put(st.hb_m, np.asarray(st.hb_m, dt) * mom_ + lr_ * eh.sum(0) / n)
        _put(st.hid_bias, np.asarray(st.hid_bias, dt) + np.asarray(st.hb_m, dt))
    if down is not None:
        _put(st.vb_m, np.asarray(st.vb_m, dt) * mom_ + lr_ * ev.sum(0) / n)
        _put(st.vis_bias, np.asarray(st.vis_bias, dt) + np.asarray(st.vb_m, dt))
    return out


def unrolled(rec, gen, data, dt=F64):
    """The forward pass of the unrolled network: (a_0 .. a_L, d_0 .. d_L); rec[0] (and gen[0], when L > 1) are ``GState``s, d_0 the
    linear reconstruction."""
    L = len(rec)
    g0 = rec[0]
    x = np.asarray(data, dt)
    a = [x, _sigmoid(((x * np.exp(-np.asarray(g0.z, dt))) @ np.asarray(g0.W, dt) + np.asarray(g0.c, dt)).astype(dt))]
    for st in rec[1:]:
        a.append(_sigmoid((a[-1] @ np.asarray(st.W, dt) + np.asarray(st.hid_bias, dt)).astype(dt)))
    down = list(gen) + [rec[-1]]
    dec = [None] * L + [a[L]]
    for l in range(L, 1, -1):
        dec[l - 1] = _sigmoid((dec[l] @ np.asarray(down[l - 1].W, dt).T + np.asarray(down[l - 1].vis_bias, dt)).astype(dt))
    out = down[0]
    dec[0] = (dec[1] @ np.asarray(out.W, dt).T + np.asarray(out.b, dt)).astype(dt)
    return a, dec


def nll(rec, gen, data):
    """J of the header on the stack's parameters, float64."""
    x = np.asarray(data, F64)
    _, dec = unrolled(rec, gen, x)
    z = np.asarray((gen[0] if len(rec) > 1 else rec[0]).z, F64)
    return float((((x - dec[0]) ** 2 * np.exp(-z) / 2).sum(1) + z.sum() / 2).mean())


def autoencoder_step(rec, gen, data, scalars, hyper, dt=F64):
    """HipEngine.gauss_autoencoder_step on the states ``rec`` (L) and ``gen`` (L - 1), updated in place.  ``scalars``: (lr, mom) per
    layer; ``hyper``: (lr_sigma_mult, z_lo, z_hi) of the Gaussian layer and of its twin.  Returns dict(recon, code, nll, mse)."""
    L = len(rec)
    x = np.asarray(data, dt)
    a, dec = unrolled(rec, gen, x, dt)
    mult, z_lo, z_hi = hyper
    lr, mom = scalars[0]
    kz = dict(lr_z=mult * lr, z_lo=z_lo, z_hi=z_hi)
    enc = rec[0]
    if L == 1:
        o = gauss_backprop_step(enc, x, down=a[1], apply=False, dt=dt)
        gauss_backprop_step(enc, x, up=o["err_h"], down=a[1], lr=lr, mom=mom, dt=dt, **kz)
        return dict(recon=dec[0], code=a[1], nll=o["nll"], mse=o["mse"])
    o = gauss_backprop_step(gen[0], x, down=dec[1], lr=lr, mom=mom, dt=dt, **kz)
    e = o["err_h"]
    for l in range(2, L):
        e = backprop_step(gen[l - 1], down=(dec[l], e), lr=scalars[l - 1][0], mom=scalars[l - 1][1], dt=dt)["err_h"]
    top = rec[-1]
    f = backprop_step(top, down=(a[L], e), apply=False, dt=dt)["err_h"]
    f = backprop_step(top, up=(a[L - 1], f), down=(a[L], e), lr=scalars[L - 1][0], mom=scalars[L - 1][1], dt=dt)["err_v"]
    for l in range(L - 1, 1, -1):
        f = backprop_step(rec[l - 1], up=(a[l - 1], f), lr=scalars[l - 1][0], mom=scalars[l - 1][1], dt=dt)["err_v"]
    gauss_backprop_step(enc, x, up=f, lr=lr, mom=mom, dt=dt, **kz)
    return dict(recon=dec[0], code=a[L], nll=o["nll"], mse=o["mse"])


def bern_state(W, hid_bias, vis_bias, weight_decay=0.0, dt=F64, W_m=None, hb_m=None, vb_m=None):
    z = lambda x, like: np.zeros_like(np.asarray(like, dt)) if x is None else np.array(x, dt)
    return SimpleNamespace(W=np.array(W, dt), hid_bias=np.array(hid_bias, dt), vis_bias=np.array(vis_bias, dt), W_m=z(W_m, W),
                           hb_m=z(hb_m, hid_bias), vb_m=z(vb_m, vis_bias), weight_decay=float(weight_decay))
