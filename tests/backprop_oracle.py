"""float64 numpy twin of the backprop fine-tuning calls (imdbn_rbm_backprop_step, HipEngine.autoencoder_step).

``backprop_step`` and ``autoencoder_step`` work on ``pcd_oracle.rbm_state`` objects -- or on any object with W / hid_bias / vis_bias /
W_m / hb_m / vb_m / weight_decay arrays, ``f64_state`` makes float64 ones for the finite-difference check -- and do all arithmetic in
float64; the update is applied in place as ``updown_oracle.delta_step`` applies it, rounded once into the arrays' own dtype.  No draws.

TEST INFRASTRUCTURE ONLY."""
from types import SimpleNamespace

import numpy as np

F64 = np.float64
KEYS = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")


def f64_state(st):
    """A float64 copy of a state (parameters, momenta, weight decay)."""
    return SimpleNamespace(weight_decay=float(st.weight_decay), **{k: np.array(getattr(st, k), F64) for k in KEYS})


def _sigmoid(a):
    return 1.0 / (1.0 + np.exp(-np.asarray(a, F64)))


def backprop_step(st, up=None, down=None, lr=0.0, mom=0.0, apply=True):
    """imdbn_rbm_backprop_step.  ``up`` = (x_v, e_h), ``down`` = (x_h, e_v).  Returns dict(err_v, err_h, mag_v, mag_h), float64 or None:
    err_v = (e_h W^T) x_v (1 - x_v), err_h = (e_v W) x_h (1 - x_h) from the parameters on entry, and alongside the magnitude sums
    mag_v = (|e_h| |W|^T) x_v (1 - x_v), mag_h = (|e_v| |W|) x_h (1 - x_h) an error bound of the product is stated in.  With ``apply``
    the update, in place."""
    W = np.asarray(st.W, F64)
    out = dict(err_v=None, err_h=None, mag_v=None, mag_h=None)
    g = np.zeros_like(W)
    n = None
    if up is not None:
        xv, eh = np.asarray(up[0], F64), np.asarray(up[1], F64)
        d = xv * (1.0 - xv)
        out["err_v"], out["mag_v"] = (eh @ W.T) * d, (np.abs(eh) @ np.abs(W).T) * d
        g += xv.T @ eh
        n = xv.shape[0]
    if down is not None:
        xh, ev = np.asarray(down[0], F64), np.asarray(down[1], F64)
        d = xh * (1.0 - xh)
        out["err_h"], out["mag_h"] = (ev @ W) * d, (np.abs(ev) @ np.abs(W)) * d
        g += ev.T @ xh
        n = xh.shape[0]
    if not apply:
        return out
    g /= n
    st.W_m *= mom
    st.W_m += lr * (g - st.weight_decay * W)
    st.W += st.W_m
    if up is not None:
        st.hb_m *= mom
        st.hb_m += lr * eh.sum(0) / n
        st.hid_bias += st.hb_m
    if down is not None:
        st.vb_m *= mom
        st.vb_m += lr * ev.sum(0) / n
        st.vis_bias += st.vb_m
    return out


def unrolled(rec, gen, data):
    """The forward pass of the unrolled network: (a_0 .. a_L, d_0 .. d_L, z) -- the encoder's activations, the decoder's (d_L = a_L,
    d_0 the reconstruction) and the decoder's output logits."""
    L = len(rec)
    a = [np.asarray(data, F64)]
    for st in rec:
        a.append(_sigmoid(a[-1] @ np.asarray(st.W, F64) + np.asarray(st.hid_bias, F64)))
    down = list(gen) + [rec[-1]]
    dec = [None] * L + [a[L]]
    z = None
    for l in range(L, 0, -1):
        z = dec[l] @ np.asarray(down[l - 1].W, F64).T + np.asarray(down[l - 1].vis_bias, F64)
        dec[l - 1] = _sigmoid(z)
    return a, dec, z


def xent(rec, gen, data):
    """The loss: minus the batch mean of the rows' sum_j data_j z_j - softplus(z_j)."""
    x = np.asarray(data, F64)
    z = unrolled(rec, gen, x)[2]
    return -float((x * z - np.logaddexp(0.0, z)).sum(1).mean())


def autoencoder_step(rec, gen, data, scalars):
    """HipEngine.autoencoder_step on states ``rec`` (L) and ``gen`` (L - 1), updated in place; ``scalars``: (lr, mom) per layer.
    Returns dict(recon, code, xent, mse), the monitors as floats on the parameters on entry."""
    L = len(rec)
    x = np.asarray(data, F64)
    a, dec, z = unrolled(rec, gen, x)
    loss = -float((x * z - np.logaddexp(0.0, z)).sum(1).mean())
    e = x - dec[0]
    mse = float((e * e).mean())
    for l in range(1, L):
        e = backprop_step(gen[l - 1], down=(dec[l], e), lr=scalars[l - 1][0], mom=scalars[l - 1][1])["err_h"]
    top = rec[-1]
    f = backprop_step(top, down=(a[L], e), apply=False)["err_h"]
    f = backprop_step(top, up=(a[L - 1], f), down=(a[L], e), lr=scalars[L - 1][0], mom=scalars[L - 1][1])["err_v"]
    for l in range(L - 1, 0, -1):
        f = backprop_step(rec[l - 1], up=(a[l - 1], f), lr=scalars[l - 1][0], mom=scalars[l - 1][1])["err_v"]
    return dict(recon=dec[0], code=a[L], xent=loss, mse=mse)
