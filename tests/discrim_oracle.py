"""float64 numpy twin of imdbn_rbm_label_backprop_step and HipEngine.discriminative_step, built on the twins of
the two calls it joins: tests/labelgrad_oracle.py (the joint RBM's exact class posterior, states as dicts W / b / c / Wm / bm / cm) and
tests/backprop_oracle.py (one sigmoid layer, states as objects with W / hid_bias / ... arrays, updated in place).

  e = hpos - hneg        g_z = e W[:Dz]^T = d log p(t | z) / d z        err_z = g_z z (1 - z)

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import backprop_oracle as Bp
import labelgrad_oracle as Lg

F64 = np.float64


def class_values(W, b, c, z, K):
    """a [N, K]: minus the free energy of [z, e_k] per class, float64."""
    W, b, c, z = (np.asarray(x, F64) for x in (W, b, c, z))
    Dz = z.shape[1]
    o = (z @ W[:Dz] + c)[:, None, :] + W[Dz:][None, :, :]
    return (z @ b[:Dz])[:, None] + b[Dz:][None, :] + np.logaddexp(0.0, o).sum(2)


def head(W, b, c, z, K, gt):
    """The output layer on the parameters given: dict(logp [N], pred [N], gap [N] (the top class value minus the second), e [N, H],
    g_z, err_z [N, Dz], and the two magnitude sums a bound on err_z is stated in: wsum [Dz] = sum_j |W_ij| and
    mag [N, Dz] = z (1 - z) sum_j |e_j| |W_ij|).  A row with a label outside [0, K) has logp = NaN and zero rows of e, g_z, err_z."""
    q = Lg.rows(W, b, c, z, K, gt)
    z = np.asarray(z, F64)
    Dz = z.shape[1]
    Wz = np.asarray(W, F64)[:Dz]
    a = class_values(W, b, c, z, K)
    top = np.sort(a, 1)
    e = q["hpos"] - q["hneg"]
    d = z * (1.0 - z)
    g_z = e @ Wz.T
    return dict(logp=q["logp"], pred=a.argmax(1), gap=top[:, -1] - top[:, -2], e=e, g_z=g_z, err_z=g_z * d,
                wsum=np.abs(Wz).sum(1), mag=(np.abs(e) @ np.abs(Wz).T) * d)


def label_backprop_step(st, z, K, gt, lr=0.0, mom=0.0, wd=0.0, apply=True):
    """-> (head(...) on the state on entry, the state after: labelgrad_oracle.step's with ``apply``, else the state itself)."""
    out = head(st["W"], st["b"], st["c"], z, K, gt)
    return out, (Lg.step(st, z, K, gt, lr, mom, wd)[1] if apply else st)


def forward(layers, data):
    """a_0 .. a_L of the recognition pass."""
    a = [np.asarray(data, F64)]
    for s in layers:
        a.append(Bp._sigmoid(a[-1] @ np.asarray(s.W, F64) + np.asarray(s.hid_bias, F64)))
    return a


def mean_logp(layers, joint, data, K, gt):
    """The objective: mean over the rows of log p(gt | data) of the whole model."""
    z = forward(layers, data)[-1]
    return float(Lg.rows(joint["W"], joint["b"], joint["c"], z, K, gt)["logp"].mean())


def discriminative_step(layers, joint, data, K, gt, scalars, head_scalars, head_wd=0.0, train_head=True):
    """HipEngine.discriminative_step: ``layers`` updated in place, -> (dict(code, nll, acc, head), the joint state after)."""
    L = len(layers)
    a = forward(layers, data)
    out, joint = label_backprop_step(joint, a[L], K, gt, head_scalars[0], head_scalars[1], head_wd, train_head)
    ok = np.isfinite(out["logp"])
    f = out["err_z"]
    for l in range(L, 0, -1):
        f = Bp.backprop_step(layers[l - 1], up=(a[l - 1], f), lr=scalars[l - 1][0], mom=scalars[l - 1][1])["err_v"]
    return dict(code=a[L], nll=-float(np.nanmean(out["logp"])), acc=float((out["pred"][ok] == np.asarray(gt)[ok]).mean()), head=out), joint
