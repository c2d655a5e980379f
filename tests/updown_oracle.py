"""numpy twin of the up-down fine-tuning calls (imdbn_rbm_delta_step, HipEngine.updown_step), built from the CPU
oracle's propagations (``oracle.rbm_oracle``), ``oracle.draws.PhiloxStream`` and ``pcd_oracle.pcd_step`` for the top RBM.

``delta_step`` works on any object with W / hid_bias / vis_bias / W_m / hb_m / vb_m / weight_decay arrays, in the dtype ``dt``: float32
is the engine's arithmetic, float64 serves the autograd check of tests/test_updown_cpu.py.  The row log-probability is always summed
in float64 on the logits as computed.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import oracle.rbm_oracle as O
import pcd_oracle as P

F32 = np.float32
F64 = np.float64


def logits(st, direction, x, dt=F32):
    x = np.asarray(x, dt)
    if direction == "up":
        return ((x @ st.W.astype(dt, copy=False)) + st.hid_bias.astype(dt, copy=False)).astype(dt)
    return ((x @ st.W.astype(dt, copy=False).T) + st.vis_bias.astype(dt, copy=False)).astype(dt)


def _sigmoid(a, dt):
    return O.sigmoid(a) if dt is F32 else 1.0 / (1.0 + np.exp(-a))


def row_logp(a, target):
    """sum_j target_j a_j - softplus(a_j) in float64: log p(target | in) of the factorial Bernoulli layer."""
    a = np.asarray(a, F64)
    return (np.asarray(target, F64) * a - np.logaddexp(0.0, a)).sum(1)


def delta_step(st, direction, x, target, lr=None, mom=0.0, dt=F32):
    """imdbn_rbm_delta_step: returns out_rowlp (float64 [B], from the parameters on entry); with ``lr`` the update, in place."""
    x, t = np.asarray(x, dt), np.asarray(target, dt)
    a = logits(st, direction, x, dt)
    lp = row_logp(a, t)
    if lr is None:
        return lp
    r = (t - _sigmoid(a, dt)).astype(dt)
    n = dt(x.shape[0])
    g = ((x.T @ r) if direction == "up" else (r.T @ x)).astype(dt) / n
    st.W_m *= dt(mom)
    st.W_m += dt(lr) * (g - dt(st.weight_decay) * st.W)
    st.W += st.W_m
    bias, m = (st.hid_bias, st.hb_m) if direction == "up" else (st.vis_bias, st.vb_m)
    m *= dt(mom)
    m += dt(lr) * r.sum(0, dtype=dt) / n
    bias += m
    return lp


def updown_step(rec, gen, data, scalars, cd_k, rng, chains=None):
    """HipEngine.updown_step on oracle states ``rec`` (L) and ``gen`` (L - 1), updated in place.  ``chains``: None (CD-``cd_k`` from
    the top wake state) or a dict holding the top RBM's persistent chains under "pcd" (created on first use as the engine creates
    them: 1[s_top > U] on one ("u", V_top) draw, which is s_top).  Returns dict(wake, sleep, particles, wake_nll, sleep_nll, top_loss)."""
    wake = [np.asarray(data, F32)]
    for st in rec[:-1]:
        p = O.forward(st, wake[-1])
        wake.append(O._bern(p, rng.uniform(p.shape)))
    s_top = wake[-1]
    if chains is None:
        particles = s_top.copy()
    else:
        if "pcd" not in chains:
            chains["pcd"] = (s_top > rng.uniform(s_top.shape)).astype(F32)      # a 0/1 "probability": no margin to speak of
        particles = chains["pcd"]
    lr, mom = scalars[-1]
    loss, v = P.pcd_step(rec[-1], s_top, particles, cd_k, rng, lr, mom)
    if chains is not None:
        chains["pcd"] = v
    sleep = [v]
    for g in reversed(gen):
        sleep.insert(0, O.sample_visible(g, O.visible_probs(g, sleep[0]), rng))
    lp_w = [delta_step(g, "down", wake[l + 1], wake[l], *scalars[l]) for l, g in enumerate(gen)]
    lp_s = [delta_step(r, "up", sleep[l], sleep[l + 1], *scalars[l]) for l, r in enumerate(rec[:-1])]
    nll = lambda lps: -float(np.sum(lps, 0).mean()) if lps else 0.0
    return dict(wake=wake[1:], sleep=sleep[:-1], particles=v, wake_nll=nll(lp_w), sleep_nll=nll(lp_s), top_loss=loss)


def sample_values(rec, gen, top_minus_f, v, mode, rng):
    """The untied ``dbn_sample_values`` before the top term's log Z: float64 [B] = sum_l [log p_G(s_l | s_{l+1}) + E_l] - F_top(s_L-1),
    ``top_minus_f(state)`` giving -F of the top RBM.  Returns (values, top state)."""
    cur = np.asarray(v, F32)
    acc = np.zeros(cur.shape[0], F64)
    for r, g in zip(rec[:-1], gen):
        a = logits(r, "up", cur)
        p = O.sigmoid(a)
        h = O._bern(p, rng.uniform(p.shape))
        acc += row_logp(logits(g, "down", h), cur) - row_logp(a, h if mode == "logq" else p)
        cur = h
    return acc + top_minus_f(cur), cur
