"""numpy twin of the centered update (imdbn_rbm_centered_step) on the phases of the CPU oracle
(``oracle.rbm_oracle.cd_statistics``) and of the persistent-chain twin (``pcd_oracle``).  The update itself works in the dtype of the
state it is given: float32 mirrors the engine's order of operations, float64 serves the algebra check of tests/test_centered_cpu.py.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import oracle.rbm_oracle as O
import pcd_oracle as T

F32 = np.float32


def offsets_and_gradient(s, n, mu, lam, slide, mode, dt=F32):
    """Steps 1-3 of the header: (mu', lam', gW, dv, dh) from un-normalised statistics `s` (the keys of O.cd_statistics)."""
    a = lambda x: np.asarray(x, dt)
    n, slide = dt(n), dt(slide)
    svp, svn, shp, shn = a(s["data_sum"]), a(s["v_sum"]), a(s["pos_h_sum"]), a(s["neg_h_sum"])
    dv, dh = (svp - svn) / n, (shp - shn) / n
    mv = (svp + svn) / (dt(2) * n) if mode else svp / n
    mh = (shp + shn) / (dt(2) * n) if mode else shp / n
    mu2 = ((dt(1) - slide) * a(mu) + slide * mv).astype(dt)
    lam2 = ((dt(1) - slide) * a(lam) + slide * mh).astype(dt)
    gW = ((a(s["pos_assoc"]) - a(s["neg_assoc"])) / n - np.outer(mu2, dh) - np.outer(dv, lam2)).astype(dt)
    return mu2, lam2, gW, dv, dh


def apply_centered_update(st, s, lr, mom, n, sparsity, mu, lam, slide, mode):
    """Steps 1-5 on `st` in place, in the dtype of st.W; returns (mu', lam').  With zero offsets and slide = 0 every operation is
    that of O.apply_cd_update, in its order."""
    dt = st.W.dtype.type
    a = lambda x: np.asarray(x, dt)
    mu2, lam2, gW, _, _ = offsets_and_gradient(s, n, mu, lam, slide, mode, dt)
    lr_, mom_, n_ = dt(lr), dt(mom), dt(n)
    st.W_m *= mom_
    st.W_m += lr_ * (gW - dt(st.weight_decay) * st.W)
    st.W += st.W_m
    st.hb_m *= mom_
    st.hb_m += lr_ * (a(s["pos_h_sum"]) - a(s["neg_h_sum"])) / n_
    st.hb_m -= lr_ * (gW.T @ mu2).astype(dt)
    if sparsity:
        Q = (a(s["pos_h_sum"]) / n_).astype(dt)
        st.hb_m += dt(-lr) * (Q - dt(st.sparsity_factor))
    st.hid_bias += st.hb_m
    st.vb_m *= mom_
    st.vb_m += lr_ * (a(s["data_sum"]) - a(s["v_sum"])) / n_
    st.vb_m -= lr_ * (gW @ lam2).astype(dt)
    st.vis_bias += st.vb_m
    return mu2, lam2


def pcd_statistics(st, data, particles, cd_k, rng):
    """The phases of pcd_oracle.pcd_step without its update: (statistics, loss, particles after cd_k Gibbs steps)."""
    data = np.asarray(data, F32)
    pos_h = O.forward(st, data)
    v = np.asarray(particles, F32).copy()
    for _ in range(int(cd_k)):
        v = T.gibbs(st, v, rng)
    h_neg = O.forward(st, v)
    loss = F32(((data - O.visible_probs(st, pos_h)) ** 2).astype(F32).mean(dtype=F32))
    s = dict(pos_assoc=(data.T @ pos_h).astype(F32), neg_assoc=(v.T @ h_neg).astype(F32),
             pos_h_sum=pos_h.sum(0, dtype=F32), neg_h_sum=h_neg.sum(0, dtype=F32), data_sum=data.sum(0, dtype=F32), v_sum=v.sum(0, dtype=F32))
    return s, loss, v


def centered_step(st, data, particles, cd_k, rng, lr, mom, mu, lam, slide, mode):
    """imdbn_rbm_centered_step: updates `st` in place; returns (loss, particles after the Gibbs steps or None, mu', lam')."""
    data = np.asarray(data, F32)
    if particles is None:
        s = O.cd_statistics(st, data, cd_k, rng)
        loss, v = F32(s["sq_err"].mean(dtype=F32)), None
    else:
        s, loss, v = pcd_statistics(st, data, particles, cd_k, rng)
    mu2, lam2 = apply_centered_update(st, s, lr, mom, data.shape[0], st.sparsity, mu, lam, slide, mode)
    return loss, v, mu2, lam2
