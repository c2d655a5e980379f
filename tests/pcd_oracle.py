"""numpy twin of the persistent-chain calls (imdbn_rbm_pcd_step, imdbn_rbm_pt_sweep), built from the CPU oracle's
propagations (``oracle.rbm_oracle``: forward, visible_probs, sample_visible, apply_cd_update and their ``T`` arguments) and
``oracle.draws.PhiloxStream``.  The exchange's Delta is in float64 on the oracle's fp32 logits.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import oracle.rbm_oracle as O

F32 = np.float32
F64 = np.float64


def rbm_state(c, lr=0.1, weight_decay=1e-4, momentum=0.5, sparsity=False, sparsity_factor=0.05):
    """The oracle state of a case dict (pcd_cases.case), momentum buffers included."""
    st = O.RBMState.create(c["W"], lr, weight_decay, momentum, softmax_groups=c["groups"], hid_bias=c["c"], vis_bias=c["b"],
                           sparsity=sparsity, sparsity_factor=sparsity_factor)
    if "W_m" in c:
        st.W_m, st.hb_m, st.vb_m = c["W_m"].copy(), c["hb_m"].copy(), c["vb_m"].copy()
    return st


def gibbs(st, v, rng, T=1.0):
    """h = 1[p(h | v) > U], v' = sample_visible(p(v | h)), both at temperature T."""
    h_prob = O.forward(st, v, T)
    h = O._bern(h_prob, rng.uniform(h_prob.shape))
    return O.sample_visible(st, O.visible_probs(st, h, T), rng)


def pcd_step(st, data, particles, cd_k, rng, lr, mom):
    """imdbn_rbm_pcd_step: updates `st` in place; returns (loss, the particles after cd_k Gibbs steps)."""
    data = np.asarray(data, F32)
    pos_h = O.forward(st, data)
    v = np.asarray(particles, F32).copy()
    for _ in range(int(cd_k)):
        v = gibbs(st, v, rng)
    h_neg = O.forward(st, v)
    loss = F32(((data - O.visible_probs(st, pos_h)) ** 2).astype(F32).mean(dtype=F32))      # the parameters on entry
    s = dict(pos_assoc=(data.T @ pos_h).astype(F32), neg_assoc=(v.T @ h_neg).astype(F32),
             pos_h_sum=pos_h.sum(0, dtype=F32), neg_h_sum=h_neg.sum(0, dtype=F32), data_sum=data.sum(0, dtype=F32), v_sum=v.sum(0, dtype=F32))
    O.apply_cd_update(st, s, lr, mom, data.shape[0], st.sparsity)
    return loss, v


def softplus_sum(beta, x):
    """S(beta, v) = sum_j softplus(beta x_j(v)) in float64."""
    return np.logaddexp(0.0, F64(beta) * np.asarray(x, F64)).sum(-1)


def exchange_delta(st, u_lo, u_hi, b_lo, b_hi):
    """Delta of exchanging u_lo (at b_lo) and u_hi (at b_hi), float64 [M]."""
    x_lo = (np.asarray(u_lo, F32) @ st.W) + st.hid_bias
    x_hi = (np.asarray(u_hi, F32) @ st.W) + st.hid_bias
    bv = (np.asarray(u_lo, F64) - np.asarray(u_hi, F64)) @ st.vis_bias.astype(F64)
    return ((F64(b_hi) - F64(b_lo)) * bv + softplus_sum(b_lo, x_hi) + softplus_sum(b_hi, x_lo)
            - softplus_sum(b_lo, x_lo) - softplus_sum(b_hi, x_hi))


def pt_sweep(st, state, betas, n_sweeps, rng):
    """imdbn_rbm_pt_sweep on state [R M, V]: returns (state, swap_try [max(R - 1, 1)], swap_acc, smallest |log U - Delta|)."""
    betas = np.asarray(betas, F32)
    R = len(betas)
    v = np.asarray(state, F32).copy()
    RM, V = v.shape
    M = RM // R
    tries, accs = np.zeros(max(R - 1, 1), np.int64), np.zeros(max(R - 1, 1), np.int64)
    margin = float("inf")
    for s in range(int(n_sweeps)):
        T = [float(F32(1.0) / betas[r]) for r in range(R)]
        rows = [slice(r * M, (r + 1) * M) for r in range(R)]
        h_prob = np.concatenate([O.forward(st, v[rows[r]], T[r]) for r in range(R)], 0)
        h = O._bern(h_prob, rng.uniform(h_prob.shape))
        v = O.sample_visible(st, np.concatenate([O.visible_probs(st, h[rows[r]], T[r]) for r in range(R)], 0), rng)
        if R < 2:
            continue
        with np.errstate(divide="ignore"):
            logu = np.log(rng.uniform((RM, 1))[:, 0].astype(F64))
        for r in range(s % 2, R - 1, 2):
            lo, hi = rows[r], rows[r + 1]
            delta = exchange_delta(st, v[lo], v[hi], betas[r], betas[r + 1])
            acc = logu[lo] < delta
            margin = min(margin, float(np.abs(logu[lo] - delta).min()))
            tries[r] += M
            accs[r] += int(acc.sum())
            a, b = v[lo].copy(), v[hi].copy()
            v[lo] = np.where(acc[:, None], b, a)
            v[hi] = np.where(acc[:, None], a, b)
    return v, tries, accs, margin


def log_tempered_marginal(st, v, beta):
    """log of the unnormalised p_beta(v) = sum_h exp(-beta E(v, h)) by enumeration over h (tiny H only), float64."""
    W, b, c = st.W.astype(F64), st.vis_bias.astype(F64), st.hid_bias.astype(F64)
    H = W.shape[1]
    hs = ((np.arange(2 ** H)[:, None] >> np.arange(H)[None, :]) & 1).astype(F64)
    v = np.asarray(v, F64)
    e = F64(beta) * ((v @ b)[:, None] + hs @ c + (v @ W) @ hs.T)
    m = e.max(1, keepdims=True)
    return (m[:, 0] + np.log(np.exp(e - m).sum(1)))
