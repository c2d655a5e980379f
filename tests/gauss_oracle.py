"""numpy twin of the Gaussian-visible calls (imdbn_rbm_gauss_*), drawing through ``oracle.draws.PhiloxStream``
(or any source with ``uniform`` / ``normal``).  Every function works in the dtype it is given: float64 is the reference the GPU
tests compare with, float32 restates the engine's arithmetic and measures what fp32 alone costs (tests/gauss_cases.fp32_errors).

Cho, Ilin & Raiko 2011, with z the log-variance and u = v e^{-z}:
    E(v, h)  = sum_i (v_i - b_i)^2 / (2 sigma_i^2) - sum_ij (v_i / sigma_i^2) W_ij h_j - sum_j c_j h_j
    p(h | v) = sigmoid(c + u W),   p(v | h) = N(b + h W^T, sigma^2),   F(v) = sum (v - b)^2 / (2 sigma^2) - sum softplus(c + u W)

TEST INFRASTRUCTURE ONLY."""
import itertools

import numpy as np

F32, F64 = np.float32, np.float64
MARGIN = {"min": float("inf")}          # the smallest |p - u| of a Bernoulli decision since reset_margin()


def reset_margin():
    MARGIN["min"] = float("inf")


class GState:
    """Parameters and momenta of a Gaussian-visible RBM in one dtype."""
    KEYS = ("W", "b", "c", "z", "W_m", "vb_m", "hb_m", "z_m")

    def __init__(self, W, b, c, z, W_m=None, vb_m=None, hb_m=None, z_m=None, weight_decay=0.0, sparsity=False, target=0.0, dt=F64):
        a = lambda x, like: np.zeros_like(np.asarray(like, dt)) if x is None else np.array(x, dt)
        self.dt = dt
        self.W, self.b, self.c, self.z = a(W, W), a(b, b), a(c, c), a(z, z)
        self.W_m, self.vb_m, self.hb_m, self.z_m = a(W_m, W), a(vb_m, b), a(hb_m, c), a(z_m, z)
        self.weight_decay, self.sparsity, self.target = weight_decay, bool(sparsity), target

    def copy(self, dt=None):
        dt = dt or self.dt
        return GState(*(getattr(self, k) for k in self.KEYS), weight_decay=self.weight_decay, sparsity=self.sparsity, target=self.target, dt=dt)


def sigmoid(x):
    return (1 / (1 + np.exp(-x))).astype(x.dtype)


def softplus(x):
    return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20)))).astype(x.dtype)


def scale(st, v):
    return (np.asarray(v, st.dt) * np.exp(-st.z)).astype(st.dt)


def prop_up(st, v, T=1.0):
    return sigmoid(((scale(st, v) @ st.W + st.c) / st.dt(max(1e-6, T))).astype(st.dt))


def prop_down(st, h):
    return (np.asarray(h, st.dt) @ st.W.T + st.b).astype(st.dt)


def sample_visible(st, mean, rng):
    n = np.asarray(rng.normal(mean.shape), st.dt)
    return (np.asarray(mean, st.dt) + np.exp(st.dt(0.5) * st.z) * n).astype(st.dt)


def bern(p, u):
    u = np.asarray(u, p.dtype)
    if p.size:
        MARGIN["min"] = min(MARGIN["min"], float(np.abs(p - u).min()))
    return (p > u).astype(p.dtype)


def free_energy(st, v):
    v = np.asarray(v, st.dt)
    x = (scale(st, v) @ st.W + st.c).astype(st.dt)
    return (((v - st.b) ** 2 * (st.dt(0.5) * np.exp(-st.z))).sum(1) - softplus(x).sum(1)).astype(st.dt)


def gradients(st, data, u0, P0, v1, u1, P1, n):
    """(gW, gb, gc, gz) of the header from the two phases; W, b, z of `st` as on entry.  The expectations may be weighted sums:
    pass n = 1 with rows already weighted (exact_gradients)."""
    dt = st.dt
    n = dt(n)
    S = (u0.T @ P0 - u1.T @ P1).astype(dt)
    q0, q1 = ((data - st.b) ** 2).sum(0), ((v1 - st.b) ** 2).sum(0)
    r = (st.W * S).sum(1)
    return S / n, (u0 - u1).sum(0) / n, (P0 - P1).sum(0) / n, np.exp(-st.z) * (q0 - q1) / (dt(2) * n) - r / n, S


def cd_step(st, data, cd_k, rng, lr, mom, lr_z, z_lo=-np.inf, z_hi=np.inf, sample_v=True, record=None):
    """imdbn_rbm_gauss_cd_step on `st` in place; returns the loss mean((data - m_last)^2).  `record` (a dict) receives the h samples
    ("h": list), the means ("m": list) and the gradients ("g")."""
    dt = st.dt
    data = np.asarray(data, dt)
    n = data.shape[0]
    u0 = scale(st, data)
    P0 = sigmoid((u0 @ st.W + st.c).astype(dt))
    h = bern(P0, rng.uniform(P0.shape))
    hs, ms = [h], []
    for it in range(int(cd_k)):
        m = prop_down(st, h)
        ms.append(m)
        v = sample_visible(st, m, rng) if sample_v else m
        u = scale(st, v)
        P = sigmoid((u @ st.W + st.c).astype(dt))
        if it < cd_k - 1:
            h = bern(P, rng.uniform(P.shape))
            hs.append(h)
    gW, gb, gc, gz, S = gradients(st, data, u0, P0, v, u, P, n)
    loss = dt(((data - m) ** 2).mean())
    lr_, mom_ = dt(lr), dt(mom)
    st.W_m *= mom_
    st.W_m += lr_ * (gW - dt(st.weight_decay) * st.W)
    st.W += st.W_m
    st.vb_m *= mom_
    st.vb_m += lr_ * gb
    st.b += st.vb_m
    st.hb_m *= mom_
    st.hb_m += lr_ * gc
    if st.sparsity:
        st.hb_m += dt(-lr) * (P0.sum(0) / dt(n) - dt(st.target))
    st.c += st.hb_m
    if lr_z != 0:
        st.z_m *= mom_
        st.z_m += dt(lr_z) * gz
        st.z[:] = np.minimum(np.maximum(st.z + st.z_m, dt(z_lo)), dt(z_hi))
    if record is not None:
        record.update(h=hs, m=ms, g=(gW, gb, gc, gz), v=v)
    return loss


# ---- the exact model by enumeration over h (tiny H only), float64 -------------------------------------------------------------------
def _hidden_states(H):
    return np.array(list(itertools.product((0.0, 1.0), repeat=H)), F64)


def log_partition(W, b, c, z):
    """log Z = log sum_h prod_i sqrt(2 pi sigma_i^2) exp(c.h + sum_i ((b_i + (W h)_i)^2 - b_i^2) / (2 sigma_i^2)): v integrated in
    closed form."""
    hs = _hidden_states(W.shape[1])
    m = b[None, :] + hs @ W.T
    t = hs @ c + ((m ** 2 - b[None, :] ** 2) * (0.5 * np.exp(-z))[None, :]).sum(1)
    return 0.5 * (np.log(2 * np.pi) + z).sum() + t.max() + np.log(np.exp(t - t.max()).sum()), t, hs, m


def mean_log_likelihood(W, b, c, z, data):
    st = GState(W, b, c, z)
    return float((-free_energy(st, data)).mean() - log_partition(W, b, c, z)[0])


def exact_gradients(st, data):
    """The twin's (gW, gb, gc, gz) with the negative statistics replaced by exact model expectations: per h the visible moments of
    N(m_h, sigma^2) in closed form, E[u] = m e^{-z}, E[(v - b)^2] = (m - b)^2 + sigma^2, weighted by p(h); rows weighted so that n = 1."""
    data = np.asarray(data, F64)
    n = data.shape[0]
    _, t, hs, m = log_partition(st.W, st.b, st.c, st.z)
    p = np.exp(t - t.max())
    p /= p.sum()
    u0 = scale(st, data)
    P0 = prop_up(st, data)
    iv = np.exp(-st.z)
    S = u0.T @ P0 / n - ((m * iv).T * p) @ hs
    q = ((data - st.b) ** 2).mean(0) - (p[:, None] * ((m - st.b) ** 2 + np.exp(st.z))).sum(0)
    gb = u0.mean(0) - (p[:, None] * m * iv).sum(0)
    gc = P0.mean(0) - p @ hs
    return S, gb, gc, iv * q / 2 - (st.W * S).sum(1)
