"""Float64 reference and fp32 numpy twin of the deep Boltzmann machine arithmetic (imdbn_dbm_layer, HipEngine.dbm_infer / dbm_gibbs /
dbm_step, kernels_dbm.hpp), exact quantities by enumeration, and the error bounds of the device's results,
derived here and not tuned.

A model is ``Ws`` (L weight matrices, ``Ws[l]`` of shape [N_l, N_{l+1}]) and ``bs`` (L + 1 layer biases).  Everything works in the
dtype ``dt`` it is given.

Summation order of the kernel (stated in its header): fp32 fused multiply-adds; the reduction axis [0, K_lo) ++ [0, K_hi) is cut into
at most 16 slices; per slice each side's products are added in index order, the two finished side sums are scaled and added; the slices
are added in slice order; then the bias.  The twin states the same sums in numpy's order (``x @ W`` in fp32), which the bound covers.

Bound.  With u = 2^-24, K = K_lo + K_hi and T = |bias| + |s_lo| |x_lo| |W_lo| + |s_hi| |x_hi| |W_hi|^T, the device's pre-activation
differs from the float64 one of the SAME inputs by at most ``(K + 24) u T``: K products summed in any order, at most 16 slice
additions, two scalings, the seam addition, the bias addition, and room for the second-order terms.  Inputs that already differ by
dx_lo / dx_hi move it by ``|s_lo| dx_lo |W_lo| + |s_hi| dx_hi |W_hi|^T`` more.  A sigmoid has slope <= 1/4; its fp32 evaluation
(expf 2 u, the addition u, the division 2 u, of a value <= 1) adds 5 u <= 2^-21 =: EPS_P.  The damping arithmetic (1 - damp, two
products, one sum) adds 4 u more: a new magnetisation is within ``damp dm_old + (1 - damp) dpre / 4 + 2^-20`` (EPS_M = 2^-20 >= 9 u).

TEST INFRASTRUCTURE ONLY."""
import itertools

import numpy as np

import oracle.rbm_oracle as O

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
EPS_P, EPS_M = 2.0 ** -21, 2.0 ** -20


def sigmoid(x):
    with np.errstate(over="ignore"):
        return (x.dtype.type(1) / (x.dtype.type(1) + np.exp(-x))).astype(x.dtype)


# ---- one layer half-step --------------------------------------------------------------------------------------------------------------
def pre(W_lo, x_lo, s_lo, W_hi, x_hi, s_hi, bias, dt):
    """s_lo x_lo W_lo + s_hi x_hi W_hi^T + bias; W_lo [K_lo, N] or None, W_hi [N, K_hi] or None."""
    t = None
    if W_lo is not None:
        t = (dt(s_lo) * (np.asarray(x_lo, dt) @ np.asarray(W_lo, dt)).astype(dt)).astype(dt)
    if W_hi is not None:
        h = (dt(s_hi) * (np.asarray(x_hi, dt) @ np.asarray(W_hi, dt).T).astype(dt)).astype(dt)
        t = h if t is None else (t + h).astype(dt)
    return (t + np.asarray(bias, dt)).astype(dt)


def pre_bound(W_lo, x_lo, s_lo, W_hi, x_hi, s_hi, bias, dx_lo=None, dx_hi=None):
    """How far the device's pre-activation may be from ``pre(..., F64)`` (module docstring)."""
    T = np.abs(np.asarray(bias, F64))
    K, d = 0, 0.0
    for W, x, s, dx, lo in ((W_lo, x_lo, s_lo, dx_lo, True), (W_hi, x_hi, s_hi, dx_hi, False)):
        if W is None:
            continue
        aW = np.abs(np.asarray(W, F64))
        aW = aW if lo else aW.T
        K += aW.shape[0]
        T = T + abs(s) * (np.abs(np.asarray(x, F64)) @ aW)
        if dx is not None:
            d = d + abs(s) * (dx @ aW)
    return (K + 24) * U * T + d


def mean_field(W_lo, x_lo, s_lo, W_hi, x_hi, s_hi, bias, m, damp, dt):
    """(new m, p, residual per row)."""
    p = sigmoid(pre(W_lo, x_lo, s_lo, W_hi, x_hi, s_hi, bias, dt))
    m = np.asarray(m, dt)
    return (dt(damp) * m + (dt(1) - dt(damp)) * p).astype(dt), p, np.abs(p - m).max(1)


# ---- exact quantities by enumeration (odd layers summed out analytically) ------------------------------------------------------------
def _bits(n):
    return np.array(list(itertools.product((0.0, 1.0), repeat=n)), F64).reshape(-1, n)


def _neighbours(Ws, bs, states, l):
    """pre-activation of layer l given the states of its neighbours (float64)."""
    L = len(Ws)
    x = np.asarray(bs[l], F64)
    if l > 0:
        x = x + states[l - 1] @ np.asarray(Ws[l - 1], F64)
    if l < L:
        x = x + states[l + 1] @ np.asarray(Ws[l], F64).T
    return x


def _even_configs(Ws, bs, v=None):
    """Every joint state of the even layers (layer 0 fixed to the row ``v`` when given): (dict layer -> [C, N_l], log weight [C] with
    the odd layers summed out)."""
    L = len(Ws)
    sizes = [np.asarray(b).size for b in bs]
    even = [l for l in range(0, L + 1, 2) if not (l == 0 and v is not None)]
    parts = [_bits(sizes[l]) for l in even]
    C = int(np.prod([p.shape[0] for p in parts])) if parts else 1
    states = {}
    rep = C
    for l, p in zip(even, parts):
        rep //= p.shape[0]
        states[l] = np.tile(np.repeat(p, rep, 0), (C // (rep * p.shape[0]), 1))
    if v is not None:
        states[0] = np.tile(np.asarray(v, F64)[None, :], (C, 1))
    logw = np.zeros(C)
    for l in range(0, L + 1, 2):
        logw = logw + states[l] @ np.asarray(bs[l], F64)
    full = [states.get(l) for l in range(L + 1)]
    for l in range(1, L + 1, 2):
        logw = logw + np.logaddexp(0.0, _neighbours(Ws, bs, full, l)).sum(1)
    return full, logw


def _lse(x):
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


def log_z(Ws, bs):
    return _lse(_even_configs(Ws, bs)[1])


def log_p(Ws, bs, v, lz=None):
    """Exact log p(v) per row."""
    lz = log_z(Ws, bs) if lz is None else lz
    return np.array([_lse(_even_configs(Ws, bs, row)[1]) - lz for row in np.asarray(v, F64)])


def marginals(Ws, bs):
    """Exact p(unit = 1) of every layer."""
    full, logw = _even_configs(Ws, bs)
    w = np.exp(logw - _lse(logw))
    out = []
    for l in range(len(bs)):
        out.append(w @ (full[l] if l % 2 == 0 else sigmoid(_neighbours(Ws, bs, full, l))))
    return out


def entropy(m):
    m = np.asarray(m, F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -(np.where(m > 0, m * np.log(m), 0.0) + np.where(m < 1, (1 - m) * np.log(1 - m), 0.0))


def variational_bound(Ws, bs, v, mus, lz):
    """E_q[-E] + H(q) - log Z per row, q the product of Bernoulli(mu)."""
    s = [np.asarray(v, F64)] + [np.asarray(m, F64) for m in mus]
    out = -lz + sum(s[l] @ np.asarray(bs[l], F64) for l in range(len(s)))
    for l, W in enumerate(Ws):
        out = out + ((s[l] @ np.asarray(W, F64)) * s[l + 1]).sum(1)
    return out + sum(entropy(m).sum(1) for m in s[1:])


# ---- mean-field inference --------------------------------------------------------------------------------------------------------------
def infer(Ws, bs, v, n_mf, damp=0.0, dt=F64, init=None, trace=None):
    """([mu_1 .. mu_L], res [B]): HipEngine.dbm_infer.  ``trace``: a list that receives a copy of the magnetisations after every sweep."""
    L = len(Ws)
    v = np.asarray(v, dt)
    if init is None:
        mu = []
        for l in range(1, L + 1):
            x = v if l == 1 else mu[-1]
            mu.append(sigmoid(pre(Ws[l - 1], x, 2.0 if l < L else 1.0, None, None, 1.0, bs[l], dt)))
    else:
        mu = [np.asarray(m, dt).copy() for m in init]
    res = np.zeros(v.shape[0], dt)
    if trace is not None:
        trace.append([m.copy() for m in mu])
    for _ in range(int(n_mf)):
        res = np.zeros(v.shape[0], dt)
        for l in range(1, L + 1):
            x_lo = v if l == 1 else mu[l - 2]
            hi = (Ws[l], mu[l]) if l < L else (None, None)
            mu[l - 1], _, r = mean_field(Ws[l - 1], x_lo, 1.0, hi[0], hi[1], 1.0, bs[l], mu[l - 1], damp, dt)
            res = np.maximum(res, r)
        if trace is not None:
            trace.append([m.copy() for m in mu])
    return mu, res


def infer_bounded(Ws, bs, v, n_mf, damp=0.0):
    """The float64 inference with the bound of the module docstring carried through the start and the sweeps:
    (mu, res, dmu, res_bound [B])."""
    L = len(Ws)
    v = np.asarray(v, F64)
    mu, dmu = [], []
    for l in range(1, L + 1):
        x, dx = (v, None) if l == 1 else (mu[-1], dmu[-1])
        s = 2.0 if l < L else 1.0
        mu.append(sigmoid(pre(Ws[l - 1], x, s, None, None, 1.0, bs[l], F64)))
        dmu.append(pre_bound(Ws[l - 1], x, s, None, None, 1.0, bs[l], dx) / 4 + EPS_M)
    res, rb = np.zeros(v.shape[0]), np.zeros(v.shape[0])
    for _ in range(int(n_mf)):
        res, rb = np.zeros(v.shape[0]), np.zeros(v.shape[0])
        for l in range(1, L + 1):
            x_lo, dx_lo = (v, None) if l == 1 else (mu[l - 2], dmu[l - 2])
            W_hi, x_hi, dx_hi = (Ws[l], mu[l], dmu[l]) if l < L else (None, None, None)
            dp = pre_bound(Ws[l - 1], x_lo, 1.0, W_hi, x_hi, 1.0, bs[l], dx_lo, dx_hi) / 4
            new, _, r = mean_field(Ws[l - 1], x_lo, 1.0, W_hi, x_hi, 1.0, bs[l], mu[l - 1], damp, F64)
            res, rb = np.maximum(res, r), np.maximum(rb, (dp + EPS_P + dmu[l - 1] + U).max(1))
            dmu[l - 1] = damp * dmu[l - 1] + (1 - damp) * dp + EPS_M
            mu[l - 1] = new
    return mu, res, dmu, rb


# ---- block Gibbs -------------------------------------------------------------------------------------------------------------------------
def gibbs(Ws, bs, states, n_sweeps, src, dt=F64, clamp_bottom=None, margins=None):
    """HipEngine.dbm_gibbs on copies of ``states``: per sweep the odd layers bottom to top, then the even layers bottom to top, each
    from one ``src.uniform((M, N_l))``.  ``margins``: a list that receives, per draw, min(|p - U| - bound of p): the room every
    comparison has before fp32 rounding could flip it."""
    L = len(Ws)
    s = [np.asarray(x, dt).copy() for x in states]
    if clamp_bottom is not None:
        s[0] = np.asarray(clamp_bottom, dt).copy()
    for _ in range(int(n_sweeps)):
        for parity in (1, 0):
            for l in range(parity, L + 1, 2):
                if l == 0 and clamp_bottom is not None:
                    continue
                lo = (Ws[l - 1], s[l - 1]) if l > 0 else (None, None)
                hi = (Ws[l], s[l + 1]) if l < L else (None, None)
                p = sigmoid(pre(lo[0], lo[1], 1.0, hi[0], hi[1], 1.0, bs[l], dt))
                u = np.asarray(src.uniform(p.shape), dt)
                if margins is not None:
                    b = pre_bound(lo[0], lo[1], 1.0, hi[0], hi[1], 1.0, bs[l]) / 4 + EPS_P
                    margins.append(float((np.abs(p.astype(F64) - u.astype(F64)) - b).min()))
                s[l] = (p > u).astype(dt)
    return s


# ---- the update ------------------------------------------------------------------------------------------------------------------------
def states_as(sts, dt):
    out = []
    for st in sts:
        s = st.copy()
        for k in ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m"):
            setattr(s, k, np.asarray(getattr(st, k), dt).copy())
        out.append(s)
    return out


def model_of(sts):
    """(Ws, bs) of a list of RBM states under the bias convention: layer 0 = sts[0].vis_bias, layer l >= 1 = sts[l-1].hid_bias."""
    return [s.W for s in sts], [sts[0].vis_bias] + [s.hid_bias for s in sts]


def step(sts, data, particles, scalars, n_mf, damp, gibbs_k, src, monitor=True, margins=None):
    """HipEngine.dbm_step in the dtype of sts[0].W: updates the RBM states in place (the momentum / decay rule is
    O.apply_cd_update's, without the sparsity term); returns dict(mu, particles, res, recon_loss, grads) -- ``grads``: per RBM the
    (dW, d hid_bias, d vis_bias) the step applied, (pos - neg) / B.  ``margins`` as in ``gibbs``."""
    dt = sts[0].W.dtype.type
    Ws, bs = model_of(sts)
    data = np.asarray(data, dt)
    mu, res = infer(Ws, bs, data, n_mf, damp, dt)
    recon = None
    if monitor:
        rec = sigmoid(pre(None, None, 1.0, Ws[0], mu[0], 1.0, bs[0], dt))
        recon = dt(((rec - data) ** 2).astype(dt).mean(dtype=dt))
    neg = gibbs(Ws, bs, particles, gibbs_k, src, dt, margins=margins)
    pos = [data] + mu
    n = data.shape[0]
    stats = []
    for l in range(len(sts)):
        stats.append({"pos_assoc": (pos[l].T @ pos[l + 1]).astype(dt), "neg_assoc": (neg[l].T @ neg[l + 1]).astype(dt),
                      "pos_h_sum": pos[l + 1].sum(0, dtype=dt), "neg_h_sum": neg[l + 1].sum(0, dtype=dt),
                      "data_sum": pos[l].sum(0, dtype=dt), "v_sum": neg[l].sum(0, dtype=dt)})
    grads = []
    for st, s, (lr, mom) in zip(sts, stats, scalars):
        O.apply_cd_update(st, s, lr, mom, n, False)
        grads.append(((s["pos_assoc"] - s["neg_assoc"]) / dt(n), (s["pos_h_sum"] - s["neg_h_sum"]) / dt(n), (s["data_sum"] - s["v_sum"]) / dt(n)))
    return dict(mu=mu, particles=neg, res=res, recon_loss=recon, grads=grads)


def rel_frobenius(x, ref):
    x, ref = np.asarray(x, F64), np.asarray(ref, F64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))
