"""Float64 reference and fp32 numpy twin of the multimodal deep Boltzmann machine arithmetic (imdbn_dbm_group_layer, HipEngine.mdbm_infer /
mdbm_gibbs / mdbm_step, kernels_dbm_group.hpp), exact quantities by enumeration, and the error bounds of the device's
results, derived here and not tuned.  The sigmoid layers and their bounds are tests/dbm_oracle.py's.

A model is ``Ws`` (the L image weight matrices, ``Ws[l]`` [N_l, N_{l+1}], N_L = Dz), ``WJ`` ([Dz + K, J], the joint RBM's matrix over
``[z_img | y]``) and ``bs`` (the L + 3 layer biases b_0 .. b_L, b_J, b_Y).  Everything works in the dtype ``dt`` it is given.

Summation order of the softmax (stated in the kernel's header): per group the maximum, e_j = exp(x_j - max), the sum of the e_j over four
columns per lane and then a butterfly over 64 lanes, p_j = e_j / sum.  The twin states the same sums in numpy's order, which the bound
covers.

Bound of the softmax.  Let the device's logits x~ differ from the float64 ones x by at most d within a row's group (d = the largest
``dbm_oracle.pre_bound`` of the group: dpre <= (K + 24) u T, plus what the inputs' own errors move).  In exact arithmetic
softmax(x~)_j / softmax(x)_j = e^{d_j} sum e^x / sum e^{x + d_i} lies in [e^{-2d}, e^{2d}].  In fp32 (u = 2^-24), with r the largest
|x~_j - max| <= range(x) + 2 d of the group and n its width: the subtraction moves the exponent by at most u r, expf is within 2 u
relative, so every e_j carries a relative error (r + 2) u; a sum of n positive terms in any order n u more (the largest term is exactly 1:
no overflow, and a term that underflows is below 2^-126 absolutely); the division u.  Together, with room for the second-order terms,
    |p^_j - p_j| <= p_j (expm1(2 d) + e^{2 d} (2 r + n + 8) u) + 2^-100 =: dp_j.
A new magnetisation is within ``damp dm_old + (1 - damp) dp + EPS_D`` (EPS_D = 2^-22 = 4 u: 1 - damp, two products, one sum, of values
<= 1); a residual within ``max_j (dp_j + dm_old_j) + u``.

Bound of a Philox pick.  The device adds c_j = clamp(p^_j, 1e-8, 1) left to right in fp32 and takes the first j whose cumulative sum
exceeds fl(U tot).  A cumulative sum of the device differs from the float64 one of the float64 p by at most sum_j dp_j + n u tot, the
threshold by at most that again plus u tot.  ``pick`` returns, per row, the distance of U tot to the two cumulative sums that decide the
pick; where it exceeds ``pick_bound = 2 sum_j dp_j + (2 n + 4) u tot`` the float64 reference alone decides the index.

TEST INFRASTRUCTURE ONLY."""
import itertools

import numpy as np

import dbm_oracle as Dt
import oracle.rbm_oracle as O

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
EPS_D = 2.0 ** -22
TINY = 2.0 ** -100


def ends_to_groups(ends):
    return list(zip([0] + list(ends[:-1]), ends))


# ---- one categorical layer half-step ---------------------------------------------------------------------------------------------------
def softmax(x, groups, dt):
    """Per group of columns: exp(x - max) / sum."""
    x = np.asarray(x, dt)
    out = np.empty_like(x)
    for s, e in groups:
        z = (x[:, s:e] - x[:, s:e].max(1, keepdims=True)).astype(dt)
        ex = np.exp(z).astype(dt)
        out[:, s:e] = (ex / ex.sum(1, keepdims=True, dtype=dt)).astype(dt)
    return out


def softmax_bound(x64, p64, groups, dpre):
    """dp (module docstring) for float64 logits ``x64``, their softmax ``p64`` and the bound ``dpre`` [B, N] of the device's logits."""
    out = np.empty_like(p64)
    for s, e in groups:
        d = np.asarray(dpre, F64)[:, s:e].max(1, keepdims=True)
        r = (x64[:, s:e].max(1, keepdims=True) - x64[:, s:e].min(1, keepdims=True)) + 2 * d
        out[:, s:e] = p64[:, s:e] * (np.expm1(2 * d) + np.exp(2 * d) * (2 * r + (e - s) + 8) * U) + TINY
    return out


def group_mean_field(W_lo, x_lo, W_hi, x_hi, bias, groups, m, damp, dt):
    """(new m, p, residual per row)."""
    p = softmax(Dt.pre(W_lo, x_lo, 1.0, W_hi, x_hi, 1.0, bias, dt), groups, dt)
    m = np.asarray(m, dt)
    return (dt(damp) * m + (dt(1) - dt(damp)) * p).astype(dt), p, np.abs(p - m).max(1)


def philox_uniform(seed, draw, row0, B):
    """The uniform of the ("c", .) draw number ``draw``: element (row, 0) of a [B, 1] tensor."""
    from oracle.draws import PhiloxStream
    return PhiloxStream(seed, draw, row0).uniform_silent((B, 1))[:, 0]


def pick(p, u, dt=F64):
    """(index [B], margin [B], tot [B]): the inverse-CDF walk over clamp(p, 1e-8, 1) against u tot in ``dt``; the margin is the
    distance of u tot to the cumulative sums on either side of the pick that could flip it (infinite where none can)."""
    c = np.clip(np.asarray(p, dt), dt(1e-8), dt(1.0))
    B, n = c.shape
    idx, margin, tots = np.zeros(B, np.int64), np.full(B, np.inf), np.zeros(B)
    for b in range(B):
        cum = np.zeros(n, dt)
        acc = dt(0)
        for j in range(n):
            acc = dt(acc + c[b, j])
            cum[j] = acc
        thr = dt(dt(u[b]) * acc)
        hit = np.nonzero(cum > thr)[0]
        j = int(hit[0]) if hit.size else n - 1
        sides = ([float(thr) - float(cum[j - 1])] if j > 0 else []) + ([float(cum[j]) - float(thr)] if j < n - 1 else [])
        idx[b], tots[b] = j, float(acc)
        if sides:
            margin[b] = min(sides)
    return idx, margin, tots


def pick_bound(dp, tot):
    n = dp.shape[1]
    return 2 * dp.sum(1) + (2 * n + 4) * U * tot


def one_hot(idx, n, dt=F32):
    out = np.zeros((len(idx), n), dt)
    out[np.arange(len(idx)), idx] = 1
    return out


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, Ws, WJ, bs):
        self.Ws, self.WJ, self.bs = list(Ws), WJ, list(bs)
        self.L = len(Ws)
        self.Dz = Ws[-1].shape[1]
        self.K = WJ.shape[0] - self.Dz
        self.J = WJ.shape[1]
        assert len(bs) == self.L + 3 and bs[-1].size == self.K and bs[-2].size == self.J

    @property
    def sizes(self):
        return [self.Ws[0].shape[0]] + [W.shape[1] for W in self.Ws] + [self.J]

    def as_(self, dt):
        return Model([np.asarray(W, dt) for W in self.Ws], np.asarray(self.WJ, dt), [np.asarray(b, dt) for b in self.bs])


def _lse(x):
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


def _bits(n):
    return np.array(list(itertools.product((0.0, 1.0), repeat=n)), F64).reshape(-1, n)


def configs(M, v=None, y=None):
    """Every joint state of the class of Y (the layers of parity L, and Y) with the class of J summed out, in float64; ``v`` (a row of
    layer 0) and ``y`` (a class index) fix that layer.  Returns (states: layer -> [C, N_l] for the enumerated layers, "y" -> [C, K]
    one-hot; inputs: layer or "J" -> [C, N] the input of every summed-out layer; log weight [C])."""
    M = M.as_(F64)
    L, K = M.L, M.K
    own = [l for l in range(L + 1) if (l & 1) == (L & 1)]
    parts = []
    for l in own:
        parts.append(np.asarray(v, F64)[None, :] if (l == 0 and v is not None) else _bits(M.bs[l].size))
    parts.append(np.eye(K)[[int(y)]] if y is not None else np.eye(K))
    grids = np.meshgrid(*[np.arange(p.shape[0]) for p in parts], indexing="ij")
    st = {l: p[g.ravel()] for l, p, g in zip(own + ["y"], parts, grids)}
    C = st["y"].shape[0]
    logw = st["y"] @ M.bs[L + 2]
    for l in own:
        logw = logw + st[l] @ M.bs[l]
    inputs = {}
    for l in range(L + 1):
        if (l & 1) == (L & 1):
            continue
        x = np.tile(M.bs[l][None, :], (C, 1))
        if l > 0:
            x = x + st[l - 1] @ M.Ws[l - 1]
        if l < L:
            x = x + st[l + 1] @ M.Ws[l].T
        inputs[l] = x
        if l == 0 and v is not None:
            logw = logw + x @ np.asarray(v, F64)
        else:
            logw = logw + np.logaddexp(0.0, x).sum(1)
    inputs["J"] = M.bs[L + 1][None, :] + np.concatenate([st[L], st["y"]], 1) @ M.WJ
    logw = logw + np.logaddexp(0.0, inputs["J"]).sum(1)
    return st, inputs, logw


def log_z(M):
    return _lse(configs(M)[2])


def marginals(M):
    """Exact p(unit = 1) of the layers 0 .. L, of J, and the category frequencies of Y: a list of L + 3 vectors."""
    st, inp, logw = configs(M)
    w = np.exp(logw - _lse(logw))
    out = [w @ (st[l] if l in st else Dt.sigmoid(inp[l])) for l in range(M.L + 1)]
    return out + [w @ Dt.sigmoid(inp["J"]), w @ st["y"]]


def label_posterior(M, v):
    """Exact p(y | v) per row, [B, K]."""
    out = []
    for row in np.asarray(v, F64):
        st, _, logw = configs(M, v=row)
        w = np.exp(logw - _lse(logw))
        out.append(w @ st["y"])
    return np.array(out)


def log_p_joint(M, v, y, lz=None):
    """Exact log p(v, y) per row (y: class indices)."""
    lz = log_z(M) if lz is None else lz
    return np.array([_lse(configs(M, v=row, y=c)[2]) - lz for row, c in zip(np.asarray(v, F64), y)])


def variational_bound(M, v, mus, lz=0.0):
    """E_q[-E] + H(q) - lz per row for q = prod Bernoulli(mu_l) x Bernoulli(mu_J) x Categorical(mu_Y); ``mus`` as ``infer`` returns
    them.  A one-hot mu_Y (the label clamped) has entropy 0: the bound is then one on log p(v, y)."""
    M = M.as_(F64)
    L = M.L
    s = [np.asarray(v, F64)] + [np.asarray(m, F64) for m in mus]
    out = -lz + sum(s[l] @ M.bs[l] for l in range(L + 3))
    for l, W in enumerate(M.Ws):
        out = out + ((s[l] @ W) * s[l + 1]).sum(1)
    out = out + ((np.concatenate([s[L], s[L + 2]], 1) @ M.WJ) * s[L + 1]).sum(1)
    my = s[L + 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        hy = -np.where(my > 0, my * np.log(my), 0.0).sum(1)
    return out + sum(Dt.entropy(m).sum(1) for m in s[1:L + 2]) + hy


# ---- mean-field inference ----------------------------------------------------------------------------------------------------------------
def infer(M, v, y, n_mf, damp=0.0, dt=F64, trace=None):
    """([mu_1 .. mu_L, mu_J, mu_Y], res [B]): HipEngine.mdbm_infer; ``y`` one-hot [B, K] or None (free).  ``trace``: a list that receives
    a copy of the magnetisations after the start and after every sweep."""
    M = M.as_(dt)
    L, Dz, K = M.L, M.Dz, M.K
    v = np.asarray(v, dt)
    B = v.shape[0]
    free = y is None
    my = np.tile(softmax(M.bs[L + 2][None, :], [(0, K)], dt), (B, 1)) if free else np.asarray(y, dt).copy()
    mu = []
    for l in range(1, L + 1):
        mu.append(Dt.sigmoid(Dt.pre(M.Ws[l - 1], v if l == 1 else mu[-1], 2.0, None, None, 1.0, M.bs[l], dt)))
    mj = Dt.sigmoid(Dt.pre(M.WJ, np.concatenate([mu[-1], my], 1), 1.0, None, None, 1.0, M.bs[L + 1], dt))
    res = np.zeros(B, dt)
    if trace is not None:
        trace.append([m.copy() for m in mu + [mj, my]])
    for _ in range(int(n_mf)):
        res = np.zeros(B, dt)
        for l in range(1, L + 1):
            W_hi, x_hi = (M.Ws[l], mu[l]) if l < L else (M.WJ[:Dz], mj)
            mu[l - 1], _, r = Dt.mean_field(M.Ws[l - 1], v if l == 1 else mu[l - 2], 1.0, W_hi, x_hi, 1.0, M.bs[l], mu[l - 1], damp, dt)
            res = np.maximum(res, r)
        mj, _, r = Dt.mean_field(M.WJ, np.concatenate([mu[-1], my], 1), 1.0, None, None, 1.0, M.bs[L + 1], mj, damp, dt)
        res = np.maximum(res, r)
        if free:
            my, _, r = group_mean_field(None, None, M.WJ[Dz:], mj, M.bs[L + 2], [(0, K)], my, damp, dt)
            res = np.maximum(res, r)
        if trace is not None:
            trace.append([m.copy() for m in mu + [mj, my]])
    return mu + [mj, my], res


def infer_bounded(M, v, y, n_mf, damp=0.0):
    """The float64 inference with the bounds of the two module docstrings carried through the start and the sweeps:
    (mu, res, dmu, res_bound [B])."""
    M = M.as_(F64)
    L, Dz, K = M.L, M.Dz, M.K
    v = np.asarray(v, F64)
    B = v.shape[0]
    free = y is None
    G = [(0, K)]
    if free:
        x0 = np.tile(M.bs[L + 2][None, :], (B, 1))
        my = softmax(x0, G, F64)
        dmy = softmax_bound(x0, my, G, np.zeros_like(x0))
    else:
        my, dmy = np.asarray(y, F64).copy(), np.zeros((B, K))
    mu, dmu = [], []
    for l in range(1, L + 1):
        x, dx = (v, None) if l == 1 else (mu[-1], dmu[-1])
        mu.append(Dt.sigmoid(Dt.pre(M.Ws[l - 1], x, 2.0, None, None, 1.0, M.bs[l], F64)))
        dmu.append(Dt.pre_bound(M.Ws[l - 1], x, 2.0, None, None, 1.0, M.bs[l], dx) / 4 + Dt.EPS_M)
    zy, dzy = np.concatenate([mu[-1], my], 1), np.concatenate([dmu[-1], dmy], 1)
    mj = Dt.sigmoid(Dt.pre(M.WJ, zy, 1.0, None, None, 1.0, M.bs[L + 1], F64))
    dmj = Dt.pre_bound(M.WJ, zy, 1.0, None, None, 1.0, M.bs[L + 1], dzy) / 4 + Dt.EPS_M
    res, rb = np.zeros(B), np.zeros(B)
    for _ in range(int(n_mf)):
        res, rb = np.zeros(B), np.zeros(B)
        for l in range(1, L + 1):
            x_lo, dx_lo = (v, None) if l == 1 else (mu[l - 2], dmu[l - 2])
            W_hi, x_hi, dx_hi = (M.Ws[l], mu[l], dmu[l]) if l < L else (M.WJ[:Dz], mj, dmj)
            dp = Dt.pre_bound(M.Ws[l - 1], x_lo, 1.0, W_hi, x_hi, 1.0, M.bs[l], dx_lo, dx_hi) / 4
            new, _, r = Dt.mean_field(M.Ws[l - 1], x_lo, 1.0, W_hi, x_hi, 1.0, M.bs[l], mu[l - 1], damp, F64)
            res, rb = np.maximum(res, r), np.maximum(rb, (dp + Dt.EPS_P + dmu[l - 1] + U).max(1))
            dmu[l - 1] = damp * dmu[l - 1] + (1 - damp) * dp + Dt.EPS_M
            mu[l - 1] = new
        zy, dzy = np.concatenate([mu[-1], my], 1), np.concatenate([dmu[-1], dmy], 1)
        dp = Dt.pre_bound(M.WJ, zy, 1.0, None, None, 1.0, M.bs[L + 1], dzy) / 4
        new, _, r = Dt.mean_field(M.WJ, zy, 1.0, None, None, 1.0, M.bs[L + 1], mj, damp, F64)
        res, rb = np.maximum(res, r), np.maximum(rb, (dp + Dt.EPS_P + dmj + U).max(1))
        dmj = damp * dmj + (1 - damp) * dp + Dt.EPS_M
        mj = new
        if free:
            x = Dt.pre(None, None, 1.0, M.WJ[Dz:], mj, 1.0, M.bs[L + 2], F64)
            dpre = Dt.pre_bound(None, None, 1.0, M.WJ[Dz:], mj, 1.0, M.bs[L + 2], None, dmj)
            p = softmax(x, G, F64)
            dp = softmax_bound(x, p, G, dpre)
            res, rb = np.maximum(res, np.abs(p - my).max(1)), np.maximum(rb, (dp + dmy + U).max(1))
            dmy = damp * dmy + (1 - damp) * dp + EPS_D
            my = damp * my + (1 - damp) * p
    return mu + [mj, my], res, dmu + [dmj, dmy], rb


# ---- block Gibbs -------------------------------------------------------------------------------------------------------------------------
def gibbs(M, states, n_sweeps, src, dt=F64, clamp_bottom=None, clamp_labels=None, margins=None):
    """HipEngine.mdbm_gibbs on copies of ``states`` = [s_0 .. s_{L-1}, zy, s_J]: per sweep the class of J bottom to top, then the other
    class bottom to top with Y right after layer L; a sigmoid layer takes one ``src.uniform((M, N_l))``, Y one ``src.categorical(p)``
    (indices).  ``margins`` as in ``dbm_oracle.gibbs`` (sigmoid layers only)."""
    M = M.as_(dt)
    L, Dz, K = M.L, M.Dz, M.K
    parts = [np.asarray(x, dt).copy() for x in states]
    s = parts[:L] + [parts[L][:, :Dz].copy(), parts[L + 1]]
    y = parts[L][:, Dz:].copy()
    if clamp_bottom is not None:
        s[0] = np.asarray(clamp_bottom, dt).copy()
    if clamp_labels is not None:
        y = np.asarray(clamp_labels, dt).copy()
    for _ in range(int(n_sweeps)):
        for parity in ((L + 1) & 1, L & 1):
            for l in range(parity, L + 2, 2):
                if l == 0 and clamp_bottom is not None:
                    continue
                if l <= L:
                    lo = (M.Ws[l - 1], s[l - 1]) if l > 0 else (None, None)
                    hi = (M.Ws[l], s[l + 1]) if l < L else (M.WJ[:Dz], s[L + 1])
                    bias = M.bs[l]
                else:
                    lo, hi, bias = (M.WJ, np.concatenate([s[L], y], 1)), (None, None), M.bs[L + 1]
                p = Dt.sigmoid(Dt.pre(lo[0], lo[1], 1.0, hi[0], hi[1], 1.0, bias, dt))
                u = np.asarray(src.uniform(p.shape), dt)
                if margins is not None:
                    b = Dt.pre_bound(lo[0], lo[1], 1.0, hi[0], hi[1], 1.0, bias) / 4 + Dt.EPS_P
                    margins.append(float((np.abs(p.astype(F64) - u.astype(F64)) - b).min()))
                s[l] = (p > u).astype(dt)
                if l == L and clamp_labels is None:
                    py = softmax(Dt.pre(None, None, 1.0, M.WJ[Dz:], s[L + 1], 1.0, M.bs[L + 2], dt), [(0, K)], dt)
                    y = one_hot(np.asarray(src.categorical(py)), K, dt)
    return s[:L] + [np.concatenate([s[L], y], 1), s[L + 1]]


# ---- the update ------------------------------------------------------------------------------------------------------------------------
def model_of(sts):
    """The Model of the RBM states ``sts`` (the image RBMs bottom first, the joint RBM last) under the bias convention."""
    img, jt = sts[:-1], sts[-1]
    Dz = img[-1].W.shape[1]
    return Model([s.W for s in img], jt.W, [img[0].vis_bias] + [s.hid_bias for s in img] + [jt.hid_bias, jt.vis_bias[Dz:]])


def step(sts, data, y, particles, scalars, n_mf, damp, gibbs_k, src, monitor=True, margins=None):
    """HipEngine.mdbm_step in the dtype of sts[0].W: updates the RBM states in place (O.apply_cd_update without the sparsity term);
    returns dict(mu, particles, res, recon_loss)."""
    dt = sts[0].W.dtype.type
    M = model_of(sts)
    L = M.L
    data, y = np.asarray(data, dt), np.asarray(y, dt)
    mu, res = infer(M, data, y, n_mf, damp, dt)
    recon = None
    if monitor:
        rec = Dt.sigmoid(Dt.pre(None, None, 1.0, M.Ws[0], mu[0], 1.0, M.bs[0], dt))
        recon = dt(((rec - data) ** 2).astype(dt).mean(dtype=dt))
    neg = gibbs(M, particles, gibbs_k, src, dt, margins=margins)
    pos = [data] + mu[:L - 1] + [np.concatenate([mu[L - 1], y], 1), mu[L]]
    n = data.shape[0]
    stats = []
    for l in range(L + 1):
        pv, nv = pos[l], neg[l]                   # RBM l < L: layer l -> layer l + 1 (z_img of the zy row); RBM L: the joint RBM
        ph, nh = (pos[l + 1][:, :M.Dz], neg[l + 1][:, :M.Dz]) if l + 1 == L else (pos[l + 1], neg[l + 1])
        stats.append({"pos_assoc": (pv.T @ ph).astype(dt), "neg_assoc": (nv.T @ nh).astype(dt), "pos_h_sum": ph.sum(0, dtype=dt),
                      "neg_h_sum": nh.sum(0, dtype=dt), "data_sum": pv.sum(0, dtype=dt), "v_sum": nv.sum(0, dtype=dt)})
    for st, s, (lr, mom) in zip(sts, stats, scalars):
        O.apply_cd_update(st, s, lr, mom, n, False)
    return dict(mu=mu, particles=neg, res=res, recon_loss=recon)


# ---- the CPU engine double ---------------------------------------------------------------------------------------------------------------
from types import SimpleNamespace  # noqa: E402

import torch  # noqa: E402

from dbm_engine_double import DbmOracleEngine  # noqa: E402
from oracle_engine import _Src, _np  # noqa: E402


def _as_rbm(r):
    """An RBM, or a view of a W standing for one (HipEngine._dbm_operands)."""
    return SimpleNamespace(W=SimpleNamespace(data=r)) if isinstance(r, torch.Tensor) else r


class MdbmOracleEngine(DbmOracleEngine):
    """``DbmOracleEngine`` plus ``HipEngine.dbm_group_layer`` / ``mdbm_infer`` / ``mdbm_gibbs`` / ``mdbm_step`` on the fp32 twin above:
    the CPU suite runs the host logic of ``imdbn.models.mdbm`` through it."""
    name = "oracle-test-double-mdbm"

    def _dbm_layer(self, lo, hi, x_lo, x_hi, bias, m, damp, s_lo, s_hi, sample, rng, want_p, want_res, s_out=None):
        return super()._dbm_layer(_as_rbm(lo), _as_rbm(hi), x_lo, x_hi, bias, m, damp, s_lo, s_hi, sample, rng, want_p, want_res, s_out=s_out)

    def dbm_group_layer(self, lo, hi, x_lo, x_hi, bias, groups, m=None, damp=0.0, sample=False, rng=None, want_p=False, want_res=False,
                        s_out=None):
        self.calls.append(("dbm_group_layer", lo is not None, hi is not None, bool(sample)))
        lo, hi = _as_rbm(lo), _as_rbm(hi)
        W_lo = None if lo is None else lo.W.data.numpy()
        W_hi = None if hi is None else hi.W.data.numpy()
        xl = None if lo is None else _np(x_lo)
        xh = None if hi is None else _np(x_hi)
        b = _np(bias.data if isinstance(bias, torch.nn.Parameter) else bias)
        gs = [(int(s), int(e)) for s, e in groups]
        if sample:
            p = softmax(Dt.pre(W_lo, xl, 1.0, W_hi, xh, 1.0, b, F32), gs, F32)
            src = _Src(rng)
            s = np.zeros_like(p)
            for g0, g1 in gs:
                s[:, g0:g1] = one_hot(np.asarray(src.categorical(np.clip(p[:, g0:g1], F32(1e-8), F32(1.0)))), g1 - g0)
            src.done()
            smp = self._t(s)
            if s_out is not None:
                smp = s_out.copy_(smp)                         # in place, as the engine
            return (self._t(p), smp) if want_p else smp
        new, _, res = group_mean_field(W_lo, xl, W_hi, xh, b, gs, _np(m), damp, F32)
        m.copy_(torch.from_numpy(new))                         # in place, as the engine
        return self._t(res) if want_res else None

    # the three compositions are the engine's own host code, run on this double's calls
    def mdbm_infer(self, image_layers, joint, biases, v, y, n_mf, damp=0.0, want_res=True):
        from imdbn.engine.hip_engine import HipEngine
        self.calls.append(("mdbm_infer", tuple(v.shape), y is not None, int(n_mf), float(damp)))
        return HipEngine.mdbm_infer(self, image_layers, joint, biases, v, y, n_mf, damp=damp, want_res=want_res)

    def mdbm_gibbs(self, image_layers, joint, biases, particles, n_sweeps, rng, clamp_bottom=None, clamp_labels=None):
        from imdbn.engine.hip_engine import HipEngine
        self.calls.append(("mdbm_gibbs", int(n_sweeps), clamp_bottom is not None, clamp_labels is not None))
        return HipEngine.mdbm_gibbs(self, image_layers, joint, biases, particles, n_sweeps, rng, clamp_bottom=clamp_bottom,
                                    clamp_labels=clamp_labels)

    def mdbm_step(self, image_layers, joint, data, labels, particles, epoch_scalars, n_mf, damp, gibbs_k, rng, monitor=True):
        from imdbn.engine.hip_engine import HipEngine
        self.calls.append(("mdbm_step", tuple(data.shape), int(n_mf), float(damp), int(gibbs_k), bool(monitor)))
        return HipEngine.mdbm_step(self, image_layers, joint, data, labels, particles, epoch_scalars, n_mf, damp, gibbs_k, rng, monitor=monitor)

    @staticmethod
    def _mdbm_check(who, image_layers, joint, biases):
        from imdbn.engine.hip_engine import HipEngine
        return HipEngine._mdbm_check(who, image_layers, joint, biases)
