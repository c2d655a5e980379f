"""Cases and the derived score tolerance of the pair-score tests (tests/test_retrieval_cpu.py, tests/test_retrieval_gpu.py).

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import retrieval_oracle as RO

F32 = np.float32
U = 2.0 ** -24          # unit roundoff of fp32


def tau(H, D1, D2, xmax, bdot=0.0):
    """Bound on |device score - float64 score|.  ``xmax`` bounds, over every pair and hidden unit, the ABSOLUTE sum
    |c_j| + sum_i |z_i| |W_ij| (it dominates max |x|); ``bdot`` bounds sum_i |z_i| |b_i| over a pair.
      per term   x = a + b: each half is an fp32 accumulation of D1 (D2) fp32-exact products plus the bias, any order:
                 (D1 + D2 + 8) u xmax, and softplus is 1-Lipschitz; the fp32 add a + b: u xmax;
                 exp2 argument rounding, v_exp_f32 (1 ulp, result <= 1), the rounding of 1 + t, v_log_f32 (1 ulp, result <= 1) and the
                 multiplication by ln 2, all on values <= 2: 2^-21 together; the final fma rounding: u (xmax + 1)
      sum        H terms in double: H 2^-52 |S|, below everything else
      bias dots  (D1 + D2 + 16) u bdot
      total      rounded to fp32: u |S|, |S| <= H (xmax + 1) + bdot; twice that covers the double sum as well"""
    per_term = (D1 + D2 + 8) * U * xmax + U * xmax + 2.0 ** -21 + U * (xmax + 1.0)
    return H * per_term + (D1 + D2 + 16) * U * bdot + 2.0 * U * (H * (xmax + 1.0) + bdot)


class Case:
    """Parameters and codes of one case: fp32 arrays, logits scaled so that they reach 31 on either side (both softplus branches beyond |x| = 30; 33 on its one side where the logits have one sign)."""

    def __init__(self, name, H, Q, N, D1, D2, binary, seed, pad=(0, 0, 0)):
        self.name, self.H, self.Q, self.N, self.D1, self.D2, self.binary, self.pad = name, H, Q, N, D1, D2, binary, pad
        g = np.random.default_rng(seed)
        code = (lambda n, d: (g.random((n, d)) > 0.5).astype(F32)) if binary else (lambda n, d: g.random((n, d)).astype(F32))
        self.z1, self.z2 = code(Q, D1), code(N, D2)
        if binary and D1 == 1 and D2 == 1:
            self.z1[0, 0] = self.z2[0, 0] = 1.0
        sign = np.where(g.random(H) > 0.5, 1.0, -1.0)          # one sign per hidden unit: no cancellation inside a logit, so the
        W = np.abs(g.standard_normal((D1 + D2, H))) * sign     # absolute sum that the tolerance takes is the logit's own magnitude
        c = np.abs(g.standard_normal(H)) * sign
        x = c[None, None, :] + (RO.f64(self.z1) @ W[:D1])[:, None, :] + (RO.f64(self.z2) @ W[D1:])[None, :, :]
        lo, hi = -x.min(), x.max()
        f = 31.0 / min(lo, hi) if min(lo, hi) > 0 else 33.0 / np.abs(x).max()
        self.W, self.c = (W * f).astype(F32), (c * f).astype(F32)
        self.b = (4 * g.standard_normal(D1 + D2)).astype(F32)
        self.gt_q = g.integers(0, N, Q).astype(np.int32)
        self.gt_n = g.integers(0, Q, N).astype(np.int32)
        self._S = None

    def x(self):
        W, c = RO.f64(self.W), RO.f64(self.c)
        return c[None, None, :] + (RO.f64(self.z1) @ W[:self.D1])[:, None, :] + (RO.f64(self.z2) @ W[self.D1:])[None, :, :]

    def xmax(self):
        Wa, D1 = np.abs(RO.f64(self.W)), self.D1
        return float((np.abs(RO.f64(self.c)) + (np.abs(RO.f64(self.z1)) @ Wa[:D1]).max(0) + (np.abs(RO.f64(self.z2)) @ Wa[D1:]).max(0)).max())

    def bdot(self):
        ba, D1 = np.abs(RO.f64(self.b)), self.D1
        return float((np.abs(RO.f64(self.z1)) @ ba[:D1]).max() + (np.abs(RO.f64(self.z2)) @ ba[D1:]).max())

    def tau(self):
        return tau(self.H, self.D1, self.D2, self.xmax(), self.bdot())

    def S64(self):
        """The twin's scores: computed once, shared, never written."""
        if self._S is None:
            self._S = RO.scores(self.W, self.c, self.b, self.D1, self.z1, self.z2)
            self._S.setflags(write=False)
        return self._S


# every H of {1, 24, 63, 64, 65, 200}, every (Q, N) of {(1, 1), (3, 130), (64, 64), (65, 129), (130, 3)}, every (D1, D2) of
# {(1, 1), (20, 16), (33, 70)}, 0/1 and real codes, padded pitches (ld1, ld2, lds beyond the row length)
_SPECS = [
    ("h1_1x1", 1, 1, 1, 1, 1, True, 1, (0, 0, 0)),
    ("h200_3x130", 200, 3, 130, 20, 16, False, 2, (3, 0, 5)),
    ("h63_64x64", 63, 64, 64, 1, 1, False, 3, (0, 7, 0)),
    ("h24_130x3_wide", 24, 130, 3, 33, 70, True, 4, (1, 1, 1)),
    ("h65_65x129", 65, 65, 129, 1, 1, False, 5, (4, 4, 3)),
    ("h64_64x64_bin", 64, 64, 64, 20, 16, True, 6, (0, 0, 0)),
    ("h24_1x1_wide", 24, 1, 1, 33, 70, True, 7, (0, 0, 0)),
]
_cache = {}


def case_names():
    return [s[0] for s in _SPECS]


def get_case(name):
    if name not in _cache:
        _cache[name] = Case(*next(s for s in _SPECS if s[0] == name))
    return _cache[name]


def planted(roll=0):
    """D1 = D2 = H = N = Q = 48, z1 = z2 = I, W[:D1] = W[D1:] = 8 I (the mod2 rows rolled by `roll`), c = -12, b = 0: every matched pair
    scores softplus(4) + 47 softplus(-12) against 2 softplus(-4) + 46 softplus(-12) for every other pair."""
    n = 48
    eye = np.eye(n, dtype=F32)
    W = np.concatenate([8 * eye, np.roll(8 * eye, roll, axis=0)]).astype(F32)
    return {"W": W, "c": np.full(n, -12, dtype=F32), "b": np.zeros(2 * n, dtype=F32), "D1": n, "z1": eye.copy(), "z2": eye.copy(),
            "gt": ((np.arange(n) + roll) % n).astype(np.int32)}


def bimodal_model(dev):
    """The iMDBN_BiModal of tests/golden/bimodal_small_100_40_20__64_30_16__j24_12.npz (the modality stacks as its generator draws
    them, the joint layers as the fixture's training left them) with its paired data as the loader: (model, X1, X2)."""
    import torch
    from golden_utils import Fixture
    from parity_cases import init_W, loader, set_params
    from imdbn.models.imdbn_bimodal import iMDBN_BiModal
    fx = Fixture("bimodal_small_100_40_20__64_30_16__j24_12.npz")
    m, s = fx.meta, fx.stream()
    K, B, NB = m["K"], m["B"], m["NB"]
    Nn = B * NB
    yi = fx["yi"]
    X1 = np.abs((s.uniform((K, 100)) > 0.7).astype(F32)[yi] - (s.uniform((Nn, 100)) > 0.9).astype(F32)).astype(F32)
    X2 = np.abs((s.uniform((K, 64)) > 0.6).astype(F32)[yi] - (s.uniform((Nn, 64)) > 0.92).astype(F32)).astype(F32)
    dl = loader(X1, X2, B)
    mdl = iMDBN_BiModal(m["sizes1"], m["sizes2"], m["joint"], params=dict(m["params"]), dataloader=dl, val_loader=dl,
                        device=torch.device(dev))
    for sizes, dbn in ((m["sizes1"], mdl.mod1_dbn), (m["sizes2"], mdl.mod2_dbn)):
        for i, r in enumerate(dbn.layers):
            set_params(r, dev, init_W(s, sizes[i], sizes[i + 1]))
    for li, r in enumerate(mdl.joint_layers):
        set_params(r, dev, fx[f"joint{li}_W"], fx[f"joint{li}_hid_bias"], fx[f"joint{li}_vis_bias"])
    return mdl, X1, X2
