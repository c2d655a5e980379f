"""Shapes, seeds and tolerances of the exact-enumeration tests, shared by tests/test_exact_cpu.py and tests/test_exact_gpu.py.

n is the width of the enumerated side, D of the other one.  The shapes cross every edge of kernels_exact.hpp: n below, at and above
the 5 walk bits (1, 2, 5, 6, 12), D around the 64 lanes and the 128-column chunk (1, 63, 64, 65, 127, 128, 129, 257, 1000), groups
that straddle a chunk edge, both sides, and one n = 23 case that takes two launches.  Weights are those of ``pll_cases``' generator
(``anneal_cases.params``) at its two scales: 1.0 up to n = 6, 0.1 above, so that pre-activations (a sum of up to n weights) stay of
order one -- the condition under which the fp32 walk keeps the tolerance, checked by the restatement test."""
import numpy as np

from anneal_cases import params
from pll_cases import SCALES

F32 = np.float32

# name -> (V, H, side, groups, gaussian, pitch)
CASES = {
    "n1_d1": (1, 1, "hidden", (), False, None),
    "n2_d63": (63, 2, "hidden", (), False, None),
    "n5_d64": (64, 5, "auto", (), False, None),
    "n6_d65": (65, 6, "hidden", (), False, None),
    "n12_d127": (127, 12, "auto", (), False, None),
    "n5_d128": (128, 5, "hidden", (), False, None),
    "n6_d129_pitch": (129, 6, "hidden", (), False, 16),            # W rows 16 floats apart, the padding poisoned with NaN
    "n12_d257": (257, 12, "hidden", (), False, None),
    "n6_d1000": (1000, 6, "auto", (), False, None),
    "vis_n5_d129": (5, 129, "visible", (), False, None),            # the visible side forced ...
    "vis_n12_d65": (12, 65, "auto", (), False, None),               # ... and chosen
    "vis_n6_d6": (6, 6, "visible", (), False, None),                # a tie: auto would take the hidden side
    "hid_wide_n12": (6, 12, "hidden", (), False, None),             # the larger side forced
    "group1": (140, 6, "auto", ((120, 135),), False, None),         # one group across the chunk edge at 128
    "group2": (270, 5, "hidden", ((122, 134), (250, 262)), False, None),    # two groups, across the chunk edges at 128 and at 256
    "gauss_n6_d65": (65, 6, "auto", (), True, None),
    "gauss_n12_d129": (129, 12, "hidden", (), True, None),
    "launches_n23_d8": (8, 23, "hidden", (), False, None),          # 2^23 states: two launches of 2^22
}
FAST = [k for k in CASES if k != "launches_n23_d8"]


def case(name):
    """dict(V, H, side, groups, W, b, c, z, pitch): fp32 parameters; z (log-variances spread over [-2, 1]) only for a Gaussian case."""
    V, H, side, groups, gauss, pitch = CASES[name]
    idx = list(CASES).index(name)
    n = V if side == "visible" or (side == "auto" and V < H and not groups and not gauss) else H
    W, b, c, _ = params(V, H, 900 + idx, SCALES[1] if n <= 6 else SCALES[0])
    z = None
    if gauss:
        z = np.linspace(-2.0, 1.0, V).astype(F32)[np.random.Generator(np.random.PCG64(idx)).permutation(V)]
    return dict(name=name, V=V, H=H, side=side, groups=[tuple(g) for g in groups], W=W, b=b, c=c, z=z, pitch=pitch, n=n, D=V + H - n)


def tol_log_z(c, want):
    """The convention of pll_cases.site_tol for a sum of D softplus terms: D 1e-5 + 1e-9 |log Z|."""
    return c["D"] * 1e-5 + 1e-9 * abs(want)


def tol_marginal(c, want_log_z, x_max=None):
    """4 tol(log Z): d e^x at |x| <= tol, plus the final normalisation; the Gaussian mean scales with max |b + a|."""
    return 4.0 * tol_log_z(c, want_log_z) * (1.0 if x_max is None else x_max)


def spike(n, D, s_star, seed, side="hidden"):
    """A model whose state s* of the enumerated side is about e^40 above every other: a bias of +-40 per unit of E matching the bits
    of s*, weights at the scale 0.01, the other side's bias at 0.1.  -> dict(V, H, W, b, c, side, bits [n])."""
    g = np.random.Generator(np.random.PCG64(seed))
    bits = ((s_star >> np.arange(n)) & 1).astype(F32)
    e = (40.0 * (2.0 * bits - 1.0)).astype(F32)
    f = (0.1 * g.standard_normal(D)).astype(F32)
    Wd = (0.01 * g.standard_normal((n, D))).astype(F32)
    if side == "hidden":
        return dict(V=D, H=n, W=np.ascontiguousarray(Wd.T), b=f, c=e, side=side, bits=bits, n=n, D=D, groups=[], z=None)
    return dict(V=n, H=D, W=Wd, b=e, c=f, side=side, bits=bits, n=n, D=D, groups=[], z=None)
