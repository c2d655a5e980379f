"""Shapes, seeds and tolerances of the label-gradient tests, shared by tests/test_labelgrad_cpu.py and tests/test_labelgrad_gpu.py.

(Dz, K, H, N) of a joint RBM over [code (Dz) | one-hot label (K)] cross the edges of the per-row kernel (kernels_labelgrad.hpp: one wave
per row, four rows per block, 64 label slots per register), of the propagation that feeds it and of the update kernel behind it."""
import numpy as np

from anneal_cases import params

F32 = np.float32

# name -> (Dz, K, H, N)
CASES = {
    "odd": (37, 3, 33, 5),            # nothing on a tile edge; H % 4 != 0: unaligned weight rows, the generic update route; N % 4 != 0
    "k65": (20, 65, 70, 6),           # K crosses a 64-slot boundary, H crosses 64
    "kmax": (16, 256, 64, 2),         # LABEL_KMAX, whole tiles
    "rows67": (130, 10, 200, 67),     # two row tiles in the propagation, a row reduction longer than a wave
    "wide": (1100, 4, 96, 3),         # 0/1 z, V > 1024
    "one": (8, 2, 4, 1),              # the smallest legal call
}
BINARY_Z = ("wide",)
SCALES = (0.1, 1.0)
LR, MOM, WD = 0.1, 0.9, 1e-4


def case(name, scale):
    """dict(Dz, K, H, N, V, W, b, c, Wm, bm, cm, z, gt): fp32 parameters at weight scale `scale`, non-zero momentum buffers, z in [0, 1]
    (0/1 for BINARY_Z), labels in [0, K) with every class of a small K present where N allows."""
    Dz, K, H, N = CASES[name]
    V = Dz + K
    idx = list(CASES).index(name)
    seed = 800 + 10 * idx + (1 if scale >= 1.0 else 0)
    W, b, c, _ = params(V, H, seed, scale)
    g = np.random.Generator(np.random.PCG64(seed + 5))
    Wm = (g.standard_normal((V, H)) * 0.01).astype(F32)
    bm = (g.standard_normal(V) * 0.01).astype(F32)
    cm = (g.standard_normal(H) * 0.01).astype(F32)
    z = g.random((N, Dz)).astype(F32)
    if name in BINARY_Z:
        z = (z > 0.5).astype(F32)
    gt = g.integers(0, K, N).astype(np.int32)
    return dict(name=name, scale=scale, Dz=Dz, K=K, H=H, N=N, V=V, W=W, b=b, c=c, Wm=Wm, bm=bm, cm=cm, z=z, gt=gt)


def state(c):
    """Copies of the six parameter and momentum arrays of a case."""
    return {k: c[k].copy() for k in ("W", "b", "c", "Wm", "bm", "cm")}


# ---- tolerances: the project's convention for the label-side kernel puts a class value within eps = H 1e-5 of float64, so
# |dp_k| <= 2 eps p_k; with |ds| <= 2.5e-6 every entry of hpos - hneg, r and r s is within 2 eps + 1e-5
def eps(H):
    return H * 1e-5


def tol_delta(H):
    return 2 * eps(H) + 1e-5


def tol_logp(H, want):
    return 2 * eps(H) + 1e-9 * np.abs(want)


def tol_param(H, want, lr):
    """Every parameter and momentum entry after one step: a gradient entry / N within tol_delta (|z| <= 1), times lr, plus fp32 rounding."""
    return lr * tol_delta(H) + 1e-6 * (np.abs(want) + lr)
