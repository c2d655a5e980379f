"""Cases of the DBM tests (tests/test_dbm_cpu.py, tests/test_dbm_gpu.py).

Layer cases are (K_lo, N, K_hi, B); weights ~ N(0, 1 / K) of their own side (pre-activations of order 1 at every size), biases
~ N(0, 0.5^2), operands uniform in (0.05, 0.95) or 0 / 1, all from ``numpy.random.default_rng(seed)``.

The constants of kernels_dbm.hpp and the shapes that sit one below / one above them:
  DBM_TN = 64    output units per tile           -> N 63 / 65
  DBM_BM = 64    batch rows per chunk            -> B 63 / 65
  DBM_KC = 32    reduction steps per stage       -> K_lo 31 / 33 with K_hi 33 / 31; K_hi = 1
  4 DBM_KC = 128 steps, the shortest K slice     -> K_lo + K_hi 255 (one slice) / 257 (two slices of 160 and 97 steps)
  the seam: with N <= 64 and B <= 64 a reduction of 256 <= K < 384 steps runs as two slices of rup(ceil(K / 2), 32) steps.
  (250, ., 20): slices [0, 160) and [160, 270), the second holds the seam at 250;  (160, ., 110): the seam is the slice edge;
  (256, ., 20): the issue's twin, slices of 160 steps, the seam at 256 inside the second.
"""
import numpy as np

F32 = np.float32

TABLE = [(67, 33, 21, 5), (128, 64, 64, 64), (1000, 132, 300, 1), (40, 260, 1000, 64)]
EDGES = [(70, 63, 40, 5), (70, 65, 40, 5), (70, 33, 40, 63), (70, 33, 40, 65), (31, 40, 33, 5), (33, 40, 31, 5), (50, 40, 1, 5),
         (200, 40, 55, 5), (200, 40, 57, 5)]
SEAM = [(250, 33, 20, 5), (160, 33, 110, 5), (256, 33, 20, 5)]
ONE_SIDED = [(67, 33, 0, 5), (0, 64, 40, 1)]
LAYER_CASES = TABLE + EDGES + SEAM + ONE_SIDED
# (s_lo, damp) variants run on every case
VARIANTS = [(1.0, 0.0), (2.0, 0.5)]

# stacks of the composition tests: (sizes, B)
STACKS = [((65, 33, 31), 1), ((65, 33, 31), 65), ((67, 64, 33, 5), 1), ((67, 64, 33, 5), 65)]

# enumerable models of the CPU tests: (sizes, weight scale)
SMALL = [((8, 6, 4), 0.3), ((8, 6, 4), 1.0), ((6, 5, 4, 3), 0.5), ((6, 5, 4, 3), 1.5)]
SMALL_SEEDS = (0, 1, 2)

LR, MOM, WEIGHT_DECAY = 0.05, 0.5, 2e-4


def layer_case(K_lo, N, K_hi, B, binary=False, seed=None):
    """dict(W_lo [K_lo, N] or None, W_hi [N, K_hi] or None, x_lo, x_hi, bias, m, u)."""
    seed = 4000 + 7 * K_lo + 3 * N + 11 * K_hi + B + (100000 if binary else 0) if seed is None else seed
    g = np.random.default_rng(seed)
    ops = (lambda s: (g.random(s) < 0.4).astype(F32)) if binary else (lambda s: (0.05 + 0.9 * g.random(s)).astype(F32))
    k = dict(K_lo=K_lo, N=N, K_hi=K_hi, B=B, W_lo=None, W_hi=None, x_lo=None, x_hi=None)
    if K_lo:
        k["W_lo"] = (g.standard_normal((K_lo, N)) / np.sqrt(K_lo)).astype(F32)
        k["x_lo"] = ops((B, K_lo))
    if K_hi:
        k["W_hi"] = (g.standard_normal((N, K_hi)) / np.sqrt(K_hi)).astype(F32)
        k["x_hi"] = ops((B, K_hi))
    k["bias"] = (g.standard_normal(N) * 0.5).astype(F32)
    k["m"] = (0.05 + 0.9 * g.random((B, N))).astype(F32)
    k["u"] = g.random((B, N)).astype(F32)
    return k


def model(sizes, scale=None, seed=0):
    """(Ws, bs): W_l ~ N(0, scale^2) (default 1 / sqrt(N_l)), b_0 ~ N(-1, 0.5^2), b_l ~ N(0, 0.5^2)."""
    g = np.random.default_rng(seed)
    Ws = [(g.standard_normal((a, b)) * (scale if scale is not None else 1.0 / np.sqrt(a))).astype(F32) for a, b in zip(sizes[:-1], sizes[1:])]
    bs = [(g.standard_normal(n) * 0.5 - (1.0 if l == 0 else 0.0)).astype(F32) for l, n in enumerate(sizes)]
    return Ws, bs


def stack_case(sizes, B, seed=None):
    """dict(Ws, bs, data 0/1 [B, N_0], particles: L + 1 0/1 tensors)."""
    seed = 9000 + sum((i + 1) * n for i, n in enumerate(sizes)) + B if seed is None else seed
    Ws, bs = model(sizes, None, seed)
    g = np.random.default_rng(seed + 1)
    data = (g.random((B, sizes[0])) < 0.3).astype(F32)
    particles = [(g.random((B, n)) < 0.5).astype(F32) for n in sizes]
    return dict(sizes=tuple(sizes), B=B, Ws=Ws, bs=bs, data=data, particles=particles, seed=seed)


class Tape:
    """A replay provider: uniforms from one numpy generator, in call order."""

    def __init__(self, seed):
        self.g = np.random.default_rng(seed)
        self.shapes = []

    def uniform(self, shape):
        self.shapes.append(tuple(shape))
        return self.g.random(shape).astype(F32)

    def normal(self, shape):
        raise AssertionError("a DBM draws no normals")

    def categorical(self, probs):
        raise AssertionError("a DBM draws no categoricals")


# ---- the composition tests: sweeps, step settings ---------------------------------------------------------------------------------
GIBBS_SWEEPS = 2
STEP_N_MF, STEP_DAMP, STEP_GIBBS_K = 3, 0.25, 2
STEP_SCALARS = [(0.05, 0.5), (0.04, 0.5), (0.03, 0.5)]
STEP_MARGIN = 1e-5

# Replay seeds, each the first of its search range at which no uniform of the case lies within the derived bound of its float64
# probability (tests/test_dbm_cpu.py asserts the margin for every entry, so a changed table cannot bring in a tie unnoticed).
# SAMPLE_SEEDS: the seed of layer_case(..., binary=True); GIBBS_SEEDS: the Tape of dbm_gibbs (free and clamped); STEP_SEEDS: the
# Tapes of two consecutive dbm_step calls.
SAMPLE_SEEDS = {(67, 33, 21, 5): 104804, (128, 64, 64, 64): 105856, (1000, 132, 300, 1): 114697, (40, 260, 1000, 64): 116589,
                (70, 63, 40, 5): 105124, (70, 65, 40, 5): 105130, (70, 33, 40, 63): 105092, (70, 33, 40, 65): 105094,
                (31, 40, 33, 5): 104705, (33, 40, 31, 5): 104697, (50, 40, 1, 5): 104486, (200, 40, 55, 5): 106130,
                (200, 40, 57, 5): 106152, (250, 33, 20, 5): 106074, (160, 33, 110, 5): 106434, (256, 33, 20, 5): 106116,
                (67, 33, 0, 5): 104573, (0, 64, 40, 1): 104633}
GIBBS_SEEDS = {((65, 33, 31), 1): 100, ((65, 33, 31), 65): 100, ((67, 64, 33, 5), 1): 100, ((67, 64, 33, 5), 65): 100}
STEP_SEEDS = {((65, 33, 31), 1): (300, 1300), ((65, 33, 31), 65): (300, 1301), ((67, 64, 33, 5), 1): (300, 1300),
              ((67, 64, 33, 5), 65): (301, 1300)}
