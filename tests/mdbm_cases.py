"""Cases of the multimodal DBM tests (tests/test_mdbm_cpu.py, tests/test_mdbm_gpu.py).

Group-layer cases are (ends, K_lo, K_hi, B): the N = ends[-1] units in len(ends) softmax groups ending at ``ends``.  Weights ~ N(0, 1 / K)
of their own side, biases ~ N(0, 0.5^2), operands uniform in (0.05, 0.95) or 0 / 1, all from ``numpy.random.default_rng(seed)``.

What the shapes sit next to (kernels_dbm.hpp, kernels_dbm_group.hpp):
  a lane holds the columns l, l + 64, l + 128, l + 192 of a group  -> widths 2, 3, 32, 63 / 64 / 65 (one slot / the second), 256 (all four)
  DBM_TN = 64 units per tile of the layer block                       -> 33 + 31 (a group across nothing, ending on the tile edge),
                                                                         64 + 2 + 65 + 256 (groups across one and across four tile edges)
  ROW_WAVES = 4 rows per block of the finish, DBM_BM = 64 rows per chunk of the block  -> B 1, 16, 17, 65
  DBM_KC = 32 steps per stage, 4 DBM_KC = 128 the shortest K slice    -> K_hi 31 / 33, 128 (one slice), 257 (slices of 160 and 97 steps)
  the seam: (250, 20) runs as the slices [0, 160) and [160, 270), the second holding the seam at 250 (tests/dbm_cases.py).
"""
import numpy as np

import dbm_cases as Dk

F32 = np.float32

WIDE = (64, 66, 131, 387)                        # 64 + 2 + 65 + 256
GROUP_CASES = [((2,), 0, 31, 1), ((3,), 0, 33, 16), ((32,), 0, 128, 17), ((63,), 0, 257, 17), ((64,), 0, 31, 65), ((65,), 0, 33, 65),
               ((256,), 0, 257, 1), ((256,), 0, 128, 16), ((33, 64), 0, 33, 17), ((33, 64), 0, 257, 65), (WIDE, 0, 31, 65),
               (WIDE, 0, 257, 1), ((33, 64), 250, 20, 5)]
DAMPS = [0.0, 0.5]


def group_case(ends, K_lo, K_hi, B, binary=False, seed=None):
    """dict(W_lo [K_lo, N] or None, W_hi [N, K_hi] or None, x_lo, x_hi, bias, m)."""
    N = ends[-1]
    seed = 7000 + 13 * sum(ends) + 7 * K_lo + 11 * K_hi + B + (100000 if binary else 0) if seed is None else seed
    g = np.random.default_rng(seed)
    ops = (lambda s: (g.random(s) < 0.4).astype(F32)) if binary else (lambda s: (0.05 + 0.9 * g.random(s)).astype(F32))
    k = dict(ends=tuple(ends), K_lo=K_lo, N=N, K_hi=K_hi, B=B, W_lo=None, W_hi=None, x_lo=None, x_hi=None)
    if K_lo:
        k["W_lo"] = (g.standard_normal((K_lo, N)) / np.sqrt(K_lo)).astype(F32)
        k["x_lo"] = ops((B, K_lo))
    if K_hi:
        k["W_hi"] = (g.standard_normal((N, K_hi)) / np.sqrt(K_hi)).astype(F32)
        k["x_hi"] = ops((B, K_hi))
    k["bias"] = (g.standard_normal(N) * 0.5).astype(F32)
    k["m"] = (0.05 + 0.9 * g.random((B, N))).astype(F32)
    return k


# Philox seeds of the sample tests, each the first of 1000, 1001, .. at which every pick of the case (rng offset 0, row0 0) is further
# from its neighbouring cumulative sums than ``mdbm_oracle.pick_bound`` (tests/test_mdbm_cpu.py asserts the margin for every entry).
# 99 seeds were tried for the 13 cases.
PICK_SEEDS = dict(zip(GROUP_CASES, (1000, 1000, 1000, 1000, 1001, 1000, 1001, 1007, 1000, 1061, 1015, 1000, 1001)))

# ---- the compositions ----------------------------------------------------------------------------------------------------------------
# (image sizes, K, J, B)
STACKS = [((65, 33), 5, 31, 1), ((65, 33), 5, 31, 65), ((67, 64, 33), 32, 5, 1), ((67, 64, 33), 32, 5, 65)]
# enumerable models of the CPU tests: (image sizes, K, J, weight scale)
SMALL = [((6, 4), 3, 4, 0.5), ((6, 4), 3, 4, 1.2), ((6, 5, 4), 4, 3, 0.5), ((6, 5, 4), 4, 3, 1.2)]
SMALL_SEEDS = (0, 1, 2)

LR, MOM, WEIGHT_DECAY = Dk.LR, Dk.MOM, Dk.WEIGHT_DECAY
GIBBS_SWEEPS = 2
STEP_N_MF, STEP_DAMP, STEP_GIBBS_K = 3, 0.25, 2
STEP_SCALARS = [(0.05, 0.5), (0.04, 0.5), (0.03, 0.5)]
STEP_MARGIN = Dk.STEP_MARGIN


def model(sizes, K, J, scale=None, seed=0):
    """(Ws, WJ, bs): W ~ N(0, scale^2) (default 1 / sqrt(fan-in)), b_0 ~ N(-1, 0.5^2), the other biases ~ N(0, 0.5^2)."""
    g = np.random.default_rng(seed)
    sd = lambda a: scale if scale is not None else 1.0 / np.sqrt(a)
    Ws = [(g.standard_normal((a, b)) * sd(a)).astype(F32) for a, b in zip(sizes[:-1], sizes[1:])]
    WJ = (g.standard_normal((sizes[-1] + K, J)) * sd(sizes[-1] + K)).astype(F32)
    bs = [(g.standard_normal(n) * 0.5 - (1.0 if l == 0 else 0.0)).astype(F32) for l, n in enumerate(list(sizes) + [J, K])]
    return Ws, WJ, bs


def stack_case(sizes, K, J, B, seed=None):
    """dict(Ws, WJ, bs, data 0/1 [B, N_0], labels [B] and their one-hot rows y, particles [s_0 .. s_{L-1}, zy, s_J])."""
    seed = 9500 + sum((i + 1) * n for i, n in enumerate(sizes)) + 3 * K + 5 * J + B if seed is None else seed
    Ws, WJ, bs = model(sizes, K, J, None, seed)
    g = np.random.default_rng(seed + 1)
    data = (g.random((B, sizes[0])) < 0.3).astype(F32)
    labels = g.integers(0, K, B)
    y = np.eye(K, dtype=F32)[labels]
    particles = [(g.random((B, n)) < 0.5).astype(F32) for n in sizes[:-1]]
    particles.append(np.concatenate([(g.random((B, sizes[-1])) < 0.5).astype(F32), np.eye(K, dtype=F32)[g.integers(0, K, B)]], 1))
    particles.append((g.random((B, J)) < 0.5).astype(F32))
    return dict(sizes=tuple(sizes), K=K, J=J, B=B, Ws=Ws, WJ=WJ, bs=bs, data=data, labels=labels, y=y, particles=particles, seed=seed)


class Tape(Dk.Tape):
    """``dbm_cases.Tape`` plus categorical indices, uniform over the width, from the same generator in call order."""

    def categorical(self, probs):
        self.shapes.append(("c",) + tuple(probs.shape))
        return self.g.integers(0, probs.shape[1], probs.shape[0])


def draws_of(shapes):
    """The schedule a Tape saw: [("u", N) | ("c", width)]."""
    return [("c", s[2]) if s[0] == "c" else ("u", s[1]) for s in shapes]


# Replay seeds, each the first of its search range at which no uniform of a sigmoid layer lies within the derived bound of its float64
# probability (tests/test_mdbm_cpu.py asserts the margin for every entry).  GIBBS_SEEDS: the Tape of mdbm_gibbs (free and clamped);
# STEP_SEEDS: the Tapes of two consecutive mdbm_step calls.
# 4 Gibbs seeds and 18 step seeds were tried for the 4 stacks.
GIBBS_SEEDS = {c: 100 for c in STACKS}
STEP_SEEDS = {c: (308, 1302) if c == ((67, 64, 33), 32, 5, 65) else (300, 1300) for c in STACKS}
