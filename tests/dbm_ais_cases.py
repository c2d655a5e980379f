"""Cases of the DBM density tests (tests/test_dbm_ais_cpu.py, tests/test_dbm_ais_gpu.py).  The operands, models and
tapes are those of tests/dbm_cases.py.

Layer cases are (K_lo, N, K_hi, B) at the edges of the block of kernels_dbm.hpp (DBM_TN = DBM_BM = 64, DBM_KC = 32, the shortest K
slice 128 steps; on 256 CUs):
  (31, 1, 33, 1)        one unit, one row, both sides shorter / longer than a stage
  (33, 63, 31, 16)      one wave's rows, N one below the tile
  (128, 64, 128, 17)    two slices of 128 steps: the seam is the slice edge
  (257, 65, 31, 65)     two tiles, two chunks; slices [0, 160) and [160, 288): the seam at 257 inside the second
  (128, 130, 257, 17)   three tiles; slices [0, 160), [160, 320), [320, 385): the seam at 128 inside the first
  (33, 130, 128, 65)    one slice of 161 steps over three tiles and two chunks
  (257, 130, 0, 65), (31, 63, 0, 17)     one-sided from below (the form of the bound)
  (0, 65, 257, 16), (0, 64, 33, 1)       one-sided from above (layer 0 of the annealing run)
"""
import numpy as np

import dbm_cases as Ck

F32 = np.float32

LAYER_CASES = [(31, 1, 33, 1), (33, 63, 31, 16), (128, 64, 128, 17), (257, 65, 31, 65), (128, 130, 257, 17), (33, 130, 128, 65),
               (257, 130, 0, 65), (31, 63, 0, 17), (0, 65, 257, 16), (0, 64, 33, 1)]
BOUND_CASES = [c for c in LAYER_CASES if c[0] > 0]          # run from below only: the hi side of a two-sided case is left out
BETA, BETA_PREV, DBETA_NEXT = 0.625, 0.37, 0.125

# whole runs: the stacks of dbm_cases with M chains in place of B rows, K temperatures that are no even ladder
STACKS = Ck.STACKS
AIS_K = 6
AIS_BETAS = np.array([0.0, 0.05, 0.2, 0.45, 0.7, 0.9, 1.0], F32)

# enumerable models of the CPU tests: (sizes, weight scale, with a base-rate bias)
SMALL = [((8, 6, 4), 0.5, False), ((6, 5, 4, 3), 0.5, True), ((8, 5), 0.5, False)]
SMALL_K, SMALL_M = 200, 64
SMALL_SEED_RANGE = range(1, 9)
# the pinned Tape seed per model.  Seeds 1 .. 8 were tried: the twin's error in standard errors was, per model in the order above,
# -0.04 -0.94 -1.53 0.03 1.42 1.20 0.16 0.94 / 0.90 0.49 -1.67 2.63 0.07 0.26 0.63 0.53 / -0.04 1.23 -0.49 -0.55 -1.32 0.24 0.75 0.34
SMALL_SEEDS = {(8, 6, 4): 1, (6, 5, 4, 3): 1, (8, 5): 1}

# Replay seeds, each the first of its search range at which no uniform of the case lies within the derived bound of its float64
# probability (tests/test_dbm_ais_cpu.py asserts the margin for every entry).  SAMPLE_SEEDS: the seed of layer_case(..., binary=True);
# AIS_SEEDS: the Tape of the whole run.
SAMPLE_SEEDS = {(31, 1, 33, 1): 200000, (33, 63, 31, 16): 200100, (128, 64, 128, 17): 200200, (257, 65, 31, 65): 200300,
                (128, 130, 257, 17): 200400, (33, 130, 128, 65): 200501, (257, 130, 0, 65): 200600, (31, 63, 0, 17): 200700,
                (0, 65, 257, 16): 200800, (0, 64, 33, 1): 200900}
AIS_SEEDS = {((65, 33, 31), 1): 500, ((65, 33, 31), 65): 500, ((67, 64, 33, 5), 1): 500, ((67, 64, 33, 5), 65): 501}


def layer_case(case):
    """dbm_cases.layer_case on 0/1 operands plus ``base`` [N], ``base_lo`` [K_lo] and magnetisations ``mu`` [B, N]."""
    k = Ck.layer_case(*case, binary=True, seed=SAMPLE_SEEDS[case])
    g = np.random.default_rng(SAMPLE_SEEDS[case] + 1)
    k["base"] = (g.standard_normal(case[1]) * 0.7).astype(F32)
    k["base_lo"] = (g.standard_normal(case[0]) * 0.7).astype(F32) if case[0] else None
    k["mu"] = k["m"]
    k["mu"][0, 0], k["mu"][-1, -1] = 0.0, 1.0                # h(0) = h(1) = 0
    return k


def small_model(sizes, scale):
    """(Ws, bs, base): the model of dbm_cases and a base-rate bias near its layer-0 bias."""
    Ws, bs = Ck.model(sizes, scale, 0)
    return Ws, bs, (bs[0] * F32(0.8)).astype(F32)


def ais_case(sizes, M):
    """(Ws, bs, base) of a whole run: the model of dbm_cases.stack_case and a base-rate bias."""
    k = Ck.stack_case(sizes, M)
    g = np.random.default_rng(k["seed"] + 2)
    return k["Ws"], k["bs"], (g.standard_normal(sizes[0]) * 0.5 - 1.0).astype(F32)
