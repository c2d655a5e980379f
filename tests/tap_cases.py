"""Cases of the TAP tests (tests/test_tap_cpu.py, tests/test_tap_gpu.py).

Weights: ``numpy.random.default_rng(seed)`` with W ~ N(0, s^2), a ~ N(0, 0.5^2) - 1, c ~ N(0, 0.5^2), drawn in that order.

Shape table, each at B in {1, 5, 64}: (67, 33) scalar paths, ragged everything; (128, 64); (1000, 132): K slices on both half-steps;
(260, 1028): more than one column tile of tap_apply (1024 columns with float4 rows) and of tap_outer (256).

The edges of kernels_tap.hpp, each with a shape one below / one above, at a batch of their own:
  TAP_TN = 64   output units per tile of tap_half             -> (63, 65): 63 visible / 65 hidden units, one tile and two
  TAP_KC = 32   reduction steps per stage                     -> (33, 31): one stage short by one / one stage and one step
  TAP_BM = 64   batch rows per chunk                          -> B = 65 (two chunks, the second with one row), B = 63
  4 TAP_KC = 128 steps: the shortest K slice                  -> (255, 257): the hidden half-step keeps K = 255 whole, the visible one
                                                                 splits K = 257 into two slices
  32 rows / 32 batch rows per block and chunk of tap_outer    -> covered by V = 33 / 31, B = 33
"""
import numpy as np

F32 = np.float32

SHAPES = [(67, 33), (128, 64), (1000, 132), (260, 1028)]
BATCHES = [1, 5, 64]
EDGES = [(63, 65, 65), (65, 63, 63), (33, 31, 33), (31, 33, 5), (255, 257, 5), (257, 255, 64)]       # (V, H, B)
TABLE = [(V, H, B) for V, H in SHAPES for B in BATCHES] + EDGES

# CPU test 3 / GPU test 5: the sixteen small models
SMALL = [(12, 7, 0.1), (12, 7, 0.3), (20, 10, 0.2), (16, 12, 0.5)]
SMALL_SEEDS = (0, 1, 2, 3)

LR, MOM, WEIGHT_DECAY, SPARSITY_TARGET = 0.05, 0.5, 2e-4, 0.1


def params(V, H, s, seed):
    g = np.random.default_rng(seed)
    W = (g.standard_normal((V, H)) * s).astype(F32)
    a = (g.standard_normal(V) * 0.5 - 1.0).astype(F32)
    c = (g.standard_normal(H) * 0.5).astype(F32)
    return W, a, c


def scale(V):
    """Weight scale of the shape table: 1 / sqrt(V), the constructor's law (pre-activations of order 1 at every size)."""
    return 1.0 / np.sqrt(V)


def case(V, H, B, seed=None):
    """dict(W, a, c, mv, mh, data): parameters, start magnetisations uniform in (0.05, 0.95), a 0/1 batch."""
    seed = 1000 + V * 7 + H * 3 + B if seed is None else seed
    W, a, c = params(V, H, scale(V), seed)
    g = np.random.default_rng(seed + 1)
    mv = (0.05 + 0.9 * g.random((B, V))).astype(F32)
    mh = (0.05 + 0.9 * g.random((B, H))).astype(F32)
    data = (g.random((B, V)) < 0.3).astype(F32)
    return dict(V=V, H=H, B=B, W=W, a=a, c=c, mv=mv, mh=mh, data=data)


def starts(n, V, seed):
    g = np.random.default_rng(seed)
    return 0.05 + 0.9 * g.random((n, V))
