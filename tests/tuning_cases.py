"""The shared case table of the unit-moments tests (tests/test_unit_tuning_gpu.py, tests/test_unit_tuning_cpu.py).

Shapes: every value of B in {1, 5, 64, 65, 300, 4099}, H in {1, 63, 64, 65, 200, 1500}, K in {0 (no cls), 1, 2, 33, 256, 1024} and
R in {0, 1, 3, 8} appears, crossed sparingly.  What each shape is for: 64 / 65 columns and rows are the tile and wave edges; B = 300
and 4099 with K <= 2 give classes of more than 256 rows (several segments per class); K = 1024 is the scan's full width; H = 1500 is
the headline layer; R = 8 is the widest regression."""
import numpy as np

#          B     H     K     R
SHAPES = [(1,    1,    0,    0),
          (5,    63,   1,    1),
          (64,   64,   2,    3),
          (65,   65,   33,   8),
          (300,  200,  256,  1),
          (300,  1,    1,    3),
          (4099, 63,   0,    8),
          (4099, 200,  2,    3),
          (4099, 1500, 33,   1),
          (4099, 64,   1024, 0),
          (65,   1500, 1024, 8)]

# class layouts (need K >= 1) and row layouts, each run at one mid-sized shape
LAYOUT_SHAPE = (300, 65, 33, 3)
LAYOUTS = ("one_class", "empty_classes", "descending", "skip_one", "skip_all", "nan_regressor")


def make(B, H, K, R, layout="uniform", exact=True, seed=0):
    """(act [B, H] fp32, cls [B] int32 or None, x [B, R] fp32 or None).  ``exact``: activations in {0, 1} and regressors that are small
    integers, so that every sum is an integer below 2^53 whatever its order; otherwise uniform activations and Gaussian regressors."""
    g = np.random.default_rng([seed, B, H, K, R])
    if exact:
        act = (g.random((B, H)) < 0.4).astype(np.float32)
        x = g.integers(-3, 4, size=(B, R)).astype(np.float32) if R else None
    else:
        act = g.random((B, H), dtype=np.float32)
        x = g.standard_normal((B, R)).astype(np.float32) if R else None
    cls = g.integers(0, K, size=B).astype(np.int32) if K else None
    if layout == "one_class":
        cls[:] = K - 1
    elif layout == "empty_classes":
        cls = (cls // 2 * 2).astype(np.int32)                         # odd classes stay empty
    elif layout == "descending":
        cls = np.sort(cls)[::-1].copy()
    elif layout == "skip_one":
        cls[B // 2] = K
    elif layout == "skip_all":
        cls[:] = -1
    elif layout == "nan_regressor":
        x[3, R - 1] = np.nan; x[B - 1, 0] = np.inf
    else:
        assert layout == "uniform", layout
    return act, cls, x
