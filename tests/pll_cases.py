"""Shapes and seeds of the pseudo-log-likelihood tests, shared by tests/test_pll_cpu.py and tests/test_pll_gpu.py.

(V, H, N) cross the edges of the site kernel (kernels_pll.hpp: 16 visible columns x 64 rows per block, hidden units in chunks of
128) and of the propagation that feeds it."""
import numpy as np

from anneal_cases import params, start_rows

F32 = np.float32

# name -> (V, H, N, groups)
CASES = {
    "odd": (70, 33, 5, ()),                        # no dimension on a tile boundary
    "rows67": (130, 200, 67, ()),                  # two row tiles, two j chunks (128 + 72)
    "wide": (1100, 96, 3, ()),                     # V > 1024: the logits come from the streaming route
    "one_tile": (64, 64, 1, ()),                   # whole tiles only, a single row
    "group_end": (47, 24, 9, ((40, 47),)),         # a group ending at V
    "two_groups": (60, 40, 6, ((10, 13), (50, 60))),
    "k65": (90, 12, 5, ((25, 90),)),               # K = 65 labels: lane 0 of pll_rows_finish takes j = 0 and 64; the ones are counted in two trips
    "k256": (280, 12, 5, ((24, 280),)),            # K = 256, the widest group: four trips of every 64-lane loop
    "four": (150, 12, 6, ((0, 5), (60, 133), (133, 140), (147, 150))),      # four groups: one at column 0, two sharing a boundary, one ending at V
}
SCALES = (0.1, 1.0)
TILE_COLS, TILE_ROWS, CHUNK = 16, 64, 128


def case(name, scale):
    """dict(V, H, N, groups, W, b, c, v): fp32 parameters at weight scale `scale`, 0/1 rows with one-hot groups."""
    V, H, N, groups = CASES[name]
    idx = list(CASES).index(name)
    W, b, c, _ = params(V, H, 700 + 10 * idx + (1 if scale >= 1.0 else 0), scale)
    groups = [tuple(g) for g in groups]
    return dict(name=name, scale=scale, V=V, H=H, N=N, groups=groups, W=W, b=b, c=c, v=start_rows(N, V, 40 + idx, groups))


def n_sites(c):
    return c["V"] - sum(e - s for s, e in c["groups"]) + len(c["groups"])


def site_tol(c, want):
    """The label-side convention (a sum of H softplus terms on the same logits): H 1e-5 + 1e-9 |value| per site."""
    return c["H"] * 1e-5 + 1e-9 * np.abs(want)


def total_tol(c, want):
    return n_sites(c) * c["H"] * 1e-5 + 1e-9 * np.abs(want)


def check_columns(c):
    """8 columns outside the groups: the first, the last, both sides of the first tile edge, the rest spread over the layer."""
    free = [i for i in range(c["V"]) if not any(s <= i < e for s, e in c["groups"])]
    cols = {free[0], free[-1]} | ({TILE_COLS - 1, TILE_COLS} & set(free))
    for i in (free[(k * len(free)) // 7] for k in range(1, 7)):
        if len(cols) < 8:
            cols.add(i)
    return sorted(cols)
