"""Cases shared by the annealing and iMDBN-bound tests (CPU and GPU): parameters from fixed generators, temperature ladders, start
rows, pinned seeds.

The Philox seeds are pinned on the CPU from the twins alone (tests/anneal_oracle.py, tests/bound_oracle.py).  The TRUTH seeds are ones
at which the twin's estimates lie within 3 of its own standard errors of the enumerated values, with and without a base-rate bias (the
test docstrings state what the seeds 1..8 gave).  Every FORWARD / GROUPS / REVERSE / PATH seed is one whose smallest Bernoulli margin
|p - u| outside the softmax groups in the twin is at least MARGIN and whose smallest categorical-CDF margin is at least MARGIN
(forward; in GROUPS the first such seed, counting from 1) or CAT_MARGIN (reverse), so the device (fp32 sigmoid and softmax, another
summation order in the logits) must take every decision as the twin does.  The `four256` rows (four groups, one 256 wide) also keep
FOUR256_CAT_MARGIN at their categorical picks.  `python tests/anneal_cases.py` prints, for every case, the first seed that meets the
margins next to the pinned one."""
from dataclasses import dataclass

import numpy as np

F32 = np.float32
MARGIN = 1e-5
CAT_MARGIN = 1e-6
REPLAY_SEED = 11
REPLAY_CASE = "tiny_bA"


def params(V, H, gen_seed, w_scale, bias_scale=0.5):
    """(W [V, H], b [V], c [H], b_A [V]) fp32 from one fixed generator."""
    g = np.random.Generator(np.random.PCG64(gen_seed))
    W = (g.standard_normal((V, H)) * w_scale).astype(F32)
    b = (g.standard_normal(V) * bias_scale).astype(F32)
    c = (g.standard_normal(H) * bias_scale).astype(F32)
    bA = (g.standard_normal(V) * bias_scale).astype(F32)
    return W, b, c, bA


def linear(K):
    return (np.arange(K + 1, dtype=np.float64) / K).astype(F32)


def uneven(K):
    """Non-uniform ladder: dense near 0, where the base-rate model hands over (beta_k = (k / K)^2)."""
    return ((np.arange(K + 1, dtype=np.float64) / K) ** 2).astype(F32)


def start_rows(R, V, seed, groups=(), p=0.5):
    """R start states [R, V] fp32 0/1 from one fixed generator; every group holds exactly one 1."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = (g.random((R, V)) < p).astype(F32)
    for s, e in groups:
        x[:, s:e] = 0.0
        x[np.arange(R), s + g.integers(0, e - s, R)] = 1.0
    return x


# ---- parity with the twin ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Row:
    V: int
    H: int
    n: int                      # M chains from the base-rate model, or R start rows (REVERSE)
    K: int
    w_scale: float
    with_bA: bool
    ladder: str                 # "linear" | "uneven"
    seed: int                   # the pinned Philox seed
    groups: tuple = ()
    pitch: int = None           # weight rows that many floats apart (None: the constructor's)
    gen_seed: int = None        # of the parameters (None: 100 + V)


FOUR256 = ((0, 5), (20, 276), (276, 290), (299, 300))
# what a pinned seed of a four256 row keeps at its categorical picks besides the table's own margin: group_cases.cat_margin(256),
# the distance two fp32 cumulative sums over 256 softmax probabilities can lie apart, rounded up
FOUR256_CAT_MARGIN = 2.5e-5


def _g(V, H, *rest, **kw):
    """A GROUPS row: its parameters come from the generator 500 + V + H."""
    return Row(V, H, *rest, gen_seed=500 + V + H, **kw)


# (V, H, M, K) cross the kernel's edges -- one partial ballot; H no multiple of 64 and M no multiple of the rows per block; V > 1024
# (streaming / bit-plane routes), H across 256, weight rows of 300 floats behind an unaligned base pitch
FORWARD = {
    "tiny": Row(20, 12, 5, 6, 1.0, False, "linear", 1),
    "tiny_bA": Row(20, 12, 5, 6, 1.0, True, "uneven", 1),
    "mid": Row(300, 70, 7, 5, 0.1, False, "uneven", 2),
    "mid_bA": Row(300, 70, 7, 5, 0.1, True, "linear", 1),
    "wide": Row(1100, 300, 5, 4, 0.05, False, "linear", 1),
    "wide_bA": Row(1100, 300, 5, 4, 0.05, True, "uneven", 1),
}

# imdbn_rbm_ais_groups
GROUPS = {
    "odd": _g(20, 12, 5, 3, 1.0, True, "uneven", 1, groups=((15, 20),)),                 # group at an odd offset, rows no multiple of 4
    "two": _g(70, 33, 70, 3, 0.3, True, "linear", 1, groups=((3, 9), (60, 70)), pitch=37),  # two groups, one across column 64; rows across a 64-row block
    "k1": _g(20, 12, 5, 1, 1.0, True, "linear", 1, groups=((15, 20),)),                  # no transition
    "plain": _g(20, 12, 5, 3, 1.0, True, "uneven", 1),                                   # n_groups = 0: imdbn_rbm_ais bit for bit
    "paper": _g(532, 256, 64, 5, 0.05, True, "linear", 14, groups=((500, 532),)),        # the paper's joint shape
    "wide": _g(1100, 40, 8, 2, 0.05, False, "linear", 2, groups=((1092, 1100),)),        # the split-K up route
    # four groups (pick[q] for q = 2, 3): one at column 0, a 256-wide one across columns 64, 128 and 256 next to its neighbour, a
    # width-1 group at the last column.  Its seed is the first whose categorical margin is also >= FOUR256_CAT_MARGIN
    "four256": _g(300, 12, 5, 3, 0.1, True, "linear", 3, groups=FOUR256),
}

# as FORWARD with R start rows in the place of M chains; one softmax group; K = 1; R = 70 (two 64-row chunks)
REVERSE = {
    "tiny": Row(20, 12, 5, 6, 1.0, False, "linear", 1),
    "tiny_bA": Row(20, 12, 5, 6, 1.0, True, "uneven", 1),
    "mid": Row(300, 70, 7, 5, 0.1, False, "uneven", 1),
    "mid_bA": Row(300, 70, 7, 5, 0.1, True, "linear", 1),
    "wide": Row(1100, 300, 5, 4, 0.05, False, "linear", 2),
    "wide_bA": Row(1100, 300, 5, 4, 0.05, True, "uneven", 2),
    "group": Row(25, 12, 6, 5, 1.0, True, "linear", 1, groups=((20, 25),)),
    "one": Row(20, 12, 5, 1, 1.0, True, "linear", 1),
    "rows70": Row(20, 12, 70, 6, 1.0, True, "uneven", 2),
    "four256": Row(300, 12, 6, 3, 0.1, True, "linear", 1, groups=FOUR256),                # as GROUPS["four256"]: the one of the wide group is found by lanes striding 64
}


def case(table, name):
    """A row of FORWARD / GROUPS / REVERSE as the dict the tests read: the parameters, the ladder, ``M`` chains or (REVERSE) ``R``
    start rows ``x``."""
    r = table[name]
    W, b, c, bA = params(r.V, r.H, 100 + r.V if r.gen_seed is None else r.gen_seed, r.w_scale)
    out = dict(V=r.V, H=r.H, K=r.K, W=W, b=b, c=c, bA=bA if r.with_bA else None, betas={"linear": linear, "uneven": uneven}[r.ladder](r.K),
               seed=r.seed, groups=list(r.groups), pitch=r.pitch)
    if table is REVERSE:
        return dict(out, R=r.n, x=start_rows(r.n, r.V, 300 + r.V + r.n, r.groups))
    return dict(out, M=r.n)


# ---- against the truth.  W ~ N(0, 1), biases ~ N(0, 0.5), linear temperatures
# forward: V = 20, H = 12, K = 200, M = 64 chains; groups: the same with 16 Bernoulli columns + one group of 4;
# reverse: V = 10, H = 6, K = 20, N = 4 rows drawn from the enumerated annealing model x M = 256 chains
FORWARD_TRUTH = dict(V=20, H=12, K=200, M=64, gen_seed=2024, w_scale=1.0)
GROUPS_TRUTH = dict(V=20, H=12, K=200, M=64, gen_seed=2025, w_scale=1.0, groups=[(16, 20)])
REVERSE_TRUTH = dict(V=10, H=6, K=20, N=4, M=256, gen_seed=2024, w_scale=1.0, row_seed=5)
TRUTH_SEED = 1


def _truth(t, with_bA, **more):
    W, b, c, bA = params(t["V"], t["H"], t["gen_seed"], t["w_scale"])
    return dict(V=t["V"], H=t["H"], M=t["M"], K=t["K"], W=W, b=b, c=c, bA=bA if with_bA else None, betas=linear(t["K"]), seed=TRUTH_SEED,
                **more)


def forward_truth(with_bA):
    return _truth(FORWARD_TRUTH, with_bA)


def groups_truth(with_bA):
    return _truth(GROUPS_TRUTH, with_bA, groups=list(GROUPS_TRUTH["groups"]))


def reverse_truth(with_bA):
    return _truth(REVERSE_TRUTH, with_bA, N=REVERSE_TRUTH["N"])


def truth_rows(log_p, states):
    """REVERSE_TRUTH["N"] rows drawn from the enumerated annealing model (inverse CDF over the state index), and their log p_ann."""
    g = np.random.Generator(np.random.PCG64(REVERSE_TRUTH["row_seed"]))
    idx = np.searchsorted(np.cumsum(np.exp(log_p)), g.random(REVERSE_TRUTH["N"]))
    idx = np.minimum(idx, states.shape[0] - 1)
    return states[idx].astype(F32), log_p[idx]


# ---- imdbn_rbm_label_loglik.  name -> (Dz, K, H, extra visible columns behind the labels, w_scale, labels of the rows 0, 2, 3, 4 or
# None: drawn like the rest).  "slots": K = 130 fills two label slots of the kernel and two lanes of a third; the first and last label
# of every slot are somebody's truth (row 1 is left out: the test gives it a label out of range)
LABEL = {"small": (12, 3, 7, 0, 0.5, None), "paper": (500, 32, 256, 0, 0.05, None), "slots": (20, 130, 70, 0, 0.2, (0, 63, 64, 129))}


def label_case(name, N, real, gen_seed=0):
    """A joint RBM [Dz | K] x H and N code rows (0/1, or uniform in [0, 1)), labels in [0, K)."""
    Dz, K, H, extra, ws, first = LABEL[name]
    W, b, c, _ = params(Dz + K + extra, H, 700 + Dz, ws)
    g = np.random.Generator(np.random.PCG64(800 + N + gen_seed))
    u = g.random((N, Dz))
    z = u.astype(F32) if real else (u > 0.5).astype(F32)
    gt = g.integers(0, K, N).astype(np.int32)
    if first is not None:
        gt[[0, 2, 3, 4]] = first
    return dict(Dz=Dz, K=K, H=H, W=W, b=b, c=c, z=z, gt=gt)


# ---- a tiny iMDBN for enumeration: image stack 8-5-4, joint RBM (4 + 3) <-> 4, W ~ N(0, 0.5)
TINY = dict(sizes=(8, 5, 4), K=3, HJ=4, w_scale=0.5, gen_seed=61)
TINY_TRUTH = dict(B=6, S_entropy=256, S_logq=2048, in_seed=9)
TINY_SEED = 1

# ---- the whole path on the device against the twin: image stack 100-40-20, joint RBM (20 + 4) <-> 16
PATH = dict(sizes=(100, 40, 20), K=4, HJ=16, w_scale=0.2, gen_seed=62, B=5, S=3, in_seed=10)
PATH_SEED = 1


def imdbn(spec):
    """([(W, b, c)] image layers bottom first, (Wj, bj, cj) joint RBM over [z | y])."""
    sizes, gs, ws = spec["sizes"], spec["gen_seed"], spec["w_scale"]
    layers = [params(sizes[l], sizes[l + 1], gs * 10 + l, ws)[:3] for l in range(len(sizes) - 1)]
    return layers, params(sizes[-1] + spec["K"], spec["HJ"], gs * 10 + 9, ws)[:3]


def inputs(B, V, K, gen_seed):
    """B rows of 0/1 images and labels in [0, K)."""
    g = np.random.Generator(np.random.PCG64(gen_seed))
    return (g.random((B, V)) > 0.5).astype(F32), g.integers(0, K, B).astype(np.int64)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import anneal_oracle as A
    from oracle.draws import PhiloxStream
    for what, table, cat in (("FORWARD", FORWARD, MARGIN), ("GROUPS", GROUPS, MARGIN), ("REVERSE", REVERSE, CAT_MARGIN)):
        for name in table:
            c = case(table, name)
            for seed in range(1, 33):
                if table is REVERSE:
                    m, cm = A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], c["groups"], c["betas"], c["x"], PhiloxStream(seed))[2:]
                else:
                    m, cm = A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], c["M"], PhiloxStream(seed), c["groups"])[2:]
                if m >= MARGIN and cm >= (max(cat, FOUR256_CAT_MARGIN) if name == "four256" else cat):
                    break
            print(f"{what} {name}: first seed {seed} (pinned {c['seed']}), margins {m:.3g} / {cm:.3g}")
