"""Cases shared by test_reverse_ais_cpu.py and test_reverse_ais_gpu.py: parameters from the fixed generators of ais_cases.py, start
rows, temperature ladders, pinned seeds.

The Philox seeds are pinned on the CPU from the twin alone (tests/reverse_ais_oracle.py): TRUTH_SEED is one for which every row's
estimate lies within 3 of its own standard errors of the enumerated log p_ann(x), with and without a base-rate bias; every PARITY
case's seed is one whose smallest Bernoulli margin |p - u| in the twin is at least MARGIN and whose smallest categorical margin is at
least CAT_MARGIN, so the device (fp32 sigmoid, another summation order in the logits) must take every decision as the twin does."""
import numpy as np

from ais_cases import linear, params, uneven

F32 = np.float32
MARGIN = 1e-5
CAT_MARGIN = 1e-6
REPLAY_SEED = 11


def start_rows(R, V, seed, groups=(), p=0.5):
    """R start states [R, V] fp32 0/1 from one fixed generator; every group holds exactly one 1."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = (g.random((R, V)) < p).astype(F32)
    for s, e in groups:
        x[:, s:e] = 0.0
        x[np.arange(R), s + g.integers(0, e - s, R)] = 1.0
    return x


# ---- against the truth: V = 10, H = 6, W ~ N(0, 1), biases ~ N(0, 0.5), K = 20 linear temperatures, N = 4 rows x M = 256 chains
TRUTH = dict(V=10, H=6, K=20, N=4, M=256, gen_seed=2024, w_scale=1.0, row_seed=5)
TRUTH_SEED = 1

# ---- parity with the twin: (V, H, R, K) cross the kernel's edges -- one partial ballot; H no multiple of 64 and R no multiple of the
# rows per block; V > 1024 (streaming / bit-plane routes), H across 256; one softmax group; K = 1; R = 70 (two 64-row chunks)
# name -> (V, H, R, K, w_scale, with b_A, ladder, groups, seed)
PARITY = {
    "tiny": (20, 12, 5, 6, 1.0, False, "linear", (), 1),
    "tiny_bA": (20, 12, 5, 6, 1.0, True, "uneven", (), 1),
    "mid": (300, 70, 7, 5, 0.1, False, "uneven", (), 1),
    "mid_bA": (300, 70, 7, 5, 0.1, True, "linear", (), 1),
    "wide": (1100, 300, 5, 4, 0.05, False, "linear", (), 2),
    "wide_bA": (1100, 300, 5, 4, 0.05, True, "uneven", (), 2),
    "group": (25, 12, 6, 5, 1.0, True, "linear", ((20, 25),), 1),
    "one": (20, 12, 5, 1, 1.0, True, "linear", (), 1),
    "rows70": (20, 12, 70, 6, 1.0, True, "uneven", (), 2),
}
REPLAY_CASE = "tiny_bA"


def parity_case(name):
    V, H, R, K, ws, with_bA, ladder, groups, seed = PARITY[name]
    W, b, c, bA = params(V, H, 100 + V, ws)
    return dict(V=V, H=H, R=R, K=K, W=W, b=b, c=c, bA=bA if with_bA else None, betas=(linear if ladder == "linear" else uneven)(K),
                groups=[tuple(g) for g in groups], x=start_rows(R, V, 300 + V + R, groups), seed=seed)


def truth_params(with_bA):
    t = TRUTH
    W, b, c, bA = params(t["V"], t["H"], t["gen_seed"], t["w_scale"])
    return dict(V=t["V"], H=t["H"], N=t["N"], M=t["M"], K=t["K"], W=W, b=b, c=c, bA=bA if with_bA else None, betas=linear(t["K"]),
                seed=TRUTH_SEED)


def truth_rows(log_p, states):
    """TRUTH["N"] rows drawn from the enumerated annealing model (inverse CDF over the state index), and their log p_ann."""
    g = np.random.Generator(np.random.PCG64(TRUTH["row_seed"]))
    idx = np.searchsorted(np.cumsum(np.exp(log_p)), g.random(TRUTH["N"]))
    idx = np.minimum(idx, states.shape[0] - 1)
    return states[idx].astype(F32), log_p[idx]
