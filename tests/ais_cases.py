"""Cases shared by test_ais_cpu.py and test_ais_gpu.py: parameters from fixed generators, temperature ladders, pinned seeds.

The Philox seeds are pinned on the CPU from the twin alone (tests/ais_oracle.py): TRUTH_SEED is one whose estimate lies within
3 standard errors of the enumerated log Z with and without a base-rate bias; every PARITY case's seed is one whose smallest
Bernoulli margin |p - u| in the twin is at least MARGIN, so the device (fp32 sigmoid, another summation order in the logits)
must take every decision as the twin does."""
import numpy as np

F32 = np.float32
MARGIN = 1e-5


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


# ---- against the truth: V = 20, H = 12, W ~ N(0, 1), biases ~ N(0, 0.5), K = 200 linear temperatures, M = 64 chains
TRUTH = dict(V=20, H=12, K=200, M=64, gen_seed=2024, w_scale=1.0)
TRUTH_SEED = 1

# ---- parity with the twin: (V, H, M, K) cross the kernel's edges -- one partial ballot; H no multiple of 64 and M no multiple of the
# rows per block; V > 1024 (streaming / bit-plane routes), H across 256, weight rows of 300 floats behind an unaligned base pitch
# name -> (V, H, M, K, w_scale, with b_A, ladder, seed)
PARITY = {
    "tiny": (20, 12, 5, 6, 1.0, False, "linear", 1),
    "tiny_bA": (20, 12, 5, 6, 1.0, True, "uneven", 1),
    "mid": (300, 70, 7, 5, 0.1, False, "uneven", 2),
    "mid_bA": (300, 70, 7, 5, 0.1, True, "linear", 1),
    "wide": (1100, 300, 5, 4, 0.05, False, "linear", 1),
    "wide_bA": (1100, 300, 5, 4, 0.05, True, "uneven", 1),
}


def parity_case(name):
    V, H, M, K, ws, with_bA, ladder, seed = PARITY[name]
    W, b, c, bA = params(V, H, 100 + V, ws)
    return dict(V=V, H=H, M=M, K=K, W=W, b=b, c=c, bA=bA if with_bA else None, betas=(linear if ladder == "linear" else uneven)(K), seed=seed)


def truth_case(with_bA):
    t = TRUTH
    W, b, c, bA = params(t["V"], t["H"], t["gen_seed"], t["w_scale"])
    return dict(V=t["V"], H=t["H"], M=t["M"], K=t["K"], W=W, b=b, c=c, bA=bA if with_bA else None, betas=linear(t["K"]), seed=TRUTH_SEED)
