"""Cases shared by test_dbn_bound_cpu.py and test_dbn_bound_gpu.py: parameters and inputs from fixed generators, pinned seeds.

The Philox seeds are pinned on the CPU from the twin alone (tests/bound_oracle.py): every PARITY and PATH case's seed is one whose
smallest Bernoulli margin |p - u| in the twin is at least MARGIN, so the device (fp32 sigmoid, another summation order in the
logits) must take every decision as the twin does; the TRUTH seeds are ones at which the twin's estimates lie within 3 of its own
standard errors of the enumerated values (test_dbn_bound_cpu.py states what the other seeds gave)."""
import numpy as np

from anneal_cases import MARGIN, params  # noqa: F401

F32 = np.float32


def inputs(M, V, gen_seed, real):
    """M rows of V visibles: 0/1 with p = 1/2, or uniform in [0, 1)."""
    g = np.random.Generator(np.random.PCG64(gen_seed))
    u = g.random((M, V))
    return u.astype(F32) if real else (u > 0.5).astype(F32)


# ---- parity of one bound_step with the twin: (V, H, M) cross the kernels' edges and the propagations' routes
# name -> (V, H, M, w_scale, real-valued input, weight-row pitch (None: the constructor's), seed)
PARITY = {
    "tiny": (20, 12, 5, 1.0, False, None, 1),            # a sub-ballot H tail
    "mid": (100, 40, 70, 0.2, True, None, 1),            # two 64-row chunks, M no multiple of the 4 rows per block
    "wide": (1100, 300, 5, 0.05, False, None, 1),        # split-K up route; float4 weight rows: k2_stream reads the bit plane
    "wide_p301": (1100, 300, 5, 0.05, True, 301, 1),     # rows 301 floats apart (unaligned): the fused K2 reads the bit plane
}


def parity_case(name):
    V, H, M, ws, real, pitch, seed = PARITY[name]
    W, b, c, _ = params(V, H, 200 + V, ws)
    return dict(V=V, H=H, M=M, W=W, b=b, c=c, v=inputs(M, V, 300 + V, real), pitch=pitch, seed=seed)


# ---- stacks.  name -> (sizes, w_scale, generator seed)
STACKS = {
    "s3": ((10, 6, 5), 0.5, 41),
    "s4": ((10, 6, 5, 4), 0.5, 42),
    "p3": ((20, 12, 8), 1.0, 43),
    "p4": ((20, 12, 8, 6), 1.0, 44),
}


def stack(name):
    """[(W, b, c)] bottom first."""
    sizes, ws, gs = STACKS[name]
    return [params(sizes[l], sizes[l + 1], gs * 10 + l, ws)[:3] for l in range(len(sizes) - 1)]


# ---- against the truth (stacks s3 / s4): B rows of 0/1 input, S samples per row
TRUTH = dict(B=6, S_entropy=256, S_logq=2048, in_seed=7)
TRUTH_SEED = {"s3": 1, "s4": 1}

# ---- the whole path on the device against the twin (stacks p3 / p4): B rows, S samples per row, both modes share the draws
PATH = dict(B=5, S=3, in_seed=8)
PATH_SEED = {"p3": 1, "p4": 2}
