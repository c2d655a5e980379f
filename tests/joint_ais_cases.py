"""Cases shared by the joint-AIS and iMDBN-bound tests (CPU and GPU): parameters from fixed generators, pinned seeds.

The Philox seeds are pinned on the CPU from the twins alone (tests/joint_ais_oracle.py).  TRUTH seeds are ones at which the twin's
estimates lie within 3 of its own standard errors of the enumerated values (the test docstrings state what the seeds 1..8 gave).
Every PARITY / LABEL / PATH seed is the first one, counting from 1, whose smallest Bernoulli margin |p - u| outside the softmax groups
AND smallest categorical-CDF margin in the twin are at least MARGIN, so the device (fp32 sigmoid and softmax, another summation order in
the logits) must take every decision as the twin does.  `python tests/joint_ais_cases.py` prints the margins of the pinned seeds."""
import numpy as np

from ais_cases import MARGIN, linear, params, uneven  # noqa: F401

F32 = np.float32

# ---- against the truth: 16 Bernoulli columns + one group of 4, H = 12, W ~ N(0, 1), biases ~ N(0, 0.5), K = 200 linear, M = 64 chains
TRUTH = dict(V=20, H=12, K=200, M=64, gen_seed=2025, w_scale=1.0, groups=[(16, 20)])
TRUTH_SEED = 1


def truth_case(with_bA):
    t = TRUTH
    W, b, c, bA = params(t["V"], t["H"], t["gen_seed"], t["w_scale"])
    return dict(V=t["V"], H=t["H"], M=t["M"], K=t["K"], W=W, b=b, c=c, bA=bA if with_bA else None, betas=linear(t["K"]), seed=TRUTH_SEED,
                groups=list(t["groups"]))


# ---- parity of imdbn_rbm_ais_groups with the twin
# name -> (V, H, M, K, groups, w_scale, with b_A, ladder, weight-row pitch (None: the constructor's), seed)
PARITY = {
    "odd": (20, 12, 5, 3, [(15, 20)], 1.0, True, "uneven", None, 1),                 # group at an odd offset, rows no multiple of 4
    "two": (70, 33, 70, 3, [(3, 9), (60, 70)], 0.3, True, "linear", 37, 1),          # two groups, one across column 64; rows across a 64-row block
    "k1": (20, 12, 5, 1, [(15, 20)], 1.0, True, "linear", None, 1),                  # no transition
    "plain": (20, 12, 5, 3, [], 1.0, True, "uneven", None, 1),                       # n_groups = 0: imdbn_rbm_ais bit for bit
    "paper": (532, 256, 64, 5, [(500, 532)], 0.05, True, "linear", None, 14),         # the paper's joint shape
    "wide": (1100, 40, 8, 2, [(1092, 1100)], 0.05, False, "linear", None, 2),        # the split-K up route
}


def parity_case(name):
    V, H, M, K, groups, ws, with_bA, ladder, pitch, seed = PARITY[name]
    W, b, c, bA = params(V, H, 500 + V + H, ws)
    return dict(V=V, H=H, M=M, K=K, W=W, b=b, c=c, bA=bA if with_bA else None, betas=(linear if ladder == "linear" else uneven)(K),
                seed=seed, groups=list(groups), pitch=pitch)


# ---- imdbn_rbm_label_loglik.  name -> (Dz, K, H, extra visible columns behind the labels, w_scale)
LABEL = {"small": (12, 3, 7, 0, 0.5), "paper": (500, 32, 256, 0, 0.05)}


def label_case(name, N, real, gen_seed=0):
    """A joint RBM [Dz | K] x H and N code rows (0/1, or uniform in [0, 1)), labels in [0, K)."""
    Dz, K, H, extra, ws = LABEL[name]
    W, b, c, _ = params(Dz + K + extra, H, 700 + Dz, ws)
    g = np.random.Generator(np.random.PCG64(800 + N + gen_seed))
    u = g.random((N, Dz))
    z = u.astype(F32) if real else (u > 0.5).astype(F32)
    return dict(Dz=Dz, K=K, H=H, W=W, b=b, c=c, z=z, gt=g.integers(0, K, N).astype(np.int32))


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
    import joint_ais_oracle as J
    from oracle.draws import PhiloxStream
    for name in PARITY:
        c = parity_case(name)
        for seed in range(1, 9):
            _, _, m, cm = J.ais_groups_logw(c["W"], c["b"], c["c"], c["bA"], c["groups"], c["betas"], c["M"], PhiloxStream(seed))
            if min(m, cm) >= MARGIN:
                break
        print(f"{name}: first seed {seed} (pinned {c['seed']}), margins {m:.3g} / {cm:.3g}")
