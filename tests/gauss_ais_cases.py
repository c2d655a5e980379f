"""Cases and pinned seeds of the Gaussian AIS tests (tests/test_gauss_ais_cpu.py, tests/test_gauss_ais_gpu.py).

Shapes (V, H, M, K), the smallest that reach each path of imdbn_rbm_gauss_ais: `tiny` 20 x 12; `ballot` 67 x 64 (a whole ballot,
H = Hb); `mid` 300 x 70 (also with weight rows 75 floats apart); `wide` 1100 x 300 (V > 1024: split-K up; k2_stream down at the
padded pitch, the fused K2 at pitch 301); `rows70` with 70 chains (two 64-row chunks); `k1` with K = 1 (weighs only, draws no h).
Every case runs with b_A = b (no base bias) and with a shifted b_A.  Parameters: W ~ s N(0, 1) with s = 0.2 for V = 20 and
1 / sqrt(V) above, b ~ 0.5 N, c ~ 0.3 N, z ~ 0.4 N, b_A = b + 0.3 N; the ladder is linear.

Seeds.  The first seed, counting from 1, at which the float64 twin's smallest Bernoulli margin |sigmoid(beta x) - U| is >= MARGIN and
the float32 restatement draws the same h everywhere -- for the replay source (oracle.draws.DrawStream) and, for PHILOX_RUNS, for
PhiloxStream.  `python tests/gauss_ais_cases.py` prints the first such seeds next to the pinned ones, the fp32 errors the GPU
tolerances are derived from and the truth runs of seeds 1-8."""
import numpy as np

import gauss_ais_oracle as GA

F32, F64 = np.float32, np.float64
MARGIN = 1e-4
# name -> (V, H, M, K, pitches the GPU test runs)
SHAPES = {
    "tiny": (20, 12, 5, 6, (None,)),
    "ballot": (67, 64, 6, 4, (None,)),
    "mid": (300, 70, 7, 5, (None, 75)),
    "wide": (1100, 300, 5, 4, (None, 301)),
    "rows70": (20, 12, 70, 3, (None,)),
    "k1": (20, 12, 5, 1, (None,)),
}
NAMES = list(SHAPES)
RUNS = [(name, bA) for name in NAMES for bA in (False, True)]
PHILOX_RUNS = [("tiny", True), ("mid", False)]
# (name, with b_A) -> pinned seed of the replay source; PHILOX_SEEDS: of PhiloxStream
SEEDS = {**{(n, a): 1 for n, a in RUNS}, ("tiny", False): 2, ("mid", False): 2, ("wide", True): 2}
PHILOX_SEEDS = {r: 1 for r in PHILOX_RUNS}
TRUTH_SEED = 1


def linear(K):
    return (np.arange(K + 1, dtype=F64) / K).astype(F32)


def _params(V, H, g, wscale):
    W = (wscale * g.standard_normal((V, H))).astype(F32)
    b, c, z = (0.5 * g.standard_normal(V)).astype(F32), (0.3 * g.standard_normal(H)).astype(F32), (0.4 * g.standard_normal(V)).astype(F32)
    return W, b, c, z, (b + 0.3 * g.standard_normal(V)).astype(F32)


def case(name, with_bA):
    V, H, M, K, pitches = SHAPES[name]
    g = np.random.Generator(np.random.PCG64(3000 + NAMES.index(name)))
    W, b, c, z, bA = _params(V, H, g, 0.2 if V == 20 else 1.0 / np.sqrt(V))
    return dict(name=name, V=V, H=H, M=M, K=K, W=W, b=b, c=c, z=z, bA=bA if with_bA else None, betas=linear(K), pitches=pitches,
                seed=SEEDS[(name, with_bA)], philox_seed=PHILOX_SEEDS.get((name, with_bA)))


def truth(with_bA, seed=TRUTH_SEED):
    """The truth case of the issue: V = 20, H = 12, K = 200 linear, M = 64."""
    g = np.random.Generator(np.random.PCG64(2900))
    W, b, c, z, bA = _params(20, 12, g, 0.2)
    return dict(name="truth", V=20, H=12, M=64, K=200, W=W, b=b, c=c, z=z, bA=bA if with_bA else None, betas=linear(200), seed=seed)


def source(kind, seed):
    from oracle.draws import DrawStream, PhiloxStream
    return DrawStream(seed) if kind == "replay" else PhiloxStream(seed)


def twin_run(c, kind="replay", seed=None, dt=F64):
    """dict(logw, v, margin, h: the h samples) of the twin on a case."""
    seed = (c["seed"] if kind == "replay" else c["philox_seed"]) if seed is None else seed
    rec = []
    logw, v, margin = GA.gauss_ais_logw(c["W"], c["b"], c["c"], c["z"], c["bA"], c["betas"], c["M"], source(kind, seed), dt=dt, record=rec)
    return dict(logw=logw, v=v, margin=margin, h=rec)


def same_h(a, b):
    return len(a["h"]) == len(b["h"]) and all(np.array_equal(x, y) for x, y in zip(a["h"], b["h"]))


def seed_ok(c, kind, seed):
    a = twin_run(c, kind, seed)
    return a["margin"] >= MARGIN and same_h(a, twin_run(c, kind, seed, dt=F32))


def rel(got, want):
    """max |got - want| / max(1, |want|)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def all_runs():
    return [(case(n, a), "replay") for n, a in RUNS] + [(case(n, a), "philox") for n, a in PHILOX_RUNS]


def fp32_errors():
    """What fp32 arithmetic alone costs: the float32 restatement against the float64 twin over every run the GPU tests make.
    {"logw": max |logw' - logw| / max(1, |logw|), "v": the same of v_K}; the h samples must agree."""
    err = {"logw": 0.0, "v": 0.0}
    for c, kind in all_runs():
        a, b = twin_run(c, kind), twin_run(c, kind, dt=F32)
        assert same_h(a, b), (c["name"], c["bA"] is not None, kind)
        err["logw"] = max(err["logw"], rel(b["logw"], a["logw"]))
        err["v"] = max(err["v"], rel(b["v"], a["v"]))
    return err


def truth_errors(seeds=range(1, 9)):
    """(seed, with b_A, error in se, se, ess) of the twin on the truth case under the project's Philox draws."""
    import anneal_oracle as A
    out = []
    for with_bA in (False, True):
        for s in seeds:
            c = truth(with_bA, s)
            t = twin_run(c, "philox", s)
            lme, se, ess = A.weight_stats(t["logw"])
            exact = GA.exact_log_z(c["W"], c["b"], c["c"], c["z"])
            out.append((s, with_bA, (GA.log_z_base(c["V"], c["H"], c["z"]) + lme - exact) / se, se, ess))
    return out


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for n, a in RUNS:
        c = case(n, a)
        first = next((s for s in range(1, 65) if seed_ok(c, "replay", s)), None) if c["K"] > 1 else 1
        print(f"{n} b_A={a}: first replay seed {first} (pinned {c['seed']})")
    for n, a in PHILOX_RUNS:
        c = case(n, a)
        print(f"{n} b_A={a}: first Philox seed {next(s for s in range(1, 65) if seed_ok(c, 'philox', s))} (pinned {c['philox_seed']})")
    print("fp32 restatement vs float64 twin:", {k: f"{v:.3g}" for k, v in fp32_errors().items()})
    for s, a, e, se, ess in truth_errors():
        print(f"truth seed {s} b_A={a}: error {e:+.2f} se, se {se:.4f}, ess {ess:.1f}")
