"""Cases and pinned seeds of the Gaussian stack-bound tests (tests/test_gauss_bound_cpu.py, tests/test_gauss_bound_gpu.py).

Parity shapes (V, H, M), the smallest that reach each path of imdbn_rbm_gauss_bound_step: `tiny` 20 x 12; `ballot` 67 x 64 (a whole
ballot, H = Hb; the composition test puts a 64 -> 20 Bernoulli layer and a 20 -> 9 top RBM above it); `mid` 300 x 70 (also with
weight rows 75 floats apart); `wide` 1100 x 300 (V > 1024: split-K up; k2_stream down at the padded pitch, the fused K2 at pitch
301); `rows70` with 70 rows (more than one 64-row chunk of the row-dealing kernels).  Every case runs in both modes.  Parameters:
W ~ s N(0, 1) with s = 0.2 for V = 20 and 1 / sqrt(V) above, b ~ 0.5 N, c ~ 0.3 N, z ~ 0.4 N; the rows are
v = b + e^{z/2} n + h W^T with a random 0/1 h, what the model itself would emit.

Seeds.  The first seed, counting from 1, at which the float64 twin's smallest Bernoulli margin |sigmoid(x) - U| is >= MARGIN and the
float32 restatement draws the same h -- for the replay source (oracle.draws.DrawStream) and, for PHILOX_RUN, for PhiloxStream.
`python tests/gauss_bound_cases.py` prints the first such seeds next to the pinned ones, the fp32 error the GPU tolerance is derived
from and the truth runs of seeds 1-8.

Truth (the issue's): stacks 6-5-4 and 6-5-4-3 from numpy.random.Generator(PCG64(7)), W ~ 0.5 N, b_1 ~ 0.5 N, c ~ 0.3 N, z ~ 0.4 N,
b_2.. ~ 0.3 N, 8 rows v = b_1 + e^{z/2} n + h W_1^T with random h."""
import numpy as np

import anneal_oracle as A
import gauss_bound_oracle as GB

F32, F64 = np.float32, np.float64
MARGIN = 1e-5
MODES = ("entropy", "logq")
# name -> (V, H, M, pitches the GPU test runs)
SHAPES = {
    "tiny": (20, 12, 5, (None,)),
    "ballot": (67, 64, 6, (None,)),
    "mid": (300, 70, 7, (None, 75)),
    "wide": (1100, 300, 5, (None, 301)),
    "rows70": (20, 12, 70, (None,)),
}
NAMES = list(SHAPES)
RUNS = [(name, mode) for name in NAMES for mode in MODES]
PHILOX_RUN = ("mid", "logq")
# (name, mode) -> pinned seed of the replay source (the draw and therefore h do not depend on the mode); PHILOX_SEED: of PhiloxStream
SEEDS = {r: 1 for r in RUNS}
PHILOX_SEED = 1
TRUTH_SEED = 1
TRUTH = dict(B=8, S_entropy=256, S_logq=2048)
UPPER = (64, 20, 9)      # the composition test: a Bernoulli layer 64 -> 20 and a top RBM 20 -> 9 above `ballot`


def _rows(W, b, z, M, g):
    h = (g.random((M, W.shape[1])) > 0.5).astype(F64)
    return (b + np.exp(0.5 * z) * g.standard_normal((M, W.shape[0])) + h @ W.T.astype(F64)).astype(F32)


def case(name, mode="entropy"):
    V, H, M, pitches = SHAPES[name]
    g = np.random.Generator(np.random.PCG64(3100 + NAMES.index(name)))
    W = ((0.2 if V == 20 else 1.0 / np.sqrt(V)) * g.standard_normal((V, H))).astype(F32)
    b, c, z = (0.5 * g.standard_normal(V)).astype(F32), (0.3 * g.standard_normal(H)).astype(F32), (0.4 * g.standard_normal(V)).astype(F32)
    return dict(name=name, mode=mode, V=V, H=H, M=M, W=W, b=b, c=c, z=z, v=_rows(W, b, z, M, g), pitches=pitches, seed=SEEDS[(name, mode)],
                philox_seed=PHILOX_SEED)


def upper_layers():
    """[(W, b, c)] of the Bernoulli layers of the composition test: 64 -> 20 directed, 20 -> 9 the top RBM."""
    g = np.random.Generator(np.random.PCG64(3190))
    out = []
    for V, H in zip(UPPER[:-1], UPPER[1:]):
        out.append(((g.standard_normal((V, H)) / np.sqrt(V)).astype(F32), (0.3 * g.standard_normal(V)).astype(F32),
                    (0.3 * g.standard_normal(H)).astype(F32)))
    return out


def truth_stack(sizes=(6, 5, 4)):
    """(z, layers, v [8, V]) of the issue's truth case; the draws of 6-5-4 are the first draws of 6-5-4-3."""
    g = np.random.Generator(np.random.PCG64(7))
    V = sizes[0]
    Ws = [(0.5 * g.standard_normal((a, b))).astype(F32) for a, b in zip(sizes[:-1], sizes[1:])]
    b1 = (0.5 * g.standard_normal(V)).astype(F32)
    cs = [(0.3 * g.standard_normal(n)).astype(F32) for n in sizes[1:]]
    z = (0.4 * g.standard_normal(V)).astype(F32)
    bs = [b1] + [(0.3 * g.standard_normal(n)).astype(F32) for n in sizes[1:-1]]
    layers = list(zip(Ws, bs, cs))
    return z, layers, _rows(Ws[0], b1, z, TRUTH["B"], g)


def source(kind, seed):
    from oracle.draws import DrawStream, PhiloxStream
    return DrawStream(seed) if kind == "replay" else PhiloxStream(seed)


def twin_run(c, kind="replay", seed=None, dt=F64):
    """dict(acc, h, margin, e, ln) of the twin on a case."""
    seed = (c["seed"] if kind == "replay" else c["philox_seed"]) if seed is None else seed
    acc, h, margin, e, ln = GB.gauss_bound_step(c["W"], c["b"], c["c"], c["z"], c["v"], c["mode"], source(kind, seed), dt=dt)
    return dict(acc=acc, h=h, margin=margin, e=e, ln=ln)


def seed_ok(c, kind, seed):
    a = twin_run(c, kind, seed)
    return a["margin"] >= MARGIN and np.array_equal(a["h"], twin_run(c, kind, seed, dt=F32)["h"])


def rel(got, want):
    """max |got - want| / max(1, |want|)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def all_runs():
    return [(case(n, m), "replay") for n, m in RUNS] + [(case(*PHILOX_RUN), "philox")]


def fp32_error():
    """What fp32 arithmetic alone costs: the float32 restatement against the float64 twin over every run the GPU tests make,
    max |acc' - acc| / max(1, |acc|); the h samples must agree."""
    err = 0.0
    for c, kind in all_runs():
        a, b = twin_run(c, kind), twin_run(c, kind, dt=F32)
        assert np.array_equal(a["h"], b["h"]), (c["name"], c["mode"], kind)
        err = max(err, rel(b["acc"], a["acc"]))
    return err


def truth_statistic(mode, seed, sizes=(6, 5, 4)):
    """(sum over the rows of estimate - exact, sqrt of the sum of the rows' se^2, per-row exact values, per-row estimates) of the twin on
    the truth stack under the project's Philox draws: mode `entropy` against the exact bound (S = 256, se = std / sqrt(S)), mode
    `logq` against the exact log p (S = 2048, se by the delta method on the weights: anneal_oracle.row_stats)."""
    from oracle.draws import PhiloxStream
    z, layers, v = truth_stack(sizes)
    lz = A.exact_log_z(*layers[-1])
    S = TRUTH["S_entropy"] if mode == "entropy" else TRUTH["S_logq"]
    w, _, _, _ = GB.gauss_dbn_values(z, layers, v, S, mode, PhiloxStream(seed), lz)
    if mode == "entropy":
        est, se, exact = w.mean(1), w.std(1, ddof=1) / np.sqrt(S), GB.exact_bound(z, layers, v)
    else:
        est, se, _ = A.row_stats(w.reshape(-1), S)
        exact = GB.exact_log_p(z, layers, v)
    return float((est - exact).sum()), float(np.sqrt((se * se).sum())), exact, est


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for n, m in RUNS:
        c = case(n, m)
        print(f"{n} {m}: first replay seed {next(s for s in range(1, 65) if seed_ok(c, 'replay', s))} (pinned {c['seed']}), "
              f"margin {twin_run(c)['margin']:.3g}")
    c = case(*PHILOX_RUN)
    print(f"{PHILOX_RUN}: first Philox seed {next(s for s in range(1, 65) if seed_ok(c, 'philox', s))} (pinned {PHILOX_SEED})")
    print(f"fp32 restatement vs float64 twin: {fp32_error():.3g}")
    z, layers, v = truth_stack()
    print("gap log p - bound per row:", (GB.exact_log_p(z, layers, v) - GB.exact_bound(z, layers, v)).round(3))
    for mode in MODES:
        for s in range(1, 9):
            d, se, _, _ = truth_statistic(mode, s)
            print(f"truth {mode} seed {s}: sum(estimate - exact) {d:+.4f} = {d / se:+.2f} se (se {se:.4f})")
