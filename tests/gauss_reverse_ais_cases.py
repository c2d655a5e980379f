"""Cases and pinned seeds of the Gaussian reverse-AIS tests (tests/test_gauss_reverse_ais_cpu.py, tests/test_gauss_reverse_ais_gpu.py).

Shapes and parameters are those of tests/gauss_ais_cases.py with R rows in place of M chains: `tiny` 20 x 12, R = 5, K = 6; `ballot`
67 x 64 (a whole ballot); `mid` 300 x 70 (also with weight rows 75 floats apart); `wide` 1100 x 300 (split-K up, both down routes;
also pitch 301); `rows70` with 70 rows (two 64-row chunks); `k1` with K = 1 (one transition, and the last pass only weighs).  Every
case runs with b_A = b and with the shifted b_A.  The rows are v = b + e^{z/2} n + h W^T with a random 0/1 h, what the model itself
would emit, from a generator of their own (the parameters stay those of gauss_ais_cases.case).

Seeds.  The first seed, counting from 1, at which the float64 twin's smallest Bernoulli margin |sigmoid(beta x) - U| is >= MARGIN and
the float32 restatement draws the same h everywhere -- for the replay source and, for PHILOX_RUNS, for PhiloxStream.

Tolerances of the GPU parity test: per run, FACTOR x the distance of the float32 restatement to the float64 twin on that run
(fp32_error), both relative to max(1, |twin|); FACTOR is the 8 of tests/test_gauss_ais_gpu.py.

Truth (the issue's): the parameters of gauss_ais_cases.truth, K = 200 linear, 16 chains per row, 32 rows v = b + e^{z/2} n; the exact
log p(v) from the 2^12 hidden states.  Each of the seeds 1-8 is gated one by one, so the slack is TRUTH_SIGMAS sample standard
deviations of the twin's mean ll over those eight seeds (truth_slack).  The stack case gates the MEAN over the eight seeds, so its
slack is TRUTH_SIGMAS standard errors of that mean (stack_slack).  Both are computed from the twin, never fixed.

`python tests/gauss_reverse_ais_cases.py` prints the first seeds next to the pinned ones, every run's fp32 error and tolerance, the
truth runs of seeds 1-8 with their slack and the stack runs with theirs."""
import numpy as np

import gauss_ais_cases as FC
import gauss_reverse_ais_oracle as GR

F32, F64 = np.float32, np.float64
MARGIN = FC.MARGIN
FACTOR = 8
SHAPES, NAMES, RUNS, PHILOX_RUNS = FC.SHAPES, FC.NAMES, FC.RUNS, FC.PHILOX_RUNS
# (name, with b_A) -> pinned seed of the replay source; PHILOX_SEEDS: of PhiloxStream
SEEDS = {**{r: 1 for r in RUNS}, ("mid", False): 3, ("mid", True): 3, ("wide", False): 3, ("wide", True): 8, ("rows70", False): 2}
PHILOX_SEEDS = {r: 1 for r in PHILOX_RUNS}
TRUTH_SEEDS = tuple(range(1, 9))
TRUTH = dict(rows=32, chains=16, K=200)
TRUTH_SIGMAS = 3.0
STACK = dict(S=8, chains=16, K=100)

linear, source, rel = FC.linear, FC.source, FC.rel


def rows(W, b, z, R, g):
    h = (g.random((R, W.shape[1])) > 0.5).astype(F64)
    return (b + np.exp(0.5 * z) * g.standard_normal((R, W.shape[0])) + h @ W.T.astype(F64)).astype(F32)


def case(name, with_bA):
    c = dict(FC.case(name, with_bA))
    c["R"] = c.pop("M")
    c["seed"], c["philox_seed"] = SEEDS[(name, with_bA)], PHILOX_SEEDS.get((name, with_bA))
    c["v"] = rows(c["W"], c["b"], c["z"], c["R"], np.random.Generator(np.random.PCG64(3300 + NAMES.index(name))))
    return c


def truth(with_bA):
    """The truth case: the parameters of gauss_ais_cases.truth, 32 rows drawn as b + e^{z/2} n, each replicated 16 times."""
    c = dict(FC.truth(with_bA))
    del c["M"], c["seed"]
    g = np.random.Generator(np.random.PCG64(3390))
    c["x"] = (c["b"] + np.exp(0.5 * c["z"]) * g.standard_normal((TRUTH["rows"], c["V"]))).astype(F32)
    c["chains"] = TRUTH["chains"]
    c["exact"] = GR.exact_log_p(c["W"], c["b"], c["c"], c["z"], c["x"])
    return c


def twin_run(c, kind="replay", seed=None, dt=F64, v=None):
    """dict(logw, v: u_1, margin, h: the h samples) of the twin on a case."""
    seed = (c["seed"] if kind == "replay" else c["philox_seed"]) if seed is None else seed
    rec = []
    logw, u1, margin = GR.gauss_reverse_ais_logw(c["W"], c["b"], c["c"], c["z"], c["bA"], c["betas"], c["v"] if v is None else v,
                                                 source(kind, seed), dt=dt, record=rec)
    return dict(logw=logw, v=u1, margin=margin, h=rec)


same_h = FC.same_h


def seed_ok(c, kind, seed):
    a = twin_run(c, kind, seed)
    return a["margin"] >= MARGIN and same_h(a, twin_run(c, kind, seed, dt=F32))


def all_runs():
    return [(case(n, a), "replay") for n, a in RUNS] + [(case(n, a), "philox") for n, a in PHILOX_RUNS]


def fp32_error(c, kind="replay"):
    """What fp32 arithmetic alone costs on one run: {"logw", "v"} of the float32 restatement against the float64 twin, each
    max |x' - x| / max(1, |x|); the h samples must agree."""
    a, b = twin_run(c, kind), twin_run(c, kind, dt=F32)
    assert same_h(a, b), (c["name"], c["bA"] is not None, kind)
    return {"logw": rel(b["logw"], a["logw"]), "v": rel(b["v"], a["v"])}


def tolerance(c, kind="replay"):
    return {k: FACTOR * e for k, e in fp32_error(c, kind).items()}


def truth_mean_ll(c, seed):
    """(mean over the rows of ll, mean ess) of the twin on the truth case under the project's Philox draws."""
    import anneal_oracle as A
    t = twin_run(c, "philox", seed, v=np.repeat(c["x"], c["chains"], axis=0))
    lme, ess = A.rows_logmeanexp(t["logw"], c["chains"])
    return float((lme - GR.log_z_base(c["V"], c["H"], c["z"])).mean()), float(ess.mean())


def truth_slack(with_bA):
    """TRUTH_SIGMAS sample standard deviations of the twin's mean ll over TRUTH_SEEDS, and those means."""
    c = truth(with_bA)
    means = np.array([truth_mean_ll(c, s)[0] for s in TRUTH_SEEDS])
    return TRUTH_SIGMAS * float(means.std(ddof=1)), means


def stack_twin(seed):
    """The twin of gaussian_dbn_conservative_bound on the 6-5-4 stack of tests/gauss_bound_cases.truth_stack (a Gaussian bottom under
    one Bernoulli RBM) under the project's Philox draws: the mean over the 8 rows of the mean over S samples."""
    import anneal_oracle as A
    import gauss_bound_cases as GBC
    import gauss_bound_oracle as GB
    from oracle.draws import PhiloxStream
    z, layers, v = GBC.truth_stack()
    S, M, K = STACK["S"], STACK["chains"], STACK["K"]
    ps = PhiloxStream(seed)
    acc, h, _, _, _ = GB.gauss_bound_step(*layers[0], z, np.repeat(v, S, axis=0), "entropy", ps)
    W, b, c = layers[1]
    logw, _, _, _ = A.reverse_ais_logw(W, b, c, None, (), linear(K), np.repeat(h, M, axis=0), ps)
    lme, _ = A.rows_logmeanexp(logw, M)
    w = acc + lme - A.log_z_base(W.shape[0], W.shape[1], None)
    return float(w.reshape(v.shape[0], S).mean(1).mean())


def stack_exact():
    import gauss_bound_cases as GBC
    import gauss_bound_oracle as GB
    z, layers, v = GBC.truth_stack()
    return float(GB.exact_bound(z, layers, v).mean())


def stack_slack():
    """TRUTH_SIGMAS standard errors of the mean over TRUTH_SEEDS of the stack twin, and the per-seed values."""
    vals = np.array([stack_twin(s) for s in TRUTH_SEEDS])
    return TRUTH_SIGMAS * float(vals.std(ddof=1) / np.sqrt(vals.size)), vals


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "multimodal-idbn_amd")]
    for n, a in RUNS:
        c = case(n, a)
        print(f"{n} b_A={a}: first replay seed {next((s for s in range(1, 65) if seed_ok(c, 'replay', s)), None)} (pinned {c['seed']})")
    for n, a in PHILOX_RUNS:
        c = case(n, a)
        print(f"{n} b_A={a}: first Philox seed {next(s for s in range(1, 65) if seed_ok(c, 'philox', s))} (pinned {c['philox_seed']})")
    for c, kind in all_runs():
        e = fp32_error(c, kind)
        print(f"{c['name']} b_A={c['bA'] is not None} {kind}: fp32 restatement vs float64 twin logw {e['logw']:.3g} v {e['v']:.3g} "
              f"-> tolerances {FACTOR * e['logw']:.3g} {FACTOR * e['v']:.3g}")
    for a in (False, True):
        slack, means = truth_slack(a)
        print(f"truth b_A={a}: exact mean log p {truth(a)['exact'].mean():.4f}; twin mean ll of seeds 1-8 {means.round(4).tolist()}; "
              f"slack {slack:.4f}")
    slack, vals = stack_slack()
    print(f"stack 6-5-4: exact bound {stack_exact():.4f}; twin of seeds 1-8 {vals.round(4).tolist()}, mean {vals.mean():.4f}; slack {slack:.4f}")
