"""CPU-only: the numpy twin of imdbn_rbm_reverse_ais (tests/anneal_oracle.py) against the enumerated annealing model, the host
logic of the reverse-AIS functions of imdbn/utils/likelihood.py on a test double of the engine, the draw schedule and the exports'
declaration and binding.

Twin against enumeration: V = 10, H = 6, W ~ N(0, 1), biases ~ N(0, 0.5), K = 20 linear temperatures, N = 4 rows drawn from the
enumerated annealing model x M = 256 chains, with and without a base-rate bias; every row's estimate within 3 of its own standard
errors of log p_ann(x).  Over the Philox seeds 1..8 all eight pass with and without b_A; the largest error was 2.05 se, se
0.028..0.045, ess 170..213 of 256.  Seed 1 is pinned (anneal_cases.TRUTH_SEED): at most 1.02 se."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import anneal_cases as Cs
import anneal_oracle as A
from bound_oracle import double, host_rbm  # noqa: F401  (the fixture, by name)
from imdbn import engine as E
from imdbn.engine import native, rng as R
from imdbn.utils import likelihood as LK
from oracle.draws import PhiloxStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bA(c):
    return None if c["bA"] is None else torch.from_numpy(c["bA"])


_TRUTH = {}


def _truth(with_bA):
    """(case, rows [N, V], exact log p_ann of the rows [N]), enumerated once."""
    if with_bA not in _TRUTH:
        c = Cs.reverse_truth(with_bA)
        lp, st = A.annealing_model(c["W"], c["b"], c["c"], c["bA"], c["betas"])
        _TRUTH[with_bA] = (c,) + Cs.truth_rows(lp, st)
    return _TRUTH[with_bA]


# ---- 1. the twin against enumeration ----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bA", [False, True])
def test_twin_estimate_is_within_three_standard_errors_of_the_enumerated_annealing_model(with_bA):
    c, x, want = _truth(with_bA)
    logw, u1, _, _ = A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], [], c["betas"], np.repeat(x, c["M"], 0), PhiloxStream(c["seed"]))
    lme, se, ess = A.row_stats(logw, c["M"])
    got = lme - A.log_z_base(c["V"], c["H"], c["bA"], [])
    print(f"b_A {with_bA}: log p_hat {got.round(4)}, exact {want.round(4)}, errors {((got - want) / se).round(2)} se, se {se.round(4)}, ess {ess.round(0)}")
    assert u1.shape == (c["N"] * c["M"], c["V"]) and set(np.unique(u1)) <= {0.0, 1.0}
    assert (se > 0).all() and (se <= 0.06).all()
    assert (np.abs(got - want) <= 3 * se).all()


def test_the_enumerated_annealing_model_approaches_the_rbm_as_the_ladder_grows():
    """p_ann is a distribution for every K, and its distance from the RBM shrinks with K (what the estimator bounds is p_ann)."""
    W, b, c, bA = Cs.params(6, 4, 3, 1.0)
    vs = ((np.arange(1 << 6)[:, None] >> np.arange(6)[None, :]) & 1).astype(np.float64)
    t = vs @ b.astype(np.float64) + A.softplus(vs @ W.astype(np.float64) + c).sum(1)
    log_p = t - (t.max() + np.log(np.exp(t - t.max()).sum()))
    kl = []
    for K in (1, 10, 100):
        lp, _ = A.annealing_model(W, b, c, bA, Cs.linear(K))
        assert np.exp(lp).sum() == pytest.approx(1.0, abs=1e-12)
        kl.append(float((np.exp(lp) * (lp - log_p)).sum()))
    print("KL(p_ann || p_RBM) for K = 1, 10, 100:", np.round(kl, 5))
    assert kl[0] > kl[1] > kl[2] >= 0 and kl[2] < 0.02


def test_one_temperature_is_one_gibbs_step_from_the_start_state():
    """K = 1: u_1 ~ T_1(. | x) at beta = 1 (no b_A in it), logw = -F(x) - Delta_1(u_1); two draws."""
    W, b, c, bA = Cs.params(9, 4, 5, 1.0)
    x = Cs.start_rows(6, 9, 1)
    ps = PhiloxStream(3)
    logw, u1, _, _ = A.reverse_ais_logw(W, b, c, bA, [], np.array([0, 1], np.float32), x, ps)
    assert ps.log == [("u", (6, 4)), ("u", (6, 9))]
    q = PhiloxStream(3)
    h = (A.sigmoid((x @ W + c).astype(np.float64)) > q.uniform((6, 4))).astype(np.float32)
    want_u = (A.sigmoid((h @ W.T + b).astype(np.float64)) > q.uniform((6, 9))).astype(np.float32)
    assert np.array_equal(u1, want_u)
    nf = x.astype(np.float64) @ b + A.softplus((x @ W + c).astype(np.float64)).sum(1)
    d1 = u1.astype(np.float64) @ (b.astype(np.float64) - bA) + (A.softplus((u1 @ W + c).astype(np.float64)) - np.log(2.0)).sum(1)
    assert np.allclose(logw, nf - d1, rtol=1e-12, atol=1e-5)          # two fp32 summation orders in the logits


def test_rows_that_are_not_states_are_nan_and_only_they():
    c = Cs.case(Cs.REVERSE, "group")
    x = c["x"].copy()
    x[1, 3] = 0.5
    x[4, 20:25] = 0.0
    x[4, 21] = x[4, 23] = 1.0
    logw, _, _, _ = A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], c["groups"], c["betas"], x, PhiloxStream(1))
    assert np.isnan(logw[[1, 4]]).all() and np.isfinite(np.delete(logw, [1, 4])).all()
    lme, ess = A.rows_logmeanexp(logw, 2)
    assert np.isnan(lme[[0, 2]]).all() and np.isfinite(lme[1]) and np.isnan(ess[[0, 2]]).all() and np.isfinite(ess[1])


def test_four_group_row_keeps_its_margins_and_marks_a_wide_group_with_two_distant_ones_or_none():
    c = Cs.case(Cs.REVERSE, "four256")
    assert [e - s for s, e in c["groups"]] == [5, 256, 14, 1]
    logw, u1, m, cm = A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], c["groups"], c["betas"], c["x"], PhiloxStream(c["seed"]))
    print(f"four256: Bernoulli margin {m:.3g}, categorical margin {cm:.3g}")
    assert m >= Cs.MARGIN and cm >= Cs.FOUR256_CAT_MARGIN >= Cs.CAT_MARGIN and np.isfinite(logw).all()
    for s, e in c["groups"]:
        assert (u1[:, s:e].sum(1) == 1).all()
    s, e = c["groups"][1]
    x = c["x"].copy()
    x[1, s:e] = 0.0
    x[1, s + 3] = x[1, s + 203] = 1.0                                   # more than 64 columns apart
    x[4, s:e] = 0.0                                                     # no one at all
    bad, _, _, _ = A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], c["groups"], c["betas"], x, PhiloxStream(c["seed"]))
    assert np.isnan(bad[[1, 4]]).all() and np.isfinite(np.delete(bad, [1, 4])).all()


# ---- 2. host logic of imdbn/utils/likelihood.py on the test double ----------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_bA", "group", "one"])
def test_schedule_is_what_the_double_consumed(double, name):
    c = Cs.case(Cs.REVERSE, name)
    r = host_rbm(c)
    rng = E.PhiloxRng(5)
    lw, u1 = double.reverse_ais(r, torch.from_numpy(c["x"]), c["betas"], rng, base_vis_bias=_bA(c), return_state=True)
    sched = R.sched_reverse_ais(c["V"], c["H"], c["groups"], c["K"])
    G = len(c["groups"])
    assert [k for k, _ in double.last_log] == [k for k, _ in sched]
    assert [n for k, n in double.last_log if k == "u"] == [n for k, n in sched if k == "u"]
    assert len(sched) == c["K"] * (2 + G) == rng.offset
    assert lw.dtype == torch.float64 and lw.shape == (c["R"],) and u1.shape == (c["R"], c["V"])
    assert R.sched_reverse_ais(3, 2, [], 2) == [("u", 2), ("u", 3), ("u", 2), ("u", 3)]
    assert R.sched_reverse_ais(5, 2, [(3, 5)], 1) == [("u", 2), ("u", 5), ("c", 2)]


def test_function_matches_the_twin_keys_and_the_seed_rule(double):
    c = Cs.case(Cs.REVERSE, "tiny_bA")
    r = host_rbm(c)
    x, M = c["x"], 3
    E.manual_seed(77)
    E.get_rng().advance(3)
    res = LK.reverse_ais_log_likelihood(r, torch.from_numpy(x), n_chains=M, betas=c["betas"], base_vis_bias=_bA(c), seed=9)
    assert E.get_rng().offset == 3 and E.get_rng().seed == 77          # a seed leaves the ambient counter alone
    assert set(res) == {"ll", "ess", "logw"}
    assert res["ll"].dtype == res["ess"].dtype == res["logw"].dtype == torch.float64
    assert res["ll"].shape == res["ess"].shape == (c["R"],) and res["logw"].shape == (c["R"], M)
    logw, _, _, _ = A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], [], c["betas"], np.repeat(x, M, 0), PhiloxStream(9))
    lme, ess = A.rows_logmeanexp(logw, M)
    assert np.array_equal(res["logw"].numpy().reshape(-1), logw)       # row b's chains are the engine rows b M .. b M + M - 1
    assert np.allclose(res["ll"].numpy(), lme - A.log_z_base(c["V"], c["H"], c["bA"], []), rtol=1e-12, atol=1e-12)
    assert np.allclose(res["ess"].numpy(), ess, rtol=1e-12)
    # seed=None draws from the ambient source, from where it stands, and advances it by one schedule
    res2 = r.log_likelihood_conservative(torch.from_numpy(x), n_chains=M, n_betas=c["K"])
    assert E.get_rng().offset == 3 + 2 * c["K"]
    logw2, _, _, _ = A.reverse_ais_logw(c["W"], c["b"], c["c"], None, [], Cs.linear(c["K"]), np.repeat(x, M, 0), PhiloxStream(77, 3))
    assert np.array_equal(res2["logw"].numpy().reshape(-1), logw2)
    assert np.allclose(res2["ll"].numpy(), A.rows_logmeanexp(logw2, M)[0] - (c["V"] + c["H"]) * np.log(2.0), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ["tiny_bA", "group"])
def test_chunking_changes_no_bit(double, name):
    """max_rows 16 against 4096: 4 chains per row, so chunks of 4 test rows against one chunk; a chunk's draws carry its first
    global engine row."""
    c = Cs.case(Cs.REVERSE, name)
    r = host_rbm(c)
    x = torch.from_numpy(Cs.start_rows(11, c["V"], 8, c["groups"]))
    kw = dict(n_chains=4, betas=c["betas"], base_vis_bias=_bA(c), seed=6)
    one = LK.reverse_ais_log_likelihood(r, x, max_rows=4096, **kw)
    assert double.calls[-1] == ("reverse_ais", 44)
    n0 = len(double.calls)
    many = LK.reverse_ais_log_likelihood(r, x, max_rows=16, **kw)
    assert [n for _, n in double.calls[n0:]] == [16, 16, 12]
    for k in ("ll", "ess", "logw"):
        assert torch.equal(one[k], many[k]), k
    # the ambient source advances by ONE schedule however many chunks ran
    E.manual_seed(3)
    LK.reverse_ais_log_likelihood(r, x, n_chains=4, betas=c["betas"], max_rows=16)
    assert E.get_rng().offset == c["K"] * (2 + len(c["groups"]))
    # max_rows below n_chains: one test row per chunk
    tiny = LK.reverse_ais_log_likelihood(r, x[:3], max_rows=1, **kw)
    assert torch.equal(tiny["ll"], one["ll"][:3])


def test_bad_arguments_raise_value_error(double):
    c = Cs.case(Cs.REVERSE, "tiny")
    r = host_rbm(c)
    x = torch.from_numpy(c["x"])
    with pytest.raises(ValueError):
        LK.reverse_ais_log_likelihood(r, x, n_chains=0, n_betas=3)
    with pytest.raises(ValueError):
        LK.reverse_ais_log_likelihood(r, x, n_chains=2, n_betas=0)
    with pytest.raises(ValueError):
        LK.reverse_ais_log_likelihood(r, x, n_chains=2, n_betas=3, max_rows=0)
    with pytest.raises(ValueError):
        LK.reverse_ais_log_likelihood(r, x[:0], n_chains=2, n_betas=3)
    with pytest.raises(ValueError):
        LK.reverse_ais_log_likelihood(r, x[:, :7], n_chains=2, n_betas=3)
    with pytest.raises(ValueError):
        LK.reverse_ais_log_likelihood(r, x, n_chains=2, n_betas=3, base_vis_bias=torch.zeros(3))
    with pytest.raises(ValueError):                                     # a replay tape cannot be keyed on the global row
        with E.use_rng(E.ReplayRng(PhiloxStream(1))):
            LK.reverse_ais_log_likelihood(r, x, n_chains=2, n_betas=3, max_rows=4)
    grouped = host_rbm(c, [(15, 20)])                                       # the AIS side of the sandwich stays binary-only
    with pytest.raises(ValueError):
        LK.evaluate_log_likelihood_sandwich(grouped, loader=[x], n_chains=4, n_betas=3)
    with pytest.raises(ValueError):
        LK.dbn_conservative_bound(r, x, n_samples=0, n_betas=3)


class _Run:
    def __init__(self): self.logged = []
    def log(self, d): self.logged.append(dict(d))


class _Stack:
    """What the evaluate_* functions need of an iDBN: layers (+ val_loader, wandb_run)."""

    def __init__(self, layers, **kw):
        self.layers = layers
        self.__dict__.update(kw)


def _golden_stack():
    """The 100-40-20 stack of the golden pickle, on the CPU."""
    import imdbn.models  # noqa: F401  (the classes the pickle names)
    with open(os.path.join(ROOT, "tests", "golden", "ref_idbn_small.pkl"), "rb") as f:
        obj = pickle.load(f)
    layers = [r.to("cpu") for r in obj["layers"]]
    assert [tuple(r.W.shape) for r in layers] == [(100, 40), (40, 20)]
    return layers


def test_sandwich_over_a_ragged_loader_on_the_golden_stack(double):
    layers = _golden_stack()
    X = torch.from_numpy(Cs.start_rows(11, 100, 4, p=0.25))
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, torch.zeros(11)), batch_size=4)      # 4 + 4 + 3 rows
    m = _Stack(layers, val_loader=loader, wandb_run=_Run())
    bA = LK.base_rate_bias(X)
    E.manual_seed(5)
    kw = dict(n_chains=8, n_betas=6, base_vis_bias=bA, seed=3)
    res = LK.evaluate_log_likelihood_sandwich(m, n_chains_reverse=4, **kw)
    assert E.get_rng().offset == 0
    assert set(res) == {"mean_ll_ais", "mean_ll_reverse", "gap", "n", "log_z", "se", "ess", "ess_reverse"}
    # the AIS side is the existing path, the reverse side continues the same private draw source batch by batch
    est = LK.estimate_log_partition(layers[0], **kw)
    assert res["n"] == 11 and res["log_z"] == pytest.approx(est["log_z"], rel=1e-12)
    assert res["se"] == pytest.approx(est["se"], rel=1e-9) and res["ess"] == pytest.approx(est["ess"], rel=1e-9)
    assert res["mean_ll_ais"] == pytest.approx(float(LK.log_likelihood(layers[0], X, est["log_z"]).mean()), rel=1e-12)
    rng = E.PhiloxRng(3)
    rng.advance(len(R.sched_ais(100, 40, 6)))
    parts = [LK._reverse_rows(layers[0], X[s:s + 4], 4, LK.linear_betas(6), bA, rng, 4096) for s in (0, 4, 8)]
    assert rng.offset == len(R.sched_ais(100, 40, 6)) + 3 * 12
    assert res["mean_ll_reverse"] == pytest.approx(float(torch.cat([p[0] for p in parts]).mean()), rel=1e-12)
    assert res["ess_reverse"] == pytest.approx(float(torch.cat([p[1] for p in parts]).mean()), rel=1e-12)
    assert res["gap"] == pytest.approx(res["mean_ll_ais"] - res["mean_ll_reverse"], rel=1e-9, abs=1e-12)
    assert np.isfinite([res[k] for k in res]).all() and 1.0 <= res["ess_reverse"] <= 4.0
    assert m.wandb_run.logged == [{"ll/" + k: res[k] for k in ("mean_ll_ais", "mean_ll_reverse", "gap", "log_z", "se", "ess", "ess_reverse")}]
    assert LK.evaluate_log_likelihood_sandwich(m, max_batches=2, n_chains_reverse=2, **kw)["n"] == 8
    m.val_loader = None
    assert LK.evaluate_log_likelihood_sandwich(m, **kw) is None            # no loader anywhere
    with pytest.raises(TypeError):
        LK.evaluate_log_likelihood_sandwich(m, loader=loader, chains=3)


def test_sandwich_reports_the_statistics_of_estimate_log_partition(double):
    """The AIS side of the sandwich under a seed IS estimate_log_partition under that seed: equal scalars, not merely close."""
    c = Cs.case(Cs.REVERSE, "tiny_bA")
    r = host_rbm(c)
    for M in (1, 5):                                                    # one chain: se = 0
        kw = dict(n_chains=M, betas=c["betas"], base_vis_bias=_bA(c), seed=4)
        res = LK.evaluate_log_likelihood_sandwich(r, loader=[torch.from_numpy(c["x"])], n_chains_reverse=2, **kw)
        est = LK.estimate_log_partition(r, **kw)
        assert all(res[k] == est[k] for k in ("log_z", "se", "ess")) and np.isfinite([res["log_z"], res["se"], res["ess"]]).all()


def test_conservative_bound_on_the_golden_stack(double):
    layers = _golden_stack()
    X = torch.from_numpy(Cs.start_rows(7, 100, 6, p=0.25))
    m = _Stack(layers)
    S, M, betas = 3, 4, LK.linear_betas(5)
    E.manual_seed(21)
    got = LK.dbn_conservative_bound(m, X, n_samples=S, n_chains=M, betas=betas, seed=8)
    assert E.get_rng().offset == 0 and got.dtype == torch.float64 and got.shape == (7,) and torch.isfinite(got).all()
    # by hand: bound_step in mode entropy on the replicated batch, then the reverse estimate on the sampled top-layer states
    rng = E.PhiloxRng(8)
    acc, h = double.bound_step(layers[0], X.repeat_interleave(S, 0), rng, mode="entropy")
    assert rng.offset == 1
    ll, _, _ = LK._reverse_rows(layers[1], h, M, betas, None, rng, 4096)
    assert rng.offset == 1 + 2 * 5
    assert torch.equal(got, (acc + ll).view(7, S).mean(1))
    # chunking the top layer's engine rows changes no bit
    assert torch.equal(got, LK.dbn_conservative_bound(m, X, n_samples=S, n_chains=M, betas=betas, seed=8, max_rows=8))
    # a stack of one is the reverse estimate itself
    one = LK.dbn_conservative_bound(layers[0], X, n_samples=1, n_chains=M, betas=betas, seed=8)
    assert torch.equal(one, LK.reverse_ais_log_likelihood(layers[0], X, n_chains=M, betas=betas, seed=8)["ll"])
    # the thin method
    from imdbn.models.idbn import iDBN
    d = iDBN.__new__(iDBN)
    d.layers = layers
    assert torch.equal(d.log_likelihood_bound_conservative(X, n_samples=S, n_chains=M, betas=betas, seed=8), got)


def test_evaluate_conservative_bound_over_a_ragged_loader(double):
    layers = _golden_stack()
    X = torch.from_numpy(Cs.start_rows(11, 100, 7, p=0.25))
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, torch.zeros(11)), batch_size=4)
    m = _Stack(layers, val_loader=loader, wandb_run=_Run())
    E.manual_seed(2)
    res = LK.evaluate_dbn_bound_conservative(m, n_samples=2, n_chains=3, n_betas=4)
    assert E.get_rng().offset == 3 * (1 + 2 * 4)                       # ambient draws: one bound_step and one schedule per batch
    E.manual_seed(2)
    parts = torch.cat([LK.dbn_conservative_bound(m, X[s:s + 4], n_samples=2, n_chains=3, n_betas=4) for s in (0, 4, 8)])
    assert res["n"] == 11 and res["n_samples"] == 2 and res["n_chains"] == 3
    assert res["sum_bound"] == pytest.approx(float(parts.sum()), rel=1e-12) and res["mean_bound"] == pytest.approx(float(parts.mean()), rel=1e-12)
    assert 1.0 <= res["ess_reverse"] <= 3.0
    assert m.wandb_run.logged == [{"ll/dbn_conservative_mean_bound": res["mean_bound"], "ll/dbn_conservative_ess_reverse": res["ess_reverse"],
                                   "ll/dbn_conservative_n_samples": 2, "ll/dbn_conservative_n_chains": 3}]
    assert LK.evaluate_dbn_bound_conservative(m, n_samples=1, n_chains=2, n_betas=3, max_batches=1, seed=4)["n"] == 4
    m.val_loader = None
    assert LK.evaluate_dbn_bound_conservative(m) is None


def test_existing_entry_points_keep_their_results(double):
    """The functions that were there return what they returned: the double's ais / bound_step are the parents' own."""
    c = Cs.case(Cs.REVERSE, "tiny_bA")
    r = host_rbm(c)
    a = LK.estimate_log_partition(r, n_chains=5, betas=c["betas"], base_vis_bias=_bA(c), seed=1)
    LK.reverse_ais_log_likelihood(r, torch.from_numpy(c["x"]), n_chains=2, betas=c["betas"], seed=1)
    b = LK.estimate_log_partition(r, n_chains=5, betas=c["betas"], base_vis_bias=_bA(c), seed=1)
    assert a["log_z"] == b["log_z"] and torch.equal(a["logw"], b["logw"])
    assert {"reverse_ais_log_likelihood", "evaluate_log_likelihood_sandwich", "dbn_conservative_bound",
            "evaluate_dbn_bound_conservative", "estimate_log_partition", "dbn_lower_bound", "imdbn_lower_bound"} <= set(LK.__all__)


# ---- 3. ABI -----------------------------------------------------------------------------------------------------------
def test_exports_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    assert re.search(r"\bint\s+imdbn_rbm_reverse_ais\s*\(", src) and re.search(r"\bint\s+imdbn_rows_logmeanexp\s*\(", src)
    assert "#define IMDBN_ABI_VERSION 4" in src and native.ABI_VERSION == 4
    assert len(native.SIGNATURES["imdbn_rbm_reverse_ais"][1]) == 14        # (test_abi_cpu.py holds the library to every declared symbol)
    assert len(native.SIGNATURES["imdbn_rows_logmeanexp"][1]) == 6
