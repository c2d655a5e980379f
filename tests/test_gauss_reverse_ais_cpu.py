"""CPU-only: the numpy twin of imdbn_rbm_gauss_reverse_ais (tests/gauss_reverse_ais_oracle.py) against the enumerated log-density,
the host logic of the Gaussian reverse-AIS functions of imdbn/utils/likelihood.py on a test double of the engine
(tests/gauss_reverse_engine_double.py), the draw schedule and the export's declaration and binding.

Truth: V = 20, H = 12 (the parameters of gauss_ais_cases.truth), K = 200 linear, 16 chains per row, 32 rows v = b + e^{z/2} n, under
the project's Philox draws, seeds 1-8.  Run once (`python tests/gauss_reverse_ais_cases.py`): exact mean log p -30.8078; the twin's
mean ll was -30.8015 -30.7981 -30.8011 -30.8020 -30.8018 -30.8120 -30.8193 -30.8191 with b_A = b (slack 0.0258 = 3 sample standard
deviations) and -30.7987 -30.8043 -30.8015 -30.8018 -30.8028 -30.8081 -30.8178 -30.8180 with the shifted b_A (slack 0.0224).
Stack 6-5-4 (S = 8, 16 chains, K = 100): exact variational bound -10.7596, mean of the twin over the seeds -10.7666, slack 0.1128 =
3 standard errors of that mean.  The slacks are recomputed here from the twin, not fixed."""
import os
import re

import numpy as np
import pytest
import torch

import anneal_oracle as A
import gauss_ais_oracle as GA
import gauss_bound_cases as GBC
import gauss_reverse_ais_cases as Cs
import gauss_reverse_ais_oracle as GR
from gauss_reverse_engine_double import GaussReverseOracleEngine
from imdbn import engine as E
from imdbn.engine import native, rng as R
from imdbn.utils import likelihood as LK
from oracle.draws import PhiloxStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
_CACHE = {}


def _once(key, compute):
    if key not in _CACHE:
        _CACHE[key] = compute()
    return _CACHE[key]


@pytest.fixture()
def double():
    eng = GaussReverseOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)
    E.set_rng(None)


def _grbm(c):
    from imdbn.models import GaussianRBM
    W = c["W"]
    r = GaussianRBM(W.shape[0], W.shape[1], 0.01, 0.0, 0.5).to("cpu")
    r.W.data = torch.from_numpy(np.array(W, F32))
    r.vis_bias.data, r.hid_bias.data = torch.from_numpy(np.array(c["b"], F32)), torch.from_numpy(np.array(c["c"], F32))
    r.logvar.data = torch.from_numpy(np.array(c["z"], F32))
    return r


def _bA(c):
    return None if c["bA"] is None else torch.from_numpy(c["bA"])


class _Run:
    def __init__(self): self.logged = []
    def log(self, d): self.logged.append(dict(d))


class _Stack:
    def __init__(self, layers, **kw):
        self.layers = layers
        self.__dict__.update(kw)


# ---- 1. the twin against enumeration ----------------------------------------------------------------------------------------------
def test_the_enumerated_log_density_is_minus_free_energy_minus_the_enumerated_log_z():
    c = Cs.truth(False)
    W, b, cc, z, x = (np.asarray(t, F64) for t in (c["W"], c["b"], c["c"], c["z"], c["x"]))
    d = x - b[None, :]
    negF = -(d * d * np.exp(-z) / 2.0).sum(1) + A.softplus((x * np.exp(-z)[None, :]) @ W + cc[None, :]).sum(1)
    assert np.allclose(c["exact"], negF - GA.exact_log_z(W, b, cc, z), rtol=0, atol=1e-10)


@pytest.mark.parametrize("with_bA", [False, True])
def test_twin_mean_ll_stays_below_the_exact_mean_plus_the_slack_for_every_seed(with_bA):
    c = Cs.truth(with_bA)
    slack, means = _once(("truth", with_bA), lambda: Cs.truth_slack(with_bA))
    exact = float(c["exact"].mean())
    print(f"b_A {with_bA}: exact mean log p {exact:.4f}, twin mean ll of seeds 1-8 {means.round(4).tolist()}, slack {slack:.4f}")
    assert 0 < slack < 0.1
    assert (means <= exact + slack).all()
    assert (means >= exact - 10 * slack).all()          # and it is an estimate of that number, not merely small


@pytest.mark.parametrize("seed", Cs.TRUTH_SEEDS)
def test_sandwich_reverse_side_stays_below_the_ais_side_plus_the_slack(double, seed):
    c = Cs.truth(False)
    slack, _ = _once(("truth", False), lambda: Cs.truth_slack(False))
    r = _grbm(c)
    res = LK.evaluate_gaussian_log_likelihood_sandwich(r, loader=[torch.from_numpy(c["x"])], n_chains=64, betas=c["betas"],
                                                       n_chains_reverse=c["chains"], seed=seed)
    print(f"seed {seed}: ais {res['mean_ll_ais']:.4f} reverse {res['mean_ll_reverse']:.4f} gap {res['gap']:+.4f} slack {slack:.4f}")
    assert res["n"] == Cs.TRUTH["rows"] and res["mean_ll_reverse"] <= res["mean_ll_ais"] + slack
    assert res["gap"] == pytest.approx(res["mean_ll_ais"] - res["mean_ll_reverse"], rel=1e-9, abs=1e-12)


def test_stack_bound_mean_over_the_seeds_stays_below_the_enumerated_bound_plus_the_slack(double):
    from imdbn.models import RBM
    z, layers, v = GBC.truth_stack()
    bottom = _grbm(dict(W=layers[0][0], b=layers[0][1], c=layers[0][2], z=z))
    W, b, c = layers[1]
    top = RBM(*W.shape, 0.1, 0.0, 0.5).to("cpu")
    top.W.data, top.vis_bias.data, top.hid_bias.data = (torch.from_numpy(np.array(t, F32)) for t in (W, b, c))
    m = _Stack([bottom, top])
    slack, twin = _once("stack", Cs.stack_slack)
    exact = Cs.stack_exact()
    S, M, K = Cs.STACK["S"], Cs.STACK["chains"], Cs.STACK["K"]
    got = np.array([float(LK.gaussian_dbn_conservative_bound(m, torch.from_numpy(v), n_samples=S, n_chains=M, n_betas=K, seed=s).mean())
                    for s in Cs.TRUTH_SEEDS])
    print(f"stack: exact bound {exact:.4f}, per seed {got.round(4).tolist()}, mean {got.mean():.4f}, slack {slack:.4f}")
    assert np.allclose(got, twin, rtol=0, atol=1e-5)          # the composition is the twin's: gauss_bound_step, then reverse AIS on h
    assert got.mean() <= exact + slack
    assert [c[0] for c in double.calls[:2]] == ["gauss_bound_step", "reverse_ais"] and double.calls[0][2] == "entropy"
    assert not [c for c in double.calls if c[0] == "gauss_reverse_ais"]


# ---- 2. host logic through the double -------------------------------------------------------------------------------------------------
def test_ll_matches_the_restatement_and_follows_the_seed_rule(double):
    c = Cs.case("tiny", True)
    r = _grbm(c)
    x, M = torch.from_numpy(c["v"]), 3
    E.manual_seed(77)
    E.get_rng().advance(3)
    res = LK.gaussian_reverse_ais_log_likelihood(r, x, n_chains=M, betas=c["betas"], base_vis_bias=_bA(c), seed=9)
    assert E.get_rng().offset == 3 and E.get_rng().seed == 77                  # seed=int: a private source
    assert double.calls[-1] == ("gauss_reverse_ais", c["R"] * M, c["K"], True)
    assert set(res) == {"ll", "ess", "logw"}
    assert res["ll"].shape == (c["R"],) and res["ess"].shape == (c["R"],) and res["logw"].shape == (c["R"], M)
    assert all(res[k].dtype == torch.float64 for k in res)
    logw, _, _ = GR.gauss_reverse_ais_logw(c["W"], c["b"], c["c"], c["z"], c["bA"], c["betas"], np.repeat(c["v"], M, 0), PhiloxStream(9), dt=F32)
    assert np.array_equal(res["logw"].numpy().reshape(-1), logw)
    lme, ess = A.rows_logmeanexp(logw, M)
    assert np.allclose(res["ll"].numpy(), lme - GA.log_z_base(c["V"], c["H"], c["z"]), rtol=1e-12, atol=1e-12)
    assert np.allclose(res["ess"].numpy(), ess, rtol=1e-12)
    # seed=None draws from the ambient source and advances it by one schedule; no base bias = the RBM's own; the thin method
    res2 = r.gaussian_log_likelihood_conservative(x, n_chains=M, betas=c["betas"])
    assert E.get_rng().offset == 3 + 2 * c["K"] and double.calls[-1] == ("gauss_reverse_ais", c["R"] * M, c["K"], False)
    logw2, _, _ = GR.gauss_reverse_ais_logw(c["W"], c["b"], c["c"], c["z"], None, c["betas"], np.repeat(c["v"], M, 0), PhiloxStream(77, 3), dt=F32)
    assert np.array_equal(res2["logw"].numpy().reshape(-1), logw2)


def test_chunking_changes_no_bit_and_the_source_advances_by_one_schedule(double):
    """max_rows 16 against 4096: 4 chains per row, so chunks of 4 test rows against one chunk; a chunk's draws carry its first
    global engine row."""
    c = Cs.case("rows70", True)
    r = _grbm(c)
    x = torch.from_numpy(c["v"][:11])
    kw = dict(n_chains=4, betas=c["betas"], base_vis_bias=_bA(c), seed=6)
    one = LK.gaussian_reverse_ais_log_likelihood(r, x, max_rows=4096, **kw)
    assert double.calls[-1][:2] == ("gauss_reverse_ais", 44)
    n0 = len(double.calls)
    many = LK.gaussian_reverse_ais_log_likelihood(r, x, max_rows=16, **kw)
    assert [n for _, n, _, _ in double.calls[n0:]] == [16, 16, 12]
    for k in ("ll", "ess", "logw"):
        assert torch.equal(one[k], many[k]), k
    E.manual_seed(3)
    LK.gaussian_reverse_ais_log_likelihood(r, x, n_chains=4, betas=c["betas"], max_rows=16)
    assert E.get_rng().offset == 2 * c["K"]
    tiny = LK.gaussian_reverse_ais_log_likelihood(r, x[:3], max_rows=1, **kw)          # max_rows below n_chains: one test row per chunk
    assert torch.equal(tiny["ll"], one["ll"][:3])


def test_a_non_finite_row_is_nan_in_that_row_only(double):
    c = Cs.case("tiny", False)
    r = _grbm(c)
    x = torch.from_numpy(c["v"].copy())
    x[2, 7] = float("inf")
    res = LK.gaussian_reverse_ais_log_likelihood(r, x, n_chains=2, betas=c["betas"], seed=1)
    assert torch.isnan(res["ll"]).tolist() == [False, False, True, False, False] and torch.isnan(res["logw"][2]).all()


def test_bad_arguments_raise_value_error(double):
    c = Cs.case("tiny", False)
    r = _grbm(c)
    x = torch.from_numpy(c["v"])
    f = LK.gaussian_reverse_ais_log_likelihood
    for kw in (dict(n_chains=0, n_betas=3), dict(n_chains=2, n_betas=0), dict(n_chains=2, n_betas=3, max_rows=0),
               dict(n_chains=2, n_betas=3, base_vis_bias=torch.zeros(3))):
        with pytest.raises(ValueError):
            f(r, x, **kw)
    with pytest.raises(ValueError, match="gaussian_reverse_ais_log_likelihood: no rows"):
        f(r, x[:0], n_chains=2, n_betas=3)
    with pytest.raises(ValueError, match="rows of 7 elements"):
        f(r, x[:, :7], n_chains=2, n_betas=3)
    with pytest.raises(ValueError, match="PhiloxRng"):                      # a replay tape cannot be keyed on the global row
        with E.use_rng(E.ReplayRng(PhiloxStream(1))):
            f(r, x, n_chains=2, n_betas=3, max_rows=4)
    with pytest.raises(TypeError, match="evaluate_gaussian_log_likelihood_sandwich"):
        LK.evaluate_gaussian_log_likelihood_sandwich(r, loader=[x], chains=3)
    with pytest.raises(ValueError):
        LK.gaussian_dbn_conservative_bound(r, x, n_samples=0, n_betas=3)
    assert not double.calls


def test_sandwich_over_a_ragged_loader_makes_one_host_copy_and_logs_its_scalars(double, monkeypatch):
    c = Cs.case("rows70", True)
    r = _grbm(c)
    X = torch.from_numpy(c["v"][:11])
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, torch.zeros(11)), batch_size=4)      # 4 + 4 + 3 rows
    m = _Stack([r, object()], val_loader=loader, wandb_run=_Run())
    kw = dict(n_chains=8, n_betas=6, base_vis_bias=_bA(c), seed=3)
    copies = []
    real = torch.Tensor.cpu

    def counted(self, *a, **k):                                                 # (the double reads its fp32 inputs with .cpu() too)
        if self.dtype == torch.float64:
            copies.append(tuple(self.shape))
        return real(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", counted)
    E.manual_seed(5)
    res = LK.evaluate_gaussian_log_likelihood_sandwich(m, n_chains_reverse=4, **kw)
    assert copies == [(7,)]                                                     # three sums and the four AIS statistics, in one copy
    monkeypatch.setattr(torch.Tensor, "cpu", real)
    assert E.get_rng().offset == 0
    assert set(res) == {"mean_ll_ais", "mean_ll_reverse", "gap", "n", "log_z", "se", "ess", "ess_reverse"}
    est = LK.estimate_gaussian_log_partition(r, **kw)
    assert res["n"] == 11 and all(res[k] == est[k] for k in ("log_z", "se", "ess"))
    assert res["mean_ll_ais"] == pytest.approx(float(LK.gaussian_log_likelihood(r, X, est["log_z"]).mean()), rel=1e-12)
    # the reverse side continues the same private draw source batch by batch
    rng = E.PhiloxRng(3)
    rng.advance(len(R.sched_gauss_ais(c["V"], c["H"], 6)))
    parts = [LK._reverse_rows(r, X[s:s + 4], 4, LK.linear_betas(6), _bA(c), rng, 4096, LK._REVERSE_GAUSSIAN) for s in (0, 4, 8)]
    assert rng.offset == 2 * 6 - 1 + 3 * 12
    assert res["mean_ll_reverse"] == pytest.approx(float(torch.cat([p[0] for p in parts]).mean()), rel=1e-12)
    assert res["ess_reverse"] == pytest.approx(float(torch.cat([p[1] for p in parts]).mean()), rel=1e-12)
    assert np.isfinite([res[k] for k in res]).all() and 1.0 <= res["ess_reverse"] <= 4.0
    assert m.wandb_run.logged == [{"ll/gaussian_" + k: res[k] for k in ("mean_ll_ais", "mean_ll_reverse", "gap", "log_z", "se", "ess",
                                                                        "ess_reverse")}]
    assert LK.evaluate_gaussian_log_likelihood_sandwich(m, max_batches=2, n_chains_reverse=2, **kw)["n"] == 8
    m.val_loader = None
    assert LK.evaluate_gaussian_log_likelihood_sandwich(m, **kw) is None        # no loader anywhere


def _idbn(double):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import iDBN
    g = np.random.Generator(np.random.PCG64(3))
    X = torch.from_numpy((0.5 + 2.0 * g.standard_normal((11, 12))).astype(F32))
    dl = DataLoader(TensorDataset(X, torch.zeros(11)), batch_size=4)
    params = {"LEARNING_RATE": 0.05, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95, "LEARNING_RATE_DYNAMIC": True,
              "CD": 1, "GAUSSIAN_VISIBLE": True}
    torch.manual_seed(0)
    net = iDBN([12, 7, 5], params, dl, dl, torch.device("cpu"))
    for r in net.layers:
        r.W.data = r.W.data.contiguous()
    net.layers[0].init_from_data(X)
    return net, X, dl


def test_conservative_bound_of_an_idbn_with_a_gaussian_bottom(double):
    net, X, dl = _idbn(double)
    S, M, betas = 3, 4, LK.linear_betas(5)
    E.manual_seed(21)
    got = LK.gaussian_dbn_conservative_bound(net, X, n_samples=S, n_chains=M, betas=betas, seed=8)
    assert E.get_rng().offset == 0 and got.dtype == torch.float64 and got.shape == (11,) and torch.isfinite(got).all()
    # by hand: the Gaussian bracket in mode entropy on the replicated batch, then the Bernoulli reverse estimate on the sampled h
    rng = E.PhiloxRng(8)
    acc, h = double.gauss_bound_step(net.layers[0], net.layers[0].logvar.data, X.repeat_interleave(S, 0), rng, mode="entropy")
    ll, _, _ = LK._reverse_rows(net.layers[1], h, M, betas, None, rng, 4096)
    assert rng.offset == 1 + 2 * 5
    assert torch.equal(got, (acc + ll).view(11, S).mean(1))
    assert torch.equal(got, LK.gaussian_dbn_conservative_bound(net, X, n_samples=S, n_chains=M, betas=betas, seed=8, max_rows=8))
    assert torch.equal(got, net.gaussian_log_likelihood_bound_conservative(X, n_samples=S, n_chains=M, betas=betas, seed=8))
    # a stack of one is the Gaussian reverse estimate itself
    one = LK.gaussian_dbn_conservative_bound(net.layers[0], X, n_samples=1, n_chains=M, betas=betas, seed=8)
    assert torch.equal(one, LK.gaussian_reverse_ais_log_likelihood(net.layers[0], X, n_chains=M, betas=betas, seed=8)["ll"])
    # over the loader
    net.wandb_run = _Run()
    E.manual_seed(2)
    res = LK.evaluate_gaussian_dbn_bound_conservative(net, n_samples=2, n_chains=3, n_betas=4)
    assert E.get_rng().offset == 3 * (1 + 2 * 4)                       # ambient draws: one bracket and one schedule per batch
    E.manual_seed(2)
    parts = torch.cat([LK.gaussian_dbn_conservative_bound(net, X[s:s + 4], n_samples=2, n_chains=3, n_betas=4) for s in (0, 4, 8)])
    assert set(res) == {"mean_bound", "sum_bound", "n", "ess_reverse", "n_samples", "n_chains"}
    assert res["n"] == 11 and res["sum_bound"] == pytest.approx(float(parts.sum()), rel=1e-12)
    assert res["mean_bound"] == pytest.approx(float(parts.mean()), rel=1e-12) and 1.0 <= res["ess_reverse"] <= 3.0
    assert net.wandb_run.logged == [{"ll/gdbn_conservative_mean_bound": res["mean_bound"], "ll/gdbn_conservative_ess_reverse": res["ess_reverse"],
                                     "ll/gdbn_conservative_n_samples": 2, "ll/gdbn_conservative_n_chains": 3}]
    net.val_loader = None
    assert LK.evaluate_gaussian_dbn_bound_conservative(net) is None


def test_each_family_refuses_the_others_layers(double):
    from imdbn.models import RBM, grbm
    net, X, dl = _idbn(double)
    g, plain = net.layers[0], RBM(12, 7, 0.1, 0.0, 0.5).to("cpu")
    B = (X > 0.5).float()
    for call in (lambda: LK.gaussian_reverse_ais_log_likelihood(plain, X, n_chains=2, n_betas=3, seed=1),
                 lambda: LK.evaluate_gaussian_log_likelihood_sandwich(plain, loader=dl, n_chains=4, n_betas=3),
                 lambda: LK.evaluate_gaussian_log_likelihood_sandwich(net.layers[1], loader=dl, n_chains=4, n_betas=3),
                 lambda: LK.gaussian_dbn_conservative_bound(plain, B, n_samples=1, n_chains=2, n_betas=3),
                 lambda: LK.evaluate_gaussian_dbn_bound_conservative(plain, loader=dl, n_samples=1, n_chains=2, n_betas=3)):
        with pytest.raises(ValueError, match="GaussianRBM"):
            call()
    for call in (lambda: LK.reverse_ais_log_likelihood(g, B, n_chains=2, n_betas=3, seed=1),
                 lambda: LK.evaluate_log_likelihood_sandwich(g, loader=[B], n_chains=4, n_betas=3),
                 lambda: LK.evaluate_log_likelihood_sandwich(net, loader=[B], n_chains=4, n_betas=3),
                 lambda: LK.dbn_conservative_bound(net, B, n_samples=1, n_chains=2, n_betas=3),
                 lambda: LK.evaluate_dbn_bound_conservative(net, loader=[B], n_samples=1, n_chains=2, n_betas=3),
                 lambda: g.log_likelihood_conservative(B), lambda: net.log_likelihood_bound_conservative(B)):
        with pytest.raises(ValueError, match="Gaussian"):
            call()
    assert "log_likelihood_conservative" in grbm.REFUSED and "gaussian_log_likelihood_conservative" not in grbm.REFUSED
    assert not [c for c in double.calls if c[0] in ("gauss_reverse_ais", "reverse_ais", "gauss_ais")]
    assert {"gaussian_reverse_ais_log_likelihood", "evaluate_gaussian_log_likelihood_sandwich", "gaussian_dbn_conservative_bound",
            "evaluate_gaussian_dbn_bound_conservative"} <= set(LK.__all__)


def test_the_bernoulli_results_keep_their_bits(double):
    """One chunking path serves both families: the Bernoulli side still equals its twin, bit for bit."""
    import anneal_cases as AC
    from bound_oracle import host_rbm
    c = AC.case(AC.REVERSE, "tiny_bA")
    r = host_rbm(c)
    x, M = c["x"], 3
    res = LK.reverse_ais_log_likelihood(r, torch.from_numpy(x), n_chains=M, betas=c["betas"], base_vis_bias=torch.from_numpy(c["bA"]), seed=9)
    logw, _, _, _ = A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], [], c["betas"], np.repeat(x, M, 0), PhiloxStream(9))
    assert np.array_equal(res["logw"].numpy().reshape(-1), logw)


# ---- 3. the draw schedule and the twin's form -------------------------------------------------------------------------------------------
def test_the_schedule_is_what_the_twin_draws():
    assert R.sched_gauss_reverse_ais(3, 2, 1) == [("u", 2), ("n", 3)]
    c = Cs.case("tiny", True)
    ps = PhiloxStream(5)
    GR.gauss_reverse_ais_logw(c["W"], c["b"], c["c"], c["z"], c["bA"], c["betas"], c["v"], ps)
    assert [(k, shape[1]) for k, shape in ps.log] == R.sched_gauss_reverse_ais(c["V"], c["H"], c["K"]) and ps.offset == 2 * c["K"]


def test_without_weights_the_weight_is_the_normal_log_density_times_z_a():
    """W = 0 and b_A = b: the softplus sums telescope and t_v vanishes, so logw - log Z_A = log N(v; b, e^z) whatever K and the draws."""
    c = Cs.case("tiny", False)
    W0 = np.zeros_like(c["W"])
    logw, _, _ = GR.gauss_reverse_ais_logw(W0, c["b"], c["c"], c["z"], None, c["betas"], c["v"], PhiloxStream(2))
    b, z, v = (np.asarray(t, F64) for t in (c["b"], c["z"], c["v"]))
    want = (-(v - b) ** 2 * np.exp(-z) / 2.0 - z / 2.0).sum(1) - 0.5 * c["V"] * np.log(2 * np.pi)
    got = logw - GA.log_z_base(c["V"], c["H"], c["z"])
    assert np.allclose(got, want, rtol=1e-9, atol=0)


def test_every_parity_seed_is_the_first_clear_of_a_tie_where_the_restatement_draws_the_same_h():
    for c, kind in Cs.all_runs():
        seed = c["seed"] if kind == "replay" else c["philox_seed"]
        assert next(s for s in range(1, 65) if Cs.seed_ok(c, kind, s)) == seed, (c["name"], c["bA"] is not None, kind)
        e = Cs.fp32_error(c, kind)
        print(f"{c['name']} b_A={c['bA'] is not None} {kind}: fp32 restatement vs float64 twin {e}")
        assert 0 < e["logw"] < 1e-5 and 0 < e["v"] < 1e-5


# ---- 4. ABI -------------------------------------------------------------------------------------------------------------------------------
def test_export_is_declared_bound_and_present():
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    assert re.search(r"\bint\s+imdbn_rbm_gauss_reverse_ais\s*\(", src) and "#define IMDBN_ABI_VERSION 4" in src
    res, args = native.SIGNATURES["imdbn_rbm_gauss_reverse_ais"]
    assert len(args) == 15
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("native library not built")
    assert hasattr(native.lib(), "imdbn_rbm_gauss_reverse_ais")
