"""CPU-only: the numpy twin of imdbn_rbm_gauss_ais (tests/gauss_ais_oracle.py) against the enumerated partition function, the host
logic of the Gaussian likelihood functions of imdbn/utils/likelihood.py on a test double of the engine, the draw schedule and the
export's declaration and binding.

Truth: V = 20, H = 12, K = 200 linear temperatures, M = 64 chains, W ~ 0.2 N, b ~ 0.5 N, c ~ 0.3 N, z ~ 0.4 N, with b_A = b and with
b_A = b + 0.3 N, under the project's Philox draws; |log Z_hat - exact| <= 3 se.  Seeds 1..8 were run once (`python
tests/gauss_ais_cases.py`): the errors in se were -0.68 +0.75 +0.53 -0.29 -0.09 -1.05 -0.42 +0.01 with b_A = b and -0.15 -0.02 +1.27
-0.46 +0.12 -0.15 +0.05 +0.56 with the shifted b_A, se <= 0.022, ess >= 62.1 of 64; seed 1 is pinned (gauss_ais_cases.TRUTH_SEED)."""
import os
import re

import numpy as np
import pytest
import torch

import anneal_oracle as A
import gauss_ais_cases as Cs
import gauss_ais_oracle as GA
import gauss_oracle as G
from gauss_engine_double import GaussOracleEngine
from imdbn import engine as E
from imdbn.engine import native, rng as R
from imdbn.utils import likelihood as LK
from oracle.draws import PhiloxStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.fixture()
def double():
    eng = GaussOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)
    E.set_rng(None)


def _grbm(W, b, c, z):
    from imdbn.models import GaussianRBM
    r = GaussianRBM(W.shape[0], W.shape[1], 0.01, 0.0, 0.5).to("cpu")
    r.W.data = torch.from_numpy(np.array(W, F32))
    r.vis_bias.data, r.hid_bias.data = torch.from_numpy(np.array(b, F32)), torch.from_numpy(np.array(c, F32))
    r.logvar.data = torch.from_numpy(np.array(z, F32))
    return r


def _small(V=6, H=4, rows=32, seed=41):
    g = np.random.Generator(np.random.PCG64(seed))
    W, b, c, z, bA = Cs._params(V, H, g, 0.2)
    data = (b + np.exp(0.5 * z) * g.standard_normal((rows, V))).astype(F32)
    return W, b, c, z, bA, data


# ---- 1. the twin against enumeration ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bA", [False, True])
def test_twin_estimate_is_within_three_standard_errors_of_the_enumerated_log_z(with_bA):
    c = Cs.truth(with_bA)
    exact = GA.exact_log_z(c["W"], c["b"], c["c"], c["z"])
    t = Cs.twin_run(c, "philox", c["seed"])
    lme, se, ess = A.weight_stats(t["logw"])
    log_z = GA.log_z_base(c["V"], c["H"], c["z"]) + lme
    print(f"b_A {with_bA}: log Z_hat {log_z:.4f}, exact {exact:.4f}, error {(log_z - exact) / se:+.2f} se, se {se:.4f}, ess {ess:.1f} of {c['M']}")
    assert t["v"].shape == (c["M"], c["V"]) and np.isfinite(t["v"]).all()
    assert 0 < se <= 0.04
    assert abs(log_z - exact) <= 3 * se


def test_the_enumeration_agrees_with_the_gaussian_twins_log_partition():
    """exact_log_z (the issue's formula) against tests/gauss_oracle.log_partition, which integrates v in another form."""
    W, b, c, z, _, _ = _small()
    assert GA.exact_log_z(W, b, c, z) == pytest.approx(G.log_partition(*(np.asarray(x, F64) for x in (W, b, c, z)))[0], rel=1e-12)


# ---- 2. the telescope ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bA", [False, True])
def test_one_temperature_without_weights_telescopes_to_the_closed_form(with_bA):
    """K = 1 and W = 0: the model factorises, log Z = log Z_A - H log 2 + sum_j softplus(c_j) in closed form, every chain's weight is
    sum_j softplus(c_j) - H log 2 + the visible term.  With b_A = b the visible term is zero and every weight IS that constant."""
    W, b, c, z, bA, _ = _small()
    W = np.zeros_like(W)
    ps = PhiloxStream(3)
    logw, v, margin = GA.gauss_ais_logw(W, b, c, z, bA if with_bA else None, np.array([0, 1], F32), 6, ps)
    assert ps.log == [("n", (6, 6))] and margin == np.inf
    const = float(A.softplus(c.astype(F64)).sum() - 4 * np.log(2.0))
    b64, bA64 = b.astype(F64), (bA if with_bA else b).astype(F64)
    want = const + (((b64 - bA64) * np.exp(-z.astype(F64)))[None, :] * (v.astype(F64) - 0.5 * (b64 + bA64)[None, :])).sum(1)
    assert np.allclose(logw, want, rtol=0, atol=1e-12)
    exact = GA.exact_log_z(W, b, c, z)
    assert exact == pytest.approx(GA.log_z_base(6, 4, z) + const, abs=1e-12)
    if not with_bA:
        assert np.array_equal(logw, np.full(6, logw[0])) and abs(logw[0] - const) <= 1e-12
        assert abs(GA.log_z_base(6, 4, z) + A.logmeanexp(logw) - exact) <= 1e-12


# ---- 3. through the double: the mean log-likelihood against enumeration ------------------------------------------------------------
def test_evaluate_gaussian_log_likelihood_is_within_three_se_of_the_exact_mean(double):
    W, b, c, z, bA, data = _small()
    r = _grbm(W, b, c, z)
    X = torch.from_numpy(data)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, torch.zeros(32)), batch_size=12)      # 12 + 12 + 8 rows
    want = G.mean_log_likelihood(*(np.asarray(x, F64) for x in (W, b, c, z)), data.astype(F64))
    for base in (None, LK.gaussian_base_rate_bias(X)):
        res = LK.evaluate_gaussian_log_likelihood(r, loader=loader, n_chains=64, n_betas=200, base_vis_bias=base, seed=1)
        print(f"b_A {'data means' if base is not None else 'b'}: mean ll {res['mean_ll']:.4f}, exact {want:.4f}, "
              f"error {(res['mean_ll'] - want) / res['se']:+.2f} se, se {res['se']:.4f}, ess {res['ess']:.1f}")
        assert res["n"] == 32 and 0 < res["se"] < 0.05
        assert abs(res["mean_ll"] - want) <= 3 * res["se"]


# ---- 4. host logic -------------------------------------------------------------------------------------------------------------------
def test_estimate_matches_the_restatement_and_follows_the_seed_rule(double):
    c = Cs.case("tiny", True)
    r = _grbm(c["W"], c["b"], c["c"], c["z"])
    bA = torch.from_numpy(c["bA"])
    E.manual_seed(77)
    E.get_rng().advance(3)
    est = LK.estimate_gaussian_log_partition(r, n_chains=c["M"], betas=c["betas"], base_vis_bias=bA, seed=9)
    assert E.get_rng().offset == 3 and E.get_rng().seed == 77                  # seed=int: a private source
    assert double.calls[-1] == ("gauss_ais", c["M"], c["K"], True)
    logw, _, _ = GA.gauss_ais_logw(c["W"], c["b"], c["c"], c["z"], c["bA"], c["betas"], c["M"], PhiloxStream(9), dt=F32)
    lme, se, ess = A.weight_stats(logw)
    lzb = GA.log_z_base(c["V"], c["H"], c["z"])
    assert set(est) == {"log_z", "log_z_base", "logw", "ess", "se"}
    assert np.array_equal(est["logw"].numpy(), logw) and est["logw"].dtype == torch.float64
    assert est["log_z_base"] == pytest.approx(lzb, rel=1e-12) and est["log_z"] == pytest.approx(lzb + lme, rel=1e-12)
    assert est["se"] == pytest.approx(se, rel=1e-9) and est["ess"] == pytest.approx(ess, rel=1e-9)
    # seed=None draws from the ambient source, from where it stands; no base bias = the RBM's own
    est2 = r.gaussian_log_partition(n_chains=c["M"], betas=c["betas"])
    assert E.get_rng().offset == 3 + 2 * c["K"] - 1 and double.calls[-1] == ("gauss_ais", c["M"], c["K"], False)
    logw2, _, _ = GA.gauss_ais_logw(c["W"], c["b"], c["c"], c["z"], None, c["betas"], c["M"], PhiloxStream(77, 3), dt=F32)
    assert np.array_equal(est2["logw"].numpy(), logw2)
    with pytest.raises(ValueError):
        LK.estimate_gaussian_log_partition(r, n_chains=4, n_betas=3, base_vis_bias=bA[:-1], seed=1)


def test_log_likelihood_is_minus_free_energy_minus_log_z_and_the_mean_is_the_column_mean(double):
    c = Cs.case("tiny", False)
    r = _grbm(c["W"], c["b"], c["c"], c["z"])
    g = np.random.Generator(np.random.PCG64(4))
    v = torch.from_numpy(g.standard_normal((6, c["V"])).astype(F32))
    ll = r.gaussian_log_likelihood(v, 12.5)
    assert ll.dtype == torch.float64 and ll.shape == (6,)
    assert torch.equal(ll, -r.free_energy(v).double() - 12.5) and torch.equal(ll, LK.gaussian_log_likelihood(r, v, 12.5))
    X = torch.from_numpy((3.0 + g.standard_normal((10, 5))).astype(F32))
    got = LK.gaussian_base_rate_bias(X)
    assert got.dtype == torch.float32 and np.allclose(got.numpy(), X.numpy().astype(F64).mean(0), rtol=1e-6)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, torch.zeros(10)), batch_size=4)
    assert np.allclose(LK.gaussian_base_rate_bias(loader).numpy(), got.numpy(), rtol=1e-6)


class _Run:
    def __init__(self): self.logged = []
    def log(self, d): self.logged.append(dict(d))


def test_evaluate_makes_one_host_copy_and_logs_its_scalars(double, monkeypatch):
    W, b, c, z, _, data = _small(rows=11)
    r = _grbm(W, b, c, z)
    X = torch.from_numpy(data)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, torch.zeros(11)), batch_size=4)      # 4 + 4 + 3 rows
    copies = []
    real = torch.Tensor.cpu

    def counted(self, *a, **k):                                                 # (the double reads its fp32 inputs with .cpu() too)
        if self.dtype == torch.float64:
            copies.append(tuple(self.shape))
        return real(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", counted)
    res = LK.evaluate_gaussian_log_likelihood(r, loader=loader, log_z=20.25)
    assert copies == [(1,)]                                                     # the one sum, after the last batch
    one = LK.gaussian_log_likelihood(r, X, 20.25)
    assert res["n"] == 11 and res["log_z"] == 20.25 and res["se"] is None and res["ess"] is None
    assert res["sum_ll"] == pytest.approx(float(one.sum()), rel=1e-12) and res["mean_ll"] == pytest.approx(float(one.mean()), rel=1e-12)
    assert LK.evaluate_gaussian_log_likelihood(r, loader=loader, log_z=20.25, max_batches=2)["n"] == 8
    assert LK.evaluate_gaussian_log_likelihood(r) is None                       # no loader anywhere
    del copies[:]
    est = LK.estimate_gaussian_log_partition(r, n_chains=8, n_betas=5, seed=3)
    assert copies == [(4,)]                                                     # [log_z, log_z_base, ess, se] in one copy

    class Stack:
        pass
    m = Stack()
    m.layers, m.val_loader, m.wandb_run = [r, object()], loader, _Run()
    E.manual_seed(5)
    res = LK.evaluate_gaussian_log_likelihood(m, n_chains=8, n_betas=5, seed=3)
    assert E.get_rng().offset == 0
    assert res["log_z"] == est["log_z"] and res["se"] == est["se"] and res["ess"] == est["ess"]
    assert m.wandb_run.logged == [{"ll/mean_ll": res["mean_ll"], "ll/log_z": res["log_z"], "ll/se": res["se"], "ll/ess": res["ess"]}]


def test_an_idbn_with_gaussian_visible_is_accepted_and_a_plain_rbm_refused(double):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import RBM, GaussianRBM, iDBN
    g = np.random.Generator(np.random.PCG64(3))
    X = torch.from_numpy((0.5 + 2.0 * g.standard_normal((16, 12))).astype(F32))
    dl = DataLoader(TensorDataset(X, torch.zeros(16)), batch_size=8)
    params = {"LEARNING_RATE": 0.05, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95, "LEARNING_RATE_DYNAMIC": True,
              "CD": 1, "GAUSSIAN_VISIBLE": True}
    torch.manual_seed(0)
    net = iDBN([12, 7, 5], params, dl, dl, torch.device("cpu"))
    bottom = net.layers[0]
    assert isinstance(bottom, GaussianRBM)
    bottom.W.data = bottom.W.data.contiguous()
    bottom.init_from_data(X)
    res = LK.evaluate_gaussian_log_likelihood(net, n_chains=8, n_betas=5, seed=2)          # its val_loader, its bottom layer
    assert res["n"] == 16 and np.isfinite(res["mean_ll"])
    assert [c for c in double.calls if c[0] == "gauss_ais"] == [("gauss_ais", 8, 5, False)]
    plain = RBM(12, 7, 0.1, 0.0, 0.5).to("cpu")
    for call in (lambda: LK.estimate_gaussian_log_partition(plain, n_chains=4, n_betas=3, seed=1),
                 lambda: LK.gaussian_log_likelihood(plain, X, 0.0),
                 lambda: LK.evaluate_gaussian_log_likelihood(plain, loader=dl, log_z=0.0),
                 lambda: LK.evaluate_gaussian_log_likelihood(net.layers[1], loader=dl, log_z=0.0)):
        with pytest.raises(ValueError, match="GaussianRBM"):
            call()


def test_the_generic_functions_and_the_inherited_names_keep_refusing_a_gaussian_layer(double):
    from imdbn.models import grbm
    c = Cs.case("tiny", False)
    r = _grbm(c["W"], c["b"], c["c"], c["z"])
    v = torch.zeros(2, c["V"])
    for call in (lambda: LK.estimate_log_partition(r, n_chains=4, n_betas=3, seed=1), lambda: LK.log_likelihood(r, v, 0.0),
                 lambda: LK.evaluate_log_likelihood(r, loader=[v], log_z=0.0), lambda: r.log_partition(n_chains=4, n_betas=3),
                 lambda: r.log_likelihood(v, 0.0)):
        with pytest.raises(ValueError, match="Gaussian"):
            call()
    assert len(grbm.REFUSED) == 13 and "log_partition" in grbm.REFUSED
    assert not [c for c in double.calls if c[0] == "gauss_ais"]


# ---- 5. the draw schedule ---------------------------------------------------------------------------------------------------------------
def test_the_schedule_is_what_the_twin_draws():
    assert R.sched_gauss_ais(3, 2, 1) == [("n", 3)]
    for K in (1, 2, 6):
        s = R.sched_gauss_ais(20, 12, K)
        assert len(s) == 2 * K - 1 and s == [("n", 20)] + (K - 1) * [("u", 12), ("n", 20)]
    c = Cs.case("tiny", True)
    ps = PhiloxStream(5)
    GA.gauss_ais_logw(c["W"], c["b"], c["c"], c["z"], c["bA"], c["betas"], c["M"], ps)
    assert [(k, shape[1]) for k, shape in ps.log] == R.sched_gauss_ais(c["V"], c["H"], c["K"]) and ps.offset == 2 * c["K"] - 1


def test_every_parity_seed_is_clear_of_a_tie_and_the_restatement_draws_the_same_h():
    for c, kind in Cs.all_runs():
        a, b = Cs.twin_run(c, kind), Cs.twin_run(c, kind, dt=F32)
        assert a["margin"] >= Cs.MARGIN and Cs.same_h(a, b), (c["name"], c["bA"] is not None, kind, a["margin"])
    e = Cs.fp32_errors()
    print("fp32 restatement vs float64 twin:", e)
    assert 0 < e["logw"] < 1e-5 and 0 < e["v"] < 1e-5


# ---- 6. ABI -------------------------------------------------------------------------------------------------------------------------------
def test_export_is_declared_bound_and_present():
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    assert re.search(r"\bint\s+imdbn_rbm_gauss_ais\s*\(", src) and "#define IMDBN_ABI_VERSION 4" in src
    res, args = native.SIGNATURES["imdbn_rbm_gauss_ais"]
    assert len(args) == 13
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("native library not built")
    assert hasattr(native.lib(), "imdbn_rbm_gauss_ais")
