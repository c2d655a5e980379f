"""CPU-only: the numpy twin of imdbn_rbm_ais against the enumerated partition function, the host logic of
imdbn/utils/likelihood.py on a test double of the engine, and the export's declaration and binding.

Twin against enumeration: V = 20, H = 12, W ~ N(0, 1), biases ~ N(0, 0.5), K = 200 linear temperatures, M = 64 chains, with and
without a base-rate bias; |log Z_hat - exact| <= 3 se.  Over the Philox seeds 1..8 the largest error of this setup was 2.4 se with
se <= 0.051 (both variants passed on every seed); seed 1 is pinned (anneal_cases.TRUTH_SEED): 0.08 se and -0.18 se."""
import os
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


# ---- 1. the twin against enumeration ----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bA", [False, True])
def test_twin_estimate_is_within_three_standard_errors_of_the_enumerated_log_z(with_bA):
    c = Cs.forward_truth(with_bA)
    exact = A.exact_log_z(c["W"], c["b"], c["c"])
    logw, v, _, _ = A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], c["M"], PhiloxStream(c["seed"]))
    lme, se, ess = A.weight_stats(logw)
    log_z = A.log_z_base(c["V"], c["H"], c["bA"]) + lme
    print(f"b_A {with_bA}: log Z_hat {log_z:.4f}, exact {exact:.4f}, error {(log_z - exact) / se:+.2f} se, se {se:.4f}, ess {ess:.1f} of {c['M']}")
    assert v.shape == (c["M"], c["V"]) and set(np.unique(v)) <= {0.0, 1.0}
    assert 0 < se <= 0.06
    assert abs(log_z - exact) <= 3 * se


def test_exact_log_z_agrees_with_the_visible_side_enumeration():
    """2^H hidden states against 2^V visible states (-F summed) on an RBM small enough for both."""
    W, b, c, _ = Cs.params(7, 5, 3, 1.0)
    vs = ((np.arange(1 << 7)[:, None] >> np.arange(7)[None, :]) & 1).astype(np.float64)
    t = vs @ b.astype(np.float64) + A.softplus(vs @ W.astype(np.float64) + c).sum(1)
    want = t.max() + np.log(np.exp(t - t.max()).sum())
    assert abs(A.exact_log_z(W, b, c) - want) <= 1e-12 * abs(want)


def test_one_temperature_is_plain_importance_sampling_from_the_base():
    """K = 1: no transition, one draw, logw = -F(v_1) + F_A(v_1) up to the constants in log Z_A."""
    W, b, c, bA = Cs.params(9, 4, 5, 1.0)
    ps = PhiloxStream(3)
    logw, v, _, _ = A.ais_logw(W, b, c, bA, np.array([0, 1], np.float32), 6, ps)
    assert ps.log == [("u", (6, 9))]
    x = (v @ W + c).astype(np.float64)
    want = v.astype(np.float64) @ (b.astype(np.float64) - bA) + (A.softplus(x) - np.log(2.0)).sum(1)
    assert np.allclose(logw, want, rtol=1e-12, atol=1e-12)


# ---- 2. host logic of imdbn/utils/likelihood.py on the test double ----------------------------------------------------
def test_schedule_is_what_the_double_consumed(double):
    c = Cs.case(Cs.FORWARD, "tiny_bA")
    r = host_rbm(c)
    rng = E.PhiloxRng(5)
    double.ais(r, c["betas"], c["M"], rng, base_vis_bias=torch.from_numpy(c["bA"]))
    sched = R.sched_ais(c["V"], c["H"], c["K"])
    assert double.last_log == sched and len(sched) == 2 * c["K"] - 1 and rng.offset == 2 * c["K"] - 1
    assert R.sched_ais(3, 2, 1) == [("u", 3)]


def test_estimate_matches_the_twin_and_a_seed_leaves_the_ambient_counter_alone(double):
    c = Cs.case(Cs.FORWARD, "tiny_bA")
    r = host_rbm(c)
    bA = torch.from_numpy(c["bA"])
    E.manual_seed(77)
    E.get_rng().advance(3)
    est = LK.estimate_log_partition(r, n_chains=c["M"], betas=c["betas"], base_vis_bias=bA, seed=c["seed"])
    assert E.get_rng().offset == 3 and E.get_rng().seed == 77
    logw, _, _, _ = A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], c["M"], PhiloxStream(c["seed"]))
    lme, se, ess = A.weight_stats(logw)
    assert np.array_equal(est["logw"].numpy(), logw) and est["logw"].dtype == torch.float64
    assert est["log_z_base"] == pytest.approx(A.log_z_base(c["V"], c["H"], c["bA"]), rel=1e-12)
    assert est["log_z"] == pytest.approx(A.log_z_base(c["V"], c["H"], c["bA"]) + lme, rel=1e-12)
    assert est["se"] == pytest.approx(se, rel=1e-9) and est["ess"] == pytest.approx(ess, rel=1e-9)
    # seed=None draws from the ambient source, from where it stands
    est2 = r.log_partition(n_chains=c["M"], betas=c["betas"])
    assert E.get_rng().offset == 3 + 2 * c["K"] - 1
    logw2, _, _, _ = A.ais_logw(c["W"], c["b"], c["c"], None, c["betas"], c["M"], PhiloxStream(77, 3))
    assert np.array_equal(est2["logw"].numpy(), logw2)
    assert est2["log_z_base"] == pytest.approx((c["V"] + c["H"]) * np.log(2.0), rel=1e-12)
    # n_betas: evenly spaced temperatures
    assert np.array_equal(LK.linear_betas(6).numpy(), Cs.linear(6))


def test_softmax_groups_raise_value_error(double):
    c = Cs.case(Cs.FORWARD, "tiny")
    r = host_rbm(c, groups=[(15, 20)])
    with pytest.raises(ValueError):
        LK.estimate_log_partition(r, n_chains=4, n_betas=3, seed=1)
    with pytest.raises(ValueError):
        LK.log_likelihood(r, torch.zeros(2, c["V"]), 0.0)
    with pytest.raises(ValueError):
        LK.evaluate_log_likelihood(r, loader=[torch.zeros(2, c["V"])], log_z=0.0)


def test_log_likelihood_is_minus_free_energy_minus_log_z(double):
    c = Cs.case(Cs.FORWARD, "tiny")
    r = host_rbm(c)
    g = np.random.Generator(np.random.PCG64(4))
    v = torch.from_numpy((g.random((6, c["V"])) > 0.5).astype(np.float32))
    ll = r.log_likelihood(v, 12.5)
    assert ll.dtype == torch.float64 and ll.shape == (6,)
    assert torch.equal(ll, -r.free_energy(v).double() - 12.5)
    # the probabilities of all 2^V states sum to one under the exact log Z (V = 7)
    W, b, cc, _ = Cs.params(7, 5, 3, 1.0)
    r7 = host_rbm((W, b, cc))
    vs = torch.from_numpy(((np.arange(1 << 7)[:, None] >> np.arange(7)[None, :]) & 1).astype(np.float32))
    total = float(torch.exp(LK.log_likelihood(r7, vs, A.exact_log_z(W, b, cc))).sum())
    assert total == pytest.approx(1.0, abs=1e-5)        # F in fp32


class _Run:
    def __init__(self): self.logged = []
    def log(self, d): self.logged.append(dict(d))


def test_evaluate_over_a_ragged_loader_equals_the_one_shot_mean(double):
    c = Cs.case(Cs.FORWARD, "tiny")
    r = host_rbm(c)
    g = np.random.Generator(np.random.PCG64(9))
    X = torch.from_numpy((g.random((11, c["V"])) > 0.4).astype(np.float32))
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, torch.zeros(11)), batch_size=4)      # 4 + 4 + 3 rows
    one = LK.log_likelihood(r, X, 20.25)
    res = LK.evaluate_log_likelihood(r, loader=loader, log_z=20.25)
    assert res["n"] == 11 and res["log_z"] == 20.25 and res["se"] is None and res["ess"] is None
    assert res["sum_ll"] == pytest.approx(float(one.sum()), rel=1e-12) and res["mean_ll"] == pytest.approx(float(one.mean()), rel=1e-12)
    assert LK.evaluate_log_likelihood(r, loader=loader, log_z=20.25, max_batches=2)["n"] == 8
    assert LK.evaluate_log_likelihood(r) is None                       # no loader anywhere

    # an iDBN-like model: the bottom layer, its val_loader, its wandb_run; log Z estimated under a private seed
    class Stack:
        pass
    m = Stack()
    m.layers, m.val_loader, m.wandb_run = [r, object()], loader, _Run()
    E.manual_seed(5)
    res = LK.evaluate_log_likelihood(m, n_chains=8, n_betas=5, seed=3)
    est = LK.estimate_log_partition(r, n_chains=8, n_betas=5, seed=3)
    assert E.get_rng().offset == 0
    assert res["log_z"] == est["log_z"] and res["se"] == est["se"] and res["ess"] == est["ess"]
    assert res["mean_ll"] == pytest.approx(float(LK.log_likelihood(r, X, est["log_z"]).mean()), rel=1e-12)
    assert m.wandb_run.logged == [{"ll/mean_ll": res["mean_ll"], "ll/log_z": res["log_z"], "ll/se": res["se"], "ll/ess": res["ess"]}]


def test_base_rate_bias_is_the_log_odds_of_the_smoothed_means():
    g = np.random.Generator(np.random.PCG64(2))
    X = (g.random((10, 6)) > 0.3).astype(np.float32)
    X[:, 0] = 0; X[:, 1] = 1                                          # a dead and a saturated pixel stay finite
    p = (X.astype(np.float64).mean(0) + 0.05) / 1.1
    want = np.log(p / (1 - p))
    got = LK.base_rate_bias(torch.from_numpy(X))
    assert got.dtype == torch.float32 and np.allclose(got.numpy(), want, rtol=1e-6, atol=1e-6) and np.isfinite(got.numpy()).all()
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.from_numpy(X), torch.zeros(10)), batch_size=4)
    assert np.allclose(LK.base_rate_bias(loader).numpy(), want, rtol=1e-6, atol=1e-6)


# ---- 3. ABI -----------------------------------------------------------------------------------------------------------
def test_export_is_declared_bound_and_present():
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    assert re.search(r"\bint\s+imdbn_rbm_ais\s*\(", src) and "#define IMDBN_ABI_VERSION 4" in src
    res, args = native.SIGNATURES["imdbn_rbm_ais"]
    assert len(args) == 12
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("native library not built")
    assert hasattr(native.lib(), "imdbn_rbm_ais")
