"""CPU-only: the float64 reference of the exact enumeration, the fp32 restatement of kernels_exact.hpp against it on every case of
the case list, and the package functions (imdbn.utils.likelihood, the model methods) through the test double."""
import numpy as np
import pytest
import torch

import anneal_oracle as A
import exact_cases as Xc
import exact_oracle as X
import gauss_ais_oracle as GA
from bound_oracle import host_rbm
from exact_engine_double import ExactOracleEngine
from imdbn import engine as E
from imdbn.engine.native import EngineError
from imdbn.utils import likelihood as LK

F32, F64 = np.float32, np.float64


@pytest.fixture()
def double():
    eng = ExactOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)
    E.set_rng(None)


def _grbm(c):
    from imdbn.models import GaussianRBM
    r = GaussianRBM(c["V"], c["H"], 0.01, 0.0, 0.5).to("cpu")
    r.W.data = torch.from_numpy(np.array(c["W"], F32))
    r.vis_bias.data, r.hid_bias.data = torch.from_numpy(np.array(c["b"], F32)), torch.from_numpy(np.array(c["c"], F32))
    r.logvar.data = torch.from_numpy(np.array(c["z"], F32))
    return r


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in Xc.FAST if Xc.CASES[k][1] <= 16 and Xc.CASES[k][0] <= 1000])
def test_reference_equals_the_existing_oracles(name):
    c = Xc.case(name)
    got = X.reference(c["W"], c["b"], c["c"], c["side"], c["groups"], c["z"])
    want = GA.exact_log_z(c["W"], c["b"], c["c"], c["z"]) if c["z"] is not None else A.exact_log_z(c["W"], c["b"], c["c"], c["groups"])
    assert got["log_z"] == pytest.approx(want, rel=1e-12, abs=1e-10)
    assert got["log_w_max"] <= got["log_z"] and got["bits"] == c["n"]


def test_reference_agrees_from_both_sides_and_with_the_free_energy_sum():
    W, b, c, _ = Xc.params(7, 5, 11, 0.7)
    hid = X.reference(W, b, c, "hidden", marginals=True)
    vis = X.reference(W, b, c, "visible", marginals=True)
    assert hid["log_z"] == pytest.approx(vis["log_z"], rel=1e-13)
    np.testing.assert_allclose(hid["vis_mean"], vis["vis_mean"], rtol=1e-11)
    np.testing.assert_allclose(hid["hid_mean"], vis["hid_mean"], rtol=1e-11)
    nf = A.neg_free_energy(W, b, c, A.visible_states(7, ()))                 # -F(v) over every v
    assert hid["log_z"] == pytest.approx(float(nf.max() + np.log(np.exp(nf - nf.max()).sum())), rel=1e-13)
    p = np.exp(nf - hid["log_z"])
    np.testing.assert_allclose(hid["vis_mean"], p @ A.visible_states(7, ()), rtol=1e-11)
    # groups: the visible states with one-hot groups
    groups = [(2, 5)]
    g = X.reference(W, b, c, "auto", groups, marginals=True)
    st = A.visible_states(7, groups)
    nf = A.neg_free_energy(W, b, c, st)
    lz = float(nf.max() + np.log(np.exp(nf - nf.max()).sum()))
    assert g["side"] == "hidden" and g["log_z"] == pytest.approx(lz, rel=1e-13)
    np.testing.assert_allclose(g["vis_mean"], np.exp(nf - lz) @ st, rtol=1e-11)
    assert g["vis_mean"][2:5].sum() == pytest.approx(1.0, rel=1e-12)


def test_reference_gaussian_marginals_are_the_mixture_mean():
    c = Xc.case("gauss_n6_d65")
    r = X.reference(c["W"], c["b"], c["c"], "hidden", (), c["z"], marginals=True)
    assert r["log_z"] == pytest.approx(GA.exact_log_z(c["W"], c["b"], c["c"], c["z"]), rel=1e-13)
    hs = A._states(c["H"], 16)
    a = hs @ c["W"].astype(F64).T
    t = hs @ c["c"].astype(F64) + ((c["b"].astype(F64) * a + 0.5 * a * a) * np.exp(-c["z"].astype(F64))).sum(1)
    w = np.exp(t - t.max()); w /= w.sum()
    np.testing.assert_allclose(r["vis_mean"], w @ (c["b"].astype(F64) + a), rtol=1e-10)
    np.testing.assert_allclose(r["hid_mean"], w @ hs, rtol=1e-10)
    assert r["x_max"] == pytest.approx(np.abs(c["b"].astype(F64) + a).max())


# ---- 2. the kernel's arithmetic keeps an eighth of the tolerance on every case --------------------------------------------------------
@pytest.mark.parametrize("name", list(Xc.CASES))
def test_fp32_restatement_stays_inside_an_eighth_of_the_tolerance(name):
    c = Xc.case(name)
    want = X.reference(c["W"], c["b"], c["c"], c["side"], c["groups"], c["z"])["log_z"]
    got = X.restate(c["W"], c["b"], c["c"], c["side"], c["groups"], c["z"])
    print(f"{name}: n {c['n']} D {c['D']} log Z {want:.6f}, restatement off by {got - want:+.3e}, tolerance {Xc.tol_log_z(c, want):.3e}")
    assert abs(got - want) <= Xc.tol_log_z(c, want) / 8


# ---- 3. the package through the double ----------------------------------------------------------------------------------------------
def test_evaluate_log_likelihood_exact_is_mean_minus_free_energy_minus_log_z(double):
    c = Xc.case("n12_d127")
    r = host_rbm(c)
    g = np.random.Generator(np.random.PCG64(3))
    rows = torch.from_numpy((g.random((10, c["V"])) < 0.5).astype(F32))
    res = LK.evaluate_log_likelihood_exact(r, loader=[rows[:6], rows[6:]])
    lz = X.reference(c["W"], c["b"], c["c"])["log_z"]
    want = float(np.mean(A.neg_free_energy(c["W"], c["b"], c["c"], rows.numpy()) - lz))
    assert res["n"] == 10 and res["log_z"] == pytest.approx(lz, rel=1e-13) and res["se"] is None and res["ess"] is None
    assert res["mean_ll"] == pytest.approx(want, abs=1e-4)                  # the free energy is the double's fp32 one
    assert LK.evaluate_log_likelihood_exact(r) is None
    assert r.log_partition_exact()["bits"] == 12
    vm, hm = r.exact_marginals()
    assert vm.shape == (c["V"],) and hm.shape == (c["H"],) and vm.dtype == torch.float32
    cg = Xc.case("gauss_n6_d65")
    gr = _grbm(cg)
    data = torch.from_numpy((cg["b"] + g.standard_normal((5, cg["V"]))).astype(F32))
    res = LK.evaluate_gaussian_log_likelihood_exact(gr, loader=[data])
    assert res["log_z"] == pytest.approx(GA.exact_log_z(cg["W"], cg["b"], cg["c"], cg["z"]), rel=1e-12)
    assert res["mean_ll"] == pytest.approx(float((-gr.free_energy(data).double() - res["log_z"]).mean()), rel=1e-12)
    assert gr.gaussian_log_partition_exact(marginals=True)["vis_mean"].shape == (cg["V"],)


def test_ais_calibration_keeps_the_ais_fields_and_adds_the_gap(double):
    W, b, c, _ = Xc.params(20, 6, 5, 0.3)
    r = host_rbm((W, b, c))
    est = LK.estimate_log_partition(r, n_chains=16, n_betas=20, seed=4)
    cal = LK.ais_calibration(r, n_chains=16, n_betas=20, seed=4)
    assert set(cal) == set(est) | {"log_z_exact", "log_z_gap"}
    for k in ("log_z", "log_z_base", "ess", "se"):
        assert cal[k] == est[k]
    assert torch.equal(cal["logw"], est["logw"])
    assert cal["log_z_exact"] == pytest.approx(A.exact_log_z(W, b, c), rel=1e-13)
    assert cal["log_z_gap"] == cal["log_z"] - cal["log_z_exact"] and abs(cal["log_z_gap"]) < 1.0
    cg = Xc.case("gauss_n6_d65")
    gr = _grbm(cg)
    calg = LK.gaussian_ais_calibration(gr, n_chains=8, n_betas=10, seed=2)
    estg = LK.estimate_gaussian_log_partition(gr, n_chains=8, n_betas=10, seed=2)
    assert calg["log_z"] == estg["log_z"] and calg["log_z_exact"] == pytest.approx(GA.exact_log_z(cg["W"], cg["b"], cg["c"], cg["z"]), rel=1e-12)


def test_chain_marginal_gap_of_exact_samples_is_within_three_standard_errors(double):
    W, b, c, _ = Xc.params(6, 4, 21, 0.8)
    st = A.visible_states(6, ())
    nf = A.neg_free_energy(W, b, c, st)
    p = np.exp(nf - nf.max()); p /= p.sum()
    M = 4000
    rows = st[np.random.Generator(np.random.PCG64(8)).choice(len(st), M, p=p)].astype(F32)
    res = LK.chain_marginal_gap(host_rbm((W, b, c)), torch.from_numpy(rows))
    mean = p @ st
    se = np.sqrt(mean * (1 - mean) / M)
    assert float(res["max_gap"]) <= 3 * se.max() and float(res["rms_gap"]) <= float(res["max_gap"])
    assert res["max_gap"].dtype == torch.float64 and res["max_gap"].dim() == 0
    off = LK.chain_marginal_gap(host_rbm((W, b, c)), torch.zeros(8, 6))      # a cloud stuck at 0 is as far off as the marginals are large
    assert float(off["max_gap"]) == pytest.approx(mean.max(), abs=1e-6)
    with pytest.raises(ValueError, match="particles"):
        LK.chain_marginal_gap(host_rbm((W, b, c)), torch.zeros(8, 5))


def test_every_refusal_carries_its_message(double):
    c = Xc.case("gauss_n6_d65")
    gr = _grbm(c)
    plain = host_rbm(Xc.case("n6_d65"))
    for call in (lambda: LK.exact_log_partition(gr), lambda: LK.evaluate_log_likelihood_exact(gr, loader=[torch.zeros(1, c["V"])]),
                 lambda: LK.ais_calibration(gr), lambda: LK.chain_marginal_gap(gr, torch.zeros(2, c["V"])),
                 lambda: gr.log_partition_exact(), lambda: gr.exact_marginals()):
        with pytest.raises(ValueError, match="Gaussian"):
            call()
    for call in (lambda: LK.exact_gaussian_log_partition(plain), lambda: LK.gaussian_ais_calibration(plain),
                 lambda: LK.evaluate_gaussian_log_likelihood_exact(plain, loader=[torch.zeros(1, 65)])):
        with pytest.raises(ValueError, match="GaussianRBM"):
            call()
    assert not double.calls
    with pytest.raises(EngineError, match=r"n = 6 .*max_bits = 5.*max_bits=6"):
        LK.exact_log_partition(plain, max_bits=5)
    wide = host_rbm(Xc.params(12, 40, 1, 0.1)[:3], groups=[(2, 6)])
    assert LK.exact_log_partition(host_rbm(Xc.params(12, 14, 1, 0.1)[:3], groups=[(2, 6)]))["side"] == "hidden"      # auto avoids the groups
    with pytest.raises(EngineError, match="max_bits"):
        LK.exact_log_partition(wide)                                        # ... and then needs 40 bits
    with pytest.raises(EngineError, match="softmax"):
        LK.exact_log_partition(wide, side="visible")
    with pytest.raises(EngineError, match="side"):
        LK.exact_log_partition(plain, side="both")
    assert {"exact_log_partition", "exact_gaussian_log_partition", "evaluate_log_likelihood_exact", "evaluate_gaussian_log_likelihood_exact",
            "ais_calibration", "gaussian_ais_calibration", "chain_marginal_gap"} <= set(LK.__all__)
