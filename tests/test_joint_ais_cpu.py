"""CPU-only: the numpy twin of imdbn_rbm_ais_groups against the enumerated partition function, the host logic of
estimate_joint_log_partition on a test double of the engine, the draw schedule, and the exports' declaration and binding.

Twin against enumeration: 16 Bernoulli columns + one softmax group of 4, H = 12, W ~ N(0, 1), biases ~ N(0, 0.5), K = 200 linear
temperatures, M = 64 chains, with and without a base-rate bias; |log Z_hat - exact| <= 3 se.  Errors over the Philox seeds 1..8, in se:
  no b_A:   -0.68 +0.84 -0.39 +0.82 +0.72 +0.20 +0.00 +0.10
  with b_A: -0.47 -0.08 +0.03 -0.08 +0.55 +0.02 +1.25 -0.23
(largest se 0.069; every seed passed); seed 1 is pinned (anneal_cases.TRUTH_SEED)."""
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


def _twin(c, M=None, seed=None, offset=0):
    return A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], c["M"] if M is None else M,
                      PhiloxStream(c["seed"] if seed is None else seed, offset), c["groups"])


# ---- 1. the twin against enumeration ----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bA", [False, True])
def test_twin_estimate_is_within_three_standard_errors_of_the_enumerated_log_z(with_bA):
    c = Cs.groups_truth(with_bA)
    exact = A.exact_log_z(c["W"], c["b"], c["c"], c["groups"])
    logw, v, _, _ = _twin(c)
    lme, se, ess = A.weight_stats(logw)
    log_z = A.log_z_base(c["V"], c["H"], c["bA"], c["groups"]) + lme
    print(f"b_A {with_bA}: log Z_hat {log_z:.4f}, exact {exact:.4f}, error {(log_z - exact) / se:+.2f} se, se {se:.4f}, ess {ess:.1f} of {c['M']}")
    assert v.shape == (c["M"], c["V"]) and set(np.unique(v)) <= {0.0, 1.0}
    assert (v[:, 16:20].sum(1) == 1).all()                              # one category per row
    assert 0 < se <= 0.08
    assert abs(log_z - exact) <= 3 * se


def test_exact_log_z_agrees_with_the_visible_side_enumeration():
    """2^H hidden states against every visible state (-F summed) on an RBM small enough for both: 4 Bernoulli columns, groups of 3 and 2."""
    W, b, c, _ = Cs.params(9, 5, 3, 1.0)
    groups = [(2, 5), (7, 9)]
    vs = A.visible_states(9, groups)
    assert vs.shape == (2 ** 4 * 3 * 2, 9) and (vs[:, 2:5].sum(1) == 1).all() and (vs[:, 7:9].sum(1) == 1).all()
    t = A.neg_free_energy(W, b, c, vs)
    want = t.max() + np.log(np.exp(t - t.max()).sum())
    assert abs(A.exact_log_z(W, b, c, groups) - want) <= 1e-12 * abs(want)
    assert abs(A.exact_log_z(W, b, c, []) - A.exact_log_z(W, b, c)) <= 1e-12 * abs(want)


def test_base_partition_function_is_that_of_the_base_model():
    """log Z_A by formula against the enumeration of the base-rate model itself (W = 0, hidden biases 0)."""
    _, _, _, bA = Cs.params(9, 5, 3, 1.0)
    groups = [(2, 5), (7, 9)]
    for b_A in (bA, None):
        want = A.exact_log_z(np.zeros((9, 5)), np.zeros(9) if b_A is None else b_A, np.zeros(5), groups)
        assert A.log_z_base(9, 5, b_A, groups) == pytest.approx(want, rel=1e-12)
    assert A.log_z_base(9, 5, None, groups) == pytest.approx(9 * np.log(2.0) + np.log(3.0) + np.log(2.0), rel=1e-12)


def test_one_temperature_is_plain_importance_sampling_from_the_base():
    """K = 1: the schedule is sched_sample_visible alone, and logw = -F(v_1) + F_A(v_1) up to the constants in log Z_A."""
    W, b, c, bA = Cs.params(9, 4, 5, 1.0)
    groups = [(2, 5), (7, 9)]
    ps = PhiloxStream(3)
    logw, v, _, _ = A.ais_logw(W, b, c, bA, np.array([0, 1], np.float32), 6, ps, groups)
    assert [(k, s[1]) if k == "u" else (k, None) for k, s in ps.log] == [("u", 9), ("c", None), ("c", None)]
    assert R.sched_ais_groups(9, 4, groups, 1) == R.sched_sample_visible(9, groups) == [("u", 9), ("c", 3), ("c", 2)]
    assert (v[:, 2:5].sum(1) == 1).all() and (v[:, 7:9].sum(1) == 1).all()
    x = (v @ W + c).astype(np.float64)
    want = v.astype(np.float64) @ (b.astype(np.float64) - bA) + (A.softplus(x) - np.log(2.0)).sum(1)
    assert np.allclose(logw, want, rtol=1e-12, atol=1e-12)


def test_without_groups_the_twin_is_the_binary_twin():
    c = Cs.case(Cs.GROUPS, "plain")
    logw, v, m, cm = _twin(c)
    lw0, v0, m0, cm0 = A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], c["M"], PhiloxStream(c["seed"]))
    assert np.array_equal(logw, lw0) and np.array_equal(v, v0) and m == m0 and cm == cm0 == float("inf")


@pytest.mark.parametrize("name", list(Cs.GROUPS))
def test_pinned_parity_seeds_keep_their_margins(name):
    """What the GPU tests rely on: no decision of a pinned case sits within 1e-5 of its draw."""
    c = Cs.case(Cs.GROUPS, name)
    _, v, m, cm = _twin(c)
    print(f"{name}: Bernoulli margin {m:.3g}, categorical margin {cm:.3g}")
    assert m >= Cs.MARGIN and cm >= Cs.MARGIN
    for s, e in c["groups"]:
        assert (v[:, s:e].sum(1) == 1).all()


def test_four_group_row_has_a_256_wide_group_and_keeps_the_wide_group_margin():
    c = Cs.case(Cs.GROUPS, "four256")
    assert [e - s for s, e in c["groups"]] == [5, 256, 14, 1] and c["groups"][0][0] == 0 and c["groups"][3][1] == c["V"]
    _, v, m, cm = _twin(c)
    assert m >= Cs.MARGIN and cm >= Cs.FOUR256_CAT_MARGIN >= Cs.MARGIN
    assert len({int(i) for i in v[:, 20:276].argmax(1)}) > 1          # the wide group's picks are not all one column


# ---- 2. host logic on the test double ---------------------------------------------------------------------------------
def _sched_view(sched):
    return [(k, n if k == "u" else None) for k, n in sched]


def test_schedule_is_what_the_double_consumed(double):
    for name in ("odd", "two"):
        c = Cs.case(Cs.GROUPS, name)
        rng = E.PhiloxRng(5)
        double.ais_groups(host_rbm(c), c["betas"], c["M"], rng, base_vis_bias=torch.from_numpy(c["bA"]))
        sched = R.sched_ais_groups(c["V"], c["H"], c["groups"], c["K"])
        G = len(c["groups"])
        assert double.last_log == _sched_view(sched)
        assert len(sched) == (c["K"] - 1) * (2 + G) + 1 + G == rng.offset
    assert R.sched_ais_groups(20, 12, [], 4) == R.sched_ais(20, 12, 4)


def test_estimate_matches_the_twin_and_a_seed_leaves_the_ambient_counter_alone(double):
    c = Cs.case(Cs.GROUPS, "odd")
    r = host_rbm(c)
    bA = torch.from_numpy(c["bA"])
    n_draws = len(R.sched_ais_groups(c["V"], c["H"], c["groups"], c["K"]))
    E.manual_seed(77)
    E.get_rng().advance(3)
    est = LK.estimate_joint_log_partition(r, n_chains=c["M"], betas=c["betas"], base_vis_bias=bA, seed=c["seed"])
    assert E.get_rng().offset == 3 and E.get_rng().seed == 77
    logw = _twin(c)[0]
    lme, se, ess = A.weight_stats(logw)
    lzb = A.log_z_base(c["V"], c["H"], c["bA"], c["groups"])
    assert np.array_equal(est["logw"].numpy(), logw) and est["logw"].dtype == torch.float64
    assert est["log_z_base"] == pytest.approx(lzb, rel=1e-12) and est["log_z"] == pytest.approx(lzb + lme, rel=1e-12)
    assert est["se"] == pytest.approx(se, rel=1e-9) and est["ess"] == pytest.approx(ess, rel=1e-9)
    # seed=None draws from the ambient source, from where it stands; no b_A: log 2 per Bernoulli column, log(width) per group
    est2 = LK.estimate_joint_log_partition(r, n_chains=c["M"], betas=c["betas"])
    assert E.get_rng().offset == 3 + n_draws
    c0 = dict(c, bA=None)
    assert np.array_equal(est2["logw"].numpy(), _twin(c0, seed=77, offset=3)[0])
    assert est2["log_z_base"] == pytest.approx((c["H"] + 15) * np.log(2.0) + np.log(5.0), rel=1e-12)
    # the binary functions keep refusing the same RBM
    with pytest.raises(ValueError):
        LK.estimate_log_partition(r, n_chains=4, n_betas=3, seed=1)


def test_an_rbm_without_groups_gets_the_binary_estimate(double):
    c = Cs.case(Cs.GROUPS, "plain")
    r = host_rbm(c)
    bA = torch.from_numpy(c["bA"])
    a = LK.estimate_joint_log_partition(r, n_chains=c["M"], betas=c["betas"], base_vis_bias=bA, seed=3)
    b = LK.estimate_log_partition(r, n_chains=c["M"], betas=c["betas"], base_vis_bias=bA, seed=3)
    assert torch.equal(a["logw"], b["logw"]) and a["log_z"] == pytest.approx(b["log_z"], rel=1e-12)


@pytest.mark.parametrize("with_bA", [False, True])
def test_without_groups_both_estimates_are_one_computation(double, with_bA):
    """Same weights, same statistics, same log Z_A: the dicts are equal, not merely close."""
    c = Cs.case(Cs.GROUPS, "plain")
    r = host_rbm(c)
    kw = dict(n_chains=c["M"], betas=c["betas"], base_vis_bias=torch.from_numpy(c["bA"]) if with_bA else None, seed=3)
    a, b = LK.estimate_joint_log_partition(r, **kw), LK.estimate_log_partition(r, **kw)
    assert set(a) == set(b) == {"log_z", "log_z_base", "logw", "ess", "se"}
    assert torch.equal(a["logw"], b["logw"]) and all(a[k] == b[k] for k in ("log_z", "log_z_base", "ess", "se"))


# ---- 3. ABI -----------------------------------------------------------------------------------------------------------
def test_exports_are_declared_bound_and_present():
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    assert "#define IMDBN_ABI_VERSION 4" in src
    for name, n_args in (("imdbn_rbm_ais_groups", 12), ("imdbn_rbm_label_loglik", 12)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src)
        assert len(native.SIGNATURES[name][1]) == n_args
    assert native.SIGNATURES["imdbn_rbm_ais_groups"] == native.SIGNATURES["imdbn_rbm_ais"]
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("native library not built")
    assert hasattr(native.lib(), "imdbn_rbm_ais_groups") and hasattr(native.lib(), "imdbn_rbm_label_loglik")
