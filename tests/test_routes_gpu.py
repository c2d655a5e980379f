"""GPU: single propagations, Gibbs steps, wide-layer chains and the clamped update on every kernel route of prop()
(csrc/host_prop.hpp), each case asserting through HipEngine.last_route() that it ran the route it names.

Single steps are compared with a float64 reference of the same operation (route_cases.py): probabilities within
5e-7 * max(1, 1 / T), raw logits within (2e-5 * max|ref| + 2e-6) / T, samples and categorical picks exactly equal to the reference's
decisions on the PhiloxStream draws (the seeds are pinned on the CPU with a margin of 1e-6, test_routes_cpu.py).  Chains and the
clamped update are compared with the oracle as test_philox_chains_and_clamped_match_oracle does.  Every call runs on a workspace
filled with NaN: stale padding must not matter."""
import contextlib

import numpy as np
import pytest
import torch

import parity_cases as P
import route_cases as RC
from golden_utils import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = lambda c: c["id"]      # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    eng = E.get_hip_engine()             # raises if the library is missing: no silent fallback
    cu, arch = eng.device_info()
    assert "gfx950" in arch, arch
    yield eng


def _rbm(c):
    from imdbn.models import RBM
    W, hb, vb = RC.params(c["V"], c["H"])
    r = RBM(c["V"], c["H"], 0.1, 1e-4, 0.5, dynamic_lr=True, final_momentum=0.95, softmax_groups=[tuple(g) for g in c["groups"]] or None)
    return P.set_params(r, DEV, W, hb, vb)


@contextlib.contextmanager
def _routed(eng, c):
    """The case's options for the duration of the call, on a NaN-filled workspace."""
    try:
        for k, v in c["opts"].items():
            eng.set_option(k, v)
        eng._workspace(torch.device(DEV), c["V"], c["H"], c["B"]).view(torch.float32).fill_(float("nan"))
        yield
    finally:
        for k in c["opts"]:
            eng.set_option(k, 0)


def _assert_route(eng, c):
    got = eng.last_route()
    assert {k: got[k] for k in c["route"]} == c["route"], f"{c['id']}: ran {got}"


def _within(got, ref, bound, what):
    d = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: max|d| = {d:.3e} (bound {bound:.3e})")
    assert np.isfinite(got).all() and d <= bound, f"{what}: max|d| = {d:.3e} > {bound:.3e}"


@pytest.mark.parametrize("c", RC.cases("up"), ids=IDS)
def test_up_step_matches_float64_on_its_route(c, _native):
    from imdbn import engine as E
    r, v = _rbm(c), P.T(RC.operand(c["operand"], c["B"], c["V"]), DEV)
    rng = E.PhiloxRng(seed=c["seed"])
    with _routed(_native, c):
        if c["kind"] == "forward":
            p, s = _native.forward(r, v, data_binary=True), None
        elif c["sample"]:
            p, s = _native.prop_up(r, v, T=c["T"], sample=True, rng=rng)
        else:
            p, s = _native.prop_up(r, v, T=c["T"]), None
        _assert_route(_native, c)
    ref, ref_s = RC.ref_up(c)
    _within(P.N(p), ref, RC.prob_bound(c["T"]), "p(h|v)")
    assert rng.offset == (1 if c["sample"] else 0)
    if c["sample"]:
        assert np.array_equal(P.N(s), ref_s), f"{int((P.N(s) != ref_s).sum())} hidden samples differ from the reference's decisions"


@pytest.mark.parametrize("c", RC.cases("down"), ids=IDS)
def test_down_step_matches_float64_on_its_route(c, _native):
    r, h = _rbm(c), P.T(RC.operand("real", c["B"], c["H"]), DEV)
    with _routed(_native, c):
        out = P.N(_native.prop_down(r, h, T=c["T"], logits_only=bool(c["logits_only"])))
        _assert_route(_native, c)
    ref, raw = RC.ref_down(c)
    if c["logits_only"]:      # every column, the softmax groups' included, stays a raw logit
        _within(out, ref, RC.logit_bound(raw, c["T"]), "logits")
    else:
        _within(out, ref, RC.prob_bound(c["T"]), "p(v|h)")


@pytest.mark.parametrize("c", RC.cases("gibbs"), ids=IDS)
def test_gibbs_step_matches_float64_on_its_routes(c, _native):
    from imdbn import engine as E
    r, v = _rbm(c), P.T(RC.operand(c["operand"], c["B"], c["V"]), DEV)
    rng = E.PhiloxRng(seed=c["seed"])
    with _routed(_native, c):
        v_next, v_prob, h, h_prob = (P.N(t) for t in _native.gibbs_step(r, v, c["sample_h"], c["sample_v"], rng))
        _assert_route(_native, c)
    r_next, r_prob, r_h, r_hprob = RC.ref_gibbs(c)
    b = RC.prob_bound(1.0)
    _within(h_prob, r_hprob, b, "p(h|v)")
    if c["sample_h"]:
        assert np.array_equal(h, r_h), f"{int((h != r_h).sum())} hidden samples differ from the reference's decisions"
    else:
        _within(h, r_h, b, "h")
    _within(v_prob, r_prob, b, "p(v|h)")
    if c["sample_v"]:
        for s, e in c["groups"]:
            assert np.array_equal(v_next[:, s:e].argmax(1), r_next[:, s:e].argmax(1)) and (v_next[:, s:e].sum(1) == 1).all(), "categorical picks"
        assert np.array_equal(v_next, r_next), f"{int((v_next != r_next).sum())} visible samples differ from the reference's decisions"
    else:
        _within(v_next, r_next, b, "v'")
    assert rng.offset == RC.gibbs_draws(c)


@pytest.mark.parametrize("c", RC.cases("chain"), ids=IDS)
def test_wide_chain_or_clamped_update_matches_oracle_on_its_routes(c, _native):
    from imdbn import engine as E
    (want, st, draws), _, _ = RC.run_oracle(c)
    r = _rbm(c)
    vk, km, mu = RC.chain_inputs(c)
    rng = E.PhiloxRng(seed=c["seed"])
    with _routed(_native, c), E.use_rng(rng):
        r._mu_pull = {"mu_k": P.T(mu, DEV), "eta0": 0.15} if mu is not None else None
        if c["method"] == "train_epoch_clamped":
            got = r.train_epoch_clamped(P.T(vk, DEV), P.T(km, DEV), RC.CLAMPED_EPOCH, RC.CLAMPED_MAX_EPOCHS, **c["kw"])
        else:
            got = getattr(r, c["method"])(P.T(vk, DEV), P.T(km, DEV), **c["kw"])
        got = P.N(got)
        _assert_route(_native, c)
    assert rng.offset == draws
    if c["method"] == "train_epoch_clamped":
        print(f"loss {float(got):.7f} oracle {float(want):.7f}")
        assert_close(float(got), want, 1e-4, "clamped loss")
        for k in P.KEYS:
            assert_close(P.N(getattr(r, k)), getattr(st, k), 1e-4, k, atol=2e-6)
    else:
        assert np.isfinite(got).all()
        assert_close(got, want, 1e-4, c["method"], atol=2e-6)
