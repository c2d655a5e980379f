"""GPU: softmax groups at the engine's limits -- four per layer, up to 256 columns wide -- on every down route behind which
finish_groups runs, against float64 (group_cases.py has the table, the layouts, the derivation of the bounds and of the categorical
margin).  Every case asserts through HipEngine.last_route() the route it names, "finish_groups": True included, and runs on a
NaN-filled workspace.

Probabilities: sigmoid columns within route_cases.prob_bound(T), softmax columns within group_cases.softmax_bound of the float64
reference.  Samples and categorical picks equal the reference's decisions on the same draws exactly, with no share left out (the seeds
are pinned on the CPU, test_groups_cpu.py); the draws consumed are asserted.  train_epoch: the loss as test_cd_routes_gpu.py holds it,
the parameters and momenta within update_cases.TOL of the float64 update.  The clamped update and the chain: against the oracle with
the tolerances of test_routes_gpu.py."""
import contextlib

import numpy as np
import pytest
import torch

import group_cases as GC
import parity_cases as P
import route_cases as RC
import update_cases as UC
from golden_utils import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
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
    for k, v in GC.OPTION_DEFAULTS.items():
        eng.set_option(k, v)
    eng._pf.clear()


def _rbm(c, groups=None):
    from imdbn.models import RBM
    W, hb, vb = RC.params(c["V"], c["H"])
    r = RBM(c["V"], c["H"], 0.1, 1e-4, 0.5, dynamic_lr=True, final_momentum=0.95,
            softmax_groups=[tuple(g) for g in (c["groups"] if groups is None else groups)] or None)
    return P.set_params(r, DEV, W, hb, vb)


@contextlib.contextmanager
def _routed(eng, c):
    """The case's options for the duration of the call, on a NaN-filled workspace and with no batch on record as prefetched."""
    try:
        for k, v in c["opts"].items():
            eng.set_option(k, v)
        eng._pf.clear()
        eng._workspace(torch.device(DEV), c["V"], c["H"], c["B"]).view(torch.float32).fill_(float("nan"))
        yield
    finally:
        for k in c["opts"]:
            eng.set_option(k, GC.OPTION_DEFAULTS[k])
        eng._pf.clear()


def _assert_route(eng, c):
    got = eng.last_route()
    assert {k: got[k] for k in c["route"]} == c["route"], f"{c['id']}: ran {got}"


def _rng(c):
    from imdbn import engine as E
    return E.PhiloxRng(seed=c["seed"]) if c["rng"] == "philox" else E.ReplayRng(GC.Tape(c["seed"]))


def _probs_within(c, got, ref, raw, T, what):
    ratio = GC.worst_ratio(got, ref, GC.prob_bounds(ref, raw, T, c["groups"]))
    print(f"{c['id']}: {what}: largest |d| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{c['id']}: {what} is {ratio:.2f} bounds from float64"
    for s, e in c["groups"]:
        assert np.abs(got[:, s:e].astype(F64).sum(1) - 1.0).max() <= (e - s + 4) * GC.U, f"{c['id']}: group ({s}, {e}) does not sum to one"


def _picks_equal(c, got, ref):
    for g, (s, e) in enumerate(c["groups"]):
        assert (got[:, s:e].sum(1) == 1).all() and set(np.unique(got[:, s:e])) <= {0.0, 1.0}, f"{c['id']}: group {g} is not one-hot"
        bad = np.nonzero(got[:, s:e].argmax(1) != ref[:, s:e].argmax(1))[0]
        assert bad.size == 0, f"{c['id']}: group {g} ({s}, {e}): {bad.size} categorical picks differ from the reference's, first row {bad[0]}"
    assert np.array_equal(got, ref), f"{c['id']}: {int((got != ref).sum())} visible samples differ from the reference's decisions"


@pytest.mark.parametrize("c", GC.cases("down"), ids=IDS)
def test_prop_down_matches_float64_on_its_route(c, _native):
    r, h = _rbm(c), P.T(RC.operand("real", c["B"], c["H"]), DEV)
    with _routed(_native, c):
        out = P.N(_native.prop_down(r, h, T=c["T"]))
        _assert_route(_native, c)
    ref, raw = GC.ref_down(c)
    _probs_within(c, out, ref, raw, c["T"], "p(v|h)")


@pytest.mark.parametrize("c", GC.cases("gibbs"), ids=IDS)
def test_gibbs_step_takes_the_references_decisions_on_its_route(c, _native):
    r, v = _rbm(c), P.T(RC.operand(c["operand"], c["B"], c["V"]), DEV)
    rng = _rng(c)
    with _routed(_native, c):
        v_next, v_prob, h, h_prob = (P.N(t) for t in _native.gibbs_step(r, v, c["sample_h"], c["sample_v"], rng))
        _assert_route(_native, c)
    r_next, r_prob, r_h, r_hprob, raw = GC.ref_gibbs(c)
    b = RC.prob_bound(1.0)
    assert GC.worst_ratio(h_prob, r_hprob, b) <= 1.0, f"{c['id']}: p(h|v)"
    if c["sample_h"]:
        assert np.array_equal(h, r_h), f"{c['id']}: {int((h != r_h).sum())} hidden samples differ from the reference's decisions"
    else:
        assert GC.worst_ratio(h, r_h, b) <= 1.0, f"{c['id']}: h"
    _probs_within(c, v_prob, r_prob, raw, 1.0, "p(v|h)")
    _picks_equal(c, v_next, r_next)
    if c["rng"] == "philox":
        assert rng.offset == RC.gibbs_draws(c) == (1 if c["sample_h"] else 0) + 1 + len(c["groups"])


@pytest.mark.parametrize("c", GC.cases("train"), ids=IDS)
def test_train_epoch_matches_the_float64_update(c, _native):
    from imdbn import engine as E
    ref, want = GC.ref_train(c)
    x = P.T(RC.operand(c["operand"], c["B"], c["V"]), DEV)
    rng = _rng(c)
    with _routed(_native, c), E.use_rng(rng):
        r = _rbm(c)
        loss = float(r.train_epoch(x, GC.TRAIN_EPOCH, GC.MAX_EPOCHS, CD=c["k"]))
        _assert_route(_native, c)
        torch.cuda.synchronize()
        got = {k: P.N(getattr(r, k)) for k in UC.KEYS}
    assert rng.offset == c["draws"]
    mse = ref["sqerr"] / (c["B"] * c["V"])
    print(f"{c['id']}: loss {loss:.8f} float64 {mse:.8f}")
    assert abs(loss - mse) <= 1e-5 * mse, (loss, mse)
    for k in UC.KEYS:
        assert np.isfinite(got[k]).all(), k
        assert_close(got[k], want[k], UC.TOL["rel"], f"{c['id']}: {k}", atol=UC.TOL["atol"])


@pytest.mark.parametrize("c", GC.cases("chain"), ids=IDS)
def test_clamped_update_and_chain_with_a_half_clamped_group_match_the_oracle(c, _native):
    from imdbn import engine as E
    (want, st, draws), _, _ = GC.run_oracle(c)
    vk, km, mu = GC.chain_inputs(c)
    rng = _rng(c)
    with _routed(_native, c), E.use_rng(rng):
        r = _rbm(c)
        r._mu_pull = {"mu_k": P.T(mu, DEV), "eta0": 0.15} if mu is not None else None
        if c["method"] == "train_epoch_clamped":
            got = r.train_epoch_clamped(P.T(vk, DEV), P.T(km, DEV), RC.CLAMPED_EPOCH, RC.CLAMPED_MAX_EPOCHS, **c["kw"])
        else:
            got = getattr(r, c["method"])(P.T(vk, DEV), P.T(km, DEV), **c["kw"])
        got = P.N(got)
        _assert_route(_native, c)
    assert rng.offset == draws
    if c["method"] == "train_epoch_clamped":
        print(f"{c['id']}: loss {float(got):.7f} oracle {float(want):.7f}")
        assert_close(float(got), want, 1e-4, "clamped loss")
        for k in P.KEYS:
            assert_close(P.N(getattr(r, k)), getattr(st, k), 1e-4, k, atol=2e-6)
    else:
        assert np.isfinite(got).all()
        assert_close(got, want, 1e-4, c["method"], atol=2e-6)


@pytest.mark.parametrize("c", GC.cases("sample"), ids=IDS)
def test_sample_visible_takes_the_references_decisions(c, _native):
    r = _rbm(c)
    rng = _rng(c)
    out = P.N(_native.sample_visible(r, P.T(GC.sample_input(c), DEV), rng))
    _picks_equal(c, out, GC.ref_sample(c))
    if c["rng"] == "philox":
        assert rng.offset == 1 + len(c["groups"])


def test_host_validation_of_group_counts_widths_and_overlaps(_native):
    from imdbn.engine import native
    c = dict(V=1040, H=36, B=3, groups=())
    h = P.T(RC.operand("real", 3, 36), DEV)
    with pytest.raises(native.EngineError, match=r"rc=-5\).*257 wide"):            # IMDBN_E_UNSUPPORTED, naming the width
        _native.prop_down(_rbm(c, ((100, 357),)), h)
    with pytest.raises(native.EngineError, match=r"rc=-1\).*overlapping"):         # IMDBN_E_INVALID
        _native.prop_down(_rbm(c, ((100, 140), (139, 150))), h)
    adjacent = ((100, 140), (140, 150))
    out = P.N(_native.prop_down(_rbm(c, adjacent), h))
    four = GC.groups_of("four", 1040)
    assert len(four) == GC.MAX_GROUPS
    out4 = P.N(_native.prop_down(_rbm(c, four), h))
    for got, groups in ((out, adjacent), (out4, four)):
        assert np.isfinite(got).all()
        for s, e in groups:
            assert np.abs(got[:, s:e].astype(F64).sum(1) - 1.0).max() <= (e - s + 4) * GC.U
