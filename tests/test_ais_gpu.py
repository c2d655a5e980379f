"""GPU: imdbn_rbm_ais / HipEngine.ais against the numpy twin (tests/anneal_oracle.py) and the enumerated partition function.

Parity: every case's seed was chosen on the CPU so that the twin's smallest Bernoulli margin |p - u| is >= 1e-5 (asserted first), so
every decision of the device must be the twin's: the final states are compared exactly.  logw is held to H * 1e-5 + 1e-9 |logw|: an
error delta in a logit moves sum_k (beta_k - beta_{k-1}) sigmoid(.) delta <= delta per hidden unit over the whole ladder, and 1e-5 is
the logit agreement the parity tests of the propagations hold (test_parity_gpu.py).  Truth: the device estimate within 5 of the
TWIN's standard errors of the enumerated log Z, its own se within twice the twin's."""
import ctypes as C

import numpy as np
import pytest
import torch

import anneal_cases as Cs
import anneal_oracle as A
from likelihood_gpu import DEV, _native, base_bias, close, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)
from oracle.draws import DrawStream, PhiloxStream

pytestmark = pytest.mark.gpu
REPLAY_SEED = 11


def _twin(name):
    """(case, logw, v_K, margin, categorical margin) of a parity case under its pinned Philox seed."""
    def run():
        c = Cs.case(Cs.FORWARD, name)
        return (c,) + A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], c["M"], PhiloxStream(c["seed"]))
    return twin(("ais", name), run)


def _close(got, want, H, what):
    close(got, want, H * 1e-5 + 1e-9 * np.abs(want), what)


# ---- 1. parity with the twin ------------------------------------------------------------------------------------------
# wide: the constructor's padded pitch (float4 weight rows: k2_stream reads the hidden bit plane); wide_bA: rows 301 floats apart
# (unaligned: the fused K2 reads the bit plane)
@pytest.mark.parametrize("name,pitch", [("tiny", None), ("tiny_bA", None), ("mid", None), ("mid_bA", 75), ("wide", None), ("wide_bA", 301)])
def test_parity_with_the_twin(eng, name, pitch):
    from imdbn import engine as E
    c, logw, vK, margin, _ = _twin(name)
    print(f"{name}: twin margin {margin:.3g}")
    assert margin >= Cs.MARGIN
    r = device_rbm(c, pitch)
    rng = E.PhiloxRng(c["seed"])
    lw, v = eng.ais(r, c["betas"], c["M"], rng, base_vis_bias=base_bias(c), return_state=True)
    torch.cuda.synchronize()
    assert lw.dtype == torch.float64 and tuple(lw.shape) == (c["M"],) and tuple(v.shape) == (c["M"], c["V"])
    assert rng.offset == 2 * c["K"] - 1
    bad = np.nonzero(v.cpu().numpy() != vK)
    assert bad[0].size == 0, f"{name}: v_K differs at {list(zip(*bad))[:6]}"
    _close(lw.cpu().numpy(), logw, c["H"], name)


# ---- 2. against the truth ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bA", [False, True])
def test_estimate_against_the_enumerated_log_z(eng, with_bA):
    from imdbn.utils import likelihood as LK
    c = Cs.forward_truth(with_bA)
    exact = A.exact_log_z(c["W"], c["b"], c["c"])
    t_logw, _, _, _ = A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], c["M"], PhiloxStream(c["seed"]))
    _, t_se, _ = A.weight_stats(t_logw)
    est = LK.estimate_log_partition(device_rbm(c), n_chains=c["M"], betas=c["betas"], base_vis_bias=base_bias(c), seed=c["seed"])
    print(f"b_A {with_bA}: device log Z {est['log_z']:.4f}, exact {exact:.4f}, error {(est['log_z'] - exact) / t_se:+.2f} twin se; "
          f"se {est['se']:.4f} (twin {t_se:.4f}), ess {est['ess']:.1f}")
    assert abs(est["log_z"] - exact) <= 5 * t_se
    assert est["se"] <= 2 * t_se
    assert est["log_z_base"] == pytest.approx(A.log_z_base(c["V"], c["H"], c["bA"]), rel=1e-6)


# ---- 3. determinism and draws -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_bA", "mid", "wide"])
def test_determinism_draw_count_and_row_keyed_draws(eng, name):
    from imdbn import engine as E
    from imdbn.engine import rng as R
    c = Cs.case(Cs.FORWARD, name)
    r = device_rbm(c)
    bA = base_bias(c)
    rng = E.PhiloxRng(c["seed"])
    a = eng.ais(r, c["betas"], c["M"], rng, base_vis_bias=bA)
    b = eng.ais(r, c["betas"], c["M"], E.PhiloxRng(c["seed"]), base_vis_bias=bA)
    assert torch.equal(a, b)
    assert rng.offset == 2 * c["K"] - 1 == len(R.sched_ais(c["V"], c["H"], c["K"]))
    # the next call draws what it would after skipping the schedule
    g = np.random.Generator(np.random.PCG64(1))
    x = torch.from_numpy((g.random((6, c["V"])) > 0.5).astype(np.float32)).to(DEV)
    _, h1 = eng.prop_up(r, x, sample=True, rng=rng)
    skip = E.PhiloxRng(c["seed"])
    eng.skip_draws(skip, R.sched_ais(c["V"], c["H"], c["K"]), c["M"])
    _, h2 = eng.prop_up(r, x, sample=True, rng=skip)
    assert torch.equal(h1, h2) and rng.offset == skip.offset == 2 * c["K"]
    # the Philox key is the row: the first 5 chains of a 9-chain run are the 5-chain run
    five = eng.ais(r, c["betas"], 5, E.PhiloxRng(c["seed"]), base_vis_bias=bA)
    nine = eng.ais(r, c["betas"], 9, E.PhiloxRng(c["seed"]), base_vis_bias=bA)
    assert torch.equal(five, nine[:5])


def test_one_temperature_and_more_than_one_batch_chunk(eng):
    """K = 1 (no transition: one draw, the weight kernel's last-step form only) and M = 70 (two 64-row chunks) against the twin."""
    from imdbn import engine as E
    c = Cs.case(Cs.FORWARD, "tiny_bA")
    r = device_rbm(c)
    one = np.array([0, 1], np.float32)
    rng = E.PhiloxRng(4)
    want, _, margin, _ = A.ais_logw(c["W"], c["b"], c["c"], c["bA"], one, 70, PhiloxStream(4))
    assert margin >= Cs.MARGIN
    lw = eng.ais(r, one, 70, rng, base_vis_bias=base_bias(c))
    assert rng.offset == 1
    _close(lw.cpu().numpy(), want, c["H"], "K = 1, M = 70")
    m70, v70, margin, _ = A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], 70, PhiloxStream(c["seed"]))
    assert margin >= Cs.MARGIN
    lw, v = eng.ais(r, c["betas"], 70, E.PhiloxRng(c["seed"]), base_vis_bias=base_bias(c), return_state=True)
    assert np.array_equal(v.cpu().numpy(), v70)
    _close(lw.cpu().numpy(), m70, c["H"], "K = 6, M = 70")


# ---- 4. replay --------------------------------------------------------------------------------------------------------
def test_replay_tape_matches_the_twin_fed_the_same_tape(eng):
    from imdbn import engine as E
    c = Cs.case(Cs.FORWARD, "tiny_bA")
    want, vK, margin, _ = A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], c["M"], DrawStream(REPLAY_SEED))
    print(f"replay: twin margin {margin:.3g}")
    assert margin >= Cs.MARGIN
    lw, v = eng.ais(device_rbm(c), c["betas"], c["M"], E.ReplayRng(DrawStream(REPLAY_SEED)), base_vis_bias=base_bias(c), return_state=True)
    assert np.array_equal(v.cpu().numpy(), vK)
    _close(lw.cpu().numpy(), want, c["H"], "replay")


# ---- 5. errors --------------------------------------------------------------------------------------------------------
def _raw(eng, r, betas, M, K=None, short=0):
    """The export called directly on a sentinel-filled logw -> (EngineError message or None, logw)."""
    from imdbn.engine import native as N, rng as R
    from imdbn import engine as E
    d = eng._desc(r, False)
    K = len(betas) - 1 if K is None else K
    arr = (C.c_float * len(betas))(*[float(x) for x in betas])
    logw = torch.full((max(M, 1),), -7.25, dtype=torch.float64, device=DEV)
    nr, _ = eng._rng(E.PhiloxRng(1), R.sched_ais(d.V, d.H, max(K, 1)), max(M, 1), torch.device(DEV))
    ws, nbytes, stream = eng._ws_tail(torch.device(DEV), d.V, d.H, max(M, 1))
    msg = None
    try:
        eng._call("imdbn_rbm_ais", C.byref(d), M, K, arr, None, C.byref(nr), C.c_void_p(logw.data_ptr()), None, d.V, ws, nbytes - short, stream)
    except N.EngineError as e:
        msg = str(e)
    torch.cuda.synchronize()
    return msg, logw


@pytest.mark.parametrize("what,code", [("groups", -5), ("K0", -1), ("flat", -1), ("first", -1), ("last", -1), ("M0", -1), ("short", -2)])
def test_invalid_arguments_launch_nothing(eng, what, code):
    c = Cs.case(Cs.FORWARD, "tiny")
    r = device_rbm(c, groups=[(15, 20)] if what == "groups" else None)
    betas = {"flat": [0, 0.5, 0.5, 1], "first": [0.1, 0.5, 1], "last": [0, 0.5, 0.9], "K0": [0.0]}.get(what, [0, 0.25, 0.5, 1])
    msg, logw = _raw(eng, r, betas, 0 if what == "M0" else 5, short=1 if what == "short" else 0)
    print(what, "->", msg)
    assert msg is not None and f"rc={code})" in msg
    assert (logw == -7.25).all()
    if what in ("flat", "first", "last"):
        assert "0.5" in msg or "0.1" in msg or "0.9" in msg          # the offending value is named
    # the same workspace still serves a good call
    msg, logw = _raw(eng, device_rbm(c), [0, 0.25, 0.5, 1], 5)
    assert msg is None and torch.isfinite(logw).all() and not (logw == -7.25).any()


def test_python_entry_raises_engine_error(eng):
    from imdbn import engine as E
    c = Cs.case(Cs.FORWARD, "tiny")
    with pytest.raises(E.EngineError):
        eng.ais(device_rbm(c), [0, 0.6, 0.4, 1], 5, E.PhiloxRng(1))
    with pytest.raises(E.EngineError):
        eng.ais(device_rbm(c, groups=[(15, 20)]), [0, 1], 5, E.PhiloxRng(1))


# ---- 6. nothing else moved --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mid_bA", "wide_bA"])
def test_free_energy_and_weights_are_untouched(eng, name):
    from imdbn import engine as E
    c = Cs.case(Cs.FORWARD, name)
    r = device_rbm(c)
    g = np.random.Generator(np.random.PCG64(2))
    x = torch.from_numpy((g.random((c["M"], c["V"])) > 0.5).astype(np.float32)).to(DEV)      # M rows: the workspace of the ais call
    W0, b0, c0 = r.W.data.clone(), r.vis_bias.data.clone(), r.hid_bias.data.clone()
    F0 = eng.free_energy(r, x)
    eng.ais(r, c["betas"], c["M"], E.PhiloxRng(c["seed"]), base_vis_bias=base_bias(c))
    F1 = eng.free_energy(r, x)
    assert torch.equal(F0, F1)
    assert torch.equal(r.W.data, W0) and torch.equal(r.vis_bias.data, b0) and torch.equal(r.hid_bias.data, c0)
