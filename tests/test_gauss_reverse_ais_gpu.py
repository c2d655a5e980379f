"""GPU: imdbn_rbm_gauss_reverse_ais / HipEngine.gauss_reverse_ais against the float64 numpy twin (tests/gauss_reverse_ais_oracle.py)
on the cases and pinned seeds of tests/gauss_reverse_ais_cases.py, and against identities that need no oracle.

Parity.  Before a case runs on the device the CPU asserts that the twin's smallest Bernoulli margin |sigmoid(beta x) - U| is >= 1e-4
and that the float32 restatement of the twin draws the same h everywhere.  Tolerances: per run, 8 x the distance of the float32
restatement to the float64 twin ON THAT RUN (gauss_reverse_ais_cases.tolerance; the factor is that of tests/test_gauss_ais_gpu.py),
both relative to max(1, |twin|) -- computed on the CPU, printed, never measured on the device.  Over the runs the restatement's
distance is 7.6e-09 .. 9.8e-07 for logw (the wide layers average their rounding over more terms) and 1.3e-07 .. 2.9e-07 for u_1.  A
flipped h would move u_1 by about |W_ij| (0.03 .. 0.2 here), four orders of magnitude outside that: the u_1 check also proves that
every draw of the device was the twin's."""
import ctypes as C

import numpy as np
import pytest
import torch

import gauss_ais_oracle as GA
import gauss_reverse_ais_cases as Cs
from likelihood_gpu import DEV, _native, close, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PARITY = [(n, a, p) for n, a in Cs.RUNS for p in Cs.SHAPES[n][4]]
PARITY_IDS = [f"{n}-{'bA' if a else 'own_b'}-{'pitch%d' % p if p else 'natural'}" for n, a, p in PARITY]


def _twin(c, kind="replay"):
    """(the float64 twin of a case, its tolerances), after the CPU-side assertions every parity case opens with."""
    def run():
        a, b = Cs.twin_run(c, kind), Cs.twin_run(c, kind, dt=F32)
        return a, Cs.same_h(a, b), {k: Cs.FACTOR * Cs.rel(b[k], a[k]) for k in ("logw", "v")}
    t, same, tol = twin(("gauss_reverse_ais", c["name"], c["bA"] is not None, kind), run)
    print(f"{c['name']} ({kind}): twin margin {t['margin']:.3g}, the float32 restatement draws the same h: {same}, tolerances {tol}")
    assert t["margin"] >= Cs.MARGIN and same and all(0 < tol[k] < 1e-4 for k in tol)
    return t, tol


def _rng(c, kind="replay"):
    from imdbn import engine as E
    return E.ReplayRng(Cs.source("replay", c["seed"])) if kind == "replay" else E.PhiloxRng(c["philox_seed"])


def _bA(c):
    return None if c["bA"] is None else dev(c["bA"])


def _run(eng, c, r=None, pitch=None, kind="replay", v=None, rng=None, z=None):
    r = device_rbm(c, pitch) if r is None else r
    lw, u1 = eng.gauss_reverse_ais(r, dev(c["z"]) if z is None else z, dev(c["v"]) if v is None else v, c["betas"],
                                   _rng(c, kind) if rng is None else rng, base_vis_bias=_bA(c), return_state=True)
    torch.cuda.synchronize()
    return lw, u1


def _check(c, t, tol, lw, u1, what):
    assert lw.dtype == torch.float64 and tuple(lw.shape) == (c["R"],) and tuple(u1.shape) == (c["R"], c["V"])
    sc_w, sc_v = np.maximum(1.0, np.abs(t["logw"])), np.maximum(1.0, np.abs(t["v"]))
    close(u1.cpu().numpy() / sc_v, t["v"] / sc_v, tol["v"], f"{what}: u_1")
    close(lw.cpu().numpy() / sc_w, t["logw"] / sc_w, tol["logw"], f"{what}: logw")


# ---- 1. parity with the twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,with_bA,pitch", PARITY, ids=PARITY_IDS)
def test_parity_with_the_twin_on_a_replay_tape(eng, name, with_bA, pitch):
    from imdbn.engine import rng as R
    c = Cs.case(name, with_bA)
    t, tol = _twin(c)
    assert len(t["h"]) == c["K"] and len(R.sched_gauss_reverse_ais(c["V"], c["H"], c["K"])) == 2 * c["K"]
    r = device_rbm(c, pitch)
    if pitch is not None:
        assert r.W.data.stride(0) == pitch
    lw, u1 = _run(eng, c, r=r)
    _check(c, t, tol, lw, u1, f"{name} b_A={with_bA} pitch={pitch}")


@pytest.mark.parametrize("name,with_bA", Cs.PHILOX_RUNS, ids=[f"{n}-{'bA' if a else 'own_b'}" for n, a in Cs.PHILOX_RUNS])
def test_parity_with_the_twin_on_the_device_draws(eng, name, with_bA):
    from imdbn import engine as E
    c = Cs.case(name, with_bA)
    t, tol = _twin(c, "philox")
    rng = E.PhiloxRng(c["philox_seed"])
    lw, u1 = _run(eng, c, kind="philox", rng=rng)
    assert rng.offset == 2 * c["K"]
    _check(c, t, tol, lw, u1, f"{name} b_A={with_bA} Philox")


# ---- 2. the exact identity: no weights, b_A = b ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_without_weights_logw_minus_log_z_a_is_the_normal_log_density(eng, name):
    """W = 0 and base_vis_bias = None: x = c exactly, the softplus sums telescope and t_v = 0, so for any v, K and draws
    logw - log Z_A = log N(v; b, e^z), here computed in float64 from the fp32 inputs."""
    from imdbn import engine as E
    c = dict(Cs.case(name, False))
    c["W"] = np.zeros_like(c["W"])
    lw, _ = _run(eng, c, kind="philox", rng=E.PhiloxRng(11))
    b, z, v = (np.asarray(c[k], F64) for k in ("b", "z", "v"))
    want = (-(v - b) ** 2 * np.exp(-z) / 2.0 - z / 2.0).sum(1) - 0.5 * c["V"] * np.log(2 * np.pi)
    got = lw.cpu().numpy() - GA.log_z_base(c["V"], c["H"], c["z"])
    print(f"{name}: max relative error {np.abs(got / want - 1).max():.3g}")
    assert np.allclose(got, want, rtol=1e-9, atol=0)


# ---- 3. same draw, same decision ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_the_first_transition_draws_the_h_of_gauss_forward_under_the_same_draw(eng, name):
    """K = 1: the one transition is at beta = 1, the logits route of gauss_forward.  With u_1 = (0 b_A + 1 m) + e^{z/2} n and
    m = b + h W^T, the call's u_1 is gauss_backward's sample from the h that gauss_forward(sample=True) draws under draw number 0,
    under draw number 1 -- to fp32 rounding; another h would move it by about |W_ij|."""
    from imdbn import engine as E
    c = Cs.case(name, True)
    r, z, v = device_rbm(c), dev(c["z"]), dev(c["v"])
    _, u1 = eng.gauss_reverse_ais(r, z, v, [0.0, 1.0], E.PhiloxRng(5), base_vis_bias=_bA(c), return_state=True)
    rng = E.PhiloxRng(5)
    _, h = eng.gauss_forward(r, z, v, sample=True, rng=rng)
    _, want = eng.gauss_backward(r, z, h, sample=True, rng=rng)
    torch.cuda.synchronize()
    assert rng.offset == 2 and 0 < float(h.mean()) < 1
    err = float((u1 - want).abs().max())
    print(f"{name}: max |u_1 - gauss_backward(gauss_forward's h)| {err:.3g}; smallest |W| step {float(r.W.data.abs().max()):.3g}")
    assert err <= 1e-5 * max(1.0, float(want.abs().max()))


# ---- 4. rows are independent, draws are keyed on the global row --------------------------------------------------------------------
def test_row_i_is_the_same_chain_whatever_r_and_whatever_the_row_offset(eng):
    from imdbn import engine as E
    c = Cs.case("mid", True)
    r, z = device_rbm(c), dev(c["z"])
    g = np.random.Generator(np.random.PCG64(12))
    v60 = dev(Cs.rows(c["W"], c["b"], c["z"], 60, g))
    full = _run(eng, c, r=r, z=z, v=v60, rng=E.PhiloxRng(3))
    five = _run(eng, c, r=r, z=z, v=v60[:5], rng=E.PhiloxRng(3))
    assert torch.equal(five[0], full[0][:5]) and torch.equal(five[1], full[1][:5])
    one = _run(eng, c, r=r, z=z, v=v60[3:4], rng=E.PhiloxRng(3, row0=3))          # row 3: not a multiple of 4
    assert torch.equal(one[0], full[0][3:4]) and torch.equal(one[1], full[1][3:4])
    again = _run(eng, c, r=r, z=z, v=v60, rng=E.PhiloxRng(3))                      # the same call, the same bits
    assert torch.equal(again[0], full[0]) and torch.equal(again[1], full[1])


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------
def _raw(eng, r, c, betas=(0, 0.25, 0.5, 1), R=5, K=None, null=(), ldv=None, ldo=None, short=0, short_tape=0):
    """The export called directly on NaN-poisoned outputs -> (EngineError message or None, logw, out_v)."""
    from imdbn.engine import native as N, rng as Rn
    d = eng._desc(r, False)
    K = len(betas) - 1 if K is None else K
    arr = (C.c_float * len(betas))(*[float(x) for x in betas])
    z, v = dev(c["z"]), dev(c["v"])
    logw = torch.full((max(R, 1),), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((max(R, 1), d.V), float("nan"), device=DEV)
    nr, keep = eng._rng(_rng(c), Rn.sched_gauss_reverse_ais(d.V, d.H, max(K, 1)), max(R, 1), torch.device(DEV))
    nr.tape_len -= short_tape
    ws, nbytes, stream = eng._ws_tail(torch.device(DEV), d.V, d.H, max(R, 1))
    P = lambda t, nm: None if nm in null else C.c_void_p(t.data_ptr())
    msg = None
    try:
        eng._call("imdbn_rbm_gauss_reverse_ais", C.byref(d), P(z, "logvar"), P(v, "v"), d.V if ldv is None else ldv, R, K,
                  None if "betas" in null else arr, None, None if "rng" in null else C.byref(nr), P(logw, "logw"), P(out, "out_v"),
                  d.V if ldo is None else ldo, ws, nbytes - short, stream)
    except N.EngineError as e:
        msg = str(e)
    torch.cuda.synchronize()
    return msg, logw, out


# what -> (keywords of _raw, return code, needle of the message)
BAD = {
    "R0": (dict(R=0), -1, "R = 0"), "K0": (dict(betas=(0.0,)), -1, "K = 0"),
    "first": (dict(betas=(0.1, 0.5, 1)), -1, "betas[0] = 0.1"), "last": (dict(betas=(0, 0.5, 0.9)), -1, "betas[2] = 0.9"),
    "flat": (dict(betas=(0, 0.5, 0.5, 1)), -1, "betas[2] = 0.5"), "down": (dict(betas=(0, 0.6, 0.4, 1)), -1, "betas[2] = 0.4"),
    "null_logvar": (dict(null=("logvar",)), -1, "null logvar"), "null_v": (dict(null=("v",)), -1, "null v"),
    "null_betas": (dict(null=("betas",)), -1, "null betas"), "null_rng": (dict(null=("rng",)), -1, "null rng"),
    "null_logw": (dict(null=("logw",)), -1, "null logw"), "ldv": (dict(ldv=19), -1, "ldv 19"), "ldo": (dict(ldo=19), -1, "ldo 19"),
    "short_ws": (dict(short=1), -2, "workspace"), "groups": (dict(), -5, "1 softmax groups"),
    "short_tape": (dict(short_tape=1), -3, "replay tape"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_invalid_arguments_launch_nothing_and_name_the_value(eng, what):
    c = Cs.case("tiny", False)
    kw, code, needle = BAD[what]
    r = device_rbm(c, groups=[(15, 20)] if what == "groups" else None)
    msg, logw, out = _raw(eng, r, c, **kw)
    print(what, "->", msg)
    assert msg is not None and f"rc={code})" in msg and needle in msg
    assert torch.isnan(logw).all() and torch.isnan(out).all()
    # the same workspace still serves a good call
    msg, logw, out = _raw(eng, device_rbm(c), c)
    assert msg is None and torch.isfinite(logw).all() and torch.isfinite(out).all()


def test_a_row_with_one_inf_is_nan_in_that_row_only(eng):
    c = Cs.case("tiny", True)
    v = dev(c["v"])
    v[2, 7] = float("inf")
    lw, _ = _run(eng, c, v=v)
    good, _ = _run(eng, c)
    assert torch.isnan(lw).tolist() == [False, False, True, False, False]
    keep = [0, 1, 3, 4]
    assert torch.equal(lw[keep], good[keep])


def test_python_entry_raises_engine_error(eng):
    from imdbn import engine as E
    c = Cs.case("tiny", False)
    r, z, v = device_rbm(c), dev(c["z"]), dev(c["v"])
    for call in (lambda: eng.gauss_reverse_ais(r, z, v, [0, 0.6, 0.4, 1], E.PhiloxRng(1)),
                 lambda: eng.gauss_reverse_ais(r, z.double(), v, [0, 1], E.PhiloxRng(1)),
                 lambda: eng.gauss_reverse_ais(r, z, v[:, :-1], [0, 1], E.PhiloxRng(1)),
                 lambda: eng.gauss_reverse_ais(r, z, v.cpu(), [0, 1], E.PhiloxRng(1)),
                 lambda: eng.gauss_reverse_ais(r, z, v, [0, 1], E.PhiloxRng(1), base_vis_bias=z[:-1]),
                 lambda: eng.gauss_reverse_ais(device_rbm(c, groups=[(15, 20)]), z, v, [0, 1], E.PhiloxRng(1))):
        with pytest.raises(E.EngineError):
            call()


# ---- 6. read-only ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pitch", [("tiny", None), ("mid", 75), ("wide", 301)])
def test_the_call_only_reads_its_parameters_logvar_and_rows(eng, name, pitch):
    c = Cs.case(name, True)
    r, z, v, bA = device_rbm(c, pitch), dev(c["z"]), dev(c["v"]), _bA(c)
    if pitch is not None:                                   # W with its row padding, poisoned: the call must neither read nor write it
        full = torch.full((c["V"], pitch), float("nan"), device=DEV)
        r.W.data = full[:, :c["H"]]
        r.W.data.copy_(dev(c["W"]))
        whole = full
    else:
        whole = r.W.data
    held = (whole, r.vis_bias.data, r.hid_bias.data, z, v, bA)
    before = [t.clone() for t in held]
    lw, u1 = eng.gauss_reverse_ais(r, z, v, c["betas"], _rng(c), base_vis_bias=bA, return_state=True)
    torch.cuda.synchronize()
    assert torch.isfinite(lw).all() and torch.isfinite(u1).all()
    for a, b in zip(before, held):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 7. the Python layer on the device -------------------------------------------------------------------------------------------------
def _grbm(c, where=DEV):
    from imdbn.models import GaussianRBM
    r = GaussianRBM(c["V"], c["H"], 0.01, 0.0, 0.5).to(where)
    for t, k in ((r.W, "W"), (r.vis_bias, "b"), (r.hid_bias, "c"), (r.logvar, "z")):
        t.data = torch.from_numpy(np.array(c[k], F32)).to(where)
    return r


def test_the_python_entry_equals_the_cpu_doubles_result_under_replay(eng):
    from gauss_reverse_engine_double import GaussReverseOracleEngine
    from imdbn import engine as E
    from imdbn.utils import likelihood as LK
    c = Cs.case("tiny", True)
    _, tol = _twin(c)
    M = 3
    kw = dict(n_chains=M, betas=c["betas"], base_vis_bias=torch.from_numpy(c["bA"]))
    E.set_engine_for_testing(GaussReverseOracleEngine())
    try:
        with E.use_rng(E.ReplayRng(Cs.source("replay", 1))):
            want = LK.gaussian_reverse_ais_log_likelihood(_grbm(c, "cpu"), torch.from_numpy(c["v"]), **kw)
    finally:
        E.set_engine_for_testing(None)
    with E.use_rng(E.ReplayRng(Cs.source("replay", 1))):
        got = _grbm(c).gaussian_log_likelihood_conservative(dev(c["v"]), **{**kw, "base_vis_bias": _bA(c)})
    torch.cuda.synchronize()
    assert got["ll"].is_cuda and got["logw"].shape == (c["R"], M) and got["ess"].shape == (c["R"],)
    for k in ("logw", "ll"):
        w = want[k].numpy()
        sc = np.maximum(1.0, np.abs(w))
        close(got[k].cpu().numpy() / sc, w / sc, tol["logw"], f"tiny: {k}")
    assert np.allclose(got["ess"].cpu().numpy(), want["ess"].numpy(), rtol=1e-4)


def test_the_sandwich_over_a_two_batch_loader_is_finite_and_its_gap_is_not_below_minus_the_slack(eng):
    from imdbn.utils import likelihood as LK
    c = Cs.truth(False)
    slack, _ = twin(("gauss_reverse_ais", "truth_slack"), lambda: Cs.truth_slack(False))
    r = _grbm(c)
    x = dev(c["x"])
    res = LK.evaluate_gaussian_log_likelihood_sandwich(r, loader=[x[:20], x[20:]], n_chains=64, betas=c["betas"],
                                                       n_chains_reverse=c["chains"], seed=1)
    print(f"sandwich: {res}; slack {slack:.4f}; exact mean log p {c['exact'].mean():.4f}")
    assert res["n"] == Cs.TRUTH["rows"] and np.isfinite([res[k] for k in res]).all()
    assert res["gap"] >= -slack
    assert res["mean_ll_reverse"] <= float(c["exact"].mean()) + slack
