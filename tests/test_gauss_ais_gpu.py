"""GPU: imdbn_rbm_gauss_ais / HipEngine.gauss_ais against the float64 numpy twin (tests/gauss_ais_oracle.py) on the cases and pinned
seeds of tests/gauss_ais_cases.py, and against the enumerated partition function.

Parity.  Before a case runs on the device the CPU asserts that the twin's smallest Bernoulli margin |sigmoid(beta x) - U| is >= 1e-4
and that the float32 restatement of the twin draws the same h everywhere: a continuous state carries its rounding into the next
logits, so the margin alone would not show that fp32 arithmetic leaves the decisions alone.  The normals and uniforms come from a
replay tape (two cases also run on the device's own Philox draws).

Tolerances follow the method of tests/test_gauss_gpu.py: nobody had measured what fp32 costs here, so each tolerance is 8 x the largest
error of the float32 restatement against the float64 twin over every run below (gauss_ais_cases.fp32_errors; the restatement alone
passes with a factor 8 to spare by construction, asserted first), both relative to max(1, |twin|):
    logw   3.4e-07 -> tolerance 2.7e-06          v_K   3.05e-07 -> 2.4e-06
A flipped h would move v_K by about |W_ij| (0.03 .. 0.2 here), four orders of magnitude outside that: the v_K check also proves
that every draw of the device was the twin's."""
import ctypes as C

import numpy as np
import pytest
import torch

import anneal_oracle as A
import gauss_ais_cases as Cs
import gauss_ais_oracle as GA
from likelihood_gpu import DEV, _native, close, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PARITY = [(n, a, p) for n, a in Cs.RUNS for p in Cs.SHAPES[n][4]]
PARITY_IDS = [f"{n}-{'bA' if a else 'own_b'}-{'pitch%d' % p if p else 'natural'}" for n, a, p in PARITY]


def _tol():
    e = twin(("gauss_ais", "fp32"), Cs.fp32_errors)
    return {k: 8 * v for k, v in e.items()}


def _twin(c, kind="replay"):
    """The float64 twin of a case, after the CPU-side assertions every parity case opens with."""
    def run():
        a, b = Cs.twin_run(c, kind), Cs.twin_run(c, kind, dt=F32)
        return a, Cs.same_h(a, b)
    t, same = twin(("gauss_ais", c["name"], c["bA"] is not None, kind), run)
    print(f"{c['name']} ({kind}): twin margin {t['margin']:.3g}, the float32 restatement draws the same h: {same}")
    assert t["margin"] >= Cs.MARGIN and same
    return t


def _rng(c, kind="replay"):
    from imdbn import engine as E
    return E.ReplayRng(Cs.source("replay", c["seed"])) if kind == "replay" else E.PhiloxRng(c["philox_seed"])


def _bA(c):
    return None if c["bA"] is None else dev(c["bA"])


def _run(eng, c, r=None, pitch=None, kind="replay", M=None, rng=None):
    r = device_rbm(c, pitch) if r is None else r
    lw, v = eng.gauss_ais(r, dev(c["z"]), c["betas"], c["M"] if M is None else M, _rng(c, kind) if rng is None else rng,
                          base_vis_bias=_bA(c), return_state=True)
    torch.cuda.synchronize()
    return lw, v


def _check(c, t, lw, v, what):
    tol = _tol()
    assert lw.dtype == torch.float64 and tuple(lw.shape) == (c["M"],) and tuple(v.shape) == (c["M"], c["V"])
    sc_w, sc_v = np.maximum(1.0, np.abs(t["logw"])), np.maximum(1.0, np.abs(t["v"]))
    close(v.cpu().numpy() / sc_v, t["v"] / sc_v, tol["v"], f"{what}: v_K")
    close(lw.cpu().numpy() / sc_w, t["logw"] / sc_w, tol["logw"], f"{what}: logw")


# ---- 1. parity with the twin ------------------------------------------------------------------------------------------------------
def test_the_fp32_restatement_alone_passes_at_the_tolerances():
    e, tol = twin(("gauss_ais", "fp32"), Cs.fp32_errors), _tol()
    print("fp32 restatement vs float64 twin:", e, "-> tolerances", tol)
    assert all(0 < e[k] <= tol[k] / 8 for k in e)


@pytest.mark.parametrize("name,with_bA,pitch", PARITY, ids=PARITY_IDS)
def test_parity_with_the_twin_on_a_replay_tape(eng, name, with_bA, pitch):
    from imdbn.engine import rng as R
    c = Cs.case(name, with_bA)
    t = _twin(c)
    assert len(t["h"]) == c["K"] - 1 and len(R.sched_gauss_ais(c["V"], c["H"], c["K"])) == 2 * c["K"] - 1
    r = device_rbm(c, pitch)
    if pitch is not None:
        assert r.W.data.stride(0) == pitch
    lw, v = _run(eng, c, r=r)
    _check(c, t, lw, v, f"{name} b_A={with_bA} pitch={pitch}")


@pytest.mark.parametrize("name,with_bA", Cs.PHILOX_RUNS, ids=[f"{n}-{'bA' if a else 'own_b'}" for n, a in Cs.PHILOX_RUNS])
def test_parity_with_the_twin_on_the_device_draws(eng, name, with_bA):
    from imdbn import engine as E
    c = Cs.case(name, with_bA)
    t = _twin(c, "philox")
    rng = E.PhiloxRng(c["philox_seed"])
    lw, v = _run(eng, c, kind="philox", rng=rng)
    assert rng.offset == 2 * c["K"] - 1
    _check(c, t, lw, v, f"{name} b_A={with_bA} Philox")


# ---- 2. against the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bA", [False, True])
def test_the_device_estimate_is_within_three_standard_errors_of_the_enumerated_log_z(eng, with_bA):
    from imdbn.models import GaussianRBM
    from imdbn.utils import likelihood as LK
    c = Cs.truth(with_bA)
    exact = GA.exact_log_z(c["W"], c["b"], c["c"], c["z"])
    r = GaussianRBM(c["V"], c["H"], 0.01, 0.0, 0.5).to(DEV)
    r.W.data.copy_(dev(c["W"])); r.vis_bias.data.copy_(dev(c["b"])); r.hid_bias.data.copy_(dev(c["c"])); r.logvar.data.copy_(dev(c["z"]))
    est = r.gaussian_log_partition(n_chains=c["M"], betas=c["betas"], base_vis_bias=_bA(c), seed=c["seed"])
    print(f"b_A {with_bA}: device log Z {est['log_z']:.4f}, exact {exact:.4f}, error {(est['log_z'] - exact) / est['se']:+.2f} se; "
          f"se {est['se']:.4f}, ess {est['ess']:.1f}")
    assert 0 < est["se"] <= 0.04
    assert abs(est["log_z"] - exact) <= 3 * est["se"]
    assert est["log_z_base"] == pytest.approx(GA.log_z_base(c["V"], c["H"], c["z"]), rel=1e-6)
    # the log-density of a batch under that estimate, and the mean over a loader
    x = dev((c["b"] + np.exp(0.5 * c["z"]) * np.random.Generator(np.random.PCG64(6)).standard_normal((9, c["V"]))).astype(F32))
    ll = r.gaussian_log_likelihood(x, est["log_z"])
    assert ll.dtype == torch.float64 and torch.equal(ll, -r.free_energy(x).double() - est["log_z"])
    res = LK.evaluate_gaussian_log_likelihood(r, loader=[x[:5], x[5:]], log_z=est["log_z"])
    assert res["n"] == 9 and res["mean_ll"] == pytest.approx(float(ll.mean()), rel=1e-12)


# ---- 3. determinism, untouched parameters, padding, row-keyed draws -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "mid", "wide"])
def test_the_same_call_twice_gives_the_same_bits_and_reads_its_parameters_only(eng, name):
    c = Cs.case(name, True)
    r, z = device_rbm(c), dev(c["z"])
    before = [t.clone() for t in (r.W.data, r.vis_bias.data, r.hid_bias.data, z)]
    outs = []
    for _ in range(2):
        lw, v = eng.gauss_ais(r, z, c["betas"], c["M"], _rng(c), base_vis_bias=_bA(c), return_state=True)
        outs.append((lw, v))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(before, (r.W.data, r.vis_bias.data, r.hid_bias.data, z)))


@pytest.mark.parametrize("name,pitch", [("mid", 75), ("wide", 301), ("wide", 304)])
def test_nan_poisoned_row_padding_changes_nothing(eng, name, pitch):
    c = Cs.case(name, True)
    outs = []
    for fill in (0.0, float("nan")):
        r = device_rbm(c, pitch)
        full = torch.full((c["V"], pitch), fill, device=DEV)
        r.W.data = full[:, :c["H"]]
        r.W.data.copy_(dev(c["W"]))
        outs.append(_run(eng, c, r=r))
        if fill != 0.0:
            assert torch.isnan(full[:, c["H"]:]).all() and not torch.isnan(full[:, :c["H"]]).any()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[1][0]).all()


def test_chain_i_is_the_same_chain_for_five_and_seven_chains(eng):
    from imdbn import engine as E
    c = Cs.case("mid", True)
    r = device_rbm(c)
    five = _run(eng, c, r=r, M=5, rng=E.PhiloxRng(3))
    seven = _run(eng, c, r=r, M=7, rng=E.PhiloxRng(3))
    assert torch.equal(five[0], seven[0][:5]) and torch.equal(five[1], seven[1][:5])


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
def _raw(eng, r, c, betas=(0, 0.25, 0.5, 1), M=5, K=None, null=(), ldo=None, short=0, short_tape=0):
    """The export called directly on a sentinel-filled logw -> (EngineError message or None, logw, out_v)."""
    from imdbn.engine import native as N, rng as R
    d = eng._desc(r, False)
    K = len(betas) - 1 if K is None else K
    arr = (C.c_float * len(betas))(*[float(x) for x in betas])
    z = dev(c["z"])
    logw = torch.full((max(M, 1),), -7.25, dtype=torch.float64, device=DEV)
    out = torch.full((max(M, 1), d.V), -7.25, device=DEV)
    nr, keep = eng._rng(_rng(c), R.sched_gauss_ais(d.V, d.H, max(K, 1)), max(M, 1), torch.device(DEV))
    nr.tape_len -= short_tape
    ws, nbytes, stream = eng._ws_tail(torch.device(DEV), d.V, d.H, max(M, 1))
    P = lambda t, nm: None if nm in null else C.c_void_p(t.data_ptr())
    msg = None
    try:
        eng._call("imdbn_rbm_gauss_ais", C.byref(d), P(z, "logvar"), None if "betas" in null else arr, K, M, None,
                  None if "rng" in null else C.byref(nr), P(logw, "logw"), P(out, "out_v"), d.V if ldo is None else ldo, ws, nbytes - short, stream)
    except N.EngineError as e:
        msg = str(e)
    torch.cuda.synchronize()
    return msg, logw, out


# what -> (keywords of _raw, return code, needle of the message)
BAD = {
    "M0": (dict(M=0), -1, "M = 0"), "K0": (dict(betas=(0.0,)), -1, "K = 0"),
    "first": (dict(betas=(0.1, 0.5, 1)), -1, "betas[0] = 0.1"), "last": (dict(betas=(0, 0.5, 0.9)), -1, "betas[2] = 0.9"),
    "flat": (dict(betas=(0, 0.5, 0.5, 1)), -1, "betas[2] = 0.5"), "down": (dict(betas=(0, 0.6, 0.4, 1)), -1, "betas[2] = 0.4"),
    "null_logvar": (dict(null=("logvar",)), -1, "null logvar"), "null_betas": (dict(null=("betas",)), -1, "null betas"),
    "null_rng": (dict(null=("rng",)), -1, "null rng"), "null_logw": (dict(null=("logw",)), -1, "null logw"),
    "ldo": (dict(ldo=19), -1, "ldo 19"), "short_ws": (dict(short=1), -2, "workspace"), "groups": (dict(), -5, "1 softmax groups"),
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
    assert (logw == -7.25).all() and (out == -7.25).all()
    # the same workspace still serves a good call
    msg, logw, out = _raw(eng, device_rbm(c), c)
    assert msg is None and torch.isfinite(logw).all() and not (logw == -7.25).any() and not (out == -7.25).any()


def test_python_entry_raises_engine_error(eng):
    from imdbn import engine as E
    c = Cs.case("tiny", False)
    r, z = device_rbm(c), dev(c["z"])
    with pytest.raises(E.EngineError):
        eng.gauss_ais(r, z, [0, 0.6, 0.4, 1], 5, E.PhiloxRng(1))
    with pytest.raises(E.EngineError):
        eng.gauss_ais(r, z.double(), [0, 1], 5, E.PhiloxRng(1))
    with pytest.raises(E.EngineError):
        eng.gauss_ais(r, z, [0, 1], 5, E.PhiloxRng(1), base_vis_bias=z[:-1])
    with pytest.raises(E.EngineError):
        eng.gauss_ais(device_rbm(c, groups=[(15, 20)]), z, [0, 1], 5, E.PhiloxRng(1))
