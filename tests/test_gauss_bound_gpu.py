"""GPU: imdbn_rbm_gauss_bound_step / HipEngine.gauss_bound_step against the float64 numpy twin (tests/gauss_bound_oracle.py) on the
cases and pinned seeds of tests/gauss_bound_cases.py.

Parity.  Before a case runs on the device the CPU asserts that the twin's smallest Bernoulli margin |sigmoid(x) - U| is >= 1e-5 and
that the float32 restatement of the twin draws the same h, so every decision of the device must be the twin's: out_h is compared bit
for bit.  The uniforms come from a replay tape (one case also runs on the device's own Philox draws, held to the noisy-chain parity
rule of tests/test_gauss_gpu.py: 1e-4 relative Frobenius, atol 2e-6).

The tolerance on acc follows the method of tests/test_gauss_gpu.py and tests/test_gauss_ais_gpu.py: 8 x the largest error of the
float32 restatement against the float64 twin over every run below (gauss_bound_cases.fp32_error; the restatement alone passes with a
factor 8 to spare by construction, asserted first), relative to max(1, |twin|):
    acc   3.09e-08 -> tolerance 2.5e-07          (observed on the MI355X: at most 4.65e-08, the 70-row case in mode logq)
Composition (the bracket, a Bernoulli bound_step on the h it returned with the same acc, the top RBM's free energy): the sum of the
three parts' rules -- the tolerance above on the Gaussian bracket, (V + H) 1e-5 + 1e-9 |a| on the Bernoulli bracket and
(V + H) 2^-24 times the magnitude of the fp32 free-energy terms on the top, the rules of tests/test_dbn_bound_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import bound_oracle as B
import gauss_bound_cases as Cs
import gauss_bound_oracle as GB
from golden_utils import assert_close
from likelihood_gpu import DEV, _native, close, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)
from oracle.draws import DrawStream, PhiloxStream

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PARITY = [(n, m, p) for n, m in Cs.RUNS for p in Cs.SHAPES[n][3]]
PARITY_IDS = [f"{n}-{m}-{'pitch%d' % p if p else 'natural'}" for n, m, p in PARITY]
SENTINEL = -7.25


def _tol():
    return 8 * twin(("gauss_bound", "fp32"), Cs.fp32_error)


def _twin(c, kind="replay"):
    """The float64 twin of a case, after the CPU-side assertions every parity case opens with."""
    def run():
        a, b = Cs.twin_run(c, kind), Cs.twin_run(c, kind, dt=F32)
        return a, bool(np.array_equal(a["h"], b["h"]))
    t, same = twin(("gauss_bound", c["name"], c["mode"], kind), run)
    print(f"{c['name']} {c['mode']} ({kind}): twin margin {t['margin']:.3g}, the float32 restatement draws the same h: {same}")
    assert t["margin"] >= Cs.MARGIN and same
    return t


def _rng(c):
    from imdbn import engine as E
    return E.ReplayRng(Cs.source("replay", c["seed"]))


def _check(c, t, acc, h, what, add=0.0):
    assert acc.dtype == torch.float64 and tuple(acc.shape) == (c["M"],) and tuple(h.shape) == (c["M"], c["H"]) and h.dtype == torch.float32
    bad = np.nonzero(h.cpu().numpy() != t["h"])
    assert bad[0].size == 0, f"{what}: h differs at {list(zip(*bad))[:6]}"
    sc = np.maximum(1.0, np.abs(t["acc"]))
    close((acc.cpu().numpy() - add) / sc, t["acc"] / sc, _tol(), f"{what}: acc")


# ---- 1. parity with the twin ------------------------------------------------------------------------------------------------------
def test_the_fp32_restatement_alone_passes_at_the_tolerance():
    e = twin(("gauss_bound", "fp32"), Cs.fp32_error)
    print("fp32 restatement vs float64 twin:", e, "-> tolerance", _tol())
    assert 0 < e <= _tol() / 8


@pytest.mark.parametrize("name,mode,pitch", PARITY, ids=PARITY_IDS)
def test_parity_with_the_twin_on_a_replay_tape(eng, name, mode, pitch):
    c = Cs.case(name, mode)
    t = _twin(c)
    r = device_rbm(c, pitch)
    if pitch is not None:
        assert r.W.data.stride(0) == pitch
    acc, h = eng.gauss_bound_step(r, dev(c["z"]), dev(c["v"]), _rng(c), mode=mode)
    torch.cuda.synchronize()
    _check(c, t, acc, h, f"{name} {mode} pitch={pitch}")


def test_parity_with_the_twin_on_the_device_draws(eng):
    from imdbn import engine as E
    c = Cs.case(*Cs.PHILOX_RUN)
    t = _twin(c, "philox")
    rng = E.PhiloxRng(c["philox_seed"])
    acc, h = eng.gauss_bound_step(device_rbm(c), dev(c["z"]), dev(c["v"]), rng, mode=c["mode"])
    torch.cuda.synchronize()
    assert rng.offset == 1
    assert np.array_equal(h.cpu().numpy(), t["h"])
    err = np.abs(acc.cpu().numpy() - t["acc"]) / np.maximum(1.0, np.abs(t["acc"]))
    print(f"Philox: max |device - twin| / max(1, |twin|) {err.max():.3g}")
    assert_close(acc.cpu().numpy(), t["acc"], 1e-4, "Philox: acc", atol=2e-6)


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_h_is_the_sample_of_gauss_forward_and_draws_are_row_keyed(eng, name):
    from imdbn import engine as E
    c = Cs.case(name, "logq")
    assert Cs.twin_run(c, "philox", 3)["margin"] >= Cs.MARGIN      # the two up propagations may sum their logits in different orders
    r, z, v = device_rbm(c), dev(c["z"]), dev(c["v"])
    rng = E.PhiloxRng(3)
    a, h = eng.gauss_bound_step(r, z, v, rng, mode="logq")
    _, hs = eng.gauss_forward(r, z, v, sample=True, rng=E.PhiloxRng(3))
    assert torch.equal(h, hs) and rng.offset == 1
    a3, h3 = eng.gauss_bound_step(r, z, v[:3], E.PhiloxRng(3), mode="logq")
    assert torch.equal(a3, a[:3]) and torch.equal(h3, h[:3])


# ---- 2. composition: the bracket, a Bernoulli bracket above it, the top RBM ---------------------------------------------------------
@pytest.mark.parametrize("mode", Cs.MODES)
def test_the_bracket_composes_with_bound_step_and_the_top_free_energy(eng, mode):
    from imdbn import engine as E
    from imdbn.models import GaussianRBM
    from imdbn.utils import likelihood as LK
    c = Cs.case("ballot", mode)
    up = Cs.upper_layers()
    layers = [(c["W"], c["b"], c["c"])] + up

    def run(src):
        w, margin, mag, h1 = GB.gauss_dbn_values(c["z"], layers, c["v"], 1, mode, src, 1.25)
        g = GB.gauss_bound_step(c["W"], c["b"], c["c"], c["z"], c["v"], mode, type(src)(c["seed"]))[0]
        a2 = B.bound_step(*up[0], h1, mode, DrawStream(0))[0]                  # its magnitude only: the draw enters E, of size <= H log 2
        return w[:, 0], margin, mag[:, 0], g, a2
    for kind, src in (("replay", DrawStream), ("philox", PhiloxStream)):
        w, margin, mag, g, a2 = twin(("gauss_bound", "compose", mode, kind), lambda: run(src(c["seed"])))
        print(f"compose {mode} ({kind}): twin margin {margin:.3g}")
        assert margin >= Cs.MARGIN
        tol = _tol() * np.maximum(1.0, np.abs(g)) + (up[0][0].shape[0] + up[0][0].shape[1]) * 1e-5 + 1e-9 * np.abs(a2) + \
            (up[1][0].shape[0] + up[1][0].shape[1]) * 2.0 ** -24 * mag
        if kind == "replay":        # by hand, on one replay source
            rng = E.ReplayRng(DrawStream(c["seed"]))
            acc, h = eng.gauss_bound_step(device_rbm(c), dev(c["z"]), dev(c["v"]), rng, mode=mode)
            acc2, h2 = eng.bound_step(device_rbm(up[0]), h, rng, acc=acc, mode=mode)
            assert acc2 is acc and tuple(h2.shape) == (c["M"], 20)
            top = device_rbm(up[1])
            got = acc + (-eng.free_energy(top, h2).double() - 1.25)
        else:                       # the public function, on the device's draws
            g0 = GaussianRBM(c["V"], c["H"], 0.01, 0.0, 0.5).to(DEV)
            g0.W.data.copy_(dev(c["W"])); g0.vis_bias.data.copy_(dev(c["b"])); g0.hid_bias.data.copy_(dev(c["c"])); g0.logvar.data.copy_(dev(c["z"]))

            class Stack:
                layers = [g0, device_rbm(up[0]), device_rbm(up[1])]
            got = LK.gaussian_dbn_sample_values(Stack(), dev(c["v"]), 1.25, n_samples=1, mode=mode, seed=c["seed"])
            assert got.dtype == torch.float64 and tuple(got.shape) == (c["M"], 1) and got.is_cuda
            got = got[:, 0]
        torch.cuda.synchronize()
        close(got.cpu().numpy(), w, tol, f"compose {mode} ({kind})")


def test_a_stack_of_one_is_gaussian_log_likelihood_bit_for_bit(eng):
    from imdbn.models import GaussianRBM
    from imdbn.utils import likelihood as LK
    c = Cs.case("mid")
    r = GaussianRBM(c["V"], c["H"], 0.01, 0.0, 0.5).to(DEV)
    r.W.data.copy_(dev(c["W"])); r.vis_bias.data.copy_(dev(c["b"])); r.hid_bias.data.copy_(dev(c["c"])); r.logvar.data.copy_(dev(c["z"]))
    v = dev(c["v"])
    assert torch.equal(LK.gaussian_dbn_sample_values(r, v, 2.5)[:, 0], LK.gaussian_log_likelihood(r, v, 2.5))


# ---- 3. determinism, untouched inputs, padding, accumulation ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "mid", "wide"])
def test_the_same_call_twice_gives_the_same_bits_and_reads_its_inputs_only(eng, name):
    c = Cs.case(name, "entropy")
    r, z, v = device_rbm(c), dev(c["z"]), dev(c["v"])
    before = [t.clone() for t in (r.W.data, r.vis_bias.data, r.hid_bias.data, z, v)]
    outs = [eng.gauss_bound_step(r, z, v, _rng(c), mode="entropy") for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(before, (r.W.data, r.vis_bias.data, r.hid_bias.data, z, v)))


@pytest.mark.parametrize("name,pitch", [("mid", 75), ("wide", 301), ("wide", 304)])
def test_nan_poisoned_row_padding_changes_nothing(eng, name, pitch):
    c = Cs.case(name, "logq")
    outs = []
    for fill in (0.0, float("nan")):
        r = device_rbm(c, pitch)
        full = torch.full((c["V"], pitch), fill, device=DEV)
        r.W.data = full[:, :c["H"]]
        r.W.data.copy_(dev(c["W"]))
        outs.append(eng.gauss_bound_step(r, dev(c["z"]), dev(c["v"]), _rng(c), mode="logq"))
        torch.cuda.synchronize()
        if fill != 0.0:
            assert torch.isnan(full[:, c["H"]:]).all() and not torch.isnan(full[:, :c["H"]]).any()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[1][0]).all()


def test_the_call_adds_to_a_non_zero_acc(eng):
    c = Cs.case("rows70", "entropy")
    t = _twin(c)
    start = torch.arange(c["M"], dtype=torch.float64, device=DEV) - 3.5
    acc, h = eng.gauss_bound_step(device_rbm(c), dev(c["z"]), dev(c["v"]), _rng(c), acc=start, mode="entropy")
    torch.cuda.synchronize()
    assert acc is start
    _check(c, t, acc, h, "accumulate", add=np.arange(c["M"]) - 3.5)


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
def _raw(eng, r, c, M=5, mode=0, null=(), ldv=None, ldh=None, short=0, short_tape=0):
    """The export called directly on sentinel-filled acc / out_h -> (EngineError message or None, acc, out_h)."""
    from imdbn.engine import native as N, rng as R
    d = eng._desc(r, False)
    z, v = dev(c["z"]), dev(c["v"])
    acc = torch.full((max(M, 1),), SENTINEL, dtype=torch.float64, device=DEV)
    out = torch.full((max(M, 1), d.H), SENTINEL, device=DEV)
    nr, keep = eng._rng(_rng(c), R.sched_bound(d.H), max(M, 1), torch.device(DEV))
    nr.tape_len -= short_tape
    ws, nbytes, stream = eng._ws_tail(torch.device(DEV), d.V, d.H, max(M, 1))
    P = lambda t, nm: None if nm in null else C.c_void_p(t.data_ptr())
    msg = None
    try:
        eng._call("imdbn_rbm_gauss_bound_step", C.byref(d), P(z, "logvar"), P(v, "v"), d.V if ldv is None else ldv, M, mode,
                  None if "rng" in null else C.byref(nr), P(acc, "acc"), P(out, "out_h"), d.H if ldh is None else ldh, ws, nbytes - short, stream)
    except N.EngineError as e:
        msg = str(e)
    torch.cuda.synchronize()
    return msg, acc, out


# what -> (keywords of _raw, return code, needle of the message)
BAD = {
    "M0": (dict(M=0), -1, "M = 0"), "mode": (dict(mode=7), -1, "mode 7"),
    "null_logvar": (dict(null=("logvar",)), -1, "null logvar"), "null_v": (dict(null=("v",)), -1, "null v"),
    "null_rng": (dict(null=("rng",)), -1, "null rng"), "null_acc": (dict(null=("acc",)), -1, "null acc"),
    "null_out_h": (dict(null=("out_h",)), -1, "null out_h"), "ldv": (dict(ldv=19), -1, "ldv 19"), "ldh": (dict(ldh=11), -1, "ldh 11"),
    "short_ws": (dict(short=1), -2, "workspace"), "groups": (dict(), -5, "1 softmax groups"), "short_tape": (dict(short_tape=1), -3, "replay tape"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_invalid_arguments_launch_nothing_and_name_the_value(eng, what):
    c = Cs.case("tiny")
    kw, code, needle = BAD[what]
    r = device_rbm(c, groups=[(15, 20)] if what == "groups" else None)
    msg, acc, out = _raw(eng, r, c, **kw)
    print(what, "->", msg)
    assert msg is not None and f"rc={code})" in msg and needle in msg and "gauss_bound_step" in msg
    assert (acc == SENTINEL).all() and (out == SENTINEL).all()
    # the same workspace still serves a good call
    msg, acc, out = _raw(eng, device_rbm(c), c)
    assert msg is None and torch.isfinite(acc).all() and not (acc == SENTINEL).any() and not (out == SENTINEL).any()


def test_python_entry_raises_engine_error(eng):
    from imdbn import engine as E
    c = Cs.case("tiny")
    r, z, v = device_rbm(c), dev(c["z"]), dev(c["v"])
    with pytest.raises(E.EngineError):
        eng.gauss_bound_step(r, z, v, E.PhiloxRng(1), mode="mean")
    with pytest.raises(E.EngineError):
        eng.gauss_bound_step(r, z.double(), v, E.PhiloxRng(1))
    with pytest.raises(E.EngineError):
        eng.gauss_bound_step(r, z, v, E.PhiloxRng(1), acc=torch.zeros(c["M"], device=DEV))
    with pytest.raises(E.EngineError):
        eng.gauss_bound_step(r, z, v, E.PhiloxRng(1), acc=torch.zeros(c["M"] + 1, dtype=torch.float64, device=DEV))
    with pytest.raises(E.EngineError):
        eng.gauss_bound_step(device_rbm(c, groups=[(15, 20)]), z, v, E.PhiloxRng(1))
