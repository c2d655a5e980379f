"""GPU: the imdbn_rbm_gauss_* calls, GaussianRBM.train_epoch and iDBN(GAUSSIAN_VISIBLE) against the float64 numpy twin
(tests/gauss_oracle.py) on the cases and pinned Philox seeds of tests/gauss_cases.py.

Tolerances.  W, the biases and their momenta: the centered test's for an update, 1e-4 relative (Frobenius) with atol 2e-6, the loss
within 5e-7.  The h samples are bit-equal: the seeds keep every Bernoulli decision of the twin 1e-6 clear of a tie
(tests/test_gauss_cpu.py asserts that), and in the parity cases the normals come from a replay tape, so they are the twin's.  logvar
and logvar_m rest on r_i, an fp32 dot of H terms, and F(v) on two fp32 sums: nobody had measured those, so each tolerance is 8 x the
largest error of a float32 numpy restatement of the twin against the float64 twin over every run of gauss_cases.RUNS
(gauss_cases.fp32_errors; the restatement alone passes with a factor 8 to spare by construction, asserted below).  Measured:
    logvar   5.5e-07 -> tolerance 4.4e-06 absolute          logvar_m   5.5e-07 -> 4.4e-06 absolute
    F(v)     1.36e-05 relative to max(1, |F|) -> 1.1e-04
The means b + h W^T are fp32 dots of exact 0/1 products: 1e-5 relative to max(1, |mean|).  The two Philox-mode runs draw their normals
on the device; they use the tolerance of the noisy-chain parity tests (tests/test_parity_gpu.py) for every tensor: 1e-4 relative
Frobenius, atol 2e-6."""
import ctypes as C

import numpy as np
import pytest
import torch

import gauss_cases as Gc
import gauss_oracle as G
from golden_utils import assert_close, rel_fro
from likelihood_gpu import DEV, _native, close, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)
from oracle.draws import PhiloxStream

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIX = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")
TWIN_KEY = dict(W="W", hid_bias="c", vis_bias="b", W_m="W_m", hb_m="hb_m", vb_m="vb_m")
LR_Z = Gc.LR_Z_MULT * Gc.LR
RUN_IDS = [f"{n}-cd{k}-{'sampled' if sv else 'mean'}" for n, k, sv in Gc.RUNS]


def _tol():
    e = twin(("gauss", "fp32"), Gc.fp32_errors)
    return {k: 8 * v for k, v in e.items()}


def _twin(c, k, sv):
    return twin(("gauss", c["name"], k, sv), lambda: Gc.twin_run(c, k, sv))


def _rbm(c, pitch=None, wm_offset=0):
    """The case's RBM on the device with its momenta, weight decay and sparsity setting; `pitch`: W and W_m as views of NaN-filled
    [V, pitch] buffers; `wm_offset`: W_m starts that many floats into its buffer (4 bytes each: not 16-byte aligned)."""
    r = device_rbm(c)
    r.weight_decay, r.sparsity, r.sparsity_factor = Gc.WEIGHT_DECAY, c["sparsity"], Gc.SPARSITY_TARGET
    V, H = c["V"], c["H"]
    p = H if pitch is None else pitch
    if pitch is not None:
        r.W.data = torch.full((V, p), float("nan"), device=DEV)[:, :H]
        r.W.data.copy_(dev(c["W"]))
    elif wm_offset:
        r.W.data = dev(c["W"])
    flat = torch.full((V * p + wm_offset,), float("nan"), device=DEV)
    r.W_m = flat[wm_offset:].view(V, p)[:, :H] if (pitch is not None or wm_offset) else torch.zeros_like(r.W.data)
    r.W_m.copy_(dev(c["W_m"]))
    r.hb_m, r.vb_m = dev(c["hb_m"]), dev(c["vb_m"])
    return r


def _t(r, k):
    x = getattr(r, k)
    return x.data if k in SIX[:3] else x


def _replay(seed):
    from imdbn import engine as E
    return E.ReplayRng(PhiloxStream(seed))


def _step(eng, c, k, sv, r=None, data=None, rng=None, lr_z=LR_Z, **kw):
    """One gauss_cd_step of the case on the device: (rbm, logvar, logvar_m, loss)."""
    r = _rbm(c) if r is None else r
    z, zm = dev(c["z"]), dev(c["z_m"])
    loss = eng.gauss_cd_step(r, z, zm, dev(c["data"]) if data is None else data, Gc.LR, Gc.MOM, k, _replay(c["seed"]) if rng is None else rng,
                             lr_z, sample_v=sv, **kw)
    torch.cuda.synchronize()
    return r, z, zm, loss


def _check(t, got, what, philox=False):
    r, z, zm, loss = got
    tol, st = _tol(), t["st"]
    have = {k: _t(r, k).cpu().numpy() for k in SIX}
    print(f"{what}: rel-Frobenius vs twin:", ", ".join(f"{k} {rel_fro(have[k], getattr(st, TWIN_KEY[k])):.2e}" for k in SIX),
          f"; |loss - twin| {abs(float(loss) - float(t['loss'])):.3g}")
    if philox:
        assert_close(z.cpu().numpy(), st.z, 1e-4, f"{what}: logvar", atol=2e-6)
        assert_close(zm.cpu().numpy(), st.z_m, 1e-4, f"{what}: logvar_m", atol=2e-6)
    else:
        close(z.cpu().numpy(), st.z, tol["z"], f"{what}: logvar")
        close(zm.cpu().numpy(), st.z_m, tol["z_m"], f"{what}: logvar_m")
    for k in SIX:
        assert_close(have[k], getattr(st, TWIN_KEY[k]), 1e-4, f"{what}: {k}", atol=2e-6)
    assert abs(float(loss) - float(t["loss"])) < (5e-6 if philox else 5e-7)


# ---- 1. against the twin ------------------------------------------------------------------------------------------------------
def test_the_fp32_restatement_alone_passes_at_the_tolerances():
    e, tol = twin(("gauss", "fp32"), Gc.fp32_errors), _tol()
    print("fp32 restatement vs float64 twin:", e, "-> tolerances", tol)
    assert all(0 < e[k] <= tol[k] / 8 for k in e)


@pytest.mark.parametrize("name,k,sv", Gc.RUNS, ids=RUN_IDS)
def test_gauss_cd_step_matches_the_twin(eng, name, k, sv):
    from imdbn.engine import rng as R
    c = Gc.case(name)
    t = _twin(c, k, sv)
    assert len(R.sched_gauss_cd(c["V"], c["H"], k, sv)) == k * (1 + sv) == t["offset"]      # the wrapper checks draws_used against it
    _check(t, _step(eng, c, k, sv), f"{name} CD-{k} sample_v={sv}")


@pytest.mark.parametrize("name,k,sv", [("rows67", 1, True), ("odd", 2, False)], ids=["rows67-sampled", "odd-cd2-mean"])
def test_philox_mode_matches_the_twin_on_device_normals(eng, name, k, sv):
    from imdbn import engine as E
    c = Gc.case(name)
    rng = E.PhiloxRng(c["seed"])
    got = _step(eng, c, k, sv, rng=rng)
    assert rng.offset == k * (1 + sv)
    _check(_twin(c, k, sv), got, f"{name} CD-{k} Philox", philox=True)


@pytest.mark.parametrize("name", Gc.CASES)
def test_propagations_samples_and_free_energy_match_the_twin(eng, name):
    from imdbn import engine as E
    c = Gc.case(name)
    t = _twin(c, c["cd_ks"][-1], True)
    st = Gc.state(c)
    r, z, x = _rbm(c), dev(c["z"]), dev(c["data"])
    p, h = eng.gauss_forward(r, z, x, sample=True, rng=_replay(c["seed"]))
    close(p.cpu().numpy(), G.prop_up(st, c["data"]), 2e-6, f"{name}: p(h | v)")
    flips = int((h.cpu().numpy() != t["rec"]["h"][0]).sum())
    print(f"{name}: h elements off the twin {flips}")
    assert flips == 0
    # the chain of the CD pass, step by step: means, then every further h sample, all on the twin's draws
    src = PhiloxStream(c["seed"])
    src.uniform(h.shape)
    for it, (hs, m) in enumerate(zip(t["rec"]["h"], t["rec"]["m"])):
        mean, v = eng.gauss_backward(r, z, dev(hs.astype(F32)), sample=True, rng=E.ReplayRng(src))
        close(mean.cpu().numpy() / np.maximum(1, np.abs(m)), m / np.maximum(1, np.abs(m)), 1e-5, f"{name}: mean of step {it}")
        if it + 1 < len(t["rec"]["h"]):
            _, h2 = eng.gauss_forward(r, z, v, sample=True, rng=E.ReplayRng(src))
            assert int((h2.cpu().numpy() != t["rec"]["h"][it + 1]).sum()) == 0
    F = eng.gauss_free_energy(r, z, x).cpu().numpy()
    close(F / np.maximum(1, np.abs(t["F"])), t["F"] / np.maximum(1, np.abs(t["F"])), _tol()["F"], f"{name}: F(v)")
    p2 = eng.gauss_forward(r, z, x, T=2.0)
    close(p2.cpu().numpy(), G.prop_up(st, c["data"], 2.0), 2e-6, f"{name}: p(h | v) at T = 2")
    m0 = dev(t["rec"]["m"][0].astype(F32))
    v = eng.gauss_sample_visible(r, z, m0, _replay(7))
    want = G.sample_visible(Gc.state(c, F32), m0.cpu().numpy(), PhiloxStream(7))
    assert_close(v.cpu().numpy(), want, 1e-6, f"{name}: sample_visible", atol=1e-6)


# ---- 2. determinism, identity with the Bernoulli engine's logits ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "rows67", "wide"])
def test_the_same_call_twice_gives_the_same_bits(eng, name):
    c = Gc.case(name)
    outs = []
    for _ in range(2):
        r, z, zm, loss = _step(eng, c, c["cd_ks"][-1], True)
        outs.append([z, zm, loss] + [_t(r, q) for q in SIX])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("name", Gc.CASES)
def test_the_mean_is_prop_down_logits_bit_for_bit(eng, name):
    c = Gc.case(name)
    r, z = _rbm(c), dev(c["z"])
    g = np.random.Generator(np.random.PCG64(5))
    for h in (dev((g.random((c["B"], c["H"])) < 0.5).astype(F32)), dev(g.random((c["B"], c["H"])).astype(F32))):
        assert torch.equal(eng.gauss_backward(r, z, h), eng.prop_down(r, h, logits_only=True))


def test_lr_z_zero_touches_neither_logvar_nor_its_momentum_and_takes_a_null_momentum(eng):
    c = Gc.case("odd")
    r, z, zm, loss = _step(eng, c, 1, True, lr_z=0.0)
    assert torch.equal(z, dev(c["z"])) and torch.equal(zm, dev(c["z_m"]))
    t = twin(("gauss", "odd", "fixed"), lambda: Gc.twin_run(c, 1, True, lr_z=0.0))
    _check(t, (r, z, zm, loss), "odd, fixed variances")
    r2 = _rbm(c)
    args, keep = _args(eng, r2, c, lr_z=0.0, null=("logvar_m",))
    assert _raw(eng, args) is None
    assert all(torch.equal(_t(r, q), _t(r2, q)) for q in SIX)


def test_the_clamps_hold(eng):
    c = Gc.case("odd")
    r, z, zm, loss = _step(eng, c, 1, True, lr_z=5.0, z_lo=-0.25, z_hi=0.5)
    st = Gc.state(c)
    G.cd_step(st, c["data"], 1, PhiloxStream(c["seed"]), Gc.LR, Gc.MOM, 5.0, z_lo=-0.25, z_hi=0.5)
    assert float(z.min()) >= -0.25 and float(z.max()) <= 0.5 and bool((z == -0.25).any()) and bool((z == 0.5).any())
    close(z.cpu().numpy(), st.z, 8 * 5.0 / LR_Z * _tol()["z"], "clamped logvar")     # the same fp32 error of gz, times this lr_z


# ---- 3. layout ------------------------------------------------------------------------------------------------------------------------
def test_the_float4_and_the_scalar_kernels_agree(eng):
    """rows67 (H = 200): once with 16-byte aligned buffers (gauss_apply<true>), once with W_m one float off alignment, which sends
    the statistics pass and gauss_apply down their scalar forms."""
    c = Gc.case("rows67")
    a = _step(eng, c, 1, True)
    r = _rbm(c, wm_offset=1)
    assert r.W_m.data_ptr() % 16 == 4 and r.W.data.data_ptr() % 16 == 0
    b = _step(eng, c, 1, True, r=r)
    _check(_twin(c, 1, True), b, "rows67, scalar kernels")
    for q in SIX:
        assert_close(_t(b[0], q).cpu().numpy(), _t(a[0], q).cpu().numpy(), 1e-4, f"scalar vs float4: {q}", atol=2e-6)
    close(b[1].cpu().numpy(), a[1].cpu().numpy(), _tol()["z"], "scalar vs float4: logvar")


@pytest.mark.parametrize("name,pitch", [("odd", 41), ("rows67", 208), ("wide", 104)])
def test_strided_data_and_nan_poisoned_row_padding(eng, name, pitch):
    c = Gc.case(name)
    k = c["cd_ks"][-1]
    ref = _step(eng, c, k, True)
    big = torch.full((c["B"] + 2, c["V"] + 7), float("nan"), device=DEV)
    big[:c["B"], :c["V"]] = dev(c["data"])
    d = big[:c["B"], :c["V"]]
    r = _rbm(c, pitch)
    assert r.W.data.stride(0) == pitch == r.W_m.stride(0) and not d.is_contiguous()
    got = _step(eng, c, k, True, r=r, data=d)
    assert r.W.data.stride(0) == pitch == r.W_m.stride(0)
    _check(_twin(c, k, True), got, f"{name} strided")
    for q in SIX:
        assert torch.equal(_t(got[0], q), _t(ref[0], q)), q
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
    for q in ("W", "W_m"):
        full = torch.as_strided(_t(r, q), (c["V"], pitch), (pitch, 1))
        assert torch.isnan(full[:, c["H"]:]).all() and not torch.isnan(full[:, :c["H"]]).any(), q


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
def _raw(eng, args, name="imdbn_rbm_gauss_cd_step"):
    from imdbn.engine import native as Nt
    try:
        eng._call(name, *args)
    except Nt.EngineError as e:
        torch.cuda.synchronize()
        return str(e)
    torch.cuda.synchronize()
    return None


def _args(eng, r, c, z=None, zm=None, loss=None, scratch=None, need_m=True, B=None, ldd=None, cd_k=1, lr_z=LR_Z, z_lo=float("-inf"),
          z_hi=float("inf"), sample_v=1, groups=0, null=(), **fields):
    from imdbn.engine import native as Nt
    from imdbn.engine import rng as R
    d = eng._desc(r, True)
    if not need_m or groups:
        d = Nt.RbmDesc.from_buffer_copy(d)
        if not need_m:
            d.hb_m = None
        if groups:
            d.n_groups, d.group_start[0], d.group_end[0] = 1, 0, 4
    o = eng._opts(r, Gc.LR, Gc.MOM, cd_k)
    for k, v in fields.items():
        setattr(o, k, v)
    data = dev(c["data"])
    B = data.size(0) if B is None else B
    z, zm = dev(c["z"]) if z is None else z, dev(c["z_m"]) if zm is None else zm
    scratch = torch.empty(int(eng._lib.imdbn_gauss_scratch_floats(d.V, d.H, max(B, 1))), device=DEV) if scratch is None else scratch
    rn, keep = eng._rng(_replay(c["seed"]), R.sched_gauss_cd(d.V, d.H, max(cd_k, 1), bool(sample_v)), max(B, 1), torch.device(DEV))
    P = lambda t, nm: None if (nm in null or t is None) else C.c_void_p(t.data_ptr())
    return (C.byref(d), P(z, "logvar"), P(zm, "logvar_m"), P(data, "data"), data.stride(0) if ldd is None else ldd, B,
            None if "opts" in null else C.byref(o), lr_z, z_lo, z_hi, sample_v, None if "rng" in null else C.byref(rn), P(loss, "loss"),
            P(scratch, "scratch"), *eng._ws_tail(torch.device(DEV), d.V, d.H, max(B, 1))), (d, o, rn, keep, data, z, zm, scratch)


# what -> (keywords of _args, return code, needle of the message)
BAD = {
    "momentum": (dict(need_m=False), -1, "null momentum buffer"), "groups": (dict(groups=1), -5, "1 softmax groups"),
    "null_logvar": (dict(null=("logvar",)), -1, "null logvar"), "null_logvar_m": (dict(null=("logvar_m",)), -1, "null logvar_m"),
    "null_data": (dict(null=("data",)), -1, "null data"), "null_opts": (dict(null=("opts",)), -1, "null opts"),
    "null_scratch": (dict(null=("scratch",)), -1, "null scratch"), "null_rng": (dict(null=("rng",)), -1, "null rng"),
    "ldd": (dict(ldd=36), -1, "ldd 36"), "B0": (dict(B=0), -1, "B = 0"), "cd_k0": (dict(cd_k=0), -1, "cd_k = 0"),
    "lr_z_nan": (dict(lr_z=float("nan")), -1, "lr_z = nan"), "empty_clamp": (dict(z_lo=1.0, z_hi=0.5), -1, "clamp [1, 0.5]"),
    "clamp_nan": (dict(z_lo=float("nan")), -1, "clamp [nan"), "sample_v2": (dict(sample_v=2), -1, "sample_v = 2"),
    "data_slot": (dict(data_slot=1), -1, "data_slot 1"), "next_slot": (dict(next_slot=2), -1, "next_slot 2"),
    "fwd_out": (dict(fwd_out=64), -1, "fwd_out 0x40"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_invalid_arguments_touch_nothing_and_a_good_call_follows(eng, what):
    c = Gc.case("odd")
    kw, rc, needle = BAD[what]
    r = _rbm(c)
    before = {k: _t(r, k).clone() for k in SIX}
    S = lambda *shape: torch.full(shape, -7.25, device=DEV)
    z, zm, loss = S(c["V"]), S(c["V"]), S(1)
    scratch = S(int(eng._lib.imdbn_gauss_scratch_floats(c["V"], c["H"], c["B"])))
    args, keep = _args(eng, r, c, z, zm, loss, scratch, **kw)
    msg = _raw(eng, args)
    print(what, "->", msg)
    assert msg is not None and f"rc={rc})" in msg and needle in msg
    assert (z == -7.25).all() and (zm == -7.25).all() and (loss == -7.25).all() and (scratch == -7.25).all()
    assert all(torch.equal(_t(r, k), before[k]) for k in SIX)
    # a good call follows on the same workspace and scratch
    z, zm = dev(c["z"]), dev(c["z_m"])
    args, keep = _args(eng, r, c, z, zm, loss, scratch)
    assert _raw(eng, args) is None
    _check(_twin(c, 1, True), (r, z, zm, loss), f"after {what}")


def test_a_replay_tape_that_is_too_short_is_an_rng_error_and_touches_nothing(eng):
    c = Gc.case("odd")
    r = _rbm(c)
    before = {k: _t(r, k).clone() for k in SIX}
    args, keep = _args(eng, r, c)
    rn = keep[2]
    rn.tape_len -= 1
    msg = _raw(eng, args)
    print(msg)
    assert msg is not None and "replay tape" in msg and "rc=-3)" in msg
    assert torch.equal(keep[5], dev(c["z"])) and all(torch.equal(_t(r, k), before[k]) for k in SIX)


def test_the_propagation_entries_name_their_bad_argument(eng):
    c = Gc.case("odd")
    r, z, x = _rbm(c), dev(c["z"]), dev(c["data"])
    d = eng._desc(r, False)
    out = torch.full((c["B"], c["H"]), -7.25, device=DEV)
    tail = eng._ws_tail(torch.device(DEV), d.V, d.H, c["B"])
    P = lambda t: C.c_void_p(t.data_ptr())
    msg = _raw(eng, (C.byref(d), None, P(x), x.stride(0), c["B"], 1.0, None, P(out), d.H, None, 0, *tail), "imdbn_rbm_gauss_prop_up")
    assert msg is not None and "null logvar" in msg and "rc=-1)" in msg
    msg = _raw(eng, (C.byref(d), P(z), P(x), 36, c["B"], 1.0, None, P(out), d.H, None, 0, *tail), "imdbn_rbm_gauss_prop_up")
    assert msg is not None and "ldv 36" in msg
    msg = _raw(eng, (C.byref(d), P(z), P(out), d.H, c["B"], None, P(x), 36, None, 0, *tail), "imdbn_rbm_gauss_prop_down")
    assert msg is not None and "ldo 36" in msg
    msg = _raw(eng, (C.byref(d), P(z), P(x), x.stride(0), 0, P(out), *tail), "imdbn_rbm_gauss_free_energy")
    assert msg is not None and "B = 0" in msg
    assert (out == -7.25).all()
    from imdbn import engine as E
    with pytest.raises(E.EngineError):
        eng.gauss_forward(r, z.double(), x)
    with pytest.raises(E.EngineError):
        eng.gauss_cd_step(r, z, dev(c["z_m"])[:-1], x, Gc.LR, Gc.MOM, 1, _replay(1), LR_Z)


# ---- 5. the model classes on the device against the double -------------------------------------------------------------------------
def _cpu_copy(r):
    """A CPU GaussianRBM / RBM with the parameters, momenta and settings of `r` as they stand (through its pickle state)."""
    import pickle
    q = pickle.loads(pickle.dumps(r)).to("cpu")
    q.W_m, q.hb_m, q.vb_m = r.W_m.cpu().contiguous(), r.hb_m.cpu().clone(), r.vb_m.cpu().clone()
    if hasattr(r, "logvar"):
        q.logvar_m = r._zm().cpu().clone()
    return q


def _same_model(a, b, what):
    tol = _tol()
    for k in SIX:
        assert_close(_t(a, k).cpu().numpy(), _t(b, k).cpu().numpy(), 1e-4, f"{what}: {k}", atol=2e-6)
    if hasattr(a, "logvar"):
        close(a.logvar.data.cpu().numpy(), b.logvar.data.numpy(), 2 * tol["z"], f"{what}: logvar")      # fp32 against fp32: both sides' error
        close(a.logvar_m.cpu().numpy(), b.logvar_m.numpy(), 2 * tol["z_m"], f"{what}: logvar_m")


def test_gaussian_rbm_train_epoch_on_the_device_equals_the_double(eng):
    from gauss_engine_double import GaussOracleEngine
    from imdbn import engine as E
    from imdbn.models import GaussianRBM
    c = Gc.case("rows67")
    r = GaussianRBM(c["V"], c["H"], Gc.LR, Gc.WEIGHT_DECAY, Gc.MOM, dynamic_lr=True, lr_sigma_mult=Gc.LR_Z_MULT).to(DEV)
    r.W.data.copy_(dev(c["W"])); r.vis_bias.data.copy_(dev(c["b"])); r.hid_bias.data.copy_(dev(c["c"])); r.logvar.data.copy_(dev(c["z"]))
    q = _cpu_copy(r)
    x = dev(c["data"])
    E.manual_seed(c["seed"])
    try:
        loss = r.train_epoch(x, 3, 10)
        torch.cuda.synchronize()
        used = E.get_rng().offset
        E.set_engine_for_testing(GaussOracleEngine())
        E.manual_seed(c["seed"])
        want = q.train_epoch(x.cpu(), 3, 10)
        assert used == E.get_rng().offset == 2
    finally:
        E.set_engine_for_testing(None)
        E.set_rng(None)
    assert abs(float(loss) - float(want)) < 5e-6
    _same_model(r, q, "GaussianRBM.train_epoch")


def test_a_two_layer_idbn_epoch_on_the_device_equals_the_double(eng):
    from torch.utils.data import DataLoader, TensorDataset
    from gauss_engine_double import GaussOracleEngine
    from imdbn import engine as E
    from imdbn.models import GaussianRBM, iDBN
    g = np.random.Generator(np.random.PCG64(3))
    X = torch.from_numpy((0.5 + 2.0 * g.standard_normal((16, 12))).astype(F32))
    dl = DataLoader(TensorDataset(X, torch.zeros(16)), batch_size=8)
    params = {"LEARNING_RATE": 0.05, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95, "LEARNING_RATE_DYNAMIC": True,
              "CD": 1, "GAUSSIAN_VISIBLE": True}
    torch.manual_seed(0)
    net = iDBN([12, 7, 5], params, dl, dl, torch.device(DEV))
    assert isinstance(net.layers[0], GaussianRBM) and net.layers[0].W.is_cuda
    net.layers[0].init_from_data(X)
    twins = [_cpu_copy(r) for r in net.layers]
    seed = 1
    for seed in range(1, 33):                             # a seed whose Bernoulli decisions are clear of a tie in the double's run
        G.reset_margin()
        import oracle.rbm_oracle as O
        O.reset_margin()
        cpu = iDBN([12, 7, 5], params, dl, dl, torch.device("cpu"))
        cpu.layers = [_cpu_copy(r) for r in twins]
        E.set_engine_for_testing(GaussOracleEngine())
        E.manual_seed(seed)
        try:
            cpu.train(1)
        finally:
            E.set_engine_for_testing(None)
            E.set_rng(None)
        if min(O.BERNOULLI_MARGIN["min"], G.MARGIN["min"]) > 3e-6:
            break
    E.manual_seed(seed)
    try:
        net.train(1)
        torch.cuda.synchronize()
    finally:
        E.set_rng(None)
    assert torch.allclose(net.loss_history[0], cpu.loss_history[0], atol=5e-6)
    for a, b in zip(net.layers, cpu.layers):
        _same_model(a, b, "iDBN(GAUSSIAN_VISIBLE).train")
    close(net.represent(X).cpu().numpy(), cpu_represent(cpu, X), 1e-5, "represent")


def cpu_represent(cpu, X):
    from gauss_engine_double import GaussOracleEngine
    from imdbn import engine as E
    E.set_engine_for_testing(GaussOracleEngine())
    try:
        return cpu.represent(X).numpy()
    finally:
        E.set_engine_for_testing(None)
