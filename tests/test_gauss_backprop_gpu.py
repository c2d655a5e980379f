"""GPU: imdbn_rbm_gauss_backprop_step and HipEngine.gauss_autoencoder_step against the float64 numpy twin
(tests/gauss_backprop_oracle.py) on the cases of tests/gauss_backprop_cases.py.

Tolerances.  W, the biases and their momenta: the project's for an update, 1e-4 relative (Frobenius) with atol 2e-6.  err_h: the derived
bound of DESIGN section 26, (V + 16) 2^-23 (sum_i |e_0,bi| |W_ij|) x_h (1 - x_h) per element, evaluated in float64 from the twin; the
largest measured share of it is printed.  logvar, logvar_m, nll and mse had no tolerance: each is 8 x the largest error of the float32
numpy restatement against the float64 twin over every single call and composed run (gauss_backprop_cases.fp32_errors, measured on the
CPU when the tests run; nll and mse relative to max(1, |twin|)), the convention and margin of tests/test_gauss_gpu.py.  The mean m the
call works on is read back from its scratch and must be gauss_backward's bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import gauss_backprop_cases as Cs
import gauss_backprop_oracle as Go
from golden_utils import assert_close, rel_fro
from likelihood_gpu import DEV, _native, close, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIX = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")
TWIN_KEY = dict(W="W", hid_bias="c", vis_bias="b", W_m="W_m", hb_m="hb_m", vb_m="vb_m")
RUN_IDS = [f"{s}-{f}" for s, f in Cs.RUNS]


def _tol():
    e = twin(("gauss_backprop", "fp32"), Cs.fp32_errors)
    return {k: 8 * v for k, v in e.items()}


def _twin(c, form):
    return twin(("gauss_backprop", c["name"], form), lambda: Cs.twin_call(c, form))


def _rbm(c, pitch=None):
    """The case's RBM on the device with its momenta and weight decay.  `pitch`: W and W_m as views of NaN-filled [V, pitch]
    buffers; a case with w_offset has W and W_m start that many floats into theirs (not 16-byte aligned)."""
    r = device_rbm(c)
    r.weight_decay = Cs.WEIGHT_DECAY
    V, H, off = c["V"], c["H"], c["w_offset"]
    if pitch is not None or off:
        p = H if pitch is None else pitch
        for nm in ("W", "W_m"):
            flat = torch.full((V * p + off,), float("nan"), device=DEV)
            t = flat[off:].view(V, p)[:, :H]
            t.copy_(dev(c[nm]))
            if nm == "W":
                r.W.data = t
            else:
                r.W_m = t
    else:
        r.W_m = torch.zeros_like(r.W.data)
        r.W_m.copy_(dev(c["W_m"]))
    r.hb_m, r.vb_m = dev(c["hb_m"]), dev(c["vb_m"])
    return r


def _t(r, k):
    x = getattr(r, k)
    return x.data if k in SIX[:3] else x


def _step(eng, c, form, r=None, data=None, e_h=None, x_h=None, lr_z=Cs.LR_Z, **kw):
    """One gauss_backprop_step of `form` on the device: (rbm, logvar, logvar_m, err_h, nll, mse)."""
    r = _rbm(c) if r is None else r
    z, zm = dev(c["z"]), dev(c["z_m"])
    a = Cs.form_args(c, form)
    up = None if a["up"] is None else (dev(a["up"]) if e_h is None else e_h)
    down = None if a["down"] is None else (dev(a["down"]) if x_h is None else x_h)
    err_h, nll, mse = eng.gauss_backprop_step(r, z, zm, dev(c["data"]) if data is None else data, up=up, down=down, lr=Cs.LR, mom=Cs.MOM,
                                              lr_z=lr_z, apply=a["apply"], want_h=down is not None, monitor=down is not None, **kw)
    torch.cuda.synchronize()
    return r, z, zm, err_h, nll, mse


def _mean_of_last_call(eng, c):
    """The mean m the last call on this shape left in its scratch: [B][V] behind the V H statistics (padded to 4 floats)."""
    V, H, B = c["V"], c["H"], c["B"]
    s = eng._ws[("gauss_backprop", torch.device(DEV), V, H, B, torch.cuda.current_stream(torch.device(DEV)).cuda_stream)]
    off = (V * H + 3) // 4 * 4
    return s[off:off + B * V].view(B, V).clone()


def _check(c, form, t, got, what):
    r, z, zm, err_h, nll, mse = got
    tol, st, out = _tol(), t["st"], t["out"]
    have = {k: _t(r, k).cpu().numpy() for k in SIX}
    print(f"{what}: rel-Frobenius vs twin:", ", ".join(f"{k} {rel_fro(have[k], getattr(st, TWIN_KEY[k])):.2e}" for k in SIX))
    for k in SIX:
        assert_close(have[k], getattr(st, TWIN_KEY[k]), 1e-4, f"{what}: {k}", atol=2e-6)
    close(z.cpu().numpy(), st.z, tol["z"], f"{what}: logvar")
    close(zm.cpu().numpy(), st.z_m, tol["z_m"], f"{what}: logvar_m")
    if out["err_h"] is not None:
        bound = (c["V"] + 16) * 2.0 ** -23 * out["mag_h"]
        err = np.abs(err_h.cpu().numpy().astype(F64) - out["err_h"])
        print(f"{what}: err_h largest share of the bound {float((err / bound).max()):.3g}")
        assert (err <= bound).all()
        for k, v in (("nll", nll), ("mse", mse)):
            e = abs(float(v) - out[k]) / max(1.0, abs(out[k]))
            print(f"{what}: {k} {float(v):.7g} vs twin {out[k]:.7g}: relative error {e:.3g} (tolerance {tol[k]:.3g})")
            assert e <= tol[k]
    # what the call has no gradient for stays bit-equal
    same = {"up": ("vis_bias", "vb_m"), "down": ("hid_bias", "hb_m"), "both": (), "eval": SIX}[form]
    for k in same:
        assert np.array_equal(have[k], c[TWIN_KEY[k]]), f"{what}: {k} moved"
    if form == "eval":
        assert torch.equal(z, dev(c["z"])) and torch.equal(zm, dev(c["z_m"]))


# ---- 1. against the twin --------------------------------------------------------------------------------------------------------------
def test_the_fp32_restatement_alone_passes_at_the_tolerances():
    e, tol = twin(("gauss_backprop", "fp32"), Cs.fp32_errors), _tol()
    print("fp32 restatement vs float64 twin:", e, "-> tolerances", tol)
    assert all(0 < e[k] <= tol[k] / 8 for k in e)


@pytest.mark.parametrize("name,form", Cs.RUNS, ids=RUN_IDS)
def test_gauss_backprop_step_matches_the_twin(eng, name, form):
    c = Cs.case(name)
    r = _rbm(c)
    if c["w_offset"]:
        assert r.W.data.data_ptr() % 16 == 4 and c["H"] % 4 == 0
    got = _step(eng, c, form, r=r)
    _check(c, form, _twin(c, form), got, f"{name} {form}")
    if form != "up":      # the mean inside the call is gauss_backward's, bit for bit (W of a fresh RBM: the call above moved r's)
        m = _mean_of_last_call(eng, c)
        assert torch.equal(m, eng.gauss_backward(_rbm(c), dev(c["z"]), dev(c["x_h"])))


# ---- 2. invariants ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "rows67", "wide"])
def test_the_same_call_twice_gives_the_same_bits(eng, name):
    c = Cs.case(name)
    for form in ("both", "up"):
        outs = []
        for _ in range(2):
            r, z, zm, err_h, nll, mse = _step(eng, c, form)
            outs.append([z, zm] + [_t(r, q) for q in SIX] + ([err_h, nll, mse] if err_h is not None else []))
        assert all(torch.equal(a, b) for a, b in zip(*outs)), form


@pytest.mark.parametrize("name,pitch", [("odd", 41), ("rows67", 208), ("wide", 104)])
def test_strided_operands_and_nan_poisoned_row_padding(eng, name, pitch):
    c = Cs.case(name)
    B, V, H = c["B"], c["V"], c["H"]

    def inside(a, n):
        big = torch.full((B + 2, n + 7), float("nan"), device=DEV)
        big[:B, :n] = dev(a)
        return big[:B, :n]

    for form in ("both", "down", "up"):
        ref = _step(eng, c, form)
        r = _rbm(c, pitch)
        d, e, x = inside(c["data"], V), inside(c["e_h"], H), inside(c["x_h"], H)
        assert r.W.data.stride(0) == pitch == r.W_m.stride(0) and not d.is_contiguous()
        got = _step(eng, c, form, r=r, data=d, e_h=e, x_h=x)
        assert r.W.data.stride(0) == pitch == r.W_m.stride(0)
        for q in SIX:
            assert torch.equal(_t(got[0], q), _t(ref[0], q)), (form, q)
        assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
        if form != "up":
            assert all(torch.equal(a, b) for a, b in zip(got[3:], ref[3:]))
        for q in ("W", "W_m"):
            full = torch.as_strided(_t(r, q), (V, pitch), (pitch, 1))
            assert torch.isnan(full[:, H:]).all() and not torch.isnan(full[:, :H]).any(), (form, q)


def test_the_clamps_hold(eng):
    c = Cs.case("odd")
    r, z, zm, *_ = _step(eng, c, "both", lr_z=5.0, z_lo=-0.25, z_hi=0.5)
    t = Cs.twin_call(c, "both", lr_z=5.0, z_lo=-0.25, z_hi=0.5)
    assert float(z.min()) >= -0.25 and float(z.max()) <= 0.5 and bool((z == -0.25).any()) and bool((z == 0.5).any())
    close(z.cpu().numpy(), t["st"].z, 5.0 / Cs.LR_Z * _tol()["z"], "clamped logvar")      # the same fp32 error of g, times this lr_z


# ---- 3. errors ------------------------------------------------------------------------------------------------------------------------
def _raw(eng, args):
    from imdbn.engine import native as Nt
    try:
        eng._call("imdbn_rbm_gauss_backprop_step", *args)
    except Nt.EngineError as e:
        torch.cuda.synchronize()
        return str(e)
    torch.cuda.synchronize()
    return None


def _args(eng, r, c, z, zm, err_h, loss, scratch, up=True, down=True, opts=True, need_m=True, B=None, ldv=None, ldeh=None, ldxh=None,
          ldoh=None, lr_z=Cs.LR_Z, z_lo=float("-inf"), z_hi=float("inf"), groups=0, null=(), **fields):
    from imdbn.engine import native as Nt
    d = eng._desc(r, True)
    if not need_m or groups:
        d = Nt.RbmDesc.from_buffer_copy(d)
        if not need_m:
            d.hb_m = None
        if groups:
            d.n_groups, d.group_start[0], d.group_end[0] = 1, 0, 4
    o = eng._opts(r, Cs.LR, Cs.MOM, 0)
    for k, v in fields.items():
        setattr(o, k, v)
    data, eh, xh = dev(c["data"]), dev(c["e_h"]), dev(c["x_h"])
    B = data.size(0) if B is None else B
    P = lambda t, nm: None if (nm in null or t is None) else C.c_void_p(t.data_ptr())
    pick = lambda v, default: default if v is None else v
    return (C.byref(d), P(z, "logvar"), P(zm, "logvar_m"), P(data, "v"), pick(ldv, data.stride(0)), P(eh if up else None, "e_h"),
            pick(ldeh, eh.stride(0)), P(xh if down else None, "x_h"), pick(ldxh, xh.stride(0)), B, C.byref(o) if opts else None, lr_z, z_lo,
            z_hi, P(err_h, "err_h"), pick(ldoh, d.H), P(loss, "loss"), P(scratch, "scratch"),
            *eng._ws_tail(torch.device(DEV), d.V, d.H, max(B, 1))), (d, o, data, eh, xh)


# what -> (keywords of _args, return code, needle of the message); `odd` is 37 x 33
BAD = {
    "no_pair": (dict(up=False, down=False, null=("err_h", "loss")), -1, "no pair"),
    "err_h_without_down": (dict(down=False, null=("loss",)), -1, "err_h_out"), "loss_without_down": (dict(down=False, null=("err_h",)), -1, "loss_out"),
    "nothing_to_do": (dict(opts=False, null=("err_h", "loss")), -1, "nothing to do"),
    "ldv": (dict(ldv=36), -1, "ldv 36"), "ldeh": (dict(ldeh=32), -1, "ldeh 32"), "ldxh": (dict(ldxh=32), -1, "ldxh 32"),
    "ldoh": (dict(ldoh=32), -1, "ldoh 32"), "B0": (dict(B=0), -1, "B = 0"),
    "lr_z_nan": (dict(lr_z=float("nan")), -1, "lr_z = nan"), "empty_clamp": (dict(z_lo=1.0, z_hi=0.5), -1, "clamp [1, 0.5]"),
    "clamp_nan": (dict(z_hi=float("nan")), -1, "clamp ["), "null_logvar_m": (dict(null=("logvar_m",)), -1, "null logvar_m"),
    "null_logvar": (dict(null=("logvar",)), -1, "null logvar"), "null_v": (dict(null=("v",)), -1, "null v"),
    "null_scratch": (dict(null=("scratch",)), -1, "null scratch"), "momentum": (dict(need_m=False), -1, "null momentum buffer"),
    "cd_k": (dict(cd_k=1), -1, "cd_k 1"), "sparsity": (dict(sparsity=1), -1, "sparsity 1"), "data_slot": (dict(data_slot=1), -1, "data_slot 1"),
    "next_slot": (dict(next_slot=2), -1, "next_slot 2"), "fwd_out": (dict(fwd_out=64), -1, "fwd_out 0x40"),
    "groups": (dict(groups=1), -5, "1 softmax groups"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_invalid_arguments_name_their_value_touch_nothing_and_a_good_call_follows(eng, what):
    c = Cs.case("odd")
    kw, rc, needle = BAD[what]
    r = _rbm(c)
    before = {k: _t(r, k).clone() for k in SIX}
    S = lambda *shape: torch.full(shape, -7.25, device=DEV)
    z, zm, err_h, loss = S(c["V"]), S(c["V"]), S(c["B"], c["H"]), S(2)
    scratch = S(int(eng._lib.imdbn_gauss_backprop_scratch_floats(c["V"], c["H"], c["B"])))
    args, keep = _args(eng, r, c, z, zm, err_h, loss, scratch, **kw)
    msg = _raw(eng, args)
    print(what, "->", msg)
    assert msg is not None and f"rc={rc})" in msg and needle in msg
    assert all(bool((t == -7.25).all()) for t in (z, zm, err_h, loss, scratch))
    assert all(torch.equal(_t(r, k), before[k]) for k in SIX)
    # a good call follows on the same workspace and scratch
    z, zm = dev(c["z"]), dev(c["z_m"])
    args, keep = _args(eng, r, c, z, zm, err_h, loss, scratch)
    assert _raw(eng, args) is None
    _check(c, "both", _twin(c, "both"), (r, z, zm, err_h, loss[0], loss[1]), f"after {what}")


def test_lr_z_zero_takes_a_null_momentum_and_touches_no_logvar(eng):
    c = Cs.case("odd")
    r = _rbm(c)
    z, zm = dev(c["z"]), dev(c["z_m"])
    scratch = torch.empty(int(eng._lib.imdbn_gauss_backprop_scratch_floats(c["V"], c["H"], c["B"])), device=DEV)
    args, keep = _args(eng, r, c, z, zm, None, None, scratch, lr_z=0.0, null=("logvar_m",))
    assert _raw(eng, args) is None
    assert torch.equal(z, dev(c["z"])) and torch.equal(zm, dev(c["z_m"]))
    t = twin(("gauss_backprop", "odd", "fixed"), lambda: Cs.twin_call(c, "both", lr_z=0.0))
    for k in SIX:
        assert_close(_t(r, k).cpu().numpy(), getattr(t["st"], TWIN_KEY[k]), 1e-4, f"fixed variances: {k}", atol=2e-6)
    # the wrapper: lr_z = 0 needs no momentum tensor, and tensors that would have to be copied are refused
    r2 = _rbm(c)
    eng.gauss_backprop_step(r2, z, None, dev(c["data"]), up=dev(c["e_h"]), down=dev(c["x_h"]), lr=Cs.LR, mom=Cs.MOM)
    torch.cuda.synchronize()
    assert all(torch.equal(_t(r, k), _t(r2, k)) for k in SIX) and torch.equal(z, dev(c["z"]))
    from imdbn import engine as E
    with pytest.raises(E.EngineError):
        eng.gauss_backprop_step(r2, z.double(), zm, dev(c["data"]), up=dev(c["e_h"]), lr=Cs.LR, lr_z=0.1)
    with pytest.raises(E.EngineError):
        eng.gauss_backprop_step(r2, z, dev(np.zeros(2 * c["V"], F32))[::2], dev(c["data"]), up=dev(c["e_h"]), lr=Cs.LR, lr_z=0.1)
    with pytest.raises(E.EngineError):
        eng.gauss_backprop_step(r2, z, zm, dev(c["data"]), up=dev(c["e_h"]), want_h=True)


# ---- 4. the composed step through the model ---------------------------------------------------------------------------------------------
def _net(s):
    """An iDBN(GAUSSIAN_VISIBLE) on the device holding the stack's parameters and momenta."""
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import GaussianRBM, iDBN
    X = torch.from_numpy(s["data"])
    dl = DataLoader(TensorDataset(X, torch.zeros(len(X))), batch_size=len(X))
    params = {"LEARNING_RATE": Cs.LR, "WEIGHT_PENALTY": Cs.WEIGHT_DECAY, "INIT_MOMENTUM": Cs.MOM, "FINAL_MOMENTUM": Cs.MOM,
              "LEARNING_RATE_DYNAMIC": False, "CD": 1, "GAUSSIAN_VISIBLE": True, "GAUSSIAN_LR_SIGMA_MULT": Cs.LR_Z_MULT}
    torch.manual_seed(0)
    net = iDBN(s["sizes"], params, dl, dl, torch.device(DEV))
    assert isinstance(net.layers[0], GaussianRBM) and net.layers[0].W.is_cuda
    for r, l in zip(net.layers, s["layers"]):
        gauss = "z" in l
        r.W.data.copy_(dev(l["W"]))
        r.vis_bias.data.copy_(dev(l["b"] if gauss else l["vis_bias"])); r.hid_bias.data.copy_(dev(l["c"] if gauss else l["hid_bias"]))
        r.W_m = torch.zeros_like(r.W.data)
        r.W_m.copy_(dev(l["W_m"]))
        r.hb_m, r.vb_m = dev(l["hb_m"]), dev(l["vb_m"])
        if gauss:
            r.logvar.data.copy_(dev(l["z"])); r.logvar_m = dev(l["z_m"])
    return net, X.to(DEV)


@pytest.mark.parametrize("name", list(Cs.STACKS))
def test_three_gaussian_autoencoder_steps_match_the_twin(eng, name):
    s = Cs.stack(name)
    t = twin(("gauss_backprop", "stack", name), lambda: Cs.twin_stack_run(s))
    tol = _tol()
    net, x = _net(s)
    L = len(net.layers)
    gen = net.gaussian_untie()
    assert len(gen) == L - 1
    for i in range(Cs.STEPS):
        want_recon = net.reconstruct(x)                     # on the parameters on entry
        out = eng.gauss_autoencoder_step(net.layers, gen, x, [(Cs.LR, Cs.MOM)] * L)
        torch.cuda.synchronize()
        assert torch.equal(out["recon"], want_recon), f"step {i}"
        w = t["steps"][i]
        for k in ("nll", "mse"):
            e = abs(float(out[k]) - w[k]) / max(1.0, abs(w[k]))
            print(f"{name} step {i}: {k} {float(out[k]):.7g} vs twin {w[k]:.7g}: relative error {e:.3g} (tolerance {tol[k]:.3g})")
            assert e <= tol[k]
        close(out["code"].cpu().numpy(), w["code"], 1e-5, f"{name} step {i}: code")
    for i, (r, st) in enumerate(zip(net.layers + gen, t["rec"] + t["gen"])):
        gauss = hasattr(st, "z")
        key = TWIN_KEY if gauss else {k: k for k in SIX}
        what = f"{name}: {'layer' if i < L else 'twin'} {i % L if i < L else i - L}"
        for k in SIX:
            assert_close(_t(r, k).cpu().numpy(), getattr(st, key[k]), 1e-4, f"{what}: {k}", atol=2e-6)
        if gauss:
            close(r.logvar.data.cpu().numpy(), st.z, tol["z"], f"{what}: logvar")
            close(r._zm().cpu().numpy(), st.z_m, tol["z_m"], f"{what}: logvar_m")


def test_the_model_step_on_the_device_is_the_engine_step(eng):
    s = Cs.stack("odd3")
    (a, x), (b, _) = _net(s), _net(s)
    m = a.gaussian_autoencoder_step(x, 0, 1)
    out = eng.gauss_autoencoder_step(b.layers, b.gaussian_untie(), x, [(Cs.LR, Cs.MOM)] * 2)
    torch.cuda.synchronize()
    assert torch.equal(m["nll"], out["nll"]) and torch.equal(m["mse"], out["mse"])
    for p, q in zip(a.layers + a.gen_layers, b.layers + b.gen_layers):
        assert all(torch.equal(_t(p, k), _t(q, k)) for k in SIX)
    assert torch.equal(a.gen_layers[0].logvar.data, b.gen_layers[0].logvar.data)
