"""GPU: imdbn_rbm_backprop_step / HipEngine.backprop_step / HipEngine.autoencoder_step / iDBN.autoencoder_step against the float64
numpy twin (tests/backprop_oracle.py) on the stacks of tests/backprop_cases.py.  Nothing draws: there are no seeds and no margins.

The six parameter and momentum tensors of an update follow tests/test_updown_gpu.py's rule (tests/test_pcd_gpu.py's): 1e-4 relative
(Frobenius), atol 2e-6.  An error output is held element by element to (N + 16) 2^-23 (sum_j |e_bj| |W_ij|) x (1 - x), N the summed
dimension: fp32 accumulation of N products in any order stays within N 2^-24 of the sum of magnitudes, the products are exact by the
three-term split, the epilogue adds two roundings, and a factor 2 is margin -- derived, not measured; the twin computes the magnitude
sum alongside.  recon / code / xent follow the per-unit budget of tests/test_dbn_bound_gpu.py (`_path_tol`, `_close`, imported): 1e-5
per unit of the layers on the path, here all L layers of the stack -- an error delta in an output logit moves the row's cross-entropy
by |data_j - sigmoid(z_j)| delta <= delta."""
import ctypes as C

import numpy as np
import pytest
import torch

import backprop_cases as Cs
import backprop_oracle as Bp
import pcd_oracle as P
from golden_utils import assert_close, rel_fro
from likelihood_gpu import DEV, _native, close, dev, eng, twin  # noqa: F401  (the fixtures, by name)
from pcd_cases import LR, MOM, WEIGHT_DECAY
from test_dbn_bound_gpu import _close, _path_tol
from test_updown_gpu import PITCH, SIX, _check6, _model, _np6, _rbm, _same6, _six

pytestmark = pytest.mark.gpu

ALL = list(Cs.CASES)
FORMS = {"up": (True, False, True), "down": (False, True, True), "both": (True, True, True), "evaluate": (True, True, False)}


def _state(l):
    return P.rbm_state(l, LR, WEIGHT_DECAY, MOM)


def _pairs(io, up, down, to=lambda a: a):
    return ((to(io["x_v"]), to(io["e_h"])) if up else None), ((to(io["x_h"]), to(io["e_v"])) if down else None)


def _err_close(got, want, mag, N, what):
    """|got - want| <= (N + 16) 2^-23 mag, element by element."""
    tol = (N + 16) * 2.0 ** -23 * mag
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"   {what}: max |device - twin| / bound {float((err / tol).max()):.3g} (largest error {err.max():.3g})")
    assert (err <= tol).all(), f"{what}: {float((err / tol).max()):.3g} times the bound"


# ---- 1. backprop_step against the twin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ALL)
def test_backprop_step_matches_the_twin(eng, name, form):
    c = Cs.case(name)
    up, down, apply = FORMS[form]
    for li in Cs.layers_of(name):
        io = Cs.layer_io(c, li)
        l = io["l"]
        V, H = l["W"].shape
        st = _state(l)
        want = Bp.backprop_step(st, *_pairs(io, up, down), LR, MOM, apply)
        r = _rbm(l)
        before = _six(r)
        ev, eh = eng.backprop_step(r, *_pairs(io, up, down, dev), LR, MOM, apply=apply, want_v=up, want_h=down)
        torch.cuda.synchronize()
        what = f"{name} layer {li} {form}"
        assert (ev is None) == (not up) and (eh is None) == (not down)
        if up:
            assert tuple(ev.shape) == (c["B"], V)
            _err_close(ev, want["err_v"], want["mag_v"], H, what + ": err_v")
        if down:
            assert tuple(eh.shape) == (c["B"], H)
            _err_close(eh, want["err_h"], want["mag_h"], V, what + ": err_h")
        after = _six(r)
        if not apply:
            assert _same6(after, before), "evaluate-only wrote a parameter"
            continue
        _check6(r, st, what)
        still = (() if up else ("hid_bias", "hb_m")) + (() if down else ("vis_bias", "vb_m"))
        for k in still:
            assert torch.equal(after[k], before[k]), f"{k} was touched"
        for k in set(SIX) - set(still):
            assert not torch.equal(after[k], before[k]), f"{k} did not move"


# ---- 2. backprop_step against the engine's own composed calls -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "rows67", "wide", "odd_real"])
def test_backprop_step_equals_the_composed_calls(eng, name):
    c = Cs.case(name)
    io = Cs.layer_io(c, 0)
    l = dict(io["l"])
    l["vb_m"] = np.zeros_like(l["vb_m"])            # the composed update decays the other bias's momentum: start it at zero
    x, e = dev(io["x_v"]), dev(io["e_h"])
    a, b, z = _rbm(l), _rbm(l), _rbm(l)
    z.vis_bias.data.zero_()
    ev = eng.backprop_step(a, up=(x, e), lr=LR, mom=MOM, want_v=True)[0]
    ref = eng.prop_down(z, e, logits_only=True) * (x * (1 - x))      # three roundings, and fma contraction either way
    eng.assoc_update(b, x, e, x, torch.zeros_like(e), LR, MOM)
    torch.cuda.synchronize()
    got, want = ev.cpu().numpy(), ref.cpu().numpy()
    ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want))
    print(f"{name}: err_v vs the composed product: {float(ulps.max()):.3g} ulps at most")
    assert (ulps <= 4).all()
    ga, gb = _np6(a), _np6(b)
    print(f"{name}: fused vs composed:", ", ".join(f"{k} {rel_fro(ga[k], gb[k]):.2e}" for k in SIX))
    for k in SIX:
        assert_close(ga[k], gb[k], 1e-4, f"{name}: {k} vs composed", atol=2e-6)


# ---- 3. autoencoder_step against the twin -------------------------------------------------------------------------------------------
def _net(c):
    """The case as an untied iDBN on the device: `layers` the recognition parameters, `gen_layers` the case's generative ones."""
    net = _model(c)
    for g, l in zip(net.untie(), c["gen"]):
        g.W.data.copy_(dev(l["W"])); g.vis_bias.data.copy_(dev(l["b"])); g.hid_bias.data.copy_(dev(l["c"]))
        g.W_m.copy_(dev(l["W_m"])); g.hb_m.copy_(dev(l["hb_m"])); g.vb_m.copy_(dev(l["vb_m"]))
    return net


def _run_device(eng, c):
    net = _net(c)
    data = dev(c["data"])
    recon0 = net.reconstruct(data).clone()
    outs = []
    for _ in range(Cs.STEPS):
        o = eng.autoencoder_step(net.layers, net.gen_layers, data, [Cs.SCALARS] * len(net.layers))
        outs.append({k: v.clone() for k, v in o.items()})
    torch.cuda.synchronize()
    return net, outs, recon0


@pytest.mark.parametrize("name", ALL)
def test_autoencoder_step_matches_the_twin(eng, name):
    c = Cs.case(name)
    t = twin(("backprop", name), lambda: Cs.twin_run(c))
    net, outs, recon0 = _run_device(eng, c)
    units, _ = _path_tol([(l["W"], l["b"], l["c"]) for l in c["rec"]], 0.0)
    assert torch.equal(outs[0]["recon"], recon0), "the first step's recon is not iDBN.reconstruct on the entry parameters"
    for s, (o, w) in enumerate(zip(outs, t["steps"])):
        assert o["xent"].dim() == 0 and o["xent"].dtype == torch.float64 and o["mse"].dim() == 0
        _close(o["recon"].cpu().numpy(), w["recon"], units, f"{name} step {s} recon")
        _close(o["code"].cpu().numpy(), w["code"], units, f"{name} step {s} code")
        _close(np.array(float(o["xent"])), np.array(w["xent"]), units, f"{name} step {s} xent")
        # mean of e^2, |e| <= 1: moves by at most twice the error of recon
        close(float(o["mse"]), w["mse"], 2 * units * 1e-5 + 1e-6, f"{name} step {s} mse")
    for i, (r, st) in enumerate(zip(net.layers, t["rec"])):
        _check6(r, st, f"{name} rec {i}")
    for i, (r, st) in enumerate(zip(net.gen_layers, t["gen"])):
        _check6(r, st, f"{name} gen {i}")


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h130", "rows67", "wide"])
def test_the_same_three_steps_twice_give_the_same_bits(eng, name):
    c = Cs.case(name)
    na, oa, _ = _run_device(eng, c)
    nb, ob, _ = _run_device(eng, c)
    for a, b in zip(na.layers + na.gen_layers, nb.layers + nb.gen_layers):
        assert _same6(_six(a), _six(b))
    for a, b in zip(oa, ob):
        assert all(torch.equal(a[k], b[k]) for k in ("recon", "code", "xent", "mse"))


# ---- 5. layout ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["up", "down", "both"])
@pytest.mark.parametrize("name,li", list(PITCH))
def test_strided_operands_and_padded_weights_give_the_contiguous_bits(eng, name, li, form):
    c = Cs.case(name)
    io = Cs.layer_io(c, li)
    l = io["l"]
    up, down, _ = FORMS[form]
    pitch = PITCH[(name, li)]
    V, H = l["W"].shape
    assert pitch > H
    plain, padded = _rbm(l, H), _rbm(l, pitch, float("nan"))
    out_a = eng.backprop_step(plain, *_pairs(io, up, down, dev), LR, MOM, want_v=up, want_h=down)
    parents = []

    def inside(a):
        parent = torch.full((a.shape[0], a.shape[1] + 7), float("nan"), device=DEV)
        parent[:, 3:3 + a.shape[1]] = dev(a)
        parents.append((parent, a.shape[1]))
        return parent[:, 3:3 + a.shape[1]]
    out_b = eng.backprop_step(padded, *_pairs(io, up, down, inside), LR, MOM, want_v=up, want_h=down)
    torch.cuda.synchronize()
    for a, b in zip(out_a, out_b):
        assert (a is None and b is None) or (torch.equal(a, b) and not torch.isnan(b).any())
    assert _same6(_six(plain), _six(padded))
    assert not any(torch.isnan(v).any() for v in _six(padded).values()), "a NaN was read"
    for r in (padded.W.data, padded.W_m):
        full = torch.as_strided(r, (V, pitch), (pitch, 1))
        assert torch.isnan(full[:, H:]).all(), "the row padding was written"
    for parent, n in parents:
        assert torch.isnan(parent[:, :3]).all() and torch.isnan(parent[:, 3 + n:]).all()


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def _raw(eng, args):
    from imdbn.engine import native as Nt
    try:
        eng._call("imdbn_rbm_backprop_step", *args)
    except Nt.EngineError as e:
        torch.cuda.synchronize()
        return str(e)
    torch.cuda.synchronize()
    return None


def _args(eng, r, t, outs, need_m=True, B=None, null=(), ld=None, groups=False, **fields):
    """The raw argument list: `t` the four device tensors by name, `outs` the two outputs; `null`: names passed as NULL ("d",
    "opts" and the tensors' names), `ld`: leading dimensions to overwrite, `fields`: members of the options to set."""
    from imdbn.engine import native as Nt
    d = eng._desc(r, True)
    if not need_m or groups:
        d = Nt.RbmDesc.from_buffer_copy(d)
        if not need_m:
            d.hb_m = None
        if groups:
            d.n_groups, d.group_start[0], d.group_end[0] = 1, 2, 6
    o = eng._opts(r, LR, MOM, 0)
    for k, v in fields.items():
        setattr(o, k, v)
    B = t["x_v"].size(0) if B is None else B
    every = dict(t, **outs)
    Pp = lambda nm: None if nm in null else C.c_void_p(every[nm].data_ptr())
    Ld = lambda nm: (ld or {}).get(nm, every[nm].stride(0))
    seq = []
    for nm in ("x_v", "e_h", "x_h", "e_v"):
        seq += [Pp(nm), Ld(nm)]
    tail = []
    for nm in ("err_v", "err_h"):
        tail += [Pp(nm), Ld(nm)]
    return (None if "d" in null else C.byref(d), *seq, B, None if "opts" in null else C.byref(o), *tail,
            *eng._ws_tail(torch.device(DEV), d.V, d.H, max(B, 1))), (d, o)


# what -> (keywords of _args, needle of the message); `odd` layer 0 is 37 x 33
BAD = {
    "null_d": (dict(null=("d",)), "null descriptor"),
    "half_up_x": (dict(null=("x_v",)), "half an up pair"), "half_up_e": (dict(null=("e_h", "err_v")), "half an up pair"),
    "half_down_x": (dict(null=("x_h",)), "half a down pair"), "half_down_e": (dict(null=("e_v", "err_h")), "half a down pair"),
    "no_pair": (dict(null=("x_v", "e_h", "x_h", "e_v", "err_v", "err_h")), "no pair at all"),
    "err_v_alone": (dict(null=("x_v", "e_h")), "err_v_out"), "err_h_alone": (dict(null=("x_h", "e_v")), "err_h_out"),
    "nothing": (dict(null=("opts", "err_v", "err_h")), "nothing to do"),
    "ldxv": (dict(ld={"x_v": 36}), "ldxv 36"), "ldeh": (dict(ld={"e_h": 32}), "ldeh 32"), "ldxh": (dict(ld={"x_h": 32}), "ldxh 32"),
    "ldev": (dict(ld={"e_v": 36}), "ldev 36"), "ldov": (dict(ld={"err_v": 36}), "ldov 36"), "ldoh": (dict(ld={"err_h": 32}), "ldoh 32"),
    "B0": (dict(B=0), "B = 0"), "momentum": (dict(need_m=False), "null momentum buffer"), "cd_k": (dict(cd_k=1), "cd_k 1"),
    "sparsity": (dict(sparsity=1), "sparsity 1"), "data_slot": (dict(data_slot=1), "data_slot 1"),
    "next_slot": (dict(next_slot=2), "next_slot 2"), "next_binary": (dict(next_binary=1), "next_binary 1"),
    "fwd_out": (dict(fwd_out=64), "fwd_out 0x40"), "next_data": (dict(next_data=128), "next_data 0x80"),
    "groups": (dict(groups=True), "softmax groups"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_bad_arguments_name_the_value_and_touch_nothing(eng, what):
    kw, needle = BAD[what]
    c = Cs.case("odd")
    io = Cs.layer_io(c, 0)
    l = io["l"]
    r = _rbm(l)
    t = {k: dev(io[k]) for k in ("x_v", "e_h", "x_h", "e_v")}
    outs = dict(err_v=torch.full_like(t["x_v"], -7.0), err_h=torch.full_like(t["x_h"], -7.0))
    before = _six(r)
    args, keep = _args(eng, r, t, outs, **kw)
    msg = _raw(eng, args)
    print(what, "->", msg)
    assert msg is not None and needle in msg, msg
    assert ("rc=-5" in msg) == (what == "groups") and ("rc=-1" in msg) == (what != "groups")
    assert _same6(_six(r), before) and all(bool((o == -7.0).all()) for o in outs.values())
    # a good call follows on the same workspace
    good, keep2 = _args(eng, r, t, outs)
    assert _raw(eng, good) is None
    st = _state(l)
    want = Bp.backprop_step(st, (io["x_v"], io["e_h"]), (io["x_h"], io["e_v"]), LR, MOM, True)
    V, H = l["W"].shape
    _err_close(outs["err_v"], want["err_v"], want["mag_v"], H, f"after {what}: err_v")
    _err_close(outs["err_h"], want["err_h"], want["mag_h"], V, f"after {what}: err_h")
    _check6(r, st, f"after {what}")


# ---- 7. model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "h130"])
def test_idbn_autoencoder_step_is_the_hand_issued_engine_calls(eng, name):
    c = Cs.case(name)
    net, ref = _model(c), _model(c)
    data = dev(c["data"])
    mons = [net.autoencoder_step(data, 0, 1) for _ in range(Cs.STEPS)]
    gen = ref.untie()
    outs = [eng.autoencoder_step(ref.layers, gen, data, [Cs.SCALARS] * len(ref.layers)) for _ in range(Cs.STEPS)]
    torch.cuda.synchronize()
    for a, b in zip(net.layers + net.gen_layers, ref.layers + gen):
        assert _same6(_six(a), _six(b))
    for m, o in zip(mons, outs):
        assert set(m) == {"xent", "mse"} and all(torch.equal(m[k], o[k]) for k in m)
    assert net.autoencoder_step(data, 0, 1, monitor=False) is None
