"""GPU: imdbn_rbm_delta_step / HipEngine.delta_step / HipEngine.updown_step / iDBN.updown_step and the untied dbn_sample_values
against the numpy twin (tests/updown_oracle.py) on the stacks of tests/updown_cases.py.

Every case's seed was pinned on the CPU so that the twin's smallest Bernoulli margin stays above pcd_cases.MARGIN: every decision of
the device must be the twin's, so wake states, sleep states and particles are compared exactly.  The six parameter and momentum
tensors of an update follow tests/test_pcd_gpu.py's rule: 1e-4 relative (Frobenius), atol 2e-6.  out_rowlp follows the per-unit
budget of tests/test_dbn_bound_gpu.py (`_path_tol`, `_close`, imported): 1e-5 per unit of the layer -- an error delta in a logit
moves target_j a_j - softplus(a_j) by |target_j - sigmoid(a_j)| delta <= delta -- so one delta_step is held to
(V + H) 1e-5 + 1e-9 |rowlp|, and a monitor (a batch mean of sums over the directed layers) to sum_l (V_l + H_l) 1e-5 + 1e-9 |value|;
top_loss within 5e-7 as test_pcd_gpu.py has it."""
import ctypes as C

import numpy as np
import pytest
import torch

import bound_oracle as Bo
import pcd_oracle as P
import updown_cases as Cs
import updown_oracle as U
from golden_utils import assert_close, rel_fro
from likelihood_gpu import DEV, _native, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)
from oracle.draws import PhiloxStream
from pcd_cases import LR, MARGIN, MOM, WEIGHT_DECAY
from test_dbn_bound_gpu import _close, _path_tol

pytestmark = pytest.mark.gpu

ALL = list(Cs.CASES)
SIX = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")
PITCH = {("odd", 0): 41, ("wide", 1): 104}


def _rng(seed):
    from imdbn import engine as E
    return E.PhiloxRng(seed)


def _rbm(l, pitch=None, fill=None):
    """A layer dict of a case as an RBM on the device with its momenta and the cases' weight decay; `pitch`: W and W_m as views of
    [V, pitch] buffers filled with `fill`."""
    r = device_rbm(l, pitch=pitch)
    V, H = l["W"].shape
    if pitch is not None and fill is not None:
        buf = torch.full((V, pitch), fill, device=DEV)
        buf[:, :H] = dev(l["W"])
        r.W.data = buf[:, :H]
    r.weight_decay = WEIGHT_DECAY
    r.W_m = (torch.full((V, pitch), 0.0 if fill is None else fill, device=DEV)[:, :H] if pitch is not None else torch.zeros_like(r.W.data))
    r.W_m.copy_(dev(l["W_m"]))
    r.hb_m, r.vb_m = dev(l["hb_m"]), dev(l["vb_m"])
    return r


def _six(r):
    return {k: (getattr(r, k).data if k in ("W", "hid_bias", "vis_bias") else getattr(r, k)).clone() for k in SIX}


def _np6(r):
    return {k: v.cpu().numpy() for k, v in _six(r).items()}


def _same6(a, b):
    return all(torch.equal(a[k], b[k]) for k in SIX)


def _check6(r, st, what):
    got = _np6(r)
    print(f"   {what}: rel-Frobenius vs twin:", ", ".join(f"{k} {rel_fro(got[k], getattr(st, k)):.2e}" for k in SIX))
    for k in SIX:
        assert_close(got[k], getattr(st, k), 1e-4, f"{what}: {k}", atol=2e-6)


def _lp_close(got, want, l, what):
    units, extra = _path_tol([(l["W"], l["b"], l["c"])], 0.0)
    _close(got.cpu().numpy(), want, units, what, extra)


def _layer_io(c, li, direction):
    """(layer dict, in, target) of a delta step on directed layer `li`: fixed 0/1 rows (the case's data at layer 0, real for
    `odd_real`) on the input side, fixed rows on the other."""
    from anneal_cases import start_rows
    l = (c["rec"] if direction == "up" or li >= len(c["gen"]) else c["gen"])[li]
    V, H = l["W"].shape
    lo = c["data"] if li == 0 else start_rows(c["B"], V, 400 + li, (), p=0.4)
    hi = start_rows(c["B"], H, 410 + li, (), p=0.4)
    if c["name"] == "odd_real":
        hi = np.random.Generator(np.random.PCG64(420 + li)).uniform(0.02, 0.98, hi.shape).astype(np.float32)
    return (l, lo, hi) if direction == "up" else (l, hi, lo)


def _dirs(name):
    n = len(Cs.CASES[name][0]) - 2
    return sorted({0, n - 1})


# ---- 1. delta_step against the twin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["up", "down"])
@pytest.mark.parametrize("name", ALL)
def test_delta_step_matches_the_twin(eng, name, direction):
    c = Cs.case(name)
    for li in _dirs(name):
        l, x, t = _layer_io(c, li, direction)
        st = P.rbm_state(l, LR, WEIGHT_DECAY, MOM)
        want = U.delta_step(st, direction, x, t, LR, MOM)
        r = _rbm(l)
        before = _six(r)
        lp = eng.delta_step(r, direction, dev(x), dev(t), LR, MOM)
        torch.cuda.synchronize()
        assert lp.dtype == torch.float64 and tuple(lp.shape) == (c["B"],)
        _lp_close(lp, want, l, f"{name} layer {li} {direction}: rowlp")
        _check6(r, st, f"{name} layer {li} {direction}")
        after = _six(r)
        for k in (("vis_bias", "vb_m") if direction == "up" else ("hid_bias", "hb_m")):
            assert torch.equal(after[k], before[k]), f"{k} was touched"
        for k in (("hid_bias", "hb_m") if direction == "up" else ("vis_bias", "vb_m")) + ("W", "W_m"):
            assert not torch.equal(after[k], before[k]), f"{k} did not move"


# ---- 2. delta_step against the engine's own composed calls ------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["up", "down"])
@pytest.mark.parametrize("name", ["odd", "rows67", "wide", "odd_real"])
def test_delta_step_equals_the_composed_calls_and_evaluate_only_touches_nothing(eng, name, direction):
    c = Cs.case(name)
    l, x, t = _layer_io(c, 0, direction)
    l = dict(l)
    other = "vb_m" if direction == "up" else "hb_m"
    l[other] = np.zeros_like(l[other])            # the composed update decays the other bias's momentum: start it at zero
    x, t = dev(x), dev(t)
    a, b = _rbm(l), _rbm(l)
    before = _six(a)
    lp0 = eng.delta_step(a, direction, x, t, apply=False)
    assert _same6(_six(a), before), "evaluate-only wrote a parameter"
    lp1 = eng.delta_step(a, direction, x, t, LR, MOM)
    assert torch.equal(lp0, lp1)
    if direction == "up":
        p = eng.prop_up(b, x)                       # sigmoid of the propagation's logits
        eng.assoc_update(b, x, t, x, p, LR, MOM)
    else:
        p = torch.sigmoid(eng.prop_down(b, x, logits_only=True))
        eng.assoc_update(b, t, x, p, x, LR, MOM)
    torch.cuda.synchronize()
    ga, gb = _np6(a), _np6(b)
    print(f"{name} {direction}: fused vs composed:", ", ".join(f"{k} {rel_fro(ga[k], gb[k]):.2e}" for k in SIX))
    for k in SIX:
        assert_close(ga[k], gb[k], 1e-4, f"{name} {direction}: {k} vs composed", atol=2e-6)


# ---- 3. updown_step against the twin ------------------------------------------------------------------------------------------------
def _stack(c, pitches=None, fill=None):
    pitches = pitches or {}
    rec = [_rbm(l, pitches.get(("rec", i)), fill) for i, l in enumerate(c["rec"])]
    gen = [_rbm(l, pitches.get(("gen", i)), fill) for i, l in enumerate(c["gen"])]
    return rec, gen


def _run_device(eng, c, persistent, rec=None, gen=None, data=None):
    if rec is None:
        rec, gen = _stack(c)
    rng = _rng(c["seed"])
    data = dev(c["data"]) if data is None else data
    outs = []
    for _ in range(Cs.STEPS):
        o = eng.updown_step(rec, gen, data, [Cs.SCALARS] * len(rec), Cs.CD, "persistent" if persistent else None, rng)
        outs.append({k: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for k, v in o.items()})
    torch.cuda.synchronize()
    return rec, gen, outs, rng


@pytest.mark.parametrize("persistent", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_updown_step_matches_the_twin(eng, name, persistent):
    from imdbn import engine as E
    c = Cs.case(name)
    t = twin(("updown", name, persistent), lambda: Cs.twin_run(c, c["seed"], persistent))
    assert t["margin"] > MARGIN
    with E.use_rng(_rng(c["seed"])) as ambient:          # the persistent chains are created from the ambient draw source
        rec, gen = _stack(c)
        outs = []
        for _ in range(Cs.STEPS):
            o = eng.updown_step(rec, gen, dev(c["data"]), [Cs.SCALARS] * len(rec), Cs.CD, "persistent" if persistent else None, ambient)
            outs.append({k: ([x.clone() for x in v] if isinstance(v, list) else v.clone()) for k, v in o.items()})
        torch.cuda.synchronize()
        assert ambient.offset == t["offset"]
    units = sum(l["W"].shape[0] + l["W"].shape[1] for l in c["gen"])
    for s, (o, w) in enumerate(zip(outs, t["steps"])):
        for k in ("wake", "sleep"):
            for li, (a, b) in enumerate(zip(o[k], w[k])):
                bad = int((a.cpu().numpy() != b).sum())
                assert bad == 0, f"{name} step {s}: {k} state {li} differs in {bad} elements"
        assert int((o["particles"].cpu().numpy() != w["particles"]).sum()) == 0, f"{name} step {s}: particles differ"
        for k in ("wake_nll", "sleep_nll"):
            _close(np.array(float(o[k])), np.array(w[k]), units, f"{name} step {s} {k}")
        assert abs(float(o["top_loss"]) - float(w["top_loss"])) < 5e-7
    for i, (r, st) in enumerate(zip(rec, t["rec"])):
        _check6(r, st, f"{name} rec {i}")
    for i, (r, st) in enumerate(zip(gen, t["gen"])):
        _check6(r, st, f"{name} gen {i}")
    if persistent:
        assert rec[-1]._pcd is not None and int((rec[-1]._pcd.cpu().numpy() != t["steps"][-1]["particles"]).sum()) == 0


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h130", "rows67", "wide"])
def test_the_same_three_steps_twice_give_the_same_bits(eng, name):
    c = Cs.case(name)
    ra, ga, oa, na = _run_device(eng, c, False)
    rb, gb, ob, nb = _run_device(eng, c, False)
    assert na.offset == nb.offset
    for a, b in zip(ra + ga, rb + gb):
        assert _same6(_six(a), _six(b))
    for a, b in zip(oa, ob):
        for k in ("wake", "sleep"):
            assert all(torch.equal(x, y) for x, y in zip(a[k], b[k]))
        assert all(torch.equal(a[k], b[k]) for k in ("particles", "wake_nll", "sleep_nll", "top_loss"))


# ---- 5. layout ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["up", "down"])
@pytest.mark.parametrize("name,li", list(PITCH))
def test_strided_operands_and_padded_weights_give_the_contiguous_bits(eng, name, li, direction):
    c = Cs.case(name)
    l, x, t = _layer_io(c, li, direction)
    pitch = PITCH[(name, li)]
    V, H = l["W"].shape
    assert pitch > H
    plain, padded = _rbm(l, H), _rbm(l, pitch, float("nan"))
    lp_a = eng.delta_step(plain, direction, dev(x), dev(t), LR, MOM)

    def inside(a):
        parent = torch.full((a.shape[0], a.shape[1] + 7), float("nan"), device=DEV)
        parent[:, 3:3 + a.shape[1]] = dev(a)
        return parent, parent[:, 3:3 + a.shape[1]]
    px, xs = inside(x)
    pt, ts = inside(t)
    lp_b = eng.delta_step(padded, direction, xs, ts, LR, MOM)
    torch.cuda.synchronize()
    assert torch.equal(lp_a, lp_b)
    assert _same6(_six(plain), _six(padded))
    for r in (padded.W.data, padded.W_m):
        full = torch.as_strided(r, (V, pitch), (pitch, 1))
        assert torch.isnan(full[:, H:]).all(), "the row padding was written"
    for parent, n in ((px, x.shape[1]), (pt, t.shape[1])):
        assert torch.isnan(parent[:, :3]).all() and torch.isnan(parent[:, 3 + n:]).all()


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def _raw(eng, args):
    from imdbn.engine import native as Nt
    try:
        eng._call("imdbn_rbm_delta_step", *args)
    except Nt.EngineError as e:
        torch.cuda.synchronize()
        return str(e)
    torch.cuda.synchronize()
    return None


def _args(eng, r, direction, x, t, lp, need_m=True, B=None, ldi=None, ldt=None, null=(), groups=False, **fields):
    from imdbn.engine import native as Nt
    d = eng._desc(r, True)
    if not need_m or groups:
        d = Nt.RbmDesc.from_buffer_copy(d)
        if not need_m:
            d.vb_m = None
        if groups:
            d.n_groups, d.group_start[0], d.group_end[0] = 1, 2, 6
    o = eng._opts(r, LR, MOM, 0)
    for k, v in fields.items():
        setattr(o, k, v)
    B = x.size(0) if B is None else B
    Pp = lambda tn, nm: None if (nm in null or tn is None) else C.c_void_p(tn.data_ptr())
    return (None if "d" in null else C.byref(d), direction, Pp(x, "in"), x.stride(0) if ldi is None else ldi, Pp(t, "target"),
            t.stride(0) if ldt is None else ldt, B, None if "opts" in null else C.byref(o), Pp(lp, "rowlp"),
            *eng._ws_tail(torch.device(DEV), d.V, d.H, max(B, 1))), (d, o)


# what -> (keywords of _args, direction code, needle of the message, expected code in the message)
BAD = {
    "null_d": (dict(null=("d",)), 0, "null descriptor"), "null_in": (dict(null=("in",)), 0, "null in"),
    "null_target": (dict(null=("target",)), 1, "null target"), "ldi": (dict(ldi=36), 0, "ldi 36"), "ldt": (dict(ldt=32), 0, "ldt 32"),
    "ldi_down": (dict(ldi=32), 1, "ldi 32"), "ldt_down": (dict(ldt=36), 1, "ldt 36"),
    "B0": (dict(B=0), 0, "B = 0"), "dir2": (dict(), 2, "dir = 2"), "dir_negative": (dict(), -1, "dir = -1"),
    "momentum": (dict(need_m=False), 0, "null momentum buffer"), "cd_k": (dict(cd_k=1), 1, "cd_k 1"),
    "sparsity": (dict(sparsity=1), 0, "sparsity 1"), "data_slot": (dict(data_slot=1), 0, "data_slot 1"),
    "next_slot": (dict(next_slot=2), 1, "next_slot 2"), "next_binary": (dict(next_binary=1), 0, "next_binary 1"),
    "fwd_out": (dict(fwd_out=64), 1, "fwd_out 0x40"), "next_data": (dict(next_data=128), 0, "next_data 0x80"),
    "nothing": (dict(null=("opts", "rowlp")), 0, "nothing to do"),
    "groups_down": (dict(groups=True), 1, "softmax groups"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_bad_arguments_name_the_value_and_touch_nothing(eng, what):
    kw, direction, needle = BAD[what]
    c = Cs.case("odd")
    up = direction != 1
    l, x, t = _layer_io(c, 0, "up" if up else "down")
    r = _rbm(l)
    x, t = dev(x), dev(t)
    lp = torch.full((c["B"],), -7.0, dtype=torch.float64, device=DEV)
    before = _six(r)
    args, keep = _args(eng, r, direction, x, t, lp, **kw)
    msg = _raw(eng, args)
    print(what, "->", msg)
    assert msg is not None and needle in msg, msg
    assert ("rc=-5" in msg) == (what == "groups_down") and ("rc=-1" in msg) == (what != "groups_down")
    assert _same6(_six(r), before) and bool((lp == -7.0).all())
    # a good call follows on the same workspace
    good, keep2 = _args(eng, r, 0 if up else 1, x, t, lp)
    assert _raw(eng, good) is None
    st = P.rbm_state(l, LR, WEIGHT_DECAY, MOM)
    want = U.delta_step(st, "up" if up else "down", x.cpu().numpy(), t.cpu().numpy(), LR, MOM)
    _lp_close(lp, want, l, f"after {what}")
    _check6(r, st, f"after {what}")


# ---- 7. model -----------------------------------------------------------------------------------------------------------------------
def _model(c):
    from imdbn.models import iDBN
    sizes = list(c["sizes"])
    net = iDBN(sizes, {"LEARNING_RATE": LR, "WEIGHT_PENALTY": WEIGHT_DECAY, "INIT_MOMENTUM": MOM, "FINAL_MOMENTUM": MOM,
                       "LEARNING_RATE_DYNAMIC": False, "CD": 1}, [], [], torch.device(DEV))
    for r, l in zip(net.layers, c["rec"]):
        r.W.data.copy_(dev(l["W"])); r.vis_bias.data.copy_(dev(l["b"])); r.hid_bias.data.copy_(dev(l["c"]))
        r.W_m.copy_(dev(l["W_m"])); r.hb_m.copy_(dev(l["hb_m"])); r.vb_m.copy_(dev(l["vb_m"]))
    return net


@pytest.mark.parametrize("name", ["odd", "h130"])
def test_idbn_updown_step_is_the_hand_issued_engine_calls(eng, name):
    from imdbn import engine as E
    c = Cs.case(name)
    net, ref = _model(c), _model(c)
    data = dev(c["data"])
    with E.use_rng(_rng(c["seed"])):
        mons = [net.updown_step(data, 0, 1, CD=Cs.CD) for _ in range(Cs.STEPS)]
    gen = ref.untie()
    assert ref.is_untied() and ref.untie() is gen
    for g, r in zip(gen, ref.layers):
        assert g.W.stride(0) == r.W.stride(0) and torch.equal(g.W.data, r.W.data) and torch.equal(g.vis_bias.data, r.vis_bias.data)
        assert g.W.data_ptr() != r.W.data_ptr() and not g.W_m.any() and not g.hb_m.any() and not g.vb_m.any()
    rng = _rng(c["seed"])
    outs = [eng.updown_step(ref.layers, gen, data, [Cs.SCALARS] * len(ref.layers), Cs.CD, None, rng) for _ in range(Cs.STEPS)]
    torch.cuda.synchronize()
    for a, b in zip(net.layers + net.gen_layers, ref.layers + gen):
        assert _same6(_six(a), _six(b))
    for m, o in zip(mons, outs):
        assert set(m) == {"wake_nll", "sleep_nll", "top_loss"} and all(torch.equal(m[k], o[k]) for k in m)
    with E.use_rng(_rng(c["seed"])):
        assert net.updown_step(data, 0, 1, monitor=False) is None


@pytest.mark.parametrize("mode", ["entropy", "logq"])
@pytest.mark.parametrize("name", ["odd", "h130"])
def test_untied_sample_values(eng, name, mode):
    from imdbn import engine as E
    from imdbn.utils import likelihood as LK
    c = Cs.case(name)
    net = _model(c)
    v = dev(c["data"])
    tied = LK.dbn_sample_values(net, v, 0.0, n_samples=2, mode=mode, seed=c["seed"])
    net.untie()
    untied = LK.dbn_sample_values(net, v, 0.0, n_samples=2, mode=mode, seed=c["seed"])
    layers = [(l["W"], l["b"], l["c"]) for l in c["rec"]]
    want, _, mag = Bo.dbn_values(layers, c["data"], 2, mode, PhiloxStream(c["seed"]))
    units, extra = _path_tol(layers, mag)
    _close(untied.cpu().numpy(), tied.cpu().numpy(), units, f"{name} {mode}: untied vs tied", extra)
    _close(untied.cpu().numpy(), want, units, f"{name} {mode}: untied vs the tied twin", extra)
    # after three steps: the twin on the parameters the device now holds
    with E.use_rng(_rng(c["seed"])):
        for _ in range(Cs.STEPS):
            net.updown_step(v, 0, 1, CD=Cs.CD, monitor=False)
    got = LK.dbn_sample_values(net, v, 0.0, n_samples=2, mode=mode, seed=c["seed"] + 1)
    torch.cuda.synchronize()
    import oracle.rbm_oracle as O

    def state(r):
        p = _np6(r)
        return dict(W=p["W"], b=p["vis_bias"], c=p["hid_bias"], groups=[])
    rec = [P.rbm_state(state(r)) for r in net.layers]
    gen = [P.rbm_state(state(r)) for r in net.gen_layers]
    top = rec[-1]
    mags = {}

    def minus_f(s):
        F, m = Bo.free_energy(top.W, top.vis_bias, top.hid_bias, s)
        mags["m"] = m
        return -F
    O.reset_margin()
    want, _ = U.sample_values(rec, gen, minus_f, np.repeat(c["data"], 2, axis=0), mode, PhiloxStream(c["seed"] + 1))
    print(f"{name} {mode}: twin margin on the device's parameters {O.BERNOULLI_MARGIN['min']:.3g}")
    assert O.BERNOULLI_MARGIN["min"] > MARGIN
    layers = [(s.W, s.vis_bias, s.hid_bias) for s in rec]
    units, extra = _path_tol(layers, mags["m"])
    _close(got.cpu().numpy().reshape(-1), want, units, f"{name} {mode}: after three steps", extra)
