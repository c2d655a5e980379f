"""GPU: imdbn_rbm_centered_step and RBM.train_epoch_centered against the numpy twin (tests/centered_oracle.py) on the cases and
pinned Philox seeds of tests/centered_cases.py.

Tolerances.  Particles are bit-equal: the seeds keep every Bernoulli and categorical decision of the twin 1e-6 clear of a tie
(tests/test_centered_cpu.py asserts that).  The six parameter and momentum tensors: tests/test_pcd_gpu.py's for an update, 1e-4
relative (Frobenius) with atol 2e-6, the loss within 5e-7.  The new offsets: 1e-6 absolute -- fp32 sums of at most 134 values in
[0, 1] divided by the row count, then a convex combination with an offset in (0, 1)."""
import ctypes as C

import numpy as np
import pytest
import torch

import centered_cases as Cc
import pcd_cases as Cs
from golden_utils import assert_close, rel_fro
from likelihood_gpu import DEV, _native, close, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

ALL = list(Cs.CASES)
SIX = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")
KINDS = [("cd", Cc.CD_K)] + [("pcd", k) for k in Cc.PCD_KS]
KIND_IDS = [f"{k}{n}" for k, n in KINDS]


def _twin(c, kind, k, mode):
    return twin(("centered", c["name"], kind, k, mode), lambda: Cc.twin_run(c, kind, k, mode))


def _rbm(c, pitch=None):
    """The case's RBM on the device with its momentum buffers, the cases' weight decay and its sparsity setting; `pitch`: W and W_m
    as views of NaN-filled [V, pitch] buffers."""
    r = device_rbm(c)
    r.weight_decay, r.sparsity, r.sparsity_factor = Cs.WEIGHT_DECAY, c["sparsity"], Cc.SPARSITY_TARGET
    if pitch is None:
        r.W_m = torch.zeros_like(r.W.data)
    else:
        r.W.data = torch.full((c["V"], pitch), float("nan"), device=DEV)[:, :c["H"]]
        r.W.data.copy_(dev(c["W"]))
        r.W_m = torch.full((c["V"], pitch), float("nan"), device=DEV)[:, :c["H"]]
    r.W_m.copy_(dev(c["W_m"]))
    r.hb_m, r.vb_m = dev(c["hb_m"]), dev(c["vb_m"])
    return r


def _t(r, k):
    x = getattr(r, k)
    return x.data if k in SIX[:3] else x


def _params(r):
    return {k: _t(r, k).cpu().numpy() for k in SIX}


def _rng(seed):
    from imdbn import engine as E
    return E.PhiloxRng(seed)


def _step(eng, c, kind, k, mode, r=None, data=None, p=None, mu=None, lam=None, slide=None, **kw):
    """One centered step of the case on the device: (rbm, particles or None, mu, lam, loss, rng)."""
    r = _rbm(c) if r is None else r
    data = dev(c["data"]) if data is None else data
    p = (None if kind == "cd" else dev(c["particles"])) if p is None else p
    mu, lam = dev(c["mu"]) if mu is None else mu, dev(c["lam"]) if lam is None else lam
    rng = _rng(Cc.seed_of(c, kind))
    loss = eng.centered_step(r, data, p, Cs.LR, Cs.MOM, k, rng, mu, lam, c["slide"] if slide is None else slide, mode, **kw)
    torch.cuda.synchronize()
    return r, p, mu, lam, loss, rng


def _check(c, t, got, what):
    r, p, mu, lam, loss, rng = got
    assert rng.offset == t["offset"]
    if t["v"] is not None:
        flips = int((p.cpu().numpy() != t["v"]).sum())
        print(f"{what}: particle elements off the twin {flips}")
        assert flips == 0
    have = _params(r)
    print(f"{what}: rel-Frobenius vs twin:", ", ".join(f"{k} {rel_fro(have[k], getattr(t['st'], k)):.2e}" for k in SIX),
          f"; |loss - twin| {abs(float(loss) - float(t['loss'])):.3g}")
    close(mu.cpu().numpy(), t["mu"], 1e-6, f"{what}: mu'")
    close(lam.cpu().numpy(), t["lam"], 1e-6, f"{what}: lam'")
    for k in SIX:
        assert_close(have[k], getattr(t["st"], k), 1e-4, f"{what}: {k}", atol=2e-6)
    assert abs(float(loss) - float(t["loss"])) < 5e-7


# ---- 1. against the twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind,k", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", ALL)
def test_centered_step_matches_the_twin(eng, name, kind, k, mode):
    c = Cc.case(name)
    got = _step(eng, c, kind, k, mode)
    _check(c, _twin(c, kind, k, mode), got, f"{name} {kind}-{k} mode {mode}")
    if kind == "pcd" and k == 0:
        assert torch.equal(got[1], dev(c["particles"]))


# ---- 2. zero offsets without slide: the engine's own plain updates ---------------------------------------------------------------
@pytest.mark.parametrize("kind,k", [("cd", 1), ("pcd", 0), ("pcd", 2)], ids=["cd1", "pcd0", "pcd2"])
@pytest.mark.parametrize("name", ALL)
def test_zero_offsets_without_slide_equal_the_plain_step_from_the_same_state(eng, name, kind, k):
    c = Cc.case(name)
    z = lambda n: torch.zeros(n, device=DEV)
    r, p, mu, lam, loss, rng = _step(eng, c, kind, k, 0, mu=z(c["V"]), lam=z(c["H"]), slide=0.0)
    h, hp, hrng = _rbm(c), dev(c["particles"]), _rng(Cc.seed_of(c, kind))
    if kind == "cd":
        want = eng.cd_step(h, dev(c["data"]), Cs.LR, Cs.MOM, k, hrng)
    else:
        want = eng.pcd_step(h, dev(c["data"]), hp, Cs.LR, Cs.MOM, k, hrng)
        assert torch.equal(p, hp)
    torch.cuda.synchronize()
    assert rng.offset == hrng.offset and not mu.any() and not lam.any()
    a, b = _params(r), _params(h)
    print(f"{name} {kind}-{k}: rel-Frobenius vs the plain step:", ", ".join(f"{q} {rel_fro(a[q], b[q]):.2e}" for q in SIX))
    for q in SIX:
        assert_close(a[q], b[q], 1e-4, f"{name} {kind}-{k}: {q}", atol=2e-6)
    assert abs(float(loss) - float(want)) < 5e-7


# ---- 3. determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "groups", "rows67", "wide"])
def test_the_same_call_twice_gives_the_same_bits(eng, name):
    c = Cc.case(name)
    outs = []
    for _ in range(2):
        o = []
        for kind, k in (("cd", 1), ("pcd", 2)):
            r, p, mu, lam, loss, _ = _step(eng, c, kind, k, 1)
            o += [mu, lam, loss] + ([] if p is None else [p]) + [_t(r, q) for q in SIX]
        outs.append(o)
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---- 4. layout ------------------------------------------------------------------------------------------------------------------------
def _padded(a, extra_rows=3, extra_cols=5):
    big = torch.full((a.shape[0] + extra_rows, a.shape[1] + extra_cols), float("nan"), device=DEV)
    big[:a.shape[0], :a.shape[1]] = dev(a)
    return big, big[:a.shape[0], :a.shape[1]]


@pytest.mark.parametrize("name,pitch", [("odd", 41), ("groups", 48), ("wide", 104)])
def test_strided_tensors_and_padded_weight_rows_give_the_contiguous_results_and_padding_stays_nan(eng, name, pitch):
    c = Cc.case(name)
    for kind, k in (("cd", 1), ("pcd", 2)):
        ref = _step(eng, c, kind, k, 0)
        bigd, d = _padded(c["data"], 2, 7)
        bigp, p = _padded(c["particles"]) if kind == "pcd" else (None, None)
        r = _rbm(c, pitch)
        assert r.W.data.stride(0) == pitch == r.W_m.stride(0) and not d.is_contiguous()
        got = _step(eng, c, kind, k, 0, r=r, data=d, p=p)
        assert r.W.data.stride(0) == pitch == r.W_m.stride(0)            # the engine took the buffers as they are
        _check(c, _twin(c, kind, k, 0), got, f"{name} {kind}-{k} strided")
        for q in SIX:
            assert torch.equal(_t(got[0], q), _t(ref[0], q)), q
        assert torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3]) and torch.equal(got[4], ref[4])
        assert torch.isnan(bigd[d.shape[0]:]).all() and torch.isnan(bigd[:, d.shape[1]:]).all()
        if p is not None:
            assert torch.equal(p, ref[1]) and torch.isnan(bigp[p.shape[0]:]).all() and torch.isnan(bigp[:, p.shape[1]:]).all()
        for q in ("W", "W_m"):
            full = torch.as_strided(_t(r, q), (c["V"], pitch), (pitch, 1))
            assert torch.isnan(full[:, c["H"]:]).all() and not torch.isnan(full[:, :c["H"]]).any(), q


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------
def _raw(eng, args):
    from imdbn.engine import native as Nt
    try:
        eng._call("imdbn_rbm_centered_step", *args)
    except Nt.EngineError as e:
        torch.cuda.synchronize()
        return str(e)
    torch.cuda.synchronize()
    return None


def _args(eng, r, c, data, p, mu, lam, loss, scratch, need_m=True, B=None, ldd=None, ldp=None, cd_k=1, slide=0.01, mode=0, null=(), **fields):
    from imdbn.engine import native as Nt
    from imdbn.engine import rng as R
    d = eng._desc(r, True)
    if not need_m:
        d = Nt.RbmDesc.from_buffer_copy(d)
        d.hb_m = None
    o = eng._opts(r, Cs.LR, Cs.MOM, cd_k)
    for k, v in fields.items():
        setattr(o, k, v)
    B = data.size(0) if B is None else B
    sched = R.sched_pcd(d.V, d.H, c["groups"], max(cd_k, 0)) if p is not None else R.sched_cd(d.V, d.H, c["groups"], max(cd_k, 1))
    rn, keep = eng._rng(_rng(Cc.seed_of(c, "cd" if p is None else "pcd")), sched, max(B, 1), torch.device(DEV))
    P = lambda t, nm: None if (nm in null or t is None) else C.c_void_p(t.data_ptr())
    return (C.byref(d), P(data, "data"), data.stride(0) if ldd is None else ldd, B, P(p, "particles"),
            (0 if p is None else p.stride(0)) if ldp is None else ldp, None if "opts" in null else C.byref(o),
            None if "rng" in null else C.byref(rn), P(mu, "mu"), P(lam, "lam"), slide, mode, P(loss, "loss"), P(scratch, "scratch"),
            *eng._ws_tail(torch.device(DEV), d.V, d.H, max(B, 1))), (d, o, rn, keep)


# what -> (keywords of _args, with particles?, needle of the message)
BAD = {
    "momentum": (dict(need_m=False), True, "null momentum buffer"),
    "null_data": (dict(null=("data",)), True, "null data"), "null_opts": (dict(null=("opts",)), True, "null opts"),
    "null_mu": (dict(null=("mu",)), False, "null mu"), "null_lam": (dict(null=("lam",)), True, "null lam"),
    "null_scratch": (dict(null=("scratch",)), False, "null scratch"),
    "ldd": (dict(ldd=36), False, "ldd 36"), "ldp": (dict(ldp=35), True, "ldp 35"), "B0": (dict(B=0), True, "B = 0"),
    "cd_k0_from_data": (dict(cd_k=0), False, "cd_k = 0"), "cd_k_negative": (dict(cd_k=-1), True, "cd_k = -1"),
    "null_rng_cd": (dict(null=("rng",)), False, "null rng"), "null_rng_pcd": (dict(null=("rng",), cd_k=2), True, "null rng with cd_k = 2"),
    "slide_high": (dict(slide=1.5), True, "slide = 1.5"), "slide_negative": (dict(slide=-0.25), False, "slide = -0.25"),
    "slide_nan": (dict(slide=float("nan")), True, "slide = nan"),
    "mode2": (dict(mode=2), False, "mode = 2"), "mode_negative": (dict(mode=-1), True, "mode = -1"),
    "data_slot": (dict(data_slot=1), True, "data_slot 1"), "next_slot": (dict(next_slot=2), False, "next_slot 2"),
    "next_binary": (dict(next_binary=1), True, "next_binary 1"), "fwd_out": (dict(fwd_out=64), False, "fwd_out 0x40"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_invalid_arguments_touch_nothing_and_a_good_call_follows(eng, what):
    c = Cc.case("odd")
    kw, chains, needle = BAD[what]
    r, data = _rbm(c), dev(c["data"])
    before = {k: v.copy() for k, v in _params(r).items()}
    S = lambda *shape: torch.full(shape, -7.25, device=DEV)
    p, mu, lam, loss = (S(c["M"], c["V"]) if chains else None), S(c["V"]), S(c["H"]), S(1)
    scratch = S(int(eng._lib.imdbn_centered_scratch_floats(c["V"], c["H"])))
    args, keep = _args(eng, r, c, data, p, mu, lam, loss, scratch, **kw)
    msg = _raw(eng, args)
    print(what, "->", msg)
    assert msg is not None and "rc=-1)" in msg and needle in msg
    assert (mu == -7.25).all() and (lam == -7.25).all() and (loss == -7.25).all() and (scratch == -7.25).all()
    assert (p is None or (p == -7.25).all()) and all(np.array_equal(v, before[k]) for k, v in _params(r).items())
    # a good call follows on the same workspace and scratch
    kind = "pcd" if chains else "cd"
    p, mu, lam = (dev(c["particles"]) if chains else None), dev(c["mu"]), dev(c["lam"])
    args, keep = _args(eng, r, c, data, p, mu, lam, loss, scratch, slide=c["slide"])
    assert _raw(eng, args) is None
    _check(c, _twin(c, kind, 1, 0), (r, p, mu, lam, loss, _Off(_twin(c, kind, 1, 0)["offset"])), f"after {what}")


class _Off:
    def __init__(self, offset):
        self.offset = offset


def test_a_replay_tape_that_is_too_short_is_an_rng_error_and_touches_nothing(eng):
    from imdbn.engine import native as Nt
    c = Cc.case("odd")
    r, data = _rbm(c), dev(c["data"])
    before = _params(r)
    S = lambda *shape: torch.full(shape, -7.25, device=DEV)
    p, mu, lam, loss = S(c["M"], c["V"]), S(c["V"]), S(c["H"]), S(1)
    scratch = S(int(eng._lib.imdbn_centered_scratch_floats(c["V"], c["H"])))
    args, keep = _args(eng, r, c, data, p, mu, lam, loss, scratch, cd_k=1)
    tape = torch.rand(c["M"] * (c["V"] + c["H"]) - 1, device=DEV)
    rn = keep[2]
    rn.mode, rn.tape, rn.tape_len = Nt.RNG_REPLAY, tape.data_ptr(), tape.numel()
    msg = _raw(eng, args)
    print(msg)
    assert msg is not None and "replay tape" in msg and "rc=-3)" in msg
    assert (p == -7.25).all() and (mu == -7.25).all() and (scratch == -7.25).all() and all(np.array_equal(v, before[k]) for k, v in _params(r).items())


def test_wrapper_refuses_tensors_it_would_have_to_copy(eng):
    from imdbn import engine as E
    c = Cc.case("odd")
    r, data, rng = _rbm(c), dev(c["data"]), _rng(1)
    mu, lam = dev(c["mu"]), dev(c["lam"])
    for bad in (dict(mu=mu.double()), dict(lam=lam[:-1]), dict(mu=torch.stack([mu, mu], 1)[:, 0]), dict(lam=lam.cpu()),
                dict(p=dev(c["particles"])[:, :-1]), dict(p=dev(c["particles"])[:-1]), dict(p=dev(c["particles"]).double())):
        kw = dict(dict(mu=mu, lam=lam, p=None), **bad)
        with pytest.raises(E.EngineError):
            eng.centered_step(r, data, kw["p"], Cs.LR, Cs.MOM, 1, rng, kw["mu"], kw["lam"], 0.01, 0)
    assert rng.offset == 0 and torch.equal(mu, dev(c["mu"]))


def test_null_loss_out_launches_no_reconstruction(eng):
    c = Cc.case("odd")
    r = _rbm(c)
    eng.prop_down(r, dev(c["state"][:, :c["H"]]), T=2.0)                  # leaves a down record the reconstruction would replace
    before = eng.last_route()
    got = _step(eng, c, "pcd", 0, 0, r=r, monitor=False)
    after = eng.last_route()
    assert got[4] is None and {k: after[k] for k in ("down", "down_epilogue")} == {k: before[k] for k in ("down", "down_epilogue")}
    t = _twin(c, "pcd", 0, 0)
    for k in SIX:
        assert_close(_params(r)[k], getattr(t["st"], k), 1e-4, f"unmonitored: {k}", atol=2e-6)
    close(got[2].cpu().numpy(), t["mu"], 1e-6, "unmonitored: mu'")


# ---- 6. RBM.train_epoch_centered ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,route", [("groups", "cd"), ("groups", "pcd"), ("groups", "tempered"), ("wide", "tempered"), ("odd", "pcd")])
def test_train_epoch_centered_equals_the_hand_issued_calls(eng, name, route):
    from imdbn import engine as E
    c = Cc.case(name)
    betas = [float(b) for b in c["betas"]] if route == "tempered" else None
    Rn, M, V, H = (c["R"] if betas else 1), c["M"], c["V"], c["H"]
    data = dev(c["data"])
    kw = dict(persistent=route != "cd", betas=betas, offsets="enhanced", slide=0.05)
    r = _rbm(c)
    E.manual_seed(c["seed"])
    try:
        losses = [r.train_epoch_centered(data, ep, 10, CD=2, **kw) for ep in (0, 7)]
        short = r.train_epoch_centered(data[:2], 7, 10, CD=1, monitor=False, **kw)
    finally:
        E.set_rng(None)
    assert short is None
    mu, lam = r.centering_offsets()
    # by hand, on the same draws
    h, rng = _rbm(c), _rng(c["seed"])
    hm, hl = torch.zeros(V, device=DEV), torch.zeros(H, device=DEV)
    chains = None if route == "cd" else torch.cat([eng.sample_visible(h, data, rng) for _ in range(Rn)], 0)
    tries = accs = None
    want = []
    for ep, slide in ((0, 1.0), (7, 0.05)):
        lr, mom = h._lr_mom(ep)
        if betas:
            tries, accs = eng.pt_sweep(h, chains, betas, 2, rng, tries, accs)
            want.append(eng.centered_step(h, data, chains[(Rn - 1) * M:], lr, mom, 0, rng, hm, hl, slide, 1))
        else:
            want.append(eng.centered_step(h, data, chains, lr, mom, 2, rng, hm, hl, slide, 1))
    lr, mom = h._lr_mom(7)
    if betas:
        part = chains.view(Rn, M, V)[:, :2].reshape(Rn * 2, V)
        tries, accs = eng.pt_sweep(h, part, betas, 1, rng, tries, accs)
        chains.view(Rn, M, V)[:, :2] = part.view(Rn, 2, V)
        eng.centered_step(h, data[:2], chains[(Rn - 1) * M:(Rn - 1) * M + 2], lr, mom, 0, rng, hm, hl, 0.05, 1, monitor=False)
    else:
        eng.centered_step(h, data[:2], None if chains is None else chains[:2], lr, mom, 1, rng, hm, hl, 0.05, 1, monitor=False)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(losses, want)) and torch.equal(mu, hm) and torch.equal(lam, hl)
    for k in SIX:
        assert torch.equal(_t(r, k), _t(h, k)), k
    if route == "cd":
        assert "_pcd" not in r.__dict__
    else:
        assert torch.equal(r._pcd, chains)
    if betas:
        assert torch.equal(r._pt_try, tries) and torch.equal(r._pt_acc, accs)
