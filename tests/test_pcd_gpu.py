"""GPU: imdbn_rbm_pcd_step, imdbn_rbm_pt_sweep and RBM.train_epoch_persistent against the numpy twin (tests/pcd_oracle.py) on the
cases and pinned Philox seeds of tests/pcd_cases.py.

Tolerances.  Samples, exchange decisions and counters are bit-equal: the seeds keep every Bernoulli and categorical decision of the
twin 1e-6 and every exchange decision 8 H 1e-5 clear of a tie (tests/test_pcd_cpu.py asserts that).  The six parameter and
momentum tensors of a PCD update: tests/test_parity_gpu.py's for a CD update, 1e-4 relative (Frobenius), the loss within 5e-7."""
import ctypes as C

import numpy as np
import pytest
import torch

import pcd_cases as Cs
import pcd_oracle as T
from golden_utils import assert_close, rel_fro
from likelihood_gpu import DEV, _native, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)
from oracle.draws import PhiloxStream

pytestmark = pytest.mark.gpu

ALL = list(Cs.CASES)
SIX = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")


def _twin(name):
    c = Cs.case(name)
    return c, twin(("pcd", name), lambda: Cs.twin_run(c, c["seed"]))


def _rbm(c):
    """The case's RBM on the device with its momentum buffers and the cases' weight decay."""
    r = device_rbm(c)
    r.weight_decay = Cs.WEIGHT_DECAY
    r.W_m = torch.zeros_like(r.W.data)
    r.W_m.copy_(dev(c["W_m"]))
    r.hb_m, r.vb_m = dev(c["hb_m"]), dev(c["vb_m"])
    return r


def _params(r):
    return {k: (getattr(r, k).data if k in ("W", "hid_bias", "vis_bias") else getattr(r, k)).cpu().numpy() for k in SIX}


def _rng(seed):
    from imdbn import engine as E
    return E.PhiloxRng(seed)


# ---- 1. pcd_step against the twin -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cd_k", [0, 1, 2])
@pytest.mark.parametrize("name", ALL)
def test_pcd_step_matches_the_twin(eng, name, cd_k):
    c, t = _twin(name)
    st, want_loss, want_v = t["pcd"][cd_k]
    r, p, rng = _rbm(c), dev(c["particles"]), _rng(c["seed"])
    loss = eng.pcd_step(r, dev(c["data"]), p, Cs.LR, Cs.MOM, cd_k, rng)
    torch.cuda.synchronize()
    assert rng.offset == cd_k * (2 + len(c["groups"]))
    flips = int((p.cpu().numpy() != want_v).sum())
    print(f"{name} cd_k {cd_k}: particle elements off the twin {flips}; |loss - twin| {abs(float(loss) - float(want_loss)):.3g}")
    assert flips == 0
    got = _params(r)
    print("   rel-Frobenius vs twin:", ", ".join(f"{k} {rel_fro(got[k], getattr(st, k)):.2e}" for k in SIX))
    for k in SIX:
        assert_close(got[k], getattr(st, k), 1e-4, f"{name} cd_k {cd_k}: {k}", atol=2e-6)
    assert abs(float(loss) - float(want_loss)) < 5e-7
    if cd_k == 0:
        assert torch.equal(p, dev(c["particles"]))


# ---- 2. pt_sweep against the twin -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_pt_sweep_states_and_counters_are_the_twins(eng, name):
    c, t = _twin(name)
    r, x, rng = device_rbm(c), dev(c["state"]), _rng(c["seed"])
    tries, accs = eng.pt_sweep(r, x, c["betas"], Cs.SWEEPS, rng)
    torch.cuda.synchronize()
    assert rng.offset == Cs.SWEEPS * (2 + len(c["groups"]) + (1 if c["R"] >= 2 else 0))
    assert tries.dtype == accs.dtype == torch.int64 and tuple(tries.shape) == (max(c["R"] - 1, 1),)
    print(f"{name}: accepted {accs.tolist()} of {tries.tolist()}; state elements off the twin {int((x.cpu().numpy() != t['state']).sum())}")
    assert np.array_equal(x.cpu().numpy(), t["state"])
    assert tries.tolist() == t["tries"].tolist() and accs.tolist() == t["accs"].tolist()
    # the counters are added to
    eng.pt_sweep(r, dev(c["state"]), c["betas"], Cs.SWEEPS, _rng(c["seed"]), tries, accs)
    assert tries.tolist() == (2 * t["tries"]).tolist() and accs.tolist() == (2 * t["accs"]).tolist()


# ---- 3. one replica is gibbs_step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "groups", "rows67", "wide"])
def test_one_replica_equals_gibbs_step_bit_for_bit(eng, name):
    c = Cs.case(name)
    r, x = device_rbm(c), dev(c["state"])
    rng = _rng(5)
    tries, accs = eng.pt_sweep(r, x, [1.0], 2, rng)
    assert rng.offset == 2 * (2 + len(c["groups"])) and tries.tolist() == [0] and accs.tolist() == [0]
    rng, want = _rng(5), dev(c["state"])
    for _ in range(2):
        want = eng.gibbs_step(r, want, True, True, rng)[0]
    assert torch.equal(x, want)


# ---- 4. determinism -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["groups", "rows67", "wide"])
def test_the_same_call_twice_gives_the_same_bits(eng, name):
    c = Cs.case(name)
    outs = []
    for _ in range(2):
        r, x, p = _rbm(c), dev(c["state"]), dev(c["particles"])
        tries, accs = eng.pt_sweep(r, x, c["betas"], Cs.SWEEPS, _rng(c["seed"]))
        loss = eng.pcd_step(r, dev(c["data"]), p, Cs.LR, Cs.MOM, 2, _rng(c["seed"]))
        outs.append([x, tries, accs, p, loss] + [getattr(r, k).data if hasattr(getattr(r, k), "data") else getattr(r, k) for k in SIX])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---- 5. strided chains ----------------------------------------------------------------------------------------------------
def _padded(a, extra_rows=3, extra_cols=5):
    big = torch.full((a.shape[0] + extra_rows, a.shape[1] + extra_cols), float("nan"), device=DEV)
    big[:a.shape[0], :a.shape[1]] = dev(a)
    return big, big[:a.shape[0], :a.shape[1]]


@pytest.mark.parametrize("name", ["odd", "groups", "wide"])
def test_strided_chains_equal_contiguous_ones_and_padding_is_never_touched(eng, name):
    c, t = _twin(name)
    big, x = _padded(c["state"])
    assert not x.is_contiguous()
    tries, accs = eng.pt_sweep(device_rbm(c), x, c["betas"], Cs.SWEEPS, _rng(c["seed"]))
    assert np.array_equal(x.cpu().numpy(), t["state"]) and accs.tolist() == t["accs"].tolist()
    assert torch.isnan(big[x.shape[0]:]).all() and torch.isnan(big[:, x.shape[1]:]).all()
    bigp, p = _padded(c["particles"])
    bigd, d = _padded(c["data"], 2, 7)
    r = _rbm(c)
    loss = eng.pcd_step(r, d, p, Cs.LR, Cs.MOM, 2, _rng(c["seed"]))
    st, want_loss, want_v = t["pcd"][2]
    assert np.array_equal(p.cpu().numpy(), want_v) and abs(float(loss) - float(want_loss)) < 5e-7
    assert torch.isnan(bigp[p.shape[0]:]).all() and torch.isnan(bigp[:, p.shape[1]:]).all()
    assert torch.isnan(bigd[d.shape[0]:]).all() and torch.isnan(bigd[:, d.shape[1]:]).all()
    assert_close(r.W.data.cpu().numpy(), st.W, 1e-4, f"{name}: W from strided tensors", atol=2e-6)


# ---- 6. rows outside every pair -------------------------------------------------------------------------------------------
def test_rows_outside_every_pair_are_not_touched_by_the_exchange(eng):
    """`odd`, R = 3, one sweep (parity 0): only the pair (0, 1) exchanges.  Replica 2 makes its Gibbs step (its draws are keyed on
    its rows) and nothing else: its rows come out the same whatever the other two replicas hold, and equal that Gibbs step."""
    c = Cs.case("odd")
    M, r = c["M"], device_rbm(c)
    a, b = dev(c["state"]), dev(c["state"])
    b[:2 * M] = 1.0 - b[:2 * M]
    ta, _ = eng.pt_sweep(r, a, c["betas"], 1, _rng(c["seed"]))
    tb, _ = eng.pt_sweep(r, b, c["betas"], 1, _rng(c["seed"]))
    assert ta.tolist() == tb.tolist() == [M, 0]
    assert torch.equal(a[2 * M:], b[2 * M:]) and not torch.equal(a[:2 * M], b[:2 * M])
    st, ps = T.rbm_state(c), PhiloxStream(c["seed"])
    want = T.pt_sweep(st, c["state"], c["betas"], 1, ps)[0]
    assert np.array_equal(a.cpu().numpy(), want)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------
def _raw(eng, name, args):
    from imdbn.engine import native as Nt
    try:
        eng._call(name, *args)
    except Nt.EngineError as e:
        torch.cuda.synchronize()
        return str(e)
    torch.cuda.synchronize()
    return None


def _pcd_args(eng, r, c, data, p, loss, need_m=True, B=None, ldd=None, ldp=None, cd_k=1, null=(), **fields):
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
    rn, keep = eng._rng(_rng(c["seed"]), R.sched_pcd(d.V, d.H, c["groups"], max(cd_k, 0)), max(B, 1), torch.device(DEV))
    P = lambda t, nm: None if nm in null else C.c_void_p(t.data_ptr())
    return (C.byref(d), P(data, "data"), data.stride(0) if ldd is None else ldd, B, P(p, "particles"), p.stride(0) if ldp is None else ldp,
            None if "opts" in null else C.byref(o), C.byref(rn), P(loss, "loss"), *eng._ws_tail(torch.device(DEV), d.V, d.H, max(B, 1))), (d, o, rn, keep)


PCD_BAD = {
    "null_data": (dict(null=("data",)), "null data"), "null_particles": (dict(null=("particles",)), "null particles"),
    "null_opts": (dict(null=("opts",)), "null opts"), "ldd": (dict(ldd=36), "ldd 36"), "ldp": (dict(ldp=35), "ldp 35"),
    "B0": (dict(B=0), "B = 0"), "cd_k": (dict(cd_k=-1), "cd_k = -1"), "momentum": (dict(need_m=False), "null momentum buffer"),
    "data_slot": (dict(data_slot=1), "data_slot 1"), "next_slot": (dict(next_slot=2), "next_slot 2"), "fwd_out": (dict(fwd_out=64), "fwd_out 0x40"),
}


@pytest.mark.parametrize("what", list(PCD_BAD))
def test_pcd_step_invalid_arguments_touch_nothing(eng, what):
    c = Cs.case("odd")
    r, data = _rbm(c), dev(c["data"])
    before = {k: v.copy() for k, v in _params(r).items()}
    p, loss = torch.full((c["M"], c["V"]), -7.25, device=DEV), torch.full((1,), -7.25, device=DEV)
    kw, needle = PCD_BAD[what]
    args, keep = _pcd_args(eng, r, c, data, p, loss, **kw)
    msg = _raw(eng, "imdbn_rbm_pcd_step", args)
    print(what, "->", msg)
    assert msg is not None and "rc=-1)" in msg and needle in msg
    assert (p == -7.25).all() and (loss == -7.25).all() and all(np.array_equal(v, before[k]) for k, v in _params(r).items())
    # a good call follows on the same workspace
    p = dev(c["particles"])
    args, keep = _pcd_args(eng, r, c, data, p, loss)
    assert _raw(eng, "imdbn_rbm_pcd_step", args) is None
    t = _twin("odd")[1]["pcd"][1]
    assert np.array_equal(p.cpu().numpy(), t[2]) and abs(float(loss) - float(t[1])) < 5e-7


def _pt_args(eng, r, c, x, tries, accs, R=None, M=None, lds=None, n=Cs.SWEEPS, betas=None, null=()):
    from imdbn.engine import rng as Rg
    d = eng._desc(r, False)
    R = c["R"] if R is None else R
    M = c["M"] if M is None else M
    b = list(c["betas"]) if betas is None else betas
    arr = (C.c_float * max(len(b), 1))(*b)
    rn, keep = eng._rng(_rng(c["seed"]), Rg.sched_pt(d.V, d.H, c["groups"], c["R"], max(n, 0)), c["R"] * c["M"], torch.device(DEV))
    P = lambda t, nm: None if nm in null else C.c_void_p(t.data_ptr())
    return (C.byref(d), P(x, "state"), x.stride(0) if lds is None else lds, R, M, None if "betas" in null else arr, n,
            None if "rng" in null else C.byref(rn), P(tries, "swap_try"), P(accs, "swap_acc"),
            *eng._ws_tail(torch.device(DEV), d.V, d.H, c["R"] * c["M"])), (d, arr, rn, keep)


PT_BAD = {
    "null_state": (dict(null=("state",)), "null state"), "null_betas": (dict(null=("betas",)), "null betas"), "null_rng": (dict(null=("rng",)), "null rng"),
    "null_try": (dict(null=("swap_try",)), "null swap_try"), "null_acc": (dict(null=("swap_acc",)), "null swap_acc"),
    "lds": (dict(lds=36), "lds 36"), "R0": (dict(R=0), "R = 0"), "M0": (dict(M=0), "M = 0"), "sweeps": (dict(n=-2), "n_sweeps = -2"),
    "beta0": (dict(betas=[0.0, 0.7, 1.0]), "betas[0] = 0"), "beta_last": (dict(betas=[0.4, 0.7, 0.9]), "betas[2] = 0.9"),
    "beta_order": (dict(betas=[0.4, 0.4, 1.0]), "betas[1] = 0.4 is not above"),
}


@pytest.mark.parametrize("what", list(PT_BAD))
def test_pt_sweep_invalid_arguments_touch_nothing(eng, what):
    c, t = _twin("odd")
    r = device_rbm(c)
    x = torch.full((c["R"] * c["M"], c["V"]), -7.25, device=DEV)
    tries, accs = torch.full((2,), -7, dtype=torch.int64, device=DEV), torch.full((2,), -7, dtype=torch.int64, device=DEV)
    kw, needle = PT_BAD[what]
    args, keep = _pt_args(eng, r, c, x, tries, accs, **kw)
    msg = _raw(eng, "imdbn_rbm_pt_sweep", args)
    print(what, "->", msg)
    assert msg is not None and "rc=-1)" in msg and needle in msg
    assert (x == -7.25).all() and (tries == -7).all() and (accs == -7).all()
    x, tries, accs = dev(c["state"]), torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    args, keep = _pt_args(eng, r, c, x, tries, accs)
    assert _raw(eng, "imdbn_rbm_pt_sweep", args) is None
    assert np.array_equal(x.cpu().numpy(), t["state"]) and accs.tolist() == t["accs"].tolist()


def test_wrapper_refuses_tensors_it_would_have_to_copy(eng):
    from imdbn import engine as E
    c = Cs.case("odd")
    r = _rbm(c)
    with pytest.raises(E.EngineError):
        eng.pt_sweep(r, dev(c["state"]).double(), c["betas"], 1, _rng(1))
    with pytest.raises(E.EngineError):
        eng.pt_sweep(r, dev(c["state"])[:-1], c["betas"], 1, _rng(1))          # rows do not divide into replicas
    with pytest.raises(E.EngineError):
        eng.pcd_step(r, dev(c["data"]), dev(c["particles"])[:, :-1], Cs.LR, Cs.MOM, 1, _rng(1))


# ---- 8. no loss, no reconstruction ----------------------------------------------------------------------------------------
def test_null_loss_out_launches_no_reconstruction(eng):
    c, t = _twin("odd")
    r, data = _rbm(c), dev(c["data"])
    eng.prop_down(r, dev(c["state"][:, :c["H"]]), T=2.0)                  # leaves a down record the reconstruction would replace
    before = eng.last_route()
    assert before["down"] is not None and before["down_epilogue"] == "general"
    p = dev(c["particles"])
    assert eng.pcd_step(r, data, p, Cs.LR, Cs.MOM, 0, _rng(c["seed"]), monitor=False) is None
    after = eng.last_route()
    assert {k: after[k] for k in ("down", "down_epilogue", "finish_groups")} == {k: before[k] for k in ("down", "down_epilogue", "finish_groups")}
    st = t["pcd"][0][0]
    got = _params(r)
    for k in SIX:                                                       # and the update is the monitored one
        assert_close(got[k], getattr(st, k), 1e-4, f"unmonitored: {k}", atol=2e-6)
    eng.pcd_step(r, data, p, Cs.LR, Cs.MOM, 0, _rng(c["seed"]))
    assert eng.last_route()["down_epilogue"] == "lean"                     # the reconstruction at T = 1 ran


# ---- 9. RBM.train_epoch_persistent ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tempered", [("groups", False), ("groups", True), ("wide", True)])
def test_train_epoch_persistent_equals_the_hand_issued_calls(eng, name, tempered):
    from imdbn import engine as E
    c = Cs.case(name)
    betas = [float(b) for b in c["betas"]] if tempered else None
    Rn, M, V = (c["R"] if tempered else 1), c["M"], c["V"]
    data = dev(c["data"])
    r = _rbm(c)
    E.manual_seed(c["seed"])
    try:
        losses = [r.train_epoch_persistent(data, ep, 10, CD=2, betas=betas) for ep in (0, 7)]
        short = r.train_epoch_persistent(data[:2], 7, 10, CD=1, betas=betas, monitor=False)
        rates = r.pt_swap_rates()
    finally:
        E.set_rng(None)
    assert short is None and tuple(r._pcd.shape) == (Rn * M, V)
    # by hand, on the same draws
    h, rng = _rbm(c), _rng(c["seed"])
    chains = torch.cat([eng.sample_visible(h, data, rng) for _ in range(Rn)], 0)
    tries = accs = None
    want = []
    for ep in (0, 7):
        lr, mom = h._lr_mom(ep)
        if tempered:
            tries, accs = eng.pt_sweep(h, chains, betas, 2, rng, tries, accs)
            want.append(eng.pcd_step(h, data, chains[(Rn - 1) * M:], lr, mom, 0, rng))
        else:
            want.append(eng.pcd_step(h, data, chains, lr, mom, 2, rng))
    lr, mom = h._lr_mom(7)
    if tempered:
        part = chains.view(Rn, M, V)[:, :2].reshape(Rn * 2, V)
        tries, accs = eng.pt_sweep(h, part, betas, 1, rng, tries, accs)
        chains.view(Rn, M, V)[:, :2] = part.view(Rn, 2, V)
        eng.pcd_step(h, data[:2], chains[(Rn - 1) * M:(Rn - 1) * M + 2], lr, mom, 0, rng, monitor=False)
    else:
        eng.pcd_step(h, data[:2], chains[:2], lr, mom, 1, rng, monitor=False)
    torch.cuda.synchronize()
    assert torch.equal(r._pcd, chains) and all(torch.equal(a, b) for a, b in zip(losses, want))
    for k in SIX:
        a, b = getattr(r, k), getattr(h, k)
        assert torch.equal(a.data if hasattr(a, "data") else a, b.data if hasattr(b, "data") else b), k
    if tempered:
        assert torch.equal(r._pt_try, tries) and torch.equal(r._pt_acc, accs)
        assert np.allclose(rates.numpy(), (accs.double() / tries.double()).cpu().numpy(), equal_nan=True)
    else:
        assert rates is None
