"""GPU: imdbn_dbm_group_layer, HipEngine.mdbm_infer / mdbm_gibbs / mdbm_step and imdbn.models.mdbm against the float64 reference and the
fp32 twin of tests/mdbm_oracle.py on the cases of tests/mdbm_cases.py.

Bounds (derived in mdbm_oracle's docstring, none tuned).  Mean field: the softmax bound ``dp`` built on ``dpre <= (K + 24) u T``, then
``(1 - damp) dp + EPS_D`` for m and ``max (dp) + u`` for res; carried through the start and the sweeps by ``infer_bounded``.  Picks:
exactly the float64 pick under Philox -- the seeds of mdbm_cases leave every pick more room than ``pick_bound`` (asserted on the CPU) --
and exactly the tape's index under replay.  mdbm_step: relative Frobenius error against float64, STEP_FACTOR times the fp32 twin's own
error per quantity, capped at 1e-4, as tests/test_dbm_gpu.py (the factor is DESIGN section 40's measured 4.0; the ratio seen here is
printed and recorded in section 42)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dbm_oracle as Dt
import mdbm_cases as Ck
import mdbm_oracle as Mt
import oracle.rbm_oracle as O
from imdbn.engine import native as N
from imdbn.engine import rng as R
from likelihood_gpu import DEV, _native, dev, eng, twin  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NAN = float("nan")
STEP_FACTOR = 4.0
E_INVALID, E_WORKSPACE, E_RNG = -1, -2, -3          # IMDBN_E_* of include/imdbn_engine.h


def _block(a, rows_above=0, rows_below=0, left=0, right=0):
    """`a` as a row / column block of a NaN-filled buffer.  (view, buffer)"""
    r, c = a.shape
    buf = torch.full((rows_above + r + rows_below, left + c + right), NAN, device=DEV)
    view = buf[rows_above:rows_above + r, left:left + c]
    view.copy_(dev(a))
    return view, buf


def _intact(view, buf):
    """Everything of `buf` outside `view` is still NaN."""
    mask = torch.ones_like(buf, dtype=torch.bool)
    r0 = (view.data_ptr() - buf.data_ptr()) // 4 // buf.stride(0)
    c0 = (view.data_ptr() - buf.data_ptr()) // 4 % buf.stride(0)
    mask[r0:r0 + view.size(0), c0:c0 + view.size(1)] = False
    return bool(torch.isnan(buf[mask]).all())


def _layer_on_device(k):
    """(lo, hi, x_lo, x_hi, bias, [(view, buffer)]): W_hi a ROW BLOCK of a taller, wider NaN-filled matrix (pitch above K_hi), W_lo with a
    pitch above N, strided x rows; all padding NaN."""
    bufs = []
    lo = hi = xl = xh = None
    if k["W_lo"] is not None:
        lo, b = _block(k["W_lo"], 0, 0, 0, 5)
        xl, bx = _block(k["x_lo"], 0, 0, 1, 2)
        bufs += [(lo, b), (xl, bx)]
    if k["W_hi"] is not None:
        hi, b = _block(k["W_hi"], 3, 2, 0, 7)
        xh, bx = _block(k["x_hi"], 0, 0, 2, 4)
        bufs += [(hi, b), (xh, bx)]
    return lo, hi, xl, xh, dev(k["bias"]), bufs


def _reference(k, binary=False):
    """(groups, float64 p, its bound dp) of a group case, once per case."""
    def compute():
        G = Mt.ends_to_groups(k["ends"])
        x = Dt.pre(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"], F64)
        p = Mt.softmax(x, G, F64)
        return G, p, Mt.softmax_bound(x, p, G, Dt.pre_bound(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"]))
    return twin(("group", k["ends"], k["K_lo"], k["K_hi"], k["B"], binary), compute)


def _garbage_workspace(eng, k):
    """Fill the engine's workspace of this shape with 0xFF bytes (NaN logits, wild counters)."""
    need = int(eng._lib.imdbn_dbm_group_layer_ws_bytes(k["K_lo"], k["K_hi"], k["N"], k["B"]))
    key = ("dbm_group_ws", torch.device(DEV), k["K_lo"], k["K_hi"], k["N"], k["B"], torch.cuda.current_stream(DEV).cuda_stream)
    ws = eng._buffer(key, lambda: torch.empty(max(need, 256), dtype=torch.uint8, device=DEV), need)
    ws.fill_(255)


# ---- the group layer: mean field ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damp", Ck.DAMPS)
@pytest.mark.parametrize("case", Ck.GROUP_CASES, ids=str)
def test_mean_field_stays_inside_the_derived_bound(eng, case, damp):
    k = Ck.group_case(*case)
    lo, hi, xl, xh, bias, bufs = _layer_on_device(k)
    G, p, dp = _reference(k)
    got = []
    for run in range(2):
        m, mb = _block(k["m"], 0, 0, 3, 4)                   # a column block
        if run == 1:
            _garbage_workspace(eng, k)
        res = eng.dbm_group_layer(lo, hi, xl, xh, bias, G, m=m, damp=damp, want_res=True)
        torch.cuda.synchronize()
        assert _intact(m, mb) and all(_intact(v, b) for v, b in bufs), "padding was written"
        got.append((m.cpu().numpy(), res.cpu().numpy()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), "a call on a workspace full of garbage differs"
    want = damp * k["m"].astype(F64) + (1 - damp) * p
    fm = np.abs(got[0][0] - want) / ((1 - damp) * dp + Mt.EPS_D)
    fr = np.abs(got[0][1] - np.abs(p - k["m"]).max(1)) / (dp.max(1) + Mt.U)
    print(f"{case} damp {damp}: largest share of the bound: m {fm.max():.3g}, res {fr.max():.3g} (dp up to {dp.max():.3g})")
    assert fm.max() <= 1.0 and fr.max() <= 1.0
    assert eng.dbm_group_layer(lo, hi, xl, xh, bias, G, m=m, damp=damp) is None


# ---- the group layer: samples --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Ck.GROUP_CASES, ids=str)
def test_philox_picks_are_the_float64_picks(eng, case):
    k = Ck.group_case(*case, binary=True)
    lo, hi, xl, xh, bias, bufs = _layer_on_device(k)
    G, p, dp = _reference(k, True)
    seed = Ck.PICK_SEEDS[case]
    got = []
    for run in range(2):
        s, sb = _block(np.zeros((k["B"], k["N"]), F32), 0, 0, 2, 3)
        prng = R.PhiloxRng(seed)
        pp, ss = eng.dbm_group_layer(lo, hi, xl, xh, bias, G, sample=True, rng=prng, want_p=True, s_out=s)
        torch.cuda.synchronize()
        assert ss is s and prng.offset == len(G) and _intact(s, sb) and all(_intact(v, b) for v, b in bufs), "padding was written"
        got.append((pp.cpu().numpy(), s.cpu().numpy()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    want = np.zeros((k["B"], k["N"]), F32)
    for g, (a, e) in enumerate(G):
        idx, _, _ = Mt.pick(p[:, a:e], Mt.philox_uniform(seed, g, 0, k["B"]))
        want[:, a:e] = Mt.one_hot(idx, e - a)
    share = (np.abs(got[0][0] - p) / dp).max()
    print(f"{case}: p uses {share:.3g} of its bound; {int((got[0][1] != want).any(1).sum())} rows pick another index")
    assert share <= 1.0 and np.array_equal(got[0][1], want)
    # without want_p the call returns the samples alone, in a fresh tensor
    alone = eng.dbm_group_layer(lo, hi, xl, xh, bias, G, sample=True, rng=R.PhiloxRng(seed))
    assert np.array_equal(alone.cpu().numpy(), want)


class _Indices:
    """A replay provider that hands out given index vectors, one per group."""

    def __init__(self, idx):
        self.idx, self.pos = idx, 0

    def categorical(self, probs):
        self.pos += 1
        return self.idx[self.pos - 1]


@pytest.mark.parametrize("case", Ck.GROUP_CASES, ids=str)
def test_replayed_picks_are_the_tapes_indices(eng, case):
    k = Ck.group_case(*case, binary=True)
    lo, hi, xl, xh, bias, _ = _layer_on_device(k)
    G, p, dp = _reference(k, True)
    g = np.random.default_rng(5)
    idx = [g.integers(0, e - a, k["B"]) for a, e in G]
    pb, buf = _block(np.zeros((k["B"], k["N"]), F32), 0, 0, 1, 6)
    # ldp > N through the C entry, with the native rng struct to read cat_used / draws_used
    tape = dev(np.concatenate(idx).astype(np.int32))
    r = N.Rng()
    r.mode, r.cat_tape, r.cat_len = N.RNG_REPLAY, tape.data_ptr(), tape.numel()
    s = torch.empty(k["B"], k["N"], device=DEV)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    ld = lambda t: 0 if t is None else t.stride(0)
    need = int(eng._lib.imdbn_dbm_group_layer_ws_bytes(k["K_lo"], k["K_hi"], k["N"], k["B"]))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ends = (C.c_int * len(G))(*k["ends"])
    rc = eng._lib.imdbn_dbm_group_layer(ptr(lo), ld(lo), k["K_lo"], ptr(xl), ld(xl), 1.0, ptr(hi), ld(hi), k["K_hi"], ptr(xh), ld(xh), 1.0,
                                        ptr(bias), k["N"], k["B"], 0, len(G), ends, None, 0, 0.0, None, C.byref(r), ptr(s), s.stride(0),
                                        ptr(pb), pb.stride(0), ptr(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and r.draws_used == len(G) and r.cat_used == len(G) * k["B"] and r.tape_used == 0 and _intact(pb, buf)
    want = np.concatenate([Mt.one_hot(i, e - a) for i, (a, e) in zip(idx, G)], 1)
    assert np.array_equal(s.cpu().numpy(), want) and (np.abs(pb.cpu().numpy() - p) <= dp).all()
    s2 = eng.dbm_group_layer(lo, hi, xl, xh, bias, G, sample=True, rng=R.ReplayRng(_Indices(idx)))
    assert torch.equal(s2, s)


# ---- the group layer: every error code ---------------------------------------------------------------------------------------------------
def test_refusals_name_their_code(eng):
    k = Ck.group_case((33, 64), 67, 21, 5)
    lo, hi, xl, xh, bias, _ = _layer_on_device(k)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    m, s = dev(k["m"]), torch.empty(5, 64, device=DEV)
    need = int(eng._lib.imdbn_dbm_group_layer_ws_bytes(67, 21, 64, 5))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    r = N.Rng()
    r.mode, r.seed = N.RNG_PHILOX, 1
    short = dev(np.zeros(9, np.int32))
    rr = N.Rng()
    rr.mode, rr.cat_tape, rr.cat_len = N.RNG_REPLAY, short.data_ptr(), 9            # two groups of five rows need ten
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(K_lo=67, K_hi=21, x_lo=xl, x_hi=xh, W_lo=lo, W_hi=hi, n=64, B=5, ends=(33, 64), G=None, mm=m, ss=None, ldm=64, lds=64, ldw_lo=None,
             ldw_hi=None, ldx_lo=None, b=bias, mode=0, ws_ptr=None, ws_bytes=need, damp=0.0, rng=r, p=None, ldp=0, null_ends=False):
        arr = None if null_ends else (C.c_int * max(len(ends), 1))(*ends)
        return eng._lib.imdbn_dbm_group_layer(ptr(W_lo), lo.stride(0) if ldw_lo is None else ldw_lo, K_lo, ptr(x_lo), xl.stride(0) if ldx_lo is None
                                              else ldx_lo, 1.0, ptr(W_hi), hi.stride(0) if ldw_hi is None else ldw_hi, K_hi, ptr(x_hi), xh.stride(0),
                                              1.0, ptr(b), n, B, mode, len(ends) if G is None else G, arr, ptr(mm), ldm, damp, None,
                                              None if rng is None else C.byref(rng), ptr(ss), lds, ptr(p), ldp,
                                              C.c_void_p(ws.data_ptr() if ws_ptr is None else ws_ptr), ws_bytes, st)

    before = m.clone()
    # imdbn_dbm_layer's refusals, in its order
    assert call(n=0) == E_INVALID and call(B=0) == E_INVALID and call(K_lo=-1) == E_INVALID
    assert call(K_lo=0, K_hi=0) == E_INVALID and call(x_lo=None, x_hi=None) == E_INVALID
    assert call(W_lo=None) == E_INVALID and call(ldw_lo=63) == E_INVALID and call(ldx_lo=66) == E_INVALID
    assert call(W_hi=None) == E_INVALID and call(ldw_hi=20) == E_INVALID
    assert call(b=None) == E_INVALID and call(mode=2) == E_INVALID
    assert call(mm=m, ss=s) == E_INVALID and call(mm=None, ss=None) == E_INVALID
    assert call(ldm=63) == E_INVALID and call(damp=1.0) == E_INVALID and call(damp=NAN) == E_INVALID
    assert call(mm=None, ss=s, lds=63) == E_INVALID and call(mm=None, ss=s, p=s, ldp=63) == E_INVALID
    assert call(mm=None, ss=s, rng=None) == E_INVALID
    assert call(mm=None, ss=s, rng=rr) == E_RNG
    assert call(ws_ptr=0) == E_WORKSPACE and call(ws_ptr=ws.data_ptr() + 4) == E_INVALID and call(ws_bytes=need - 1) == E_WORKSPACE
    # the groups
    assert call(G=0) == E_INVALID and call(ends=(10, 20, 30, 40, 64), G=5) == E_INVALID and call(null_ends=True) == E_INVALID
    assert call(ends=(33, 63)) == E_INVALID and call(ends=(33, 65)) == E_INVALID          # do not tile [0, N)
    assert call(ends=(63, 64)) == E_INVALID and call(ends=(0, 64)) == E_INVALID and call(ends=(40, 33, 64)) == E_INVALID      # widths 1, 0, < 0
    assert call(K_lo=0, x_lo=None, n=300, ends=(300,), ldm=300) == E_INVALID                                # wider than 256
    assert eng._lib.imdbn_dbm_group_layer_ws_bytes(0, 0, 64, 5) == 0 and eng._lib.imdbn_dbm_group_layer_ws_bytes(67, 21, 0, 5) == 0
    torch.cuda.synchronize()
    assert torch.equal(m, before), "a refused call touched m"
    assert call() == 0
    G = [(0, 33), (33, 64)]
    for bad in ([(0, 33)], [(0, 33), (34, 64)], [(1, 33), (33, 64)], [(0, 10), (10, 20), (20, 30), (30, 40), (40, 64)]):
        with pytest.raises(N.EngineError, match="tile"):
            eng.dbm_group_layer(lo, hi, xl, xh, bias, bad, m=m)
    with pytest.raises(N.EngineError):
        eng.dbm_group_layer(None, None, None, None, bias, G, m=m)
    with pytest.raises(N.EngineError):
        eng.dbm_group_layer(lo, hi, xl, xh, bias, G)
    with pytest.raises(N.EngineError):
        eng.dbm_group_layer(lo, hi, xl, xh, bias, G, m=m.t().contiguous().t())
    torch.cuda.synchronize()


# ---- the compositions ----------------------------------------------------------------------------------------------------------------------
def _stack_on_device(k):
    """(image RBMs, joint RBM, biases) with the constructor's padded pitches."""
    from imdbn.models import RBM
    L, Dz, K = len(k["Ws"]), k["sizes"][-1], k["K"]
    rbms = []
    for l, W in enumerate(list(k["Ws"]) + [k["WJ"]]):
        V, H = W.shape
        r = RBM(V, H, Ck.LR, Ck.WEIGHT_DECAY, Ck.MOM, softmax_groups=[(Dz, Dz + K)] if l == L else None).to(DEV)
        r.W.data.copy_(dev(W))
        r.hid_bias.data.copy_(dev(k["bs"][l + 1]))
        vb = k["bs"][0] if l == 0 else (np.concatenate([np.zeros(Dz, F32), k["bs"][L + 2]]) if l == L else np.zeros(V, F32))
        r.vis_bias.data.copy_(dev(vb))
        r.W_m.zero_()
        r.hb_m, r.vb_m = torch.zeros_like(r.hid_bias.data), torch.zeros_like(r.vis_bias.data)
        rbms.append(r)
    layers, joint = rbms[:L], rbms[L]
    biases = [layers[0].vis_bias.data] + [r.hid_bias.data for r in layers] + [joint.hid_bias.data, joint.vis_bias.data[Dz:]]
    return layers, joint, biases


@pytest.mark.parametrize("free", [False, True], ids=["clamped", "free"])
@pytest.mark.parametrize("case", Ck.STACKS, ids=str)
def test_inference_stays_inside_the_accumulated_bound(eng, case, free):
    k = Ck.stack_case(*case)
    layers, joint, biases = _stack_on_device(k)
    mu, res = eng.mdbm_infer(layers, joint, biases, dev(k["data"]), None if free else dev(k["y"]), 3, damp=0.25)
    torch.cuda.synchronize()
    M = Mt.Model(k["Ws"], k["WJ"], k["bs"])
    want, wres, dmu, rb = twin(("minfer", case, free), lambda: Mt.infer_bounded(M, k["data"], None if free else k["y"], 3, 0.25))
    f = max(float((np.abs(m.cpu().numpy() - w) / np.maximum(d, 2.0 ** -100)).max()) for m, w, d in zip(mu, want, dmu))
    fr = float((np.abs(res.cpu().numpy() - wres) / rb).max())
    print(f"{case} {'free' if free else 'clamped'}: largest share of the bound: mu {f:.3g}, res {fr:.3g}")
    assert f <= 1.0 and fr <= 1.0 and len(mu) == len(k["Ws"]) + 2
    if not free:
        assert np.array_equal(mu[-1].cpu().numpy(), k["y"])


@pytest.mark.parametrize("clamp", [False, True], ids=["free", "clamped"])
@pytest.mark.parametrize("case", Ck.STACKS, ids=str)
def test_gibbs_states_are_the_oracles(eng, case, clamp):
    k = Ck.stack_case(*case)
    layers, joint, biases = _stack_on_device(k)
    parts = [dev(p) for p in k["particles"]]
    tape = Ck.Tape(Ck.GIBBS_SEEDS[case])
    eng.mdbm_gibbs(layers, joint, biases, parts, Ck.GIBBS_SWEEPS, R.ReplayRng(tape), clamp_bottom=dev(k["data"]) if clamp else None,
                   clamp_labels=dev(k["y"]) if clamp else None)
    torch.cuda.synchronize()
    want = Mt.gibbs(Mt.Model(k["Ws"], k["WJ"], k["bs"]), k["particles"], Ck.GIBBS_SWEEPS, Ck.Tape(Ck.GIBBS_SEEDS[case]), F64,
                    clamp_bottom=k["data"] if clamp else None, clamp_labels=k["y"] if clamp else None)
    assert Ck.draws_of(tape.shapes) == R.sched_mdbm_gibbs(list(k["sizes"]) + [k["J"]], k["K"], Ck.GIBBS_SWEEPS, clamp_bottom=clamp, clamp_labels=clamp)
    assert all(np.array_equal(p.cpu().numpy(), w.astype(F32)) for p, w in zip(parts, want))
    if clamp:
        assert np.array_equal(parts[0].cpu().numpy(), k["data"]) and np.array_equal(parts[-2][:, k["sizes"][-1]:].cpu().numpy(), k["y"])


def _states(k, dt):
    sts = [O.RBMState.create(W, Ck.LR, Ck.WEIGHT_DECAY, Ck.MOM, hid_bias=k["bs"][l + 1],
                             vis_bias=k["bs"][l] if l == 0 else np.zeros_like(k["bs"][l])) for l, W in enumerate(k["Ws"])]
    L, Dz = len(k["Ws"]), k["sizes"][-1]
    sts.append(O.RBMState.create(k["WJ"], Ck.LR, Ck.WEIGHT_DECAY, Ck.MOM, hid_bias=k["bs"][L + 1],
                                 vis_bias=np.concatenate([np.zeros(Dz, F32), k["bs"][L + 2]]), softmax_groups=[(Dz, Dz + k["K"])]))
    return Dt.states_as(sts, dt)


def _model_quantities(sts):
    """name -> array of everything the model owns: W, W_m per RBM (the joint RBM last), the L + 3 layer biases and their momenta."""
    out = {}
    L = len(sts) - 1
    Dz = sts[L - 1].W.shape[1]
    for l, s in enumerate(sts):
        out[f"W{l}"], out[f"W_m{l}"], out[f"b{l + 1}"], out[f"b_m{l + 1}"] = s.W, s.W_m, s.hid_bias, s.hb_m
    out["b0"], out["b_m0"] = sts[0].vis_bias, sts[0].vb_m
    out["bY"], out["b_mY"] = sts[L].vis_bias[Dz:], sts[L].vb_m[Dz:]
    return out


@pytest.mark.parametrize("case", Ck.STACKS, ids=str)
def test_two_steps_follow_the_twin(eng, case):
    k = Ck.stack_case(*case)
    layers, joint, _ = _stack_on_device(k)
    rbms = layers + [joint]
    scal = Ck.STEP_SCALARS[:len(rbms)]
    parts = [dev(p) for p in k["particles"]]
    ref, tw = _states(k, F64), _states(k, F32)
    rparts = tparts = k["particles"]
    Dz = k["sizes"][-1]
    for i, seed in enumerate(Ck.STEP_SEEDS[case]):
        out = eng.mdbm_step(layers, joint, dev(k["data"]), dev(k["y"]), parts, scal, Ck.STEP_N_MF, Ck.STEP_DAMP, Ck.STEP_GIBBS_K,
                            R.ReplayRng(Ck.Tape(seed)))
        torch.cuda.synchronize()
        r = Mt.step(ref, k["data"], k["y"], rparts, scal, Ck.STEP_N_MF, Ck.STEP_DAMP, Ck.STEP_GIBBS_K, Ck.Tape(seed))
        t = Mt.step(tw, k["data"], k["y"], tparts, scal, Ck.STEP_N_MF, Ck.STEP_DAMP, Ck.STEP_GIBBS_K, Ck.Tape(seed))
        rparts, tparts = r["particles"], t["particles"]
        assert all(np.array_equal(p.cpu().numpy(), w.astype(F32)) for p, w in zip(parts, rparts)), "a particle bit differs from float64"
        have = {}
        for l, rb in enumerate(rbms):
            have[f"W{l}"], have[f"W_m{l}"] = rb.W.data.cpu().numpy(), rb.W_m.cpu().numpy()
            have[f"b{l + 1}"], have[f"b_m{l + 1}"] = rb.hid_bias.data.cpu().numpy(), rb.hb_m.cpu().numpy()
        have["b0"], have["b_m0"] = layers[0].vis_bias.data.cpu().numpy(), layers[0].vb_m.cpu().numpy()
        have["bY"], have["b_mY"] = joint.vis_bias.data[Dz:].cpu().numpy(), joint.vb_m[Dz:].cpu().numpy()
        rq, tq = _model_quantities(ref), _model_quantities(tw)
        worst = 0.0
        for name in rq:
            e_dev, e_twin = Dt.rel_frobenius(have[name], rq[name]), Dt.rel_frobenius(tq[name], rq[name])
            tol = min(1e-4, STEP_FACTOR * max(e_twin, 2.0 ** -24))
            worst = max(worst, e_dev / max(e_twin, 2.0 ** -24))
            assert e_dev <= tol, f"step {i} {name}: device {e_dev:.3g}, twin {e_twin:.3g}"
        loss = float(out["recon_loss"])
        print(f"{case} step {i}: worst device / twin error ratio {worst:.3g}; recon_loss {loss:.7f} vs {float(r['recon_loss']):.7f}")
        assert abs(loss - float(r["recon_loss"])) <= 1e-5 * max(1.0, abs(float(r["recon_loss"])))


# ---- the model through the real engine ---------------------------------------------------------------------------------------------------
def test_finetune_runs_two_epochs_without_a_host_read_and_repeats_its_bits(eng, monkeypatch):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn import engine as E
    from imdbn.models import iMDBN
    g = np.random.default_rng(21)
    K = 6
    protos = (g.random((K, 100)) < 0.3).astype(F32)
    labels = g.integers(0, K, 64)
    X = protos[labels]
    X = np.where(g.random(X.shape) < 0.03, 1 - X, X).astype(F32)
    Xd, Yd = dev(X), dev(np.eye(K, dtype=F32)[labels])                     # the loader hands out device tensors: no copy to wait for
    dl = DataLoader(TensorDataset(Xd, Yd), batch_size=32)
    params = {"LEARNING_RATE": 0.05, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.5, "LEARNING_RATE_DYNAMIC": False,
              "CD": 1, "JOINT_CD": 1}
    torch.manual_seed(3)
    net = iMDBN([100, 40, 20], 24, params=params, dataloader=dl, val_loader=dl, device=torch.device(DEV), num_labels=K)
    before = [r.W.data.clone() for r in net.image_idbn.layers + [net.joint_rbm]]
    runs = []
    for _ in range(2):
        dbm = net.to_dbm()
        E.manual_seed(7)
        dbm.train_step(Xd[:32], Yd[:32], 0, 2, lr_scale=0.2, monitor=False)           # creates the particles
        with monkeypatch.context() as mp:
            def read(*a, **kw):
                raise AssertionError("finetune(log_every=0) read from the device")
            for name in ("cpu", "item", "tolist", "numpy"):
                mp.setattr(torch.Tensor, name, read)
            dbm.finetune(2, n_mf=5, gibbs_k=2, lr_scale=0.2, log_every=0)
        torch.cuda.synchronize()
        runs.append([r.W.data.clone() for r in dbm._rbms()] + [p.clone() for p in dbm.particles])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])) and dbm.history == []
    assert all(bool(torch.isfinite(t).all()) for t in runs[0])
    assert all(torch.equal(r.W.data, b) for r, b in zip(net.image_idbn.layers + [net.joint_rbm], before)), "to_dbm touched the iMDBN"
    assert bool((dbm.particles[2][:, 20:].sum(1) == 1).all())
    dbm.finetune(1, n_mf=5, gibbs_k=2, lr_scale=0.2, log_every=1)
    mu_y, pred = dbm.predict_labels(Xd)
    img = dbm.generate(torch.arange(K), n_sweeps=5)
    torch.cuda.synchronize()
    assert [h[0] for h in dbm.history] == [0] and tuple(mu_y.shape) == (64, K) and tuple(img.shape) == (K, 100)
    assert torch.allclose(mu_y.sum(1), torch.ones(64, device=DEV), atol=1e-5)
    E.set_rng(None)
