"""GPU: imdbn_rbm_tap_iterate / imdbn_rbm_tap_step and imdbn.utils.tap against the float64 reference and the fp32 twin of
tests/tap_oracle.py on the cases of tests/tap_cases.py.

Bounds.  Magnetisations after tap_iterate: the bound derived in tap_oracle's docstring, elementwise, carried through the iterations
by ``iterate_bounded`` -- nothing in it comes from the kernel.  Gamma: of the device's own final magnetisations, against
``gamma`` of them in float64 within ``gamma_bound``.  The residual: within twice ``res_bound`` of the twin's (both are within
one of the float64 value).  tap_step: relative Frobenius error against the float64 oracle; the fp32 twin's own error against
float64 is measured on the same cases, the kernel gets four times the twin's worst figure per quantity (its summation order differs
from numpy's), capped by the 1e-4 parity bound of DESIGN section 5."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle.rbm_oracle as O
import tap_cases as Ck
import tap_oracle as Tt
from likelihood_gpu import DEV, _native, dev, eng, twin  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIX = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")
IDS = [f"{V}x{H}b{B}" for V, H, B in Ck.TABLE]
NAN = float("nan")


def _rbm(k, pitch=None, sparsity=False, wd=Ck.WEIGHT_DECAY):
    """The case's RBM on the device; `pitch`: W and W_m as views of NaN-filled [V, pitch] buffers."""
    from imdbn.models import RBM
    V, H = k["W"].shape
    r = RBM(V, H, Ck.LR, wd, Ck.MOM, sparsity=sparsity, sparsity_factor=Ck.SPARSITY_TARGET).to(DEV)
    p = H if pitch is None else pitch
    r.W.data = torch.full((V, p), NAN, device=DEV)[:, :H]
    r.W.data.copy_(dev(k["W"]))
    r.W_m = torch.full((V, p), NAN, device=DEV)[:, :H]
    g = np.random.default_rng(77)
    k.setdefault("W_m", (g.standard_normal((V, H)) * 1e-3).astype(F32))
    k.setdefault("hb_m", (g.standard_normal(H) * 1e-3).astype(F32))
    k.setdefault("vb_m", (g.standard_normal(V) * 1e-3).astype(F32))
    r.W_m.copy_(dev(k["W_m"]))
    r.hb_m, r.vb_m = dev(k["hb_m"]), dev(k["vb_m"])
    r.vis_bias.data.copy_(dev(k["a"]))
    r.hid_bias.data.copy_(dev(k["c"]))
    return r


def _state(k, dt, sparsity=False, wd=Ck.WEIGHT_DECAY):
    st = O.RBMState.create(k["W"].copy(), Ck.LR, wd, Ck.MOM, sparsity=sparsity, sparsity_factor=Ck.SPARSITY_TARGET)
    st.vis_bias[:], st.hid_bias[:] = k["a"], k["c"]
    st.W_m[:], st.hb_m[:], st.vb_m[:] = k["W_m"], k["hb_m"], k["vb_m"]
    return Tt.state_as(st, dt)


def _have(r):
    return {n: (getattr(r, n).data if n in SIX[:3] else getattr(r, n)).cpu().numpy() for n in SIX}


# ---- 1. tap_iterate against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damp", [0.0, 0.5])
@pytest.mark.parametrize("n_iters", [1, 3])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("V,H,B", Ck.TABLE, ids=IDS)
def test_tap_iterate_stays_inside_the_derived_bound(eng, V, H, B, order, n_iters, damp):
    k = Ck.case(V, H, B)
    r = _rbm(k)
    mv, mh = dev(k["mv"]), dev(k["mh"])
    gamma, res = eng.tap_iterate(r, mv, mh, n_iters, damp=damp, order=order)
    torch.cuda.synchronize()
    rv, rh, rres, dmv, dmh, rb = twin(("it", V, H, B, order, n_iters, damp),
                                      lambda: Tt.iterate_bounded(k["W"], k["a"], k["c"], k["mv"], k["mh"], n_iters, damp, order))
    gv, gh = mv.cpu().numpy(), mh.cpu().numpy()
    fv, fh = np.abs(gv - rv) / dmv, np.abs(gh - rh) / dmh
    print(f"{V}x{H} B {B} order {order} iters {n_iters} damp {damp}: largest fraction of the bound: mv {fv.max():.3g}, mh {fh.max():.3g}"
          f" (bound up to {dmv.max():.3g} / {dmh.max():.3g})")
    assert fv.max() <= 1.0 and fh.max() <= 1.0
    # Gamma of the device's own final state
    want, gb = Tt.gamma(k["W"], k["a"], k["c"], gv, gh, order), Tt.gamma_bound(k["W"], k["a"], k["c"], gv, gh, order)
    fg = np.abs(gamma.cpu().numpy() - want) / gb
    print(f"   Gamma: largest fraction of its bound {fg.max():.3g} (bound up to {gb.max():.3g})")
    assert gamma.dtype == torch.float64 and fg.max() <= 1.0
    _, _, tres = twin(("itw", V, H, B, order, n_iters, damp), lambda: Tt.iterate(k["W"], k["a"], k["c"], k["mv"], k["mh"], n_iters, damp, order, F32))
    fr = np.abs(res.cpu().numpy().astype(F64) - tres.astype(F64)) / (2 * rb)
    print(f"   residual: largest fraction of its bound against the twin {fr.max():.3g}")
    assert fr.max() <= 1.0


# ---- 2. bit-level invariants -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,H,B", [(67, 33, 5), (1000, 132, 64), (260, 1028, 1), (257, 255, 64)], ids=lambda v: str(v))
def test_bits_padding_and_views(eng, V, H, B):
    k = Ck.case(V, H, B)
    pitch = H + 3 if H % 4 else H + 4
    out = []
    for run in range(2):
        r = _rbm(k, pitch=pitch)
        pv, ph = torch.full((B, V + 5), NAN, device=DEV), torch.full((B, H + 7), NAN, device=DEV)
        mv, mh = pv[:, 2:2 + V], ph[:, 3:3 + H]          # column-offset views of larger tensors
        mv.copy_(dev(k["mv"])); mh.copy_(dev(k["mh"]))
        if run == 1:                                     # whatever the workspace and the scratch hold changes nothing
            for key, buf in eng._ws.items():
                if key[0] in ("tap", "tap_ws"):
                    buf.view(torch.uint8).fill_(0xFF)    # NaN as floats, -1 as counters
        g1, r1 = eng.tap_iterate(r, mv, mh, 2, damp=0.5, order=2)
        loss = eng.tap_step(r, dev(k["data"]), mv, mh, Ck.LR, Ck.MOM, 2)
        torch.cuda.synchronize()
        Wb = torch.as_strided(r.W.data, (V, pitch), (pitch, 1))
        Mb = torch.as_strided(r.W_m, (V, pitch), (pitch, 1))
        assert torch.isnan(Wb[:, H:]).all() and torch.isnan(Mb[:, H:]).all(), "the row padding of W / W_m was written"
        assert torch.isnan(pv[:, :2]).all() and torch.isnan(pv[:, 2 + V:]).all() and torch.isnan(ph[:, :3]).all() and torch.isnan(ph[:, 3 + H:]).all()
        have = _have(r)
        assert all(np.isfinite(v).all() for v in have.values()) and torch.isfinite(mv).all() and torch.isfinite(mh).all()
        assert torch.isfinite(g1).all() and torch.isfinite(r1).all() and torch.isfinite(loss)
        out.append((have, mv.cpu().numpy().copy(), mh.cpu().numpy().copy(), g1.cpu().numpy(), r1.cpu().numpy(), float(loss)))
    a, b = out
    assert all(np.array_equal(a[0][n], b[0][n]) for n in SIX) and all(np.array_equal(x, y) for x, y in zip(a[1:5], b[1:5])) and a[5] == b[5]
    # the same magnetisations as contiguous tensors on unpadded weights: the same bits
    r = _rbm(k)
    mv, mh = dev(k["mv"]), dev(k["mh"])
    g1, r1 = eng.tap_iterate(r, mv, mh, 2, damp=0.5, order=2)
    torch.cuda.synchronize()
    assert np.array_equal(g1.cpu().numpy(), a[3]) and np.array_equal(r1.cpu().numpy(), a[4])


def test_magnetisations_that_would_be_copied_are_refused(eng):
    from imdbn.engine.native import EngineError
    k = Ck.case(67, 33, 5)
    r, mv, mh = _rbm(k), dev(k["mv"]), dev(k["mh"])
    for bv, bh in ((mv.double(), mh), (mv.cpu(), mh), (mv[:4], mh), (mv, mh.t().contiguous().t()), (mv[:, ::2], mh)):
        with pytest.raises(EngineError):
            eng.tap_iterate(r, bv, bh, 1)
        with pytest.raises(EngineError):
            eng.tap_step(r, dev(k["data"]), bv, bh, 0.1, 0.5, 1)


# ---- 3. tap_step against the oracle -------------------------------------------------------------------------------------------------
STEP_ITERS = (0, 1, 3)
QUANT = SIX + ("mv", "mh", "loss")


def _settings(i):
    """sparsity and weight decay vary over the table: sparsity on in every third case, no weight decay in every fourth."""
    return i % 3 == 1, (0.0 if i % 4 == 2 else Ck.WEIGHT_DECAY)


def _oracle_step(i, order, n_iters, dt):
    V, H, B = Ck.TABLE[i]
    k = Ck.case(V, H, B)
    _rbm_fields(k)
    sp, wd = _settings(i)
    st = _state(k, dt, sp, wd)
    loss, mv, mh = Tt.tap_step(st, k["data"], k["mv"], k["mh"], Ck.LR, Ck.MOM, n_iters, 0.5, order)
    out = {n: getattr(st, n) for n in SIX}
    out.update(mv=mv, mh=mh, loss=np.array([loss]))
    return out


def _rbm_fields(k):
    V, H = k["W"].shape
    g = np.random.default_rng(77)
    k.setdefault("W_m", (g.standard_normal((V, H)) * 1e-3).astype(F32))
    k.setdefault("hb_m", (g.standard_normal(H) * 1e-3).astype(F32))
    k.setdefault("vb_m", (g.standard_normal(V) * 1e-3).astype(F32))


def _ref(i, order, n_iters):
    return twin(("step64", i, order, n_iters), lambda: _oracle_step(i, order, n_iters, F64))


def _step_bounds():
    """{quantity: min(4 x the twin's worst relative Frobenius error against float64 over every case of test 3, 1e-4)}."""
    def compute():
        worst = dict.fromkeys(QUANT, 0.0)
        for i in range(len(Ck.TABLE)):
            for order in (1, 2):
                for n_iters in STEP_ITERS:
                    ref, tw = _ref(i, order, n_iters), _oracle_step(i, order, n_iters, F32)
                    for q in QUANT:
                        worst[q] = max(worst[q], Tt.rel_frobenius(tw[q], ref[q]))
        print("the twin's worst relative Frobenius error against float64:", ", ".join(f"{q} {v:.3g}" for q, v in worst.items()))
        return {q: min(4 * v, 1e-4) for q, v in worst.items()}
    return twin("step_bounds", compute)


def _check_step(what, got, ref):
    bounds = _step_bounds()
    errs = {q: Tt.rel_frobenius(got[q], ref[q]) for q in QUANT}
    print(f"{what}: rel-Frobenius vs float64 (bound):", ", ".join(f"{q} {errs[q]:.2e} ({bounds[q]:.2e})" for q in QUANT))
    bad = [q for q in QUANT if not errs[q] <= bounds[q]]
    assert not bad, f"{what}: {bad}"


@pytest.mark.parametrize("n_iters", STEP_ITERS)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("i", range(len(Ck.TABLE)), ids=IDS)
def test_tap_step_matches_the_float64_oracle(eng, i, order, n_iters):
    V, H, B = Ck.TABLE[i]
    k = Ck.case(V, H, B)
    sp, wd = _settings(i)
    r = _rbm(k, sparsity=sp, wd=wd)
    mv, mh = dev(k["mv"]), dev(k["mh"])
    loss = eng.tap_step(r, dev(k["data"]), mv, mh, Ck.LR, Ck.MOM, n_iters, damp=0.5, order=order)
    torch.cuda.synchronize()
    got = _have(r)
    got.update(mv=mv.cpu().numpy(), mh=mh.cpu().numpy(), loss=np.array([float(loss)]))
    _check_step(f"{V}x{H} B {B} order {order} iters {n_iters} sparsity {sp} wd {wd}", got, _ref(i, order, n_iters))
    if n_iters == 0:
        assert np.array_equal(got["mv"], k["mv"]) and np.array_equal(got["mh"], k["mh"])


def test_the_step_cases_switch_sparsity_and_weight_decay():
    s = [_settings(i) for i in range(len(Ck.TABLE))]
    assert any(sp for sp, _ in s) and any(not sp for sp, _ in s) and any(wd == 0 for _, wd in s) and any(wd > 0 for _, wd in s)


# ---- 4. a sequence --------------------------------------------------------------------------------------------------------------------
def test_five_steps_over_different_batches_follow_five_oracle_steps(eng):
    V, H, B = 128, 64, 64
    k = Ck.case(V, H, B)
    r = _rbm(k)
    st = _state(k, F64)
    g = np.random.default_rng(5)
    mv, mh = dev(k["mv"]), dev(k["mh"])
    rv, rh = k["mv"].astype(F64), k["mh"].astype(F64)
    for step in range(5):
        data = (g.random((B, V)) < 0.2 + 0.1 * step).astype(F32)
        loss = eng.tap_step(r, dev(data), mv, mh, Ck.LR, Ck.MOM, 2, damp=0.5, order=2)
        rl, rv, rh = Tt.tap_step(st, data, rv, rh, Ck.LR, Ck.MOM, 2, 0.5, 2)
    torch.cuda.synchronize()
    got = _have(r)
    got.update(mv=mv.cpu().numpy(), mh=mh.cpu().numpy(), loss=np.array([float(loss)]))
    ref = {n: getattr(st, n) for n in SIX}
    ref.update(mv=rv, mh=rh, loss=np.array([rl]))
    _check_step("five steps at 128x64 B 64", got, ref)


# ---- 5. log Z end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", Ck.SMALL_SEEDS)
@pytest.mark.parametrize("V,H,s", Ck.SMALL)
def test_tap_log_partition_on_the_device_meets_the_calibration_condition(eng, V, H, s, seed):
    from imdbn.utils import tap
    W, a, c = Ck.params(V, H, s, seed)
    r = _rbm(dict(W=W, a=a, c=c))
    log_z = Tt.log_z_enumerated(W, a, c)
    exact = float(eng.exact_log_z(r)["log_z"])
    cal = tap.tap_calibration(r, n_starts=8, max_iters=200, check_every=50, tol=1e-6)
    print(f"({V}, {H}, {s}) seed {seed}: log Z enumerated {log_z:.6f}, on the device {exact:.6f}; gap order 1 {cal['gap_nmf']:.3g}, order 2 {cal['gap_tap']:.3g}")
    assert cal["converged"] and abs(cal["log_z_exact"] - exact) == 0
    for truth in (log_z, exact):
        err1, err2 = truth - cal["log_z_nmf"], abs(truth - cal["log_z_tap"])
        assert err1 > 0 and err2 < 0.1 * err1


# ---- 6. bad arguments through the raw entry ----------------------------------------------------------------------------------------
def test_every_bad_argument_is_refused_before_any_launch(eng):
    from imdbn.engine import native as N
    lib = N.lib()
    k = Ck.case(67, 33, 5)
    V, H, B = 67, 33, 5
    r = _rbm(k)
    d = eng._desc(r, True)
    SENT = 123.25
    mv, mh = torch.full((B, V), SENT, device=DEV), torch.full((B, H), SENT, device=DEV)
    gam, res = torch.full((B,), SENT, dtype=torch.float64, device=DEV), torch.full((B,), SENT, device=DEV)
    loss = torch.full((1,), SENT, device=DEV)
    data = dev(k["data"])
    nws, nsc = int(lib.imdbn_rbm_tap_ws_bytes(V, H, B)), int(lib.imdbn_rbm_tap_scratch_floats(V, H))
    assert nws > int(lib.imdbn_ws_bytes(V, H, B)) and nsc >= 2 * V * H and lib.imdbn_rbm_tap_ws_bytes(0, H, B) == 0
    ws, sc = torch.zeros(nws, dtype=torch.uint8, device=DEV), torch.full((nsc,), SENT, device=DEV)
    o = eng._opts(r, 0.1, 0.5, 0)
    before = _have(r)
    P = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    grp = eng._build_desc(r, True)
    grp.n_groups, grp.group_start[0], grp.group_end[0] = 1, 60, 67

    def iterate(d_=d, mv_=mv, mh_=mh, B_=B, n=1, damp=0.5, order=2, ws_=ws, nws_=nws):
        return lib.imdbn_rbm_tap_iterate(C.byref(d_) if d_ is not None else None, P(mv_), V, P(mh_), H, B_, n, damp, order, P(gam), P(res),
                                         P(ws_), nws_, st)

    def step(d_=d, data_=data, mv_=mv, mh_=mh, o_=o, B_=B, n=1, damp=0.5, order=2, sc_=sc, nsc_=nsc, ws_=ws, nws_=nws):
        return lib.imdbn_rbm_tap_step(C.byref(d_) if d_ is not None else None, P(data_), V, B_, P(mv_), V, P(mh_), H,
                                      C.byref(o_) if o_ is not None else None, n, damp, order, P(loss), P(sc_), nsc_, P(ws_), nws_, st)

    common = [dict(d_=None), dict(mv_=None), dict(mh_=None), dict(ws_=None), dict(order=0), dict(order=3), dict(damp=1.0), dict(damp=-0.1),
              dict(damp=NAN), dict(n=-1), dict(B_=0), dict(nws_=nws - 1), dict(d_=grp)]
    for kw in common:
        assert iterate(**kw) == N_INVALID, ("tap_iterate", kw)
        assert step(**kw) == N_INVALID, ("tap_step", kw)
    for kw in (dict(data_=None), dict(o_=None), dict(sc_=None), dict(nsc_=nsc - 1)):
        assert step(**kw) == N_INVALID, ("tap_step", kw)
    nomom = eng._build_desc(r, True)
    nomom.W_m = None
    assert step(d_=nomom) == N_INVALID
    torch.cuda.synchronize()
    for t in (mv, mh, gam, res, loss, sc):
        assert bool((t == SENT).all())
    after = _have(r)
    assert all(np.array_equal(before[n], after[n]) for n in SIX)


N_INVALID = -1      # IMDBN_E_INVALID
