"""GPU: the convergence-tracing family at its edge shapes (trace_cases.py has the cases, the derivations and the reasoning; DESIGN
section 39 the figures): partial trace windows on both chain routes against slices of the full windows, bit for bit;
imdbn_trace_code_scan and imdbn_rbm_prop_down_sqerr against float64 within bounds that come from the number formats;
imdbn_trace_patience_scan equal to the oracle on dyadic inputs; one odd-shaped panel in both directions.  No out-of-range ref_row
entry is ever passed; every bad-argument case is one the host refuses before a launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import trace_cases as TC
import trace_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
SENT = -7.0                                     # sentinel of buffers the kernels must leave alone (no probability, step or error is negative)
E_INVALID, E_UNSUPPORTED = -1, -5               # include/imdbn_engine.h
WORST = {}


def _note(what, frac):
    WORST[what] = max(WORST.get(what, 0.0), float(frac))


@pytest.fixture(scope="module", autouse=True)
def eng():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    e = E.get_hip_engine()                      # raises if the library is missing: no silent fallback
    assert "gfx950" in e.device_info()[1]
    yield e
    e.set_option("no_chain_kernel", 0)
    for k, v in sorted(WORST.items()):
        print(f"[trace scans] {k}: largest fraction of the bound {v:.3g}")


def _t(x):
    return torch.from_numpy(np.array(x)).to(DEV)         # a copy: the cases' arrays are read-only


def _padded(x, pad=3, fill=float("nan")):
    """x as a view [..., :n] of a `fill`-filled parent whose rows are `pad` longer."""
    t = _t(x)
    wide = torch.full((*t.shape[:-1], t.size(-1) + pad), fill, device=DEV)
    wide[..., :t.size(-1)] = t
    return wide[..., :t.size(-1)]


def _rbm(W, hb, vb, groups=None):
    from imdbn.models import RBM
    r = RBM(W.shape[0], W.shape[1], 0.1, 1e-4, 0.5, softmax_groups=groups).to(DEV)
    r.W.data.copy_(_t(W)); r.hid_bias.data.copy_(_t(hb)); r.vis_bias.data.copy_(_t(vb))
    return r


def _poison_ws(eng, V, H, B):
    eng._workspace(torch.device(DEV), V, H, B).view(torch.float32).fill_(float("nan"))


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


# ---- A: partial windows -------------------------------------------------------------------------------------------------------------------
def _chain(prob, i, trace=None, trace_h=None):
    d = {"v_known": _t(prob["vk"]), "mask": _t(prob["mask"][i]), "steps": TC.window_steps(i), "init_uniform": True}
    if trace is not None:
        d["trace"] = trace
    if trace_h is not None:
        d["trace_h"] = trace_h
    return d


def _philox():
    from imdbn import engine as E
    return E.PhiloxRng(seed=TC.WIN_SEED)


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


@pytest.mark.parametrize("no_kernel", [0, 1], ids=["kernel", "per_launch"])
@pytest.mark.parametrize("B", TC.WIN_BATCHES)
def test_partial_windows_are_slices_of_the_full_windows(eng, B, no_kernel):
    V, H = TC.WIN_V, TC.WIN_H
    prob = TC.window_problem(B)
    r = _rbm(prob["W"], prob["hb"], prob["vb"], [TC.WIN_GROUP])
    eng.set_option("no_chain_kernel", no_kernel)
    try:
        _poison_ws(eng, V, H, B)
        rng0 = _philox()
        fin0 = eng.chain(r, _t(prob["vk"]), _t(prob["mask"][0]), TC.window_steps(0), rng0)
        full = {}
        for base in (0, 1):
            rg = _philox()
            ((fin, vis, hid),) = eng.chain_traced_vh(r, _chain(prob, 0, (0, V, base), (0, H)), None, rg)
            assert eng.last_chain()["route"] == TC.window_route(no_kernel, False)
            _same(fin, fin0, "final state under full windows"); assert rg.offset == rng0.offset
            assert vis.shape == (TC.WIN_STEPS + base, B, V) and hid.shape == (TC.WIN_STEPS, B, H)
            full[base] = (vis, hid)
        _same(full[1][0][1:], full[0][0], "the baseline slot moved the step slots"); _same(full[1][1], full[0][1], "the baseline slot moved the hidden slots")
        assert torch.isfinite(full[1][0]).all() and torch.isfinite(full[1][1]).all()
        for tr, th in TC.window_calls():
            rg = _philox()
            ((fin, vis, hid),) = eng.chain_traced_vh(r, _chain(prob, 0, tr, th), None, rg)
            assert eng.last_chain()["route"] == TC.window_route(no_kernel, False), (tr, th)
            _same(fin, fin0, f"final state, windows {tr} {th}"); assert rg.offset == rng0.offset
            fv, fh = full[tr[2] if tr else 0]
            if tr:
                _same(vis, fv[:, :, tr[0]:tr[1]], f"visible window {tr} (hidden {th})")
            else:
                assert vis is None
            if th:
                _same(hid, fh[:, :, th[0]:th[1]], f"hidden window {th} (visible {tr})")
            else:
                assert hid is None
        # the same visible windows through chain_traced (no hidden argument at all)
        for tr in ((3, 70, 1), (72, 77, 0)):
            rg = _philox()
            ((fin, vis),) = eng.chain_traced(r, _chain(prob, 0, tr), None, rg)
            _same(fin, fin0, "chain_traced final"); _same(vis, full[tr[2]][0][:, :, tr[0]:tr[1]], f"chain_traced window {tr}")
    finally:
        eng.set_option("no_chain_kernel", 0)


@pytest.mark.parametrize("no_kernel", [0, 1], ids=["kernel", "per_launch"])
@pytest.mark.parametrize("B", TC.WIN_BATCHES)
def test_pair_with_different_windows(eng, B, no_kernel):
    V, H = TC.WIN_V, TC.WIN_H
    prob = TC.window_problem(B)
    r = _rbm(prob["W"], prob["hb"], prob["vb"], [TC.WIN_GROUP])
    eng.set_option("no_chain_kernel", no_kernel)
    try:
        _poison_ws(eng, V, H, B)
        rng0 = _philox()
        fa0, fb0 = eng.chain_pair(r, _chain(prob, 0), _chain(prob, 1), rng0)
        full = {}
        for ba, bb in ((0, 0), (1, 1), (1, 0), (0, 1)):
            rg = _philox()
            ra, rb = eng.chain_traced_vh(r, _chain(prob, 0, (0, V, ba), (0, H)), _chain(prob, 1, (0, V, bb), (0, H)), rg)
            assert eng.last_chain()["route"] == TC.window_route(no_kernel, True)
            _same(ra[0], fa0, "pair final a"); _same(rb[0], fb0, "pair final b"); assert rg.offset == rng0.offset
            full[(ba, bb)] = (ra, rb)
        for (ta, ha), (tb, hb) in TC.window_pairs():
            rg = _philox()
            ra, rb = eng.chain_traced_vh(r, _chain(prob, 0, ta, ha), _chain(prob, 1, tb, hb), rg)
            assert eng.last_chain()["route"] == TC.window_route(no_kernel, True)
            _same(ra[0], fa0, "pair final a"); _same(rb[0], fb0, "pair final b"); assert rg.offset == rng0.offset
            fa, fb = full[(ta[2] if ta else 0, tb[2] if tb else 0)]
            for got, ref, tr, th, who in ((ra, fa, ta, ha, "a"), (rb, fb, tb, hb, "b")):
                if tr:
                    _same(got[1], ref[1][:, :, tr[0]:tr[1]], f"chain {who} visible window {tr}")
                else:
                    assert got[1] is None
                if th:
                    _same(got[2], ref[2][:, :, th[0]:th[1]], f"chain {who} hidden window {th}")
                else:
                    assert got[2] is None
    finally:
        eng.set_option("no_chain_kernel", 0)


@pytest.mark.parametrize("no_kernel", [0, 1], ids=["kernel", "per_launch"])
def test_windows_under_the_wrapper_leave_every_sentinel(eng, no_kernel):
    """The specs as HipEngine._chain_specs builds them, `out` re-pointed into a larger sentinel-filled buffer with ld_row = width + 3
    and step_stride = B * ld_row + 5."""
    V, H, B = TC.WIN_V, TC.WIN_H, 5
    prob = TC.window_problem(B)
    r = _rbm(prob["W"], prob["hb"], prob["vb"], [TC.WIN_GROUP])
    tr, th = (*TC.RAW_VIS, 1), TC.RAW_HID
    eng.set_option("no_chain_kernel", no_kernel)
    try:
        ((fin0, vis0, hid0),) = eng.chain_traced_vh(r, _chain(prob, 0, tr, th), None, _philox())
        d = eng._desc(r, False)
        rng = _philox()
        Bc, dev, specs, traces, results, sched, keep, hidden = eng._chain_specs("test", r, d, (_chain(prob, 0, tr, th), None), True)
        bufs = []
        for t, slots, w in ((traces[0], TC.WIN_STEPS + 1, tr[1] - tr[0]), (hidden[0][0], TC.WIN_STEPS, th[1] - th[0])):
            ld, ss = w + 3, B * (w + 3) + 5
            buf = torch.full((7 + slots * ss + 11,), SENT, device=DEV)
            t.out, t.ld_row, t.step_stride = buf.data_ptr() + 4 * 7, ld, ss
            bufs.append((buf, slots, w, ld, ss))
        rn, keep_r = eng._rng(rng, sched, Bc, dev)
        eng._call("imdbn_rbm_chain_traced_vh", C.byref(d), Bc, C.byref(specs[0]), C.byref(traces[0]), C.byref(hidden[0][0]), None, None, None,
                  C.byref(rn), *eng._ws_tail(dev, d.V, d.H, Bc))
        eng._done(rng, rn, sched)
        assert eng.last_chain()["route"] == TC.window_route(no_kernel, False)
        torch.cuda.synchronize()
        _same(results[0][0], fin0, "final state")
        for (buf, slots, w, ld, ss), want, what in zip(bufs, (vis0, hid0), ("visible", "hidden")):
            idx = (7 + torch.arange(slots, device=DEV)[:, None, None] * ss + torch.arange(B, device=DEV)[None, :, None] * ld
                   + torch.arange(w, device=DEV)[None, None, :])
            _same(buf[idx], want, f"{what} window in the pitched buffer")
            inside = torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
            inside[idx.reshape(-1)] = True
            assert int(inside.sum()) == slots * B * w
            assert (buf[~inside] == SENT).all(), f"{what}: {int((buf[~inside] != SENT).sum())} elements outside the window were written"
    finally:
        eng.set_option("no_chain_kernel", 0)


# ---- B: code scan -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dz", TC.CODE_DZ)
def test_code_scan_against_float64(eng, Dz):
    bz, bd = TC.code_scan_bounds(Dz)
    for c in (c for c in TC.code_cases() if c["Dz"] == Dz):
        zs, z0 = TC.code_inputs(c)
        tr, zi = (_padded(zs), _padded(z0)) if c["strided"] else (_t(zs), _t(z0))
        if c["strided"]:
            assert tr.stride(0) == c["B"] * (Dz + 3) and tr.stride(1) == Dz + 3 and zi.stride(0) == Dz + 3
        zn, dz = eng.code_scan(tr, zi, c["beta"])
        zn, dz = zn.cpu().numpy(), dz.cpu().numpy()
        assert zn.shape == zs.shape and dz.shape == (c["B"], c["T"])
        assert np.isfinite(zn).all() and np.isfinite(dz).all(), f"{c['id']}: the NaN padding was read"
        if c["beta"] == 0.0:
            assert np.array_equal(zn.view(np.uint32), zs.view(np.uint32)), f"{c['id']}: z_new is not the input, bit for bit"
        zr, dr = TC.code_ref(c["id"])
        if c["data"] == "grid":
            want = np.sqrt(dr ** 2).astype(F32)          # float32(sqrt(exact sum)): the sum of squares is exact in fp32 in any order
            ulps = np.abs(dz.astype(F64) - want.astype(F64)) / np.spacing(want).astype(F64)
            _note("code scan dz, grid (ulp)", ulps.max())
            assert (ulps <= 1).all(), f"{c['id']}: dz is {ulps.max():.2f} ulp from float32(sqrt(exact sum))"
        else:
            ez, ed = TC.code_errors(c, zn, dz)
            print(f"{c['id']}: z_new {ez:.3g} of {bz:.3g}, dz {ed:.3g} of {bd:.3g}")
            _note(f"code scan z_new Dz {Dz}", ez / bz); _note(f"code scan dz Dz {Dz}", ed / bd)
            assert ez <= bz, f"{c['id']}: z_new is {ez:.3g} from float64, bound {bz:.3g}"
            assert ed <= bd, f"{c['id']}: dz is {ed:.3g} (relative) from float64, bound {bd:.3g}"


@pytest.mark.parametrize("Dz,B,T", [(65, 5, 6), (130, 9, 1), (1, 1, 6)])
def test_code_scan_raw_entry_pitches_and_sentinels(eng, Dz, B, T):
    """ld_init > Dz, a pitched NaN-padded trace, output buffers larger than the batch: rows b >= B keep their sentinel."""
    g = np.random.Generator(np.random.PCG64(Dz + B))
    zs, z0 = g.random((T, B, Dz), dtype=F32), g.random((B, Dz), dtype=F32)
    beta = float(F32(0.3))
    tr, zi = _padded(zs, 5), _padded(z0, 7)
    zn = torch.full((T * B * Dz + 3 * Dz + 64,), SENT, device=DEV)
    dz = torch.full(((B + 5) * T,), SENT, device=DEV)
    rc = eng._lib.imdbn_trace_code_scan(_p(tr), tr.stride(0), tr.stride(1), T, B, Dz, _p(zi), zi.stride(0), beta, _p(zn), _p(dz), eng._stream(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    assert (zn[T * B * Dz:] == SENT).all() and (dz[B * T:] == SENT).all(), "a row past the batch was written"
    zr, dr = TO.code_scan(zs.astype(F64), z0.astype(F64), beta)
    bz, bd = TC.code_scan_bounds(Dz) if Dz in TC.CODE_DZ else (TC.PARITY, TC.PARITY)
    got_z, got_d = zn[:T * B * Dz].view(T, B, Dz).cpu().numpy(), dz[:B * T].view(B, T).cpu().numpy()
    assert np.abs(got_z - zr).max() <= bz and (np.abs(got_d - dr) / dr).max() <= bd
    # refused before a launch, nothing written
    zn.fill_(SENT); dz.fill_(SENT)
    s = eng._stream(torch.device(DEV))
    for name, args in (("null trace", (None, tr.stride(0), tr.stride(1), T, B, Dz, zi, zi.stride(0))),
                       ("ld_row < Dz", (tr, tr.stride(0), Dz - 1, T, B, Dz, zi, zi.stride(0))),
                       ("ld_init < Dz", (tr, tr.stride(0), tr.stride(1), T, B, Dz, zi, Dz - 1)),
                       ("step_stride < B ld_row", (tr, B * tr.stride(1) - 1, tr.stride(1), T, B, Dz, zi, zi.stride(0))),
                       ("T = 0", (tr, tr.stride(0), tr.stride(1), 0, B, Dz, zi, zi.stride(0))),
                       ("B = 0", (tr, tr.stride(0), tr.stride(1), T, 0, Dz, zi, zi.stride(0)))):
        a = list(args)
        rc = eng._lib.imdbn_trace_code_scan(_p(a[0]), a[1], a[2], a[3], a[4], a[5], _p(a[6]), a[7], beta, _p(zn), _p(dz), s)
        assert rc == E_INVALID, (name, rc)
    torch.cuda.synchronize()
    assert (zn == SENT).all() and (dz == SENT).all(), "a refused call wrote"


# ---- C: patience scan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TC.patience_cases(), ids=lambda c: c["id"])
def test_patience_scan_equals_the_oracle(eng, c):
    dz, mse, rows = TC.patience_inputs(c)
    want_s, want_b = TC.patience_ref(c)
    B, T = c["B"], c["T"]
    steps = torch.full((B + 70,), -9, dtype=torch.int32, device=DEV)
    best = torch.full((B + 70,), SENT, device=DEV)
    dzt, mset = _t(dz), _t(mse)
    rc = eng._lib.imdbn_trace_patience_scan(_p(dzt), _p(mset), T, B, TC.EPS_Z, TC.MSE_TOL, c["P"], _p(steps), _p(best),
                                            eng._stream(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    assert (steps[B:] == -9).all() and (best[B:] == SENT).all(), "a row past the batch was written"
    gs, gb = steps[:B].cpu().numpy(), best[:B].cpu().numpy()
    bad = np.nonzero((gs != want_s) | (gb.astype(F64) != want_b))[0]
    named = {b: n for n, b in rows.items()}
    assert bad.size == 0, f"{c['id']}: rows {bad[:8].tolist()} ({[named.get(int(b), 'random') for b in bad[:8]]}): steps {gs[bad][:8]} vs {want_s[bad][:8]}, " \
                          f"best {gb[bad][:8]} vs {want_b[bad][:8]}"
    s2, b2 = eng.patience_scan(_t(dz), _t(mse), TC.EPS_Z, TC.MSE_TOL, c["P"])          # the wrapper gives the same
    assert np.array_equal(s2.cpu().numpy(), gs) and np.array_equal(b2.cpu().numpy().view(np.uint32), gb.view(np.uint32))


def test_patience_scan_refuses_bad_arguments(eng):
    B, T = 5, 4
    dz, mse = torch.zeros(B, T, device=DEV), torch.zeros(B, T, device=DEV)
    steps, best = torch.full((B,), -9, dtype=torch.int32, device=DEV), torch.full((B,), SENT, device=DEV)
    s = eng._stream(torch.device(DEV))
    for name, a in (("null dz", (None, mse, T, B, steps, best)), ("null mse", (dz, None, T, B, steps, best)),
                    ("null steps", (dz, mse, T, B, None, best)), ("null best", (dz, mse, T, B, steps, None)),
                    ("T = 0", (dz, mse, 0, B, steps, best)), ("B = 0", (dz, mse, T, 0, steps, best))):
        rc = eng._lib.imdbn_trace_patience_scan(_p(a[0]), _p(a[1]), a[2], a[3], TC.EPS_Z, TC.MSE_TOL, 3, _p(a[4]), _p(a[5]), s)
        assert rc == E_INVALID, (name, rc)
    torch.cuda.synchronize()
    assert (steps == -9).all() and (best == SENT).all(), "a refused call wrote"


# ---- D: decode error ----------------------------------------------------------------------------------------------------------------------
def _layers(c):
    return [_rbm(W, hb, vb) for W, hb, vb in TC.decode_layers(c)]


def _decode(eng, c, layers, chunk=1024, poison=True):
    z, ref, rows = TC.decode_inputs(c)
    zt, rt = (_padded(z, 5), _padded(ref, 5)) if c["strided"] else (_t(z), _t(ref))
    if poison:
        for i, s in enumerate(c["sizes"][:-1]):
            _poison_ws(eng, s, c["sizes"][i + 1], min(c["B"], chunk))
    out = eng.decode_sqerr(layers, zt, rt, _t(rows) if rows is not None else None, chunk=chunk)
    route = eng.last_route()
    return out, route


@pytest.mark.parametrize("c", TC.decode_cases(), ids=lambda c: c["id"])
def test_decode_sqerr_against_float64(eng, c):
    layers = _layers(c)
    out, route = _decode(eng, c, layers)
    assert route["down"] == "down_fused" and route["down_epilogue"] == "lean", route      # fewer than 4096 padded rows: one fused kernel
    out2, _ = _decode(eng, c, layers)
    assert torch.equal(out, out2), "two runs on a NaN-filled workspace differ"
    got = out.cpu().numpy()
    assert got.shape == (c["B"],) and np.isfinite(got).all(), f"{c['id']}: padding or workspace contents were read"
    mse, bound = TC.decode_ref(c)
    frac = np.abs(got.astype(F64) - mse) / bound
    print(f"{c['id']}: largest fraction of the bound {frac.max():.3g} (bound from {bound.min():.3g})")
    _note("decode error", frac.max())
    assert (frac <= 1).all(), f"{c['id']}: row {int(frac.argmax())} is {frac.max():.2f} bounds from float64"


@pytest.mark.parametrize("sizes", [(257, 33), (700, 132, 64)], ids=str)
def test_decode_sqerr_ragged_chunks_give_the_same_bits(eng, sizes):
    c = dict(id=f"chunks-{sizes}", sizes=sizes, B=130, kind="real", ref_row="repeat", strided=True)
    layers = _layers(c)
    a, _ = _decode(eng, c, layers, chunk=1024)
    b, _ = _decode(eng, c, layers, chunk=48)           # 48 + 48 + 34
    assert torch.equal(a, b), f"{int((a != b).sum())} of 130 rows differ between chunk = 1024 and chunk = 48"
    mse, bound = TC.decode_ref(c)
    assert (np.abs(a.cpu().numpy().astype(F64) - mse) <= bound).all()


def test_prop_down_sqerr_refuses_bad_arguments(eng):
    V, H, B = 257, 33, 5
    W, hb, vb = TC.layer(V, H)
    r, rg = _rbm(W, hb, vb), _rbm(W, hb, vb, [(250, 257)])
    h, ref = torch.rand(B, H, device=DEV), torch.rand(B, V, device=DEV)
    out = torch.full((B,), SENT, device=DEV)
    d, dg = eng._desc(r, False), eng._desc(rg, False)
    ws = eng._ws_tail(torch.device(DEV), V, H, B)
    call = lambda dd, hh, ldh, b, rr, ldr, oo: eng._lib.imdbn_rbm_prop_down_sqerr(C.byref(dd), _p(hh), ldh, b, _p(rr), ldr, None, _p(oo), *ws)      # noqa: E731
    assert call(dg, h, H, B, ref, V, out) == E_UNSUPPORTED
    for name, a in (("ldh < H", (d, h, H - 1, B, ref, V, out)), ("ldr < V", (d, h, H, B, ref, V - 1, out)), ("B = 0", (d, h, H, 0, ref, V, out)),
                    ("null h", (d, None, H, B, ref, V, out)), ("null ref", (d, h, H, B, None, V, out)), ("null out", (d, h, H, B, ref, V, None))):
        assert call(*a) == E_INVALID, name
    torch.cuda.synchronize()
    assert (out == SENT).all(), "a refused call wrote"
    assert call(d, h, H, B, ref, V, out) == 0
    torch.cuda.synchronize()
    assert (out >= 0).all()


# ---- E: the odd-shaped panel --------------------------------------------------------------------------------------------------------------
class _Model:
    pass


def _close(a, b, tol, what, rel=False):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b) / (np.abs(b) if rel else 1.0)
    assert err.max() <= tol, f"{what}: max err {err.max():.3g}"


def test_odd_shaped_panel_against_the_oracle(eng):
    from imdbn import engine as E
    from imdbn.models import iDBN
    from imdbn.utils import conditional_steps as CS
    seed, Dz, K, T, B = TC.PANEL_SEED, TC.PANEL_DZ, TC.PANEL_K, TC.PANEL_T, TC.PANEL_B
    w, X, Y, yi = TC.panel(seed)
    m = _Model()
    m.device = torch.device(DEV)
    idbn = iDBN.__new__(iDBN)
    idbn.device = m.device
    idbn.layers = [_rbm(w[f"img{i}_W"], w[f"img{i}_hid_bias"], w[f"img{i}_vis_bias"]) for i in range(2)]
    m.image_idbn, m.joint_rbm = idbn, _rbm(w["joint_W"], w["joint_hid_bias"], w["joint_vis_bias"], [(Dz, Dz + K)])
    m.Dz_img, m.num_labels, m.z_class_mean, m.val_loader, m.wandb_run = Dz, K, _t(w["z_class_mean"]), None, None
    with E.use_rng(E.PhiloxRng(seed=seed)):
        i2t, t2i = CS.trace_cross_panel_batch(m, _t(X), _t(Y), max_steps=T)
    (r, steps, pred, margin), o = TC.panel_oracle(seed)
    close = margin <= TC.PANEL_MARGIN
    s_gpu, p_gpu = i2t["steps"].cpu().numpy(), i2t["pred"].cpu().numpy()
    bad = (~close) & ((s_gpu != steps) | (p_gpu != pred))
    assert not bad.any(), (np.nonzero(bad)[0], s_gpu[bad], steps[bad], p_gpu[bad], pred[bad])
    _close(i2t["p_top1"].cpu(), r["p1"], 1e-5, "p_top1")
    _close(i2t["l1"].cpu(), r["l1"], 1e-5, "l1")
    close2 = o["margin"] <= TC.PANEL_MARGIN
    g2 = t2i["steps"].cpu().numpy()
    bad2 = (~close2) & (g2 != o["steps"])
    assert not bad2.any(), (np.nonzero(bad2)[0], g2[bad2], o["steps"][bad2])
    _close(t2i["z_l2"].cpu(), o["z_l2"], 1e-5, "dz")
    _close(t2i["image_mse"].cpu(), o["image_mse"], 1e-4, "image_mse", rel=True)
    n_close = int(close.sum() + close2.sum())
    print(f"odd-shaped panel: {n_close} of {2 * B} rows decided within {TC.PANEL_MARGIN} of a threshold; img2txt steps {s_gpu.tolist()}, txt2img {g2.tolist()}")
    assert n_close <= B // 4
