"""GPU: the CD pass (cd_phases / cd_prologue, csrc/engine.hip) on every route make_route gives it, the next-batch prefetch included,
against a float64 reference of rbm.py:199-209 (cd_cases.py has the table, the route mirror and the reasoning).  Every case asserts
through HipEngine.last_route() and HipEngine.last_cd() the kernels it ran, and that the draw cursor moved by the schedule's count.

The reference takes every decision on the PhiloxStream draws as the device must (seeds pinned on the CPU with a margin of 1e-6,
test_cd_routes_cpu.py), so samples and planes of samples are compared exactly, probabilities within route_cases.prob_bound(1.0) and
the packed statistics within cd_cases.stats_bound: B * 5e-7 + 2e-6 * |ref| + 2e-5 per element.

Largest |device - float64| of the packed statistics over the whole file on an MI355X, next to the bound of the element it was
measured at (every case prints its own figures and the running maximum with `-s`):

  dW     2.34e-05  (bound 8.50e-05, 0.28 of it)   cd-1040x36-B130-k1-real-real
  dc     3.14e-05  (bound 8.50e-05, 0.37)          cd-130x70-B130-k1-mixed-unknown
  db     1.69e-05  (bound 8.50e-05, 0.20)          seq-stats-1040x36-B130 step 6
  hpos   1.77e-05  (bound 1.68e-04, 0.11)          seq-stats-1040x36-B130 step 3
  sqerr  2.08e-03  (bound 6.83e-02, 0.03)          cd-1040x36-no_bits-rows12-B130-k2-binary-unknown

Only the squared-error sum is more than ten times below its bound (its relative term, 2e-6 of a sum of B V squares, is generous next
to a sum taken in double from per-block partials); the bound is derived, so it stays as it is.

Every call runs on a NaN-filled workspace (a sequence starts from one); options and the engine's prefetch record are reset after
every case."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import cd_cases as CC
import parity_cases as P
import update_cases as UC
from golden_utils import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731
WORST = {}                   # statistic -> largest |device - float64| seen (printed per case)


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    eng = E.get_hip_engine()             # raises if the library is missing: no silent fallback
    cu, arch = eng.device_info()
    assert "gfx950" in arch, arch
    assert cu == CC.CUS, f"cd_cases.route_of mirrors the routes of a device with {CC.CUS} compute units, this one has {cu}"
    yield eng
    for k, v in CC.OPTION_DEFAULTS.items():
        eng.set_option(k, v)
    eng._pf.clear()


def _hint_arg(hint):
    from imdbn.engine import native
    return {"unknown": None, "binary": True, "real": native.DATA_REAL}[hint]


def _tagged(x, hint):
    """The batch on the device, carrying the tag the engine reads a hint from (HipEngine.binary_hint)."""
    t = P.T(x, DEV)
    if hint != "unknown":
        t._imdbn_binary = hint == "binary"
    return t


def _rbm(c, st=None, step=False):
    from imdbn.models import RBM
    st = st or CC.state(c["route_name"])
    r = RBM(c["V"], c["H"], 0.1, CC.STEP_WD, 0.5, sparsity=step, sparsity_factor=UC.SPARSITY_TARGET,
            softmax_groups=[tuple(g) for g in c["groups"]] or None)
    P.set_params(r, DEV, st["W"], st["hid_bias"], st["vis_bias"])
    r.W_m.copy_(P.T(st["W_m"], DEV)); r.hb_m.copy_(P.T(st["hb_m"], DEV)); r.vb_m.copy_(P.T(st["vb_m"], DEV))
    assert r.W.stride(0) == c["H"] and r.W.data_ptr() % 16 == 0      # what route_of assumes
    return r


def _state(r):
    torch.cuda.synchronize()
    out = {k: P.N(getattr(r, k)) for k in UC.KEYS}
    for k, v in out.items():
        assert np.isfinite(v).all(), f"{k} is not finite"
    return out


@contextlib.contextmanager
def _routed(eng, c):
    """The case's options for the duration of its calls, on a NaN-filled workspace and with no batch on record as prefetched."""
    try:
        for k, v in c["opts"].items():
            eng.set_option(k, v)
        eng._pf.clear()
        eng._workspace(torch.device(DEV), c["V"], c["H"], c["B"]).view(torch.float32).fill_(float("nan"))
        yield
    finally:
        for k in c["opts"]:
            eng.set_option(k, CC.OPTION_DEFAULTS[k])
        eng._pf.clear()


def _assert_routes(eng, cid, expect, expect_cd):
    got, got_cd = eng.last_route(), eng.last_cd()
    assert {k: got[k] for k in expect} == expect, f"{cid}: ran {got}, the case names {expect}"
    assert got_cd == expect_cd, f"{cid}: the pass ran as {got_cd}, the case names {expect_cd}"


def _reader(eng, c):
    torch.cuda.synchronize()
    return lambda name, nbytes: eng.debug_buffer(DEV, c["V"], c["H"], c["B"], name, nbytes).cpu().numpy()


def _bits(buf, N, B, Bp):
    """A bit plane [ceil64(N) / 8][Bp] bytes (bit j of byte (n / 8, b) = element (b, 8 (n / 8) + j)) -> [B, N] 0/1."""
    u = np.ascontiguousarray(buf).view(np.uint8)[: (N + 7) // 8 * Bp].reshape(-1, 1, Bp)
    return ((u >> np.arange(8, dtype=np.uint8)[None, :, None]) & 1).reshape(-1, Bp)[:N, :B].T.astype(F64)


def _colsum(read, name, N, Bp):
    return read(name, Bp // 8 * N * 4).view(F32).reshape(Bp // 8, N).astype(F64).sum(0)


def _within(got, ref, bound, what):
    d = float(np.abs(np.asarray(got, F64) - ref).max())
    assert np.isfinite(got).all() and d <= bound, f"{what}: max|d| = {d:.3e} > {bound:.3e}"


def _check_planes(c, ref, read, x, data_plane="vis_tr0"):
    """The operand planes and column sums a pass leaves, against the reference (decode_planes asserts zero padding rows, no NaN)."""
    V, H, B = c["V"], c["H"], c["B"]
    Bp = (B + 63) // 64 * 64
    if data_plane:
        assert np.array_equal(UC.decode_planes(read(data_plane, 3 * V * Bp * 2), V, B, Bp, 3).astype(F32), x), f"{c['id']}: vis_tr0 does not hold the batch"
        _within(_colsum(read, "cs_vpos", V, Bp), x.astype(F64).sum(0), 1e-6 * B, f"{c['id']}: cs_vpos")
    v = UC.decode_planes(read("vis_tr1", V * Bp * 2), V, B, Bp, 1)
    assert np.array_equal(v, ref["v"]), f"{c['id']}: {int((v != ref['v']).sum())} visible samples differ from the reference's decisions"
    if c["r"]["vbits"]:
        assert np.array_equal(_bits(read("vis_bits1", (V + 63) // 64 * 8 * Bp), V, B, Bp), ref["v"]), f"{c['id']}: vis_bits1 does not hold the sample"
    _within(UC.decode_planes(read("hid_tr0", 3 * H * Bp * 2), H, B, Bp, 3), ref["hpos"], CC.prob_bound(1.0), f"{c['id']}: hid_tr0 vs P+")
    _within(UC.decode_planes(read("hid_tr1", 3 * H * Bp * 2), H, B, Bp, 3, negated=True), ref["hneg"], CC.prob_bound(1.0), f"{c['id']}: -hid_tr1 vs P-")
    pb = B * CC.prob_bound(1.0) + 1e-6 * B
    _within(_colsum(read, "cs_hpos", H, Bp), ref["hpos"].sum(0), pb, f"{c['id']}: cs_hpos")
    _within(_colsum(read, "cs_hneg", H, Bp), ref["hneg"].sum(0), pb, f"{c['id']}: cs_hneg")
    _within(_colsum(read, "cs_vneg", V, Bp), ref["v"].sum(0), 0.0, f"{c['id']}: cs_vneg")


def _check_packed(cid, V, H, B, packed, ref):
    got, want = P.N(packed).astype(F64)[: V * H + 2 * H + V + 1], CC.packed64(ref)
    assert np.isfinite(got).all(), f"{cid}: the packed statistics are not finite"
    line, bad = [], []
    for name, sl in CC.packed_parts(V, H).items():
        d, bound = np.abs(got[sl] - want[sl]), CC.stats_bound(B, want[sl])
        WORST[name] = max(WORST.get(name, 0.0), float(d.max()))
        line.append(f"{name} {float(d.max()):.2e} (bound {float(bound.min()):.2e}; suite max {WORST[name]:.2e})")
        if (d > bound).any():
            bad.append(f"{name}: max|d| {float(d.max()):.3e} at bound {float(bound[d.argmax()]):.3e}")
    print(f"{cid}: max|d| " + "  ".join(line))
    assert not bad, f"{cid}: " + "; ".join(bad)


# ---- one pass -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CC.cases("pass"), ids=IDS)
def test_cd_pass_matches_float64_on_its_route(c, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    x = CC.operand(c["data"], B, V)
    ref = CC.ref_cd(c)
    rng = E.PhiloxRng(seed=c["seed"])
    st = CC.state(c["route_name"])
    with _routed(_native, c):
        r = _rbm(c)
        packed = _native.cd_stats(r, P.T(x, DEV), c["k"], rng, data_binary=_hint_arg(c["hint"]))
        _assert_routes(_native, c["id"], c["expect"], c["expect_cd"])
        assert rng.offset == c["draws"]
        _check_planes(c, ref, _reader(_native, c), x)
        _check_packed(c["id"], V, H, B, packed, ref)
        after = _state(r)
    for k in UC.KEYS:
        assert np.array_equal(after[k], st[k]), f"{c['id']}: the statistics pass changed {k}"


# ---- the update behind the pass -------------------------------------------------------------------------------------------------------
def _step_ref(c, st, ref):
    return UC.ref_update(st, ref["stats"], CC.STEP_LR, CC.STEP_MOM, CC.STEP_WD, c["B"], sparsity=True)


def _close(cid, got, want):
    for k in UC.KEYS:
        assert_close(got[k], want[k], UC.TOL["rel"], f"{cid}: {k}", atol=UC.TOL["atol"])


@pytest.mark.parametrize("forward", (False, True), ids=("step", "step+forward"))
@pytest.mark.parametrize("c", CC.one_per_route(), ids=IDS)
def test_cd_step_after_the_pass_matches_float64(c, forward, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    x = CC.operand(c["data"], B, V)
    ref, st = CC.ref_cd(c), CC.state(c["route_name"])
    want = _step_ref(c, st, ref)
    route, cd = CC.expect_of(c["r"], c["hint"], forward=forward)
    rng = E.PhiloxRng(seed=c["seed"])
    with _routed(_native, c):
        r = _rbm(c, step=True)
        out = _native.cd_step(r, P.T(x, DEV), CC.STEP_LR, CC.STEP_MOM, c["k"], rng, data_binary=_hint_arg(c["hint"]), forward=forward)
        _assert_routes(_native, c["id"], route, cd)
        assert rng.offset == c["draws"]
        got = _state(r)
    loss = float(out[0] if forward else out)
    assert abs(loss - ref["sqerr"] / (B * V)) <= 1e-5 * ref["sqerr"] / (B * V), (loss, ref["sqerr"] / (B * V))
    _close(c["id"], got, want)
    if forward:
        p = CC.sigmoid64(x.astype(F64) @ want["W"] + want["hid_bias"])
        # the device propagates ITS updated parameters: |d logit| <= sum_i |x_i| tol(W_i) + tol(c), a sigmoid slope of at most 1/4
        tw = UC.TOL["rel"] * np.abs(want["W"]) + UC.TOL["atol"]
        tc = UC.TOL["rel"] * np.abs(want["hid_bias"]) + UC.TOL["atol"]
        bound = CC.prob_bound(1.0) + 0.25 * float((np.abs(x).astype(F64) @ tw + tc).max())
        _within(P.N(out[1]), p, bound, f"{c['id']}: forward under the updated parameters")


# ---- prefetch sequences -----------------------------------------------------------------------------------------------------------------
def _check_slot(c, s, read, nxt):
    """The slot plane the following step reads holds `nxt` in the form the route and the hint give it: `one` bf16 plane, `three`, or
    per 64-column x 64-row item one where the item is all 0/1 and three elsewhere (the other planes of such an item are not written:
    the positive-phase K1 of the next step completes them where the update kernel needs them).  Every term is a bf16 number by
    construction of the planes; they must sum to the batch exactly, padding rows zero."""
    V, B = c["V"], c["B"]
    Bp = (B + 63) // 64 * 64
    u = read(f"pf_tr{s['next_slot']}", 3 * V * Bp * 2).view(np.uint16).reshape(3, V, Bp)
    f = (u.astype(np.uint32) << 16).view(F32).astype(F64)      # [term][feature][row]
    full = np.zeros((Bp, V), F32); full[:B] = nxt
    terms = np.full((V, Bp), 3)
    if s["form"] == "one":
        terms[:] = 1
    elif s["form"] == "item":
        for v0 in range(0, V, 64):
            for b0 in range(0, Bp, 64):
                blk = full[b0:b0 + 64, v0:v0 + 64]
                if ((blk == 0) | (blk == 1)).all():
                    terms[v0:v0 + 64, b0:b0 + 64] = 1
    live = np.arange(3)[:, None, None] < terms[None]
    assert np.isfinite(f[live]).all(), f"{c['id']} step {s['i']}: NaN in a slot plane the next step reads"
    got = np.where(live, f, 0.0).sum(0).T
    assert np.array_equal(got, full.astype(F64)), f"{c['id']} step {s['i']}: slot {s['next_slot']} ({s['form']}) does not hold the hinted batch"
    if s["form"] != "one" and (terms == 3).any():
        hi, mid, lo = (np.zeros((Bp, V), F32) for _ in range(3))
        hi[:B], mid[:B], lo[:B] = UC.split3(nxt)
        for k, part in enumerate((hi, mid, lo)):
            assert np.array_equal(np.where(terms == 3, f[k], 0.0), np.where(terms == 3, part.T, 0.0)), f"{c['id']} step {s['i']}: term {k} of the slot"


@pytest.mark.parametrize("c", CC.cases("seq"), ids=IDS)
def test_prefetched_sequence_matches_float64_step_by_step(c, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    step = c["entry"] == "step"
    xs = [CC.seq_batch(s["data"], B, V, s["i"]) for s in c["steps"]]
    ts = [_tagged(x, s["hint"]) for x, s in zip(xs, c["steps"])]
    other = _tagged(np.roll(xs[3], 5, axis=0), "unknown")
    rng = E.PhiloxRng(seed=c["seed"])
    st = CC.state(c["route_name"])
    with _routed(_native, c):
        r = _rbm(c, step=step)
        for s in c["steps"]:
            i = s["i"]
            hint = {"next": ts[i + 1] if i + 1 < len(ts) else None, "other": other, None: None}[s["nxt"]]
            ref = CC.ref_seq_step(c, i, st, i * c["draws"])
            if step:
                _native.cd_step(r, ts[i], CC.STEP_LR, CC.STEP_MOM, c["k"], rng, next_data=hint)
            else:
                packed = _native.cd_stats(r, ts[i], c["k"], rng, next_data=hint)
            _assert_routes(_native, f"{c['id']} step {i}", s["expect"], s["expect_cd"])
            assert rng.offset == (i + 1) * c["draws"]
            if step:      # the next step's reference starts from the fp32 state the device holds
                got = _state(r)
                _close(f"{c['id']} step {i}", got, _step_ref(c, st, ref))
                st = got
            else:
                _check_packed(f"{c['id']} step {i}", V, H, B, packed, ref)
            if s["next_slot"]:
                _check_slot(c, s, _reader(_native, c), P.N(hint))
    assert not _native._pf


# ---- the factor block -------------------------------------------------------------------------------------------------------------------
FACTOR_CASES = [c for c in CC.cases("pass") if c["r"]["vec4"] and not c["groups"] and c["B"] <= 64]


def _ws_offset(eng, V, H, B, name):
    off = C.c_size_t(0)
    eng._call("imdbn_debug_ws_offset", int(V), int(H), int(B), name.encode(), C.byref(off))
    return int(off.value)


def _block_reader(eng, c, block):
    fb, nb = eng.factor_block(c["V"], c["H"], c["B"])
    host = block.cpu().numpy()
    assert host.size == nb

    def read(name, nbytes):
        off = _ws_offset(eng, c["V"], c["H"], c["B"], name) - fb
        assert 0 <= off and off + nbytes <= nb, f"{name} is outside the factor block"
        return host[off:off + nbytes].copy()
    return read


@pytest.mark.parametrize("c", FACTOR_CASES, ids=IDS)
def test_cd_factors_planes_on_the_routes_that_allow_them(c, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    x = CC.operand(c["data"], B, V)
    ref = CC.ref_cd(c)
    with _routed(_native, c):
        r = _rbm(c)
        assert _native.factor_mode_ok(r, B)
        rng = E.PhiloxRng(seed=c["seed"])
        block = _native.cd_factors(r, P.T(x, DEV), c["k"], rng, data_binary=_hint_arg(c["hint"])).clone()
        _assert_routes(_native, c["id"], c["expect"], c["expect_cd"])
        assert rng.offset == c["draws"]
        torch.cuda.synchronize()
        read = _block_reader(_native, c, block)
        ws_read = _reader(_native, c)
        # (the factor block carries the first term of vis_tr1 and no bit plane: vbits is checked on the workspace)
        _check_planes(c, ref, lambda name, n: ws_read(name, n) if name == "vis_bits1" else read(name, n), x)
        if c["route_name"] in ("130x72", "1040x36"):
            # the wire form of the same pass, alone and with a next batch prepared beside it, unpacks to the same planes bit for bit
            binary = c["data"] == "binary"
            Bp = (B + 63) // 64 * 64
            for nxt in (None, _tagged(np.roll(x, 3, axis=0), "unknown")):
                _native._pf.clear()
                rng = E.PhiloxRng(seed=c["seed"])
                wire = _native.cd_factors_wire(r, P.T(x, DEV), c["k"], rng, binary, next_data=nxt, data_binary=_hint_arg(c["hint"]))
                route, cd = CC.expect_of(c["r"], c["hint"], None if nxt is None else "unknown")
                if not binary and cd["adaptive"]:
                    cd = dict(cd, adaptive=False)      # a wire form with three data planes needs all three written: no compact slot form
                _assert_routes(_native, f"{c['id']} wire", route, cd)
                full = _native.unpack_factors(r, wire.reshape(1, -1), B, binary)
                wread = _block_reader(_native, c, full[0])
                for name, nbytes in (("vis_tr0", (1 if binary else 3) * V * Bp * 2), ("vis_tr1", V * Bp * 2), ("hid_tr0", 3 * H * Bp * 2),
                                     ("hid_tr1", 3 * H * Bp * 2), ("cs_hpos", Bp // 8 * H * 4), ("cs_hneg", Bp // 8 * H * 4),
                                     ("cs_vpos", Bp // 8 * V * 4), ("cs_vneg", Bp // 8 * V * 4)):
                    assert np.array_equal(wread(name, nbytes), read(name, nbytes)), f"{c['id']} wire (hint {nxt is not None}): {name} differs from cd_factors"
