"""GPU: the data-parallel exchange forms against float64 and against the numpy twin of the wire codec (exchange_cases.py has the
table, the layouts and the reasoning); one process, the ranks emulated by copies.

  W1  cd_factors + pack_factors: the compact block against the twin and the original block; unpack_factors (full and planes_only)
  W2  apply_factors(unpacked) == apply_factors_wire == apply_wire bit for bit, each launching the kernel the case names, and within
      update_cases.TOL of float64 computed from the ORIGINAL cd_factors blocks (never from anything that went through pack / unpack)
  W3  cd_factors_wire, with and without the next-batch hint, against cd_factors + pack_factors, the twin and float64
  W4  one 0.5 under a binary promise, placed: NaN in hid_bias; then a clean block packed over the bad one
  D1  cd_stats / clamped_stats: dW and the tail (dc, db, sum P+) against float64 of the planes in the workspace
  D2  apply_delta on the fp32 shard sum against float64; scalar, float4 on a pitch, misaligned `packed`, the grid rule

Every workspace is NaN-filled and every gather, compact and packed buffer 0xFF-filled before use; options are reset in a `finally`."""
import numpy as np
import pytest
import torch

import exchange_cases as XC
import parity_cases as P
import update_cases as UC
import update_gpu as G
from golden_utils import assert_close

pytestmark = pytest.mark.gpu
DEV = G.DEV
F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731
SEED = 11


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    eng = E.get_hip_engine()             # raises if the library is missing: no silent fallback
    cu, arch = eng.device_info()
    assert "gfx950" in arch, arch
    assert cu >= 16, "the automatic tiles per block of the table's shapes is 1 only with more CUs than tiles"
    yield eng
    for k, v in dict(UC.OPTION_DEFAULTS, no_prefetch=0).items():
        eng.set_option(k, v)
    eng._pf.clear()


@pytest.fixture(autouse=True)
def _options_back(_native):
    yield
    _native.set_option("no_prefetch", 0)      # not among update_cases.OPTION_DEFAULTS, which update_gpu.routed resets


def _routed(eng, c):
    return G.routed(eng, dict(c, opts={k: v for k, v in c["opts"].items() if k != "no_prefetch"}))


def _ff(t):
    t.view(torch.uint8).fill_(0xFF)
    return t


def _trailer(host_wire, w):
    return host_wire[w["c_bad"]: w["c_bad"] + 8].view(np.int32)


def _produce(eng, c, r, data=None, fill=True):
    """cd_factors + pack_factors per rank on a NaN-filled workspace: ([R, block bytes], [R, compact bytes]) device copies."""
    from imdbn import engine as E
    V, H, R, Bl = c["V"], c["H"], c["R"], c["Bl"]
    blocks, wires = [], []
    for rk in range(R):
        G.poison_ws(eng, V, H, Bl)
        if fill:
            _ff(eng._wire_buffer("wire1", r, Bl, 1, c["binary"]))
        x = P.T(XC.rank_data(c, rk) if data is None else data[rk], DEV)
        blk = eng.cd_factors(r, x, 1, E.PhiloxRng(seed=SEED, row0=rk * Bl))
        blocks.append(blk.clone())
        wires.append(eng.pack_factors(r, blk, Bl, c["binary"]).clone())
    return torch.stack(blocks), torch.stack(wires)


def _ref_from_blocks(eng, c, host_blocks, st, n, sparsity):
    blocks = []
    for hb in host_blocks:
        read = G.block_reader(eng, c, c["Bl"], hb)
        blocks.append((G.phases(c, c["Bl"], read), read))
    return UC.ref_update(st, G.stats(c, blocks), XC.LR, XC.MOM, XC.WD, n, sparsity), blocks


def _same_state(a, b, what):
    for k in UC.KEYS:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"


def _codec_check(c, host_block, host_wire, what, planes23=True):
    """The compact block against the original block through the twin."""
    V, H, Bl, binary = c["V"], c["H"], c["Bl"], c["binary"]
    L, w = XC.block_layout(V, H, Bl), XC.wire_layout(V, H, Bl, binary)
    n, nb, Bp = V * L["Bp"] * 2, w["nb"], L["Bp"]
    assert np.array_equal(host_wire[: w["head_bytes"]], host_block[: w["head_bytes"]]), f"{what}: the head is not byte-equal"
    vneg = host_block[L["vis_tr1"]: L["vis_tr1"] + n].view(np.uint16)
    got = XC.unpack_plane(host_wire[w["c_vneg"]: w["c_vneg"] + nb])
    assert np.array_equal(got, vneg), f"{what}: the sample's bit plane decodes to {int((got != vneg).sum())} wrong elements"
    assert np.array_equal(UC.decode_planes(got, V, Bl, Bp, 1), UC.decode_planes(vneg, V, Bl, Bp, 1))
    assert (host_wire[w["c_vneg"] + nb: w["c_vpos"]] == 0xFF).all(), f"{what}: pack wrote behind the sample's bit plane"
    if binary:
        vpos = host_block[L["vis_tr0"]: L["vis_tr0"] + n].view(np.uint16)
        got = XC.unpack_plane(host_wire[w["c_vpos"]: w["c_vpos"] + nb])
        if XC.bad_elements(vpos).size == 0:
            assert np.array_equal(got, vpos), f"{what}: the data's bit plane decodes to {int((got != vpos).sum())} wrong elements"
            assert np.array_equal(UC.decode_planes(got, V, Bl, Bp, 1), UC.decode_planes(vpos, V, Bl, Bp, 1))
            if c["mode"] == "exact" and planes23:
                assert not host_block[L["vis_tr0"] + n: L["vis_tr0"] + 3 * n].any(), f"{what}: 0/1 data with non-zero second / third terms"
        else:
            assert np.array_equal(got != 0, vpos != 0)
        assert (host_wire[w["c_vpos"] + nb: w["c_bad"]] == 0xFF).all(), f"{what}: pack wrote behind the data's bit plane"
    else:
        assert np.array_equal(host_wire[w["c_vpos"]: w["c_vpos"] + 3 * n], host_block[L["vis_tr0"]: L["vis_tr0"] + 3 * n]), \
            f"{what}: the three data planes are not byte-equal"
    bad = _trailer(host_wire, w)
    assert bad[1] >= 1, f"{what}: no pack epoch in the trailer"
    return bool(bad[0] == bad[1])


# ---- W1 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", XC.cases("W"), ids=IDS)
def test_compact_block_matches_the_codec_twin_and_unpack_restores_the_block(c, _native):
    V, H, R, Bl, binary = c["V"], c["H"], c["R"], c["Bl"], c["binary"]
    L, w = XC.block_layout(V, H, Bl), XC.wire_layout(V, H, Bl, binary)
    with _routed(_native, c):
        r = G.rbm(c, UC.params(V, H), XC.WD)
        assert _native.factor_mode_ok(r, Bl)
        fb_off, fb_bytes = _native.factor_block(V, H, Bl)
        assert fb_bytes == L["fb_bytes"]
        for name in ("flags", "hid_tr0", "hid_tr1", "cs_hpos", "cs_hneg", "cs_vpos", "cs_vneg", "vis_tr0", "vis_tr1"):
            assert G.ws_offset(_native, V, H, Bl, name) - fb_off == L[name], name
        assert _native.compact_bytes(V, H, Bl, binary) == w["compact_bytes"]
        blocks, wires = _produce(_native, c, r)
        hb, hw = blocks.cpu().numpy(), wires.cpu().numpy()
        assert hw.shape == (R, w["compact_bytes"]) and hb.shape == (R, L["fb_bytes"])
        for rk in range(R):
            assert not _codec_check(c, hb[rk], hw[rk], f"{c['id']} rank {rk}"), f"rank {rk}: a clean block is marked bad"
        n = V * L["Bp"] * 2
        # full unpack: every region the update reads, byte for byte; nothing else written
        _ff(_native.gather_buffer(r, Bl, R))
        full = _native.unpack_factors(r, wires, Bl, binary).cpu().numpy()
        for rk in range(R):
            assert np.array_equal(full[rk], XC.expand(hw[rk], V, H, Bl, binary)), f"rank {rk}: unpack_factors differs from the twin"
            for name, nbytes in (("flags", w["head_bytes"]), ("vis_tr1", n), ("vis_tr0", n if binary else 3 * n)):
                assert np.array_equal(full[rk, L[name]: L[name] + nbytes], hb[rk, L[name]: L[name] + nbytes]), f"rank {rk}: {name} not restored"
        # planes only: the planes, and the head of the destination untouched
        _ff(_native.gather_buffer(r, Bl, R))
        w2 = wires.clone()
        po = _native.unpack_factors(r, w2, Bl, binary, planes_only=True).cpu().numpy()
        torch.cuda.synchronize()
        assert torch.equal(w2, wires), "planes_only changed a clean wire block"
        for rk in range(R):
            assert (po[rk, : w["head_bytes"]] == 0xFF).all(), f"rank {rk}: planes_only wrote into the head"
            assert np.array_equal(po[rk, w["head_bytes"]:], full[rk, w["head_bytes"]:]), f"rank {rk}: planes_only planes differ"
    print(f"{c['id']}: {R} x {w['compact_bytes']} wire bytes of {L['fb_bytes']}, codec exact")


# ---- W2 -------------------------------------------------------------------------------------------------------------------------------
def _three_forms(eng, c, wires, st, sparsity):
    """The update from the gathered wire blocks in its three forms on fresh RBMs, each asserting the kernel it launched: [(name, loss,
    RBM)].  (A fresh RBM has a fresh descriptor, and every form records its own launch.)"""
    R, Bl, B, binary = c["R"], c["Bl"], c["R"] * c["Bl"], c["binary"]
    out = []
    for form in ("apply_factors", "apply_factors_wire", "apply_wire"):
        r = G.rbm(c, st, XC.WD, sparsity)
        _ff(eng.gather_buffer(r, Bl, R))
        w = wires.clone()
        if form == "apply_factors":
            loss = eng.apply_factors(r, eng.unpack_factors(r, w, Bl, binary), Bl, B, XC.LR, XC.MOM)
        elif form == "apply_factors_wire":
            loss = eng.apply_factors_wire(r, w, eng.unpack_factors(r, w, Bl, binary, planes_only=True), Bl, B, XC.LR, XC.MOM)
        else:
            loss = eng.apply_wire(r, w, Bl, B, binary, XC.LR, XC.MOM)
        G.assert_update(c)
        out.append((form, loss, r))
    return out


@pytest.mark.parametrize("c", XC.cases("W"), ids=IDS)
def test_update_from_the_wire_matches_float64_of_the_original_blocks(c, _native):
    V, H, R, Bl = c["V"], c["H"], c["R"], c["Bl"]
    st, sparsity = UC.params(V, H), c["R"] == 3
    with _routed(_native, c):
        blocks, wires = _produce(_native, c, G.rbm(c, st, XC.WD))
        ref, _ = _ref_from_blocks(_native, c, blocks.cpu().numpy(), st, R * Bl, sparsity)
        got = []
        for form, loss, r in _three_forms(_native, c, wires, st, sparsity):
            s = G.state(r)
            assert np.isfinite(float(loss)), form
            G.close(c, s, ref, what=f" {form}")
            got.append((form, float(loss), s))
    for form, loss, s in got[1:]:
        assert loss == got[0][1], f"{form}: loss differs from apply_factors"
        _same_state(s, got[0][2], f"{form} vs apply_factors")


# ---- W3 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", XC.cases("F"), ids=IDS)
def test_fused_producer_equals_the_separate_calls_the_twin_and_float64(c, _native):
    from imdbn import engine as E
    V, H, R, Bl, binary, T = c["V"], c["H"], c["R"], c["Bl"], c["binary"], c["steps"]
    L, w = XC.block_layout(V, H, Bl), XC.wire_layout(V, H, Bl, binary)
    st = UC.params(V, H)
    X = [[P.T(XC.rank_data(c, k, step=t), DEV) for k in range(R)] for t in range(T)]
    seq = [X[t][k] for t in range(T) for k in range(R)]
    slots = []
    with _routed(_native, c):
        _native.set_option("no_prefetch", c["opts"].get("no_prefetch", 0))
        ra, rb = G.rbm(c, st, XC.WD), G.rbm(c, st, XC.WD)
        assert _native.prefetch_ok(_native._desc(rb, True), Bl) == (not c["opts"].get("no_prefetch"))
        rng_a = [E.PhiloxRng(seed=SEED, row0=k * Bl) for k in range(R)]
        rng_b = [E.PhiloxRng(seed=SEED, row0=k * Bl) for k in range(R)]
        _native._pf.clear()
        G.poison_ws(_native, V, H, Bl)
        prev = st
        for t in range(T):
            wa, hb = [], []
            for k in range(R):
                blk = _native.cd_factors(ra, X[t][k], 1, rng_a[k])
                hb.append(blk.cpu().numpy())
                _ff(_native._wire_buffer("wire1", ra, Bl, 1, binary))
                wa.append(_native.pack_factors(ra, blk, Bl, binary).clone())
            wa = torch.stack(wa)
            _native.apply_factors_wire(ra, wa, _native.unpack_factors(ra, wa, Bl, binary, planes_only=True), Bl, R * Bl, XC.LR, XC.MOM)
            wb = []
            for k in range(R):
                i = t * R + k
                nxt = seq[i + 1] if (c["hint"] and i + 1 < len(seq)) else None
                _ff(_native._wire_buffer("wire1", rb, Bl, 1, binary))
                wb.append(_native.cd_factors_wire(rb, X[t][k], 1, rng_b[k], binary, next_data=nxt).clone())
                slots.append(_native.last_cd()["slot"])
            wb = torch.stack(wb)
            assert torch.equal(wa[:, : w["c_bad"]], wb[:, : w["c_bad"]]), f"step {t}: wire blocks differ"      # (trailer = pack epoch)
            hw = wb.cpu().numpy()
            virt = []
            for k in range(R):      # the fused blocks against the ORIGINAL cd_factors blocks through the twin, then float64 from them
                assert not _codec_check(c, hb[k], hw[k], f"{c['id']} step {t} rank {k}")
                full = XC.expand(hw[k], V, H, Bl, binary)
                virt.append(XC.with_zero_terms(full, V, H, Bl) if binary else full)
            ref, _ = _ref_from_blocks(_native, c, virt, prev, R * Bl, False)
            _ff(_native.gather_buffer(rb, Bl, R))
            _native.apply_wire(rb, wb, Bl, R * Bl, binary, XC.LR, XC.MOM)
            G.assert_update(c)
            sa, sb = G.state(ra), G.state(rb)
            _same_state(sb, sa, f"step {t}: fused vs separate")
            G.close(c, sb, ref, what=f" step {t}")
            prev = sb
        _native._pf.clear()
    want = [0] + [-1] * (T * R - 1) if c["prefetch"] else [0] * (T * R)
    assert all((s in (1, 2)) if x < 0 else s == 0 for s, x in zip(slots, want)), f"{c['id']}: prefetch slots {slots}"
    if c["prefetch"]:
        assert all(a != b for a, b in zip(slots[1:-1], slots[2:])), f"the slots do not alternate: {slots}"


# ---- W4 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", XC.cases("K"), ids=IDS)
def test_one_non_binary_element_under_a_binary_promise_poisons_the_update(c, _native):
    V, H, R, Bl = c["V"], c["H"], c["R"], c["Bl"]
    L, w = XC.block_layout(V, H, Bl), XC.wire_layout(V, H, Bl, True)
    st = UC.params(V, H)
    rk_bad = c["plant"][0]
    with _routed(_native, c):
        r0 = G.rbm(c, st, XC.WD)
        blocks, wires = _produce(_native, c, r0)
        hb, hw = blocks.cpu().numpy(), wires.cpu().numpy()
        n = V * L["Bp"] * 2
        for rk in range(R):
            plane = hb[rk, L["vis_tr0"]: L["vis_tr0"] + n].view(np.uint16)
            assert XC.bad_elements(plane).tolist() == ([XC.plant_index(c)] if rk == rk_bad else []), f"rank {rk}: the plane does not hold the planted element"
            assert _codec_check(c, hb[rk], hw[rk], f"{c['id']} rank {rk}") == (rk == rk_bad), f"rank {rk}: wrong `bad` mark"
        for form, loss, r in _three_forms(_native, c, wires, st, False):
            torch.cuda.synchronize()
            assert torch.isnan(r.hid_bias.data).any(), f"{form}: the broken promise went unnoticed"
        # a clean block packed into the compact buffer that held the bad one (not refilled: its stale mark must be ignored)
        clean = [UC.cd_data(c, rk) for rk in range(R)]
        blocks2, wires2 = _produce(_native, c, r0, data=clean, fill=False)
        wires.copy_(wires2)
        hb2, hw2 = blocks2.cpu().numpy(), wires.cpu().numpy()
        for rk in range(R):
            assert not _codec_check(c, hb2[rk], hw2[rk], f"{c['id']} clean rank {rk}"), f"rank {rk}: a stale mark made a clean block bad"
        ref, _ = _ref_from_blocks(_native, c, hb2, st, R * Bl, False)
        for form, loss, r in _three_forms(_native, c, wires, st, False):
            G.close(c, G.state(r), ref, what=f" clean {form}")


# ---- D ----------------------------------------------------------------------------------------------------------------------------------
def _nan_packed(eng, V, H):
    return _ff(torch.empty(eng.packed_floats(V, H), device=DEV))


def _run_stats(eng, c, r, lo, hi):
    """cd_stats / clamped_stats of the rows [lo, hi) on a NaN-filled workspace into a 0xFF-filled buffer: (packed, (phases, read), rows)."""
    from imdbn import engine as E
    V, H, rows = c["V"], c["H"], hi - lo
    G.poison_ws(eng, V, H, rows)
    out = _nan_packed(eng, V, H)
    rng = E.PhiloxRng(seed=SEED, row0=lo)
    if c["entry"] == "clamped_stats":
        vk, km = XC.clamped_inputs(c)
        init = r._nmf_steps(12, 3.0, 1.0, 0.9, 2, 0.9, 0.0)
        eng.clamped_stats(r, P.T(vk[lo:hi], DEV), P.T(km[lo:hi], DEV), init, None, 1, True, True, False, rng, out=out)
    else:
        eng.cd_stats(r, P.T(XC.batch(c)[lo:hi], DEV), 1, rng, out=out)
    G.assert_update(c)
    torch.cuda.synchronize()
    fb_off, fb_bytes = eng.factor_block(V, H, rows)
    host = eng._workspace(torch.device(DEV), V, H, rows)[fb_off:fb_off + fb_bytes].cpu().numpy()
    read = G.block_reader(eng, c, rows, host)
    return out, (G.phases(c, rows, read), read), rows


def _stats_close(c, packed, s, what):
    V, H = c["V"], c["H"]
    p, t = XC.split_packed(P.N(packed), V, H), XC.tail64(s)
    want = dict(dW=s["dW"], **t)
    print(f"{c['id']} {what}: max|d| " + "  ".join(f"{k} {float(np.abs(p[k] - want[k]).max()):.3e}" for k in want))
    for k in want:
        assert_close(p[k], want[k], UC.STATS_TOL["rel"], f"{c['id']} {what}: {k}", atol=UC.STATS_TOL["atol"])
    assert np.isfinite(p["sqerr"]) and p["sqerr"] >= 0


def _rbm_d(c, st):
    return G.rbm(c, st, XC.WD, c["sparsity"], groups=list(c["groups"]) or None)


@pytest.mark.parametrize("c", XC.stats_cases(), ids=IDS)
def test_packed_statistics_and_their_tail_match_float64_of_the_planes(c, _native):
    V, H, B = c["V"], c["H"], c["B"]
    st = UC.params(V, H)
    with _routed(_native, c):
        r = _rbm_d(c, st)
        total, blocks, rows = None, [], []
        for lo, hi in XC.shards(B, c["n_shards"]):
            packed, blk, n = _run_stats(_native, c, r, lo, hi)
            _stats_close(c, packed, G.stats(c, [blk], rows=[n]), f"rows {lo}..{hi}")
            total = packed.clone() if total is None else total + packed
            blocks.append(blk); rows.append(n)
        whole, blk, n = _run_stats(_native, c, r, 0, B)
        _stats_close(c, whole, G.stats(c, [blk], rows=[n]), "whole batch")
        _stats_close(c, total, G.stats(c, blocks, rows=rows), "shard sum")
        n_used = V * H + 2 * H + V + 1
        assert_close(P.N(total)[:n_used], P.N(whole)[:n_used], UC.STATS_TOL["rel"], f"{c['id']}: shard sum vs whole batch", atol=UC.STATS_TOL["atol"])
        after = G.state(r)
    for k in UC.KEYS:
        assert np.array_equal(after[k], st[k]), f"{c['id']}: the statistics pass changed {k}"


@pytest.mark.parametrize("c", XC.apply_cases(), ids=IDS)
def test_apply_delta_matches_float64_of_the_summed_statistics(c, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    st = UC.params(V, H)
    with _routed(_native, c):
        r = _rbm_d(c, st)
        if c["synthetic"]:
            host, s = XC.synthetic_stats(c)
            packed = _nan_packed(_native, V, H)
            packed[: host.size].copy_(P.T(host, DEV))
            want_loss = float(host[-1]) / (B * V)
        else:
            packed, blocks, rows = None, [], []
            for lo, hi in XC.shards(B, c["n_shards"]):
                p, blk, n = _run_stats(_native, c, r, lo, hi)
                packed = p.clone() if packed is None else packed + p          # the all-reduce: an fp32 sum
                blocks.append(blk); rows.append(n)
            s = G.stats(c, blocks, rows=rows)
            r2 = _rbm_d(c, st)
            with E.use_rng(E.PhiloxRng(seed=SEED)):
                want_loss = float(r2.train_epoch(P.T(XC.batch(c), DEV), 0, 10, CD=1))
        if c["misaligned"]:
            big = _ff(torch.empty(packed.numel() + 8, device=DEV))
            view = big[1:1 + packed.numel()]
            view.copy_(packed)
            assert view.data_ptr() % 16 == 4 and r.W.data_ptr() % 16 == 0 and r.W.stride(0) % 4 == 0 and H % 4 == 0
            packed = view
        loss = _native.apply_delta(r, packed, B, XC.LR, XC.MOM, sparsity=c["sparsity"])
        got = G.state(r)          # (asserts the padding of W and W_m is still NaN on a pitched case)
    G.close(c, got, UC.ref_update(st, s, XC.LR, XC.MOM, XC.WD, B, c["sparsity"]))
    print(f"{c['id']}: loss {float(loss):.7g} against {want_loss:.7g}")
    assert_close(float(loss), want_loss, 1e-5, f"{c['id']}: loss")
