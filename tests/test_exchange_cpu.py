"""CPU: the table of exchange_cases.py is well-formed, the numpy twin of the wire codec does what the comment in kernels_ew.hpp says,
and the float64 references are linear over shards (no GPU needed)."""
import numpy as np
import pytest

import exchange_cases as XC
import update_cases as UC

F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731


def test_case_ids_are_unique_and_the_table_stays_small():
    cs = XC.cases()
    assert len({c["id"] for c in cs}) == len(cs)
    gpu = 2 * len(XC.wire_cases()) + len(XC.fused_cases()) + len(XC.broken_cases()) + len(XC.stats_cases()) + len(XC.apply_cases())
    assert gpu <= 60, gpu
    for c in cs:
        assert set(c["opts"]) <= set(UC.OPTION_DEFAULTS) | {"no_prefetch"}, c["id"]


@pytest.mark.parametrize("c", XC.cases("W") + XC.cases("F") + XC.cases("K"), ids=IDS)
def test_factors_cases_satisfy_factor_mode_ok(c):
    assert XC.factor_mode_ok(c["H"], c["pitch"], c["Bl"]) and c["B"] == c["R"] * c["Bl"] and 1 <= c["R"] <= 3
    assert c["expect"][0] == (UC.UPDATE_RANKS if c["R"] >= 2 else UC.UPDATE_PLANES)
    for rk in range(c["R"]):
        x = XC.rank_data(c, rk)
        assert x.shape == (c["Bl"], c["V"])
        if c["binary"] and not c.get("plant"):
            assert np.isin(x, (0.0, 1.0)).all(), "a binary promise on data that are not 0/1"


def test_the_wire_table_covers_every_edge_once():
    ws = XC.wire_cases()
    assert {c["Bl"] for c in ws} == {1, 40, 64} and {c["R"] for c in ws} == {1, 2, 3}
    assert {(c["V"], c["H"]) for c in ws} == {(300, 132), (130, 36), (128, 128), (700, 132), (1100, 260)}
    assert {c["mode"] for c in ws} == {"exact", "fast"} and {c["binary"] for c in ws} == {True, False}
    assert any(c["tpb"] == 5 for c in ws) and any(c["pitch"] == 288 for c in ws)
    L = XC.block_layout(300, 132, 40)
    assert L["Vpad"] == 304 and L["size"]["flags"] == 8 * 5 * 4 and (300 * 64 // 8) % 256 != 0
    assert all(v % 256 == 0 for k, v in XC.block_layout(128, 128, 64)["size"].items() if k not in ("flags", "loss_part"))


@pytest.mark.parametrize("c", XC.cases("D"), ids=IDS)
def test_allreduce_cases_leave_the_factors_path_where_they_say(c):
    rows = [b - a for a, b in XC.shards(c["B"], c["n_shards"])]
    assert sum(rows) == c["B"] and all(r > 0 for r in rows) and all(r % 8 == 0 for r in rows[:-1])
    ok = all(XC.factor_mode_ok(c["H"], c["pitch"], r, c["groups"]) for r in rows)
    assert ok == (c["why"] == "mode"), (c["id"], rows)
    if c["why"] == "H%4":
        assert c["H"] % 4 and c["expect"] == (UC.UPDATE_GENERIC, 0)
    if c["why"] == "rows":
        assert max(rows) > 64 and XC.factor_mode_ok(c["H"], c["pitch"], 64)
    if c["why"] == "groups":
        assert c["groups"] and XC.factor_mode_ok(c["H"], c["pitch"], min(rows, default=1) if max(rows) <= 64 else 64)
        x = XC.batch(c)
        for s, e in c["groups"]:
            assert e == c["V"] and (x[:, s:e].sum(1) == 1).all()


def test_the_grid_rule_binds_for_the_shape_that_claims_it():
    assert not XC.grid_rule_binds(2100, 8) and not XC.grid_rule_binds(8, 1100)
    assert XC.grid_rule_binds(3, 260) and not XC.grid_rule_binds(3, 256) and not XC.grid_rule_binds(4, 260)
    assert all(not XC.grid_rule_binds(V, H) for V in range(4, 40) for H in range(4, 2200, 4))      # min(V, H) >= 4: never
    assert any(c["synthetic"] and (c["V"], c["H"]) == (3, 260) for c in XC.delta_cases())
    assert {c["sparsity"] for c in XC.apply_cases()} == {True, False}
    assert {c["B"] for c in XC.apply_cases()} >= {40, 64, 130, 200} and {c["n_shards"] for c in XC.apply_cases()} >= {2, 3}


@pytest.mark.parametrize("c", XC.cases("K"), ids=IDS)
def test_the_planted_element_sits_where_the_case_says(c):
    rk, row, col = c["plant"]
    Bp, nb = 64, c["V"] * 64 // 8
    for r in range(c["R"]):
        x = XC.rank_data(c, r)
        odd = np.argwhere(~np.isin(x, (0.0, 1.0)))
        assert (odd.tolist() == [[row, col]] and x[row, col] == 0.5) if r == rk else odd.size == 0
    plane = UC.encode_planes(XC.rank_data(c, rk), Bp, terms=1)
    assert XC.bad_elements(plane).tolist() == [XC.plant_index(c)]
    byte = XC.plant_index(c) // 8
    want = {"first": 0, "last": (nb - 1) if c["Bl"] == 64 else (c["V"] - 1) * 8 + (c["Bl"] - 1) // 8}.get(c["where"])
    if want is not None:
        assert byte == want
    if c["where"] == "last":
        assert byte == max(i // 8 for i in range(c["V"] * Bp) if i % Bp < c["Bl"])      # the last group that holds a real row
    if c["where"] == "last_rank":
        assert rk == c["R"] - 1 and 0 < byte < nb - 1
    assert any(c["where"] == "last" and c["Bl"] == 64 for c in XC.cases("K")), "no case puts the element into the plane's last byte"


def test_codec_twin_round_trips_and_flags_exactly_the_non_binary_elements():
    g = np.random.Generator(np.random.PCG64(5))
    plane = (g.random(300 * 64) > 0.5).astype(np.uint16) * np.uint16(XC.ONE_BF16)
    byte, bad = XC.pack_plane(plane)
    assert not bad and byte.size == plane.size // 8 and np.array_equal(XC.unpack_plane(byte), plane)
    raw = g.integers(0, 256, 2400).astype(np.uint8)
    assert np.array_equal(XC.pack_plane(XC.unpack_plane(raw))[0], raw)
    # element j of a group in bit j: a plane with only element 8 i + j set packs to 1 << j in byte i
    for j in range(8):
        one = np.zeros(64, np.uint16)
        one[8 * 5 + j] = XC.ONE_BF16
        b, bad = XC.pack_plane(one)
        assert not bad and b[5] == 1 << j and not np.delete(b, 5).any()
        assert np.flatnonzero(XC.unpack_plane(b)).tolist() == [8 * 5 + j]
    # the numpy statement agrees with numpy's own little-endian bit packing
    assert np.array_equal(byte, np.packbits(plane != 0, bitorder="little"))
    # bad: exactly the elements that are neither 0 nor 1.0 (0.5 = 0x3F00, 2.0 = 0x4000, -0.0 = 0x8000, -1.0 = 0xBF80, NaN = 0x7FC0)
    for v in (0x3F00, 0x4000, 0x8000, 0xBF80, 0x7FC0, 0x0001):
        p = plane.copy()
        p[[7, 1234, p.size - 1]] = v
        assert XC.bad_elements(p).tolist() == [7, 1234, p.size - 1] and XC.pack_plane(p)[1]
    assert XC.bad_elements(plane).size == 0
    # 1.0 in bf16 is 0x3F80: the top half of the fp32 bits
    assert int(np.array([1.0], F32).view(np.uint32)[0] >> 16) == XC.ONE_BF16
    assert np.array_equal(UC.encode_planes(np.ones((2, 1), F32), 64, terms=1)[:2], [XC.ONE_BF16] * 2)


def test_expand_is_the_inverse_of_a_host_side_pack():
    V, H, B = 130, 36, 40
    L = XC.block_layout(V, H, B)
    g = np.random.Generator(np.random.PCG64(6))
    full = g.integers(0, 256, L["fb_bytes"]).astype(np.uint8)
    x = (g.random((B, V)) > 0.6).astype(F32)
    n = V * L["Bp"] * 2
    for name in ("vis_tr0", "vis_tr1"):
        full[L[name]: L[name] + n] = UC.encode_planes(x if name == "vis_tr0" else 1 - x, L["Bp"], terms=1).view(np.uint8)
    for binary in (True, False):
        w = XC.wire_layout(V, H, B, binary)
        assert w["compact_bytes"] % 256 == 0 and w["head_bytes"] % 16 == 0 and w["c_vneg"] == w["head_bytes"] == L["vis_tr0"]
        assert w["compact_bytes"] == w["head_bytes"] + XC.up(w["nb"]) + (XC.up(w["nb"]) if binary else XC.up(3 * n)) + 256
        compact = np.full(w["compact_bytes"], 0xFF, np.uint8)
        compact[: w["head_bytes"]] = full[: w["head_bytes"]]
        compact[w["c_vneg"]: w["c_vneg"] + w["nb"]] = XC.pack_plane(full[L["vis_tr1"]: L["vis_tr1"] + n].view(np.uint16))[0]
        if binary:
            compact[w["c_vpos"]: w["c_vpos"] + w["nb"]] = XC.pack_plane(full[L["vis_tr0"]: L["vis_tr0"] + n].view(np.uint16))[0]
        else:
            compact[w["c_vpos"]: w["c_vpos"] + 3 * n] = full[L["vis_tr0"]: L["vis_tr0"] + 3 * n]
        back = XC.expand(compact, V, H, B, binary)
        assert np.array_equal(back[: L["vis_tr0"] + (n if binary else 3 * n)], full[: L["vis_tr0"] + (n if binary else 3 * n)])
        assert np.array_equal(back[L["vis_tr1"]: L["vis_tr1"] + n], full[L["vis_tr1"]: L["vis_tr1"] + n])
        if binary:
            assert (back[L["vis_tr0"] + n: L["vis_tr0"] + 3 * n] == 0xFF).all()
            assert not XC.with_zero_terms(back, V, H, B)[L["vis_tr0"] + n: L["vis_tr0"] + 3 * n].any()


def _phases(g, B, V, H):
    return ((g.random((B, V)) > 0.7).astype(F64), g.random((B, H)), (g.random((B, V)) > 0.5).astype(F64), g.random((B, H)))


@pytest.mark.parametrize("B,n", [(40, 2), (130, 3), (200, 2)])
def test_reference_update_is_the_same_from_shard_sums_and_the_tail_agrees_with_stats64(B, n):
    V, H = 300, 45
    ph = _phases(np.random.Generator(np.random.PCG64(B)), B, V, H)
    whole = UC.stats64([ph])
    parts = UC.stats64([tuple(a[lo:hi] for a in ph) for lo, hi in XC.shards(B, n)])
    for k in whole:
        np.testing.assert_allclose(parts[k], whole[k], rtol=1e-13, atol=1e-11)
    st = UC.params(V, H)
    for sp in (False, True):
        a, b = (UC.ref_update(st, s, XC.LR, XC.MOM, XC.WD, B, sp) for s in (whole, parts))
        for k in UC.KEYS:
            np.testing.assert_allclose(a[k], b[k], rtol=1e-13, atol=1e-15)
    t = XC.tail64(whole)
    vp, hp, vn, hn = ph
    np.testing.assert_allclose(t["dc"], hp.sum(0) - hn.sum(0), rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(t["db"], vp.sum(0) - vn.sum(0), rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(t["sp"], hp.sum(0), rtol=1e-13)
    # the bias update ref_update makes from stats64 is the one apply_delta makes from the tail
    lr, n_ = F64(F32(XC.LR)), F64(B)
    ref = UC.ref_update(st, whole, XC.LR, XC.MOM, XC.WD, B, True)
    hb_m = F64(F32(XC.MOM)) * st["hb_m"].astype(F64) + lr * t["dc"] / n_ - lr * (t["sp"] / n_ - F64(F32(UC.SPARSITY_TARGET)))
    np.testing.assert_allclose(ref["hb_m"], hb_m, rtol=1e-12, atol=1e-15)


def test_synthetic_statistics_pack_what_their_float64_sums_say():
    c = next(c for c in XC.delta_cases() if c["synthetic"])
    packed, s = XC.synthetic_stats(c)
    p = XC.split_packed(packed, c["V"], c["H"])
    t = XC.tail64(s)
    assert np.array_equal(p["dW"], s["dW"].astype(F32)) and packed.dtype == F32
    np.testing.assert_allclose(p["dc"], t["dc"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(p["db"], t["db"], rtol=1e-12, atol=1e-12)
    assert np.array_equal(p["sp"], t["sp"].astype(F32))
