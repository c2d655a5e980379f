"""CPU-only: the case table of chain_cases.py is sound before any kernel is involved.  Ids are unique, the table covers every path the
chain kernel and its host routing have, every case's expected record follows from the Python restatement of chain_kernel_ok /
run_chain_pair / the rows rule (pinned here on the boundary values), the LDS byte count puts each limit shape on the side it is
named for, the numpy twin of k4_terms reproduces the weights to its stated representation error, and for every PARITY case the
derived bound plus the distance between the decoded-terms reference and plain float64 stays within the project's chain tolerance."""
import numpy as np
import pytest

import chain_cases as CC

F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731
KERNEL, PAIR, PER_LAUNCH = CC.CHAIN_KERNEL, CC.CHAIN_KERNEL_PAIR, CC.CHAIN_PER_LAUNCH


def _by_id(cid):
    return next(c for c in CC.cases() if c["id"] == cid)


def test_ids_are_unique_and_every_case_is_well_formed():
    cs = CC.cases()
    assert len({c["id"] for c in cs}) == len(cs) and {c["group"] for c in cs} == set(CC.GROUPS)
    for c in cs:
        assert set(c["opts"]) <= set(CC.OPTION_DEFAULTS) and c["mode"] in ("parity", "fast") and c["rng"] in ("philox", "tape"), c["id"]
        assert 1 <= len(c["chains"]) <= 2 and all(len(ch["steps"]) == ch["n"] for ch in c["chains"]), c["id"]
        assert c["row0"] == 0 or c["rng"] == "philox", c["id"]
        for s, e in c["groups"]:
            assert 0 <= s < e <= c["V"], c["id"]
        assert c["Dz"] is None or 0 < c["Dz"] <= c["V"], c["id"]
        route, rows, blocks, recs = CC.expected(c)
        assert (route == PER_LAUNCH) == (rows == 0) == (blocks == 0) and recs == CC.n_recs(c["chains"][0]), c["id"]
        if route != PER_LAUNCH:
            assert 1 <= rows <= 16 and blocks == len(c["chains"] if route == PAIR else [0]) * CC.cdiv(CC.batch(c), rows), c["id"]
        if c["mode"] == "fast":
            assert all(CC.on_kernel(c, i) for i in range(len(c["chains"]))), c["id"]


def test_the_restatement_of_the_host_rules_on_their_boundaries():
    ok = lambda n, **kw: CC.kernel_ok(36, 24, kw.pop("groups", ()), "parity", n, kw)      # noqa: E731
    assert [ok(n) for n in (1, 2, 256, 257)] == [False, True, True, False]
    assert not ok(5, groups=((20, 26), (30, 36))) and ok(5, groups=((20, 26),)) and not ok(5, no_chain_kernel=1)
    assert CC.kernel_ok(1024, 24, (), "parity", 5) and not CC.kernel_ok(1025, 24, (), "parity", 5) and not CC.kernel_ok(36, 1025, (), "parity", 5)
    cu = 256
    assert [CC.rows_rule(B, 1, cu) for B in (1, 512, 513, 1024, 1025, 2048, 2049)] == [2, 2, 4, 4, 8, 8, 16]
    assert [CC.rows_rule(B, 2, cu) for B in (256, 257, 512, 513, 1024, 1025)] == [2, 4, 4, 8, 8, 16]
    assert CC.rows_rule(2049, 1, cu, forced=3) == 3
    want = {"steps-n1": (PER_LAUNCH, 0, 0, 1), "steps-n2": (KERNEL, 2, 2, 2), "steps-n256": (KERNEL, 2, 2, 256), "steps-n257": (PER_LAUNCH, 0, 0, 257),
            "steps-n256-baseline": (PER_LAUNCH, 0, 0, 257), "steps-n255-baseline": (KERNEL, 2, 2, 256), "steps-two-groups": (PER_LAUNCH, 0, 0, 4),
            "steps-pair-128+128": (PAIR, 2, 4, 128), "steps-pair-128+129": (KERNEL, 2, 2, 128), "steps-pair-33+7": (PAIR, 2, 4, 33),
            "steps-pair-no_chain_pair": (KERNEL, 2, 2, 5), "steps-no_chain_kernel": (PER_LAUNCH, 0, 0, 5),
            "steps-pair-no_chain_kernel": (PER_LAUNCH, 0, 0, 5), "steps-pair-baseline-a": (PAIR, 2, 4, 5), "steps-pair-baseline-b": (PAIR, 2, 4, 4),
            "steps-pair-1+4": (KERNEL, 2, 2, 1), "auto-single-2c+0": (KERNEL, 2, 256, 2), "auto-single-2c+1": (KERNEL, 4, 129, 2),
            "auto-single-4c+0": (KERNEL, 4, 256, 2), "auto-single-4c+1": (KERNEL, 8, 129, 2), "auto-single-8c+0": (KERNEL, 8, 256, 2),
            "auto-single-8c+1": (KERNEL, 16, 129, 2), "auto-pair-c+0": (PAIR, 2, 256, 2), "auto-pair-c+1": (PAIR, 4, 130, 2)}
    for cid, rec in want.items():
        assert CC.expected(_by_id(cid), cu) == rec, cid
    for cu2 in (64, 304):      # the automatic cases sit on their thresholds whatever the CU count
        assert [CC.expected(_by_id(f"auto-single-{m}c+{a}"), cu2)[1] for m in (2, 4, 8) for a in (0, 1)] == [2, 4, 4, 8, 8, 16]
        assert [CC.expected(_by_id(f"auto-pair-c+{a}"), cu2)[1] for a in (0, 1)] == [2, 4]


def test_table_covers_every_path():
    cs = CC.cases()
    g = {k: CC.cases(k) for k in CC.GROUPS}
    # 1. rows per block: every value on both shapes, single and pair, under Philox; partial last block; odd-start blocks; B = 1; row0
    for V, H in ((36, 24), (150, 48)):
        mine = [c for c in g["rows"] if (c["V"], c["H"]) == (V, H)]
        assert {(c["rows"], len(c["chains"])) for c in mine} >= {(r, n) for r in CC.ROWS for n in (1, 2)}
        for c in mine:
            B, r = CC.batch(c), c["rows"]
            assert c["rng"] == "philox" and c["opts"]["chain_rows"] == r and CC.expected(c)[1] == r
            assert r == 1 or B % r != 0, c["id"]                                            # a partial last block
            assert r % 2 == 0 or CC.cdiv(B, r) >= 3, c["id"]                                # odd rows: an odd-start block and one after it
            kinds = [s for ch in c["chains"] for s in ch["steps"]]
            assert any(s["sigma"] > 0 for s in kinds) and any(s["sample_h"] for s in kinds), c["id"]
            assert {s["vmode"] for s in kinds} >= ({0, 1, 2} if len(c["chains"]) == 1 else {0, 1}), c["id"]
    assert any(CC.batch(c) == 1 and c["rows"] == 2 for c in g["rows"])
    assert {c["rows"] for c in g["rows"] if c["row0"] == 3} == {3, 4} and all(c["groups"] for c in g["rows"] if c["row0"])
    # the automatic rule: both sides of the three thresholds, single and pair
    assert {(c["B"][1], c["B"][2], len(c["chains"])) for c in g["auto"]} == {(m, a, 1) for m in (2, 4, 8) for a in (0, 1)} | {(1, 0, 2), (1, 1, 2)}
    assert all(not c["opts"] and (c["V"], c["H"]) == (36, 24) and all(ch["n"] == 2 for ch in c["chains"]) for c in g["auto"])
    # 2. FAST: every schedule kind on the three shapes, rows 2 and 16, single and pair
    for V, H in ((36, 24), (150, 48), (532, 256)):
        mine = [c for c in g["fast"] if (c["V"], c["H"]) == (V, H)]
        assert {c["chains"][0]["kind"] for c in mine} == set(CC.KINDS) and all(c["mode"] == "fast" for c in mine)
        assert {(c["rows"], len(c["chains"])) for c in mine} == {(2, 1), (2, 2), (16, 1), (16, 2)}
        assert V == 36 or all(c["groups"] for c in mine)
        for kind in CC.KINDS:
            assert {c["rows"] for c in mine if c["chains"][0]["kind"] == kind} == {2, 16}, (V, kind)
            assert {len(c["chains"]) for c in mine if c["chains"][0]["kind"] == kind} == {1, 2}, (V, kind)
    # 3. group geometry
    geo = g["geometry"]
    assert {c["width"] for c in geo} == {1, 3, 8, 13, 16, 32, 256} and {c["where"] for c in geo} == {"end", "start", "middle"}
    assert {(c["width"], c["where"]) for c in geo} >= {(w, p) for w in (1, 3, 8, 13, 16, 32) for p in ("end", "start", "middle")}
    assert any(c["groups"][0][0] == 0 for c in geo) and any(c["groups"][0][1] == c["V"] for c in geo)
    rel = set()
    for c in geo:
        (s, e), Dz = c["groups"][0], c["Dz"]
        rel.add("before" if Dz <= s else ("inside" if Dz < e else ("at_V" if Dz == c["V"] else "after")))
        st = c["chains"][0]["steps"]
        assert {(x["vmode"], x["clamp"]) for x in st} >= {(m, cl) for m in (0, 1, 2) for cl in (True, False)} and any(x["sigma"] > 0 for x in st), c["id"]
        assert all(x["eta"] != 0 for x in st), c["id"]
    assert rel >= {"before", "inside", "at_V"}
    assert {c["rng"] for c in geo} == {"philox", "tape"} and {c["rows"] % 2 for c in geo if c["rng"] == "philox"} == {0, 1}
    assert any(c["width"] == 256 and c["V"] >= 256 and c["rng"] == r for c in geo for r in ("philox", "tape"))
    # 4. GEMM edges: every shape mean-field (two activation terms) and with sampled h (one term)
    for V, H in CC.GEMM_SHAPES:
        assert {c["chains"][0]["kind"] for c in g["gemm"] if (c["V"], c["H"]) == (V, H)} >= {"meanfield", "sampled"}, (V, H)
    tiles = lambda n: CC.cdiv(n, 16)      # noqa: E731
    assert CC.cdiv(24, 32) == 1 and (tiles(64), tiles(128)) == (4, 8) and tiles(144) == 9 and tiles(272) == 17 and 32 % 32 == 0 and 16 % 16 == 0
    # 5. the LDS limit
    assert {(c["V"], c["H"], tuple(c["groups"]), c["mode"]) for c in g["lds"]} == set(CC.LDS_ADMITTED + CC.LDS_REJECTED)
    for c in g["lds"]:
        st = c["chains"][0]["steps"]
        assert CC.batch(c) == 3 and len(st) == 3 and any(x["sample_h"] for x in st) and any(x["sigma"] > 0 for x in st), c["id"]
        assert (CC.expected(c)[0] == KERNEL) == c["admitted"], c["id"]
    # 6. step-count and pair boundaries
    st = g["steps"]
    assert {c["chains"][0]["n"] for c in st if len(c["chains"]) == 1 and not c["chains"][0]["base"]} >= {1, 2, 32, 33, 64, 65, 256, 257}
    assert {(c["chains"][0]["n"], CC.expected(c)[0]) for c in st if c["chains"][0]["base"] and len(c["chains"]) == 1} == {(256, PER_LAUNCH), (255, KERNEL)}
    assert any(len(c["groups"]) == 2 for c in st) and any(c["opts"].get("no_chain_pair") for c in st) and any(c["opts"].get("no_chain_kernel") for c in st)
    assert {tuple(ch["n"] for ch in c["chains"]) for c in st if len(c["chains"]) == 2} >= {(128, 128), (128, 129), (33, 7)}
    assert any(not ch["init_uniform"] for c in st for ch in c["chains"])
    assert {tuple(ch["base"] for ch in c["chains"]) for c in st if len(c["chains"]) == 2} >= {(True, False), (False, True)}
    assert {CC.expected(c)[0] for c in st} == {PER_LAUNCH, KERNEL, PAIR}
    # 7. pitches
    assert any(c["pitch"] > c["H"] for c in g["pitch"]) and any(c["strided"] and c["Dz"] for c in g["pitch"])
    assert {c["mode"] for c in cs} == {"parity", "fast"}


def test_wide_group_rows_reach_both_widths_every_schedule_and_the_lds_edge_of_a_256_wide_group():
    wide = CC.cases("wide")
    chains = [c for c in wide if "admitted" not in c]
    for w in (33, 256):
        mine = [c for c in chains if c["width"] == w]
        assert {(c["chains"][0]["kind"], c["rows"]) for c in mine if len(c["chains"]) == 1} == {(k, r) for k in ("mix", "noisy", "vmode2") for r in (2, 16)}
        assert sum(len(c["chains"]) == 2 for c in mine) == 1 and all(c["groups"][0][1] - c["groups"][0][0] == w for c in mine)
        assert all(CC.expected(c)[0] in (KERNEL, PAIR) and CC.expected(c)[1] == c["rows"] for c in mine)
    assert 33 > 32 and CC.GROUP_WMAX == 256
    # the admission edge at gw = 256, from kernel_ok alone: both gw terms of the byte count are at their largest
    lo, hi = CC.lds_edge(256)
    assert hi == lo + 1 and CC.lds_bytes(lo, 48, 256, "parity") <= CC.K4_LDS_BYTES < CC.lds_bytes(hi, 48, 256, "parity")
    assert (CC.K4_ROWS * 257 * 4, (CC.K4_ROWS // 2) * 256 * 8) == (16448, 16384)
    edge = {c["V"]: c for c in wide if "admitted" in c}
    assert set(edge) == {lo, hi} and edge[lo]["admitted"] and not edge[hi]["admitted"]
    assert CC.expected(edge[lo])[0] == KERNEL and CC.expected(edge[hi])[0] == PER_LAUNCH
    assert lo > CC.lds_edge(5)[0] - 300 and CC.lds_edge(5)[0] > lo      # a narrow group is admitted further out


def test_lds_byte_count_puts_the_limit_shapes_on_their_side():
    L = CC.K4_LDS_BYTES
    assert CC.lds_bytes(1024, 352, 0, "parity") == 155008 <= L and CC.lds_bytes(1024, 352, 5, "parity") == L      # the group case fills it
    assert CC.lds_bytes(1024, 384, 0, "parity") > L and CC.lds_bytes(1024, 352, 6, "parity") > L
    assert CC.lds_bytes(1024, 1024, 0, "fast") <= L < CC.lds_bytes(1024, 1024, 0, "parity")
    assert CC.lds_bytes(532, 256, 32, "parity") == 91520      # the production shape: 2 * 16 * (552 + 264) * 2 + 16 * 545 * 4 + 2112 + 256 + 2048
    for V, H, groups, mode in CC.LDS_ADMITTED:
        assert CC.kernel_ok(V, H, groups, mode, 3), (V, H, groups, mode)
    for V, H, groups, mode in CC.LDS_REJECTED:
        assert not CC.kernel_ok(V, H, groups, mode, 3), (V, H, groups, mode)
    # the arrays the kernel carves (kernels_chain.hpp k4_chain) add up to the host's count and keep the 16-byte alignment of the stage
    for V, H, gw, nt in ((1024, 352, 5, 2), (150, 48, 13, 2), (36, 24, 0, 1)):
        VK, HK = CC.rup(V, 32) + 8, CC.rup(H, 32) + 8
        SP, GW = max(CC.cdiv(H, 16), CC.cdiv(V, 16)) * 16 + 1, gw + 1
        carve = nt * 16 * VK * 2 + nt * 16 * HK * 2 + 16 * SP * 4 + 16 * GW * 4 + 16 * 4 * 4 + 8 * gw * 2 * 4
        assert carve == CC.lds_bytes(V, H, gw, "parity" if nt == 2 else "fast") and (nt * 16 * (VK + HK) * 2) % 16 == 0
        assert 16 * GW <= 16 * SP      # the clipped sampling probabilities reuse the stage


def test_terms_twin_reproduces_the_case_weights():
    seen = set()
    for c in CC.cases():
        key = (c["V"], c["H"], c["mode"])
        if key in seen or c["V"] * c["H"] > 200000 or not all(CC.on_kernel(c, i) for i in range(len(c["chains"]))):
            continue                            # (weights of a chain that runs one launch per half step are never encoded)
        seen.add(key)
        W = CC.problem(c)["W"]
        d, bound = CC.term_error(W, c["mode"])
        assert (d <= bound).all() and d.max() > 0, c["id"]
        ts = CC.terms(W, c["mode"])
        assert len(ts) == (2 if c["mode"] == "parity" else 1)
        if c["mode"] == "parity":
            assert np.array_equal(ts[0], W.astype(np.float16).astype(F32)) and np.abs(ts[1]).max() > 0
        else:
            assert not (ts[0].view(np.uint32) & 0xFFFF).any()
    x = np.array([0.0, 1.0, 0.5, 0.300048828125], F32)
    assert all(np.array_equal(sum(t.astype(F64) for t in CC.terms(x, m)), x.astype(F64)) for m in ("parity", "none"))
    assert len(CC.terms(x, "parity", exact1=True)) == 1
    # bf16 round to nearest even: ties go to the even significand, everything else to the nearest
    t = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF], np.uint32).view(F32)
    assert list(CC.terms(t, "fast")[0].view(np.uint32)) == [0x3F800000, 0x3F820000, 0x3F810000, 0x3F800000]
    assert len(seen) >= 12


@pytest.mark.parametrize("c", CC.cases(), ids=IDS)
def test_bound_and_encoding_stay_within_the_chain_tolerance(c):
    """For PARITY cases: bound + |decoded-terms reference - float64 of the undecoded operands| <= TOL on every probability of every
    half step (the record is the fp32 rounding of the reference itself).  FAST cases only walk the decoded reference."""
    src = CC.source(c)
    prob = CC.problem(c)
    for i in range(len(c["chains"])):
        r = CC.walk(c, prob, i, src, CC.encoding(c, i))
        assert r["final_equal"] and len(r["hid"]) == c["chains"][i]["n"] and len(r["vis"]) == CC.n_recs(c["chains"][i])
        assert r["ratio_h"] <= 1 and r["ratio_v"] <= 1, (c["id"], i, r["ratio_h"], r["ratio_v"])      # fp32 rounding of p: 2^-25 < the bound
        assert 0 < r["bound"] < CC.TOL, (c["id"], i, r["bound"])
        if c["mode"] == "parity":
            assert r["plain"] <= CC.TOL, (c["id"], i, r["plain"], r["bound"])
        assert all(np.isfinite(x).all() for x in r["vis"] + r["hid"])
