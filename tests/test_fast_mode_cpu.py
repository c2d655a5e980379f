"""CPU: the case table of test_fast_mode_gpu.py (fast_cases.py) -- seed margins, the discrimination condition, the reach of the `<1>`
instantiations and the agreement of its route mirrors with route_cases / cd_cases / rowoffset_cases.  No GPU, no engine."""
import numpy as np
import pytest

import cd_cases as CC
import fast_cases as FC
import route_cases as RC
import rowoffset_cases as RO

F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731


def test_case_table_is_well_formed():
    cs = FC.cases()
    assert len({c["id"] for c in cs}) == len(cs)
    assert all(c["mode"] == "fast" and c["id"].startswith("fast-") for c in cs)
    assert set(FC.SEEDS) <= {c["id"] for c in cs if FC.has_draws(c)}, "SEEDS names a case that does not exist or does not draw"
    assert max(c["B"] for c in cs) <= 256 and all(c["B"] <= 130 or c["route"]["down"] in ("down_chunks4", "down_tiled") for c in cs if "route" in c)
    up = FC.cases("up")
    assert {c["route"]["up"] for c in up} == set(RC.UP_ROUTES)
    for fam in RC.UP_ROUTES:
        mine = [c for c in up if c["route"]["up"] == fam and c["kind"] == "up"]
        if fam == "stream_bits":      # only forward(data_binary=True) gives the caller's bit plane to a single propagation
            assert [c["kind"] for c in up if c["route"]["up"] == fam] == ["forward", "forward"]
            continue
        assert {c["T"] for c in mine} == set(RC.TEMPS) and {c["sample"] for c in mine} == {False, True}, fam
        assert {c["operand"] for c in mine} == {"real", "mixed", "binary"} and {c["B"] for c in mine} >= {1, 7, 66, 130}, fam
        assert {c["route"]["up_epilogue"] for c in mine} == {"lean", "general"}, fam
    down = FC.cases("down")
    assert {c["route"]["down"] for c in down} == {"down_fused", "down_chunks2", "down_chunks4", "down_tiled"}
    for fam in ("down_fused", "down_chunks2", "down_chunks4", "down_tiled"):
        mine = [c for c in down if c["route"]["down"] == fam]
        assert {c["T"] for c in mine} == set(RC.TEMPS) and {c["logits_only"] for c in mine} == {0, 1}, fam
        assert {len(c["groups"]) for c in mine} >= {0, 1} and {c["route"]["down_epilogue"] for c in mine} == {"lean", "general"}, fam
    assert {c["H"] % 4 == 0 for c in down if c["route"]["down"] == "down_fused"} == {True, False}
    assert any(c["V"] == RC.CHAIN_V and c["groups"] == RC.CHAIN_GROUPS for c in down)
    gibbs = FC.cases("gibbs")
    assert {(c["route_name"], c["sample_h"]) for c in gibbs} == {(r[0], s) for r in FC.GIBBS_ROUTES for s in (True, False)}
    assert all(c["operand"] == "mixed" and c["sample_v"] == c["sample_h"] for c in gibbs)
    cd = FC.cases("pass")
    assert {(c["route_name"], c["data"], c["hint"]) for c in cd} == {(r[0], k, h) for r in CC.ROUTES for k, h in FC.CD_COMBOS}
    assert {c["route_name"] for c in FC.cases("seq")} == {r[0] for r in CC.ROUTES} and {c["k"] for c in cd} == {1, 2}


def test_every_one_term_instantiation_is_reached():
    got = {}
    for c in FC.cases():
        for inst in FC.reached(c):
            got.setdefault(inst, c["id"])
    missing = [r for r in FC.REQUIRED if r not in got]
    assert not missing, f"no FAST case runs {missing}"
    for inst in FC.REQUIRED:
        print(inst, "<-", got[inst])


def test_route_mirrors_agree_with_the_parity_tables():
    parity = {c["id"]: c for c in RC.cases()}
    for c in FC.cases("up") + FC.cases("down"):
        p = parity.get(c["id"][len("fast-"):])
        if p is not None:
            assert c["route"] == p["route"] and c["opts"] == p["opts"] and (c["V"], c["H"], c["B"]) == (p["V"], p["H"], p["B"]), c["id"]
        elif c["kind"] == "up":      # a ragged batch: the route of the same shape, temperature and sampling in route_cases
            twin = next(q for q in RC.cases("up") if (q["V"], q["H"], q["opts"], q["T"], q["sample"], q["kind"]) == (c["V"], c["H"], c["opts"], c["T"], c["sample"], "up"))
            assert c["route"] == twin["route"], c["id"]
        else:                        # the joint layer: gemm_down_fused as 1040 x 36 (Vpad < 4096), the same epilogue rule
            twin = next(q for q in RC.cases("down") if (q["V"], q["H"], q["B"], q["T"], q["logits_only"], bool(q["groups"])) == (1040, 36, 33, c["T"], c["logits_only"], bool(c["groups"])))
            assert c["route"] == twin["route"], c["id"]
    for c in FC.cases("gibbs"):
        name, V, H, opts, groups = next(r for r in FC.GIBBS_ROUTES if r[0] == c["route_name"])
        if c["sample_h"]:
            assert c["route"] == RO._gibbs(name, V, H, opts, groups, c["B"], 0, "exact")["route"], c["id"]
        else:      # route_cases' mean-field Gibbs steps name the same epilogues for the same up family and groups
            for q in RC.cases("gibbs"):
                if not q["sample_h"] and not q["sample_v"] and q["route"]["up"] == c["route"]["up"] and bool(q["groups"]) == bool(groups):
                    assert c["route"] == q["route"], (c["id"], q["id"])
    for c in FC.cases("pass"):
        r = CC.route_of(c["V"], c["H"], c["opts"], c["groups"], c["B"])
        assert (c["expect"], c["expect_cd"]) == CC.expect_of(r, c["hint"]) and c["r"] == r, c["id"]
    for c in FC.cases("seq"):
        assert c["steps"] == CC.by_id(c["id"][len("fast-"):])["steps"], c["id"]
    pre, grp = FC.cases("step")
    assert pre["steps"] == CC.by_id("seq-step-1040x36-B130")["steps"][:FC.STEPS] and [s["expect_cd"]["slot"] for s in pre["steps"]] == [0, 1, 2]
    assert all(s["expect_cd"]["next"] == "k1_stream" for s in pre["steps"]) and grp["groups"] == CC.GROUP
    for s in grp["steps"]:
        assert (s["expect"], s["expect_cd"]) == CC.expect_of(CC.route_of(grp["V"], grp["H"], grp["opts"], grp["groups"], grp["B"]), s["hint"])
        assert s["expect"]["finish_groups"] and s["expect_cd"]["next"] == "none"
    ch, = FC.cases("chain")      # route_cases' wide chains name the same last pair: mean-field on the default route, a sampled h through k2_stream
    assert ch["route"] == next(q for q in RC.cases("chain") if q["call"] == "cg" and q["variant"] == "default")["route"]
    assert (ch["V"], ch["groups"], ch["opts"]) == (RC.CHAIN_V, RC.CHAIN_GROUPS, {"no_chain_kernel": 1})
    assert [(s["sample_h"], s["vmode"]) for s in ch["steps"]] == [(1, 1), (1, 1), (0, 0)]


def test_midpoint_operand_sits_beside_the_rounding_midpoints():
    c = FC.FREE
    x = FC.midpoint_operand(c["B"], c["V"], c["H"])
    lo = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32).astype(F64)
    frac = (x.astype(F64) - lo) / 2.0 ** -8      # position inside the bf16 interval [lo, lo + ulp)
    assert ((x >= 0.5) & (x < 1)).all() and set(np.round(frac, 6).ravel()) == {0.5 - 2.0 ** -6, 0.5 + 2.0 ** -6}
    r = RO.rne_bf16(x).astype(F64)
    assert np.array_equal(r > x, frac > 0.5) and 0.2 < float((frac > 0.5).mean()) < 0.8


@pytest.mark.parametrize("c", [c for c in FC.cases() if FC.has_draws(c)], ids=IDS)
def test_pinned_seed_keeps_every_decision_clear_of_rounding(c):
    bm, cm = FC.margins(c)
    print(f"{c['id']}: seed {c['seed']}, Bernoulli margin {bm:.2e}, categorical {cm:.2e}")
    assert bm >= FC.MARGIN and cm >= FC.MARGIN, f"{c['id']}: seed {c['seed']} leaves margins {bm:.2e} / {cm:.2e}: replace it (python tests/fast_cases.py)"


def _gap(fast, exact, bound, what, cid):
    d = float(np.abs(fast - exact).max())
    print(f"{cid}: {what}: FAST twin vs parity reference {d:.2e} = {d / bound:.0f} bounds")
    assert d >= FC.DISCRIMINATION * bound, f"{cid}: {what}: the FAST twin is only {d / bound:.1f} bounds from the parity reference: the case cannot tell the modes apart"


@pytest.mark.parametrize("c", FC.cases(), ids=IDS)
def test_fast_twin_is_far_from_the_parity_reference(c):
    """No weight matrix here is bf16-exact, so every case must be able to tell FAST from parity arithmetic on what it compares."""
    assert not np.array_equal(RO.fast_weights(c["V"], c["H"]), RC.params(c["V"], c["H"])[0])
    if c["kind"] in ("up", "forward"):
        p, _, e, _ = FC.twin_up(c)
        _gap(p, e, RC.prob_bound(c["T"]), "p(h|v)", c["id"])
    elif c["kind"] == "down":
        ref, raw, e = FC.twin_down(c)
        _gap(ref, e, RC.logit_bound(raw, c["T"]) if c["logits_only"] else RC.prob_bound(c["T"]), "logits" if c["logits_only"] else "p(v|h)", c["id"])
    elif c["kind"] == "gibbs":
        t = FC.twin_gibbs(c)
        _gap(t["h_prob"], t["exact_h_prob"], RC.prob_bound(1.0), "p(h|v)", c["id"])
        _gap(t["v_prob"], t["exact_v_prob"], RC.prob_bound(1.0), "p(v|h)", c["id"])
    elif c["kind"] == "chain":
        for i, t in enumerate(FC.twin_chain(c)[0]):
            _gap(t["h_prob"], t["exact_h_prob"], RC.prob_bound(1.0), f"p(h|v) of step {i}", c["id"])
    elif c["kind"] == "free":
        F, bound, Fe = FC.twin_free(c)
        _gap(F, Fe, float(bound.max()), "free energy", c["id"])
    elif c["kind"] == "sqerr":
        _, _, mse, bound, mse_e = FC.twin_sqerr(c)
        _gap(mse, mse_e, float(bound.max()), "decode error", c["id"])
    else:      # a CD pass: the probabilities of both phases and dW, the packed part that multiplies two rounded operands
        for t in (FC.twin_steps(c) if c["kind"] == "step" else FC.twin_cd(c))[0]:
            _gap(t["hpos"], t["exact_hpos"], RC.prob_bound(1.0), "P+", c["id"])
            _gap(t["hneg"], t["exact_hneg"], RC.prob_bound(1.0), "P-", c["id"])
            dW = FC.stats_twin(t, FC.r64(t["hpos"].astype(F32)), FC.r64(t["hneg"].astype(F32)))["dW"]
            _gap(dW, FC.parity_dW(t), float(CC.stats_bound(c["B"], dW).max()), "dW", c["id"])


def test_half_ulp_is_the_rounding_error_of_bf16():
    g = np.random.Generator(np.random.PCG64(5))
    y = np.concatenate([g.random(20000, dtype=F32), F32(2.0) ** -g.integers(0, 20, 2000).astype(F32), [F32(0)]]).astype(F32)
    err = np.abs(RO.rne_bf16(y).astype(F64) - y.astype(F64))
    h = FC.half_ulp_bf16(y)
    assert (err <= h).all() and (err[y > 0] / h[y > 0]).max() > 0.99
    assert FC.half_ulp_bf16(F32(0.5)) == 2.0 ** -9 and FC.half_ulp_bf16(F32(0.75)) == 2.0 ** -9 and FC.half_ulp_bf16(F32(1.0)) == 2.0 ** -8


def test_rounding_is_to_nearest_even_not_toward_zero():
    """What the twin rounds with: a real operand differs from its truncation in about half of its elements."""
    x = RC.operand("real", 33, 1040)
    trunc = (x.view(np.uint32) & 0xFFFF0000).view(F32)
    r = RO.rne_bf16(x)
    assert 0.4 < float((r != trunc).mean()) < 0.6 and (np.abs(r.astype(F64) - x) <= np.abs(trunc.astype(F64) - x)).all()
    tie = np.array([0x3F808000, 0x3F818000], np.uint32).view(F32)      # halfway cases: to the even neighbour
    assert list(RO.rne_bf16(tie).view(np.uint32)) == [0x3F800000, 0x3F820000]
