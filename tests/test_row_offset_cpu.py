"""CPU: the case table of test_row_offset_gpu.py (rowoffset_cases.py) is sound before any kernel is involved.  Every pinned seed keeps
the oracle's decisions clear of rounding over the whole case (all four shards and the whole batch, every step); the float64
references at an offset take the fp32 oracle's decisions and agree with it, and with the engine double of tests/oracle_engine.py,
within the bounds the GPU file asserts; the shards' float64 statistics add up to the whole batch's, which is the promise a shard's
row0 keeps; the mirror of finish_lean says what host_prop.hpp says; and every route meets every residue and every batch."""
import itertools

import numpy as np
import pytest
import torch

import cd_cases as CC
import parity_cases as P
import route_cases as RC
import rowoffset_cases as RO
from oracle.draws import PhiloxStream

IDS = lambda c: c["id"]      # noqa: E731
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def oracle_runs():
    """case id -> (oracle results, Bernoulli margin, categorical margin), each case run once."""
    return {c["id"]: RO.run_oracle(c) for c in RO.cases()}


@pytest.fixture(scope="module")
def double():
    from oracle_engine import OracleEngine
    return OracleEngine()


# ---- seeds ---------------------------------------------------------------------------------------------------------------------------------
def test_every_seed_keeps_the_margin_over_the_whole_case(oracle_runs):
    for c in RO.cases():
        _, bm, cm = oracle_runs[c["id"]]
        assert bm >= RO.MARGIN and cm >= RO.MARGIN, f"{c['id']}: seed {c['seed']} leaves margins {bm:.2e} / {cm:.2e}: pin another (python tests/rowoffset_cases.py)"
        # (noisy_meanfield_annealed draws normals alone: no Bernoulli decision, no margin)
        assert (np.isfinite(bm) or c.get("call") == "nmf-mu") and c["seed"] >= 1, f"{c['id']} takes no decision"
    for c in RO.cases("gibbs") + RO.cases("shards"):
        assert np.isfinite(oracle_runs[c["id"]][2]) == bool(c["groups"]), c["id"]
    pc = RO.pt_case()
    assert RO.pt_ok(pc, RO.pt_run(pc, pc["seed"]))
    for name in RO.REVERSE_NAMES:
        rc = RO.reverse_case(name)
        assert RO.reverse_ok(*RO.reverse_run(rc, rc["seed"])[1:]), name


def test_seed_table_is_what_the_rule_prints():
    assert RO.pinned_seeds() == RO.SEEDS
    known = {c["id"] for c in RO.cases()} | {"pt-groups-m5"} | {f"reverse-{n}" for n in RO.REVERSE_NAMES}
    assert set(RO.SEEDS) <= known, "SEEDS names a case that no longer exists"


# ---- the mirror ------------------------------------------------------------------------------------------------------------------------------
def test_finish_lean_mirror_is_the_function_of_host_prop():
    """Every combination of the six terms against the expression of host_prop.hpp:89-92 written out once more, literally."""
    for simple, vmode, out_final, rm, tape, row0 in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1, 2, 3, 4, 5, RO.BIG)):
        want = simple and (vmode == 0 or vmode == 1) and (not out_final) and (not rm) and (vmode == 0 or tape or (row0 & 3) == 0)
        assert RO.finish_lean(simple, vmode, out_final, rm, tape, row0) == bool(want)
    # only the streaming kernels have the instantiation; the others branch on simple alone
    assert RO.epilogue("down_fused", True, 1, False, False, False, 3) == "lean" and RO.epilogue("k2_stream", True, 1, False, False, False, 3) == "general"
    assert RO.epilogue("k2_stream", True, 1, False, False, True, 3) == "lean" and RO.epilogue("stream_bits", True, 0, False, False, False, 3) == "lean"


def test_mirror_is_todays_at_aligned_offsets_and_general_on_sampling_streams_elsewhere():
    for name, V, H, opts, groups in CC.ROUTES:
        for B in (7, 14, 25, 20, 66):
            r = CC.route_of(V, H, opts, groups, B)
            for hint in CC.HINTS:
                today = CC.expect_of(r, hint)
                for row0 in (0, RO.CONTROL, 8, 2 ** 32):
                    assert RO.expect_at(r, hint, row0) == today, (name, row0)
                for row0 in RO.OFFSETS + (RO.BIG,):
                    assert RO.expect_at(r, hint, row0, tape=True) == today, (name, row0)
                    route, cd = RO.expect_at(r, hint, row0)
                    assert cd == today[1] and route["up_epilogue"] == "lean"      # the last K1 draws nothing
                    assert route["down_epilogue"] == ("general" if route["down"] == "k2_stream" else today[0]["down_epilogue"])


def test_table_reaches_the_instantiations_only_an_odd_offset_gives():
    shards = [s for c in RO.cases("shards") for s in c["shards"]]
    # k2_stream general for no reason but the offset; its control; and the sampling k1_stream kernels, bit plane and real
    odd = [s for s in shards if s["lo"] & 3 and s["expect"]["down"] == "k2_stream" and not s["r"]["neg_rm"] and not s["r"]["groups"]]
    assert odd and all(s["expect"]["down_epilogue"] == "general" for s in odd)
    assert any(s["lo"] == 0 and s["expect"]["down"] == "k2_stream" and s["expect"]["down_epilogue"] == "lean" for s in shards)
    samp = {(fam, ep, rider) for s in shards for _, fam, ep, rider in s["sampling"]}
    assert {("stream_bits", "general", False), ("stream_real", "general", False), ("stream_bits", "lean", False)} <= samp
    # the rider-plus-general k1_stream: the hinted CD-2 shard at offset 7 of every route whose preparation rides on K1
    hinted = [c for c in RO.cases("shards") if c["hinted"]]
    assert {c["route_name"] for c in hinted} == {n for n, V, H, o, g in CC.ROUTES if CC.route_of(V, H, o, g, 14)["prefetch"]}
    riders = [c for c in hinted if ("neg0", "stream_bits", "general", True) in c["hinted"]["sampling"]]
    assert riders and all(c["k"] == 2 and c["hinted"]["first"][1]["next"] == "k1_stream" for c in riders)
    assert {c["route_name"] for c in riders} == {c["route_name"] for c in hinted if c["hinted"]["r"]["next_on_k1"]}
    assert {c["hinted"]["first"][1]["next"] for c in hinted} == {"own_launch", "fused_k2", "k1_stream"}
    assert all(c["hinted"]["second"][1]["slot"] == 1 and c["hinted"]["first"][1]["slot"] == 0 for c in hinted)
    # every shard but the first has another shape than the one before it: the host drops the hint
    assert all(s["expect_cd"]["next"] == "none" for s in shards)
    # group C: the tape is lean on the streams where Philox at the offset is general
    for c in RO.cases("lean"):
        if c["expect"]["down"] == "k2_stream" and not c["r"]["neg_rm"]:
            assert (c["expect"]["down_epilogue"], c["expect_tape"]["down_epilogue"]) == ("general", "lean")
    assert {c["same_order"] for c in RO.cases("lean")} == {True, False}


def test_every_route_meets_every_residue_and_every_batch():
    cs = RO.cases()
    assert len({c["id"] for c in cs}) == len(cs)
    g = RO.cases("gibbs")
    assert [n for n, *_ in RO.A_ROUTES] == ["130x72", "1040x36", "1040x36-no_k1s", "1040x36-no_k2s", "1040x36-no_bits", "1040x37", "1040x36-group",
                                           "1040x36-k2s24"]
    for name, *_ in RO.A_ROUTES:
        for mode in ("exact", "fast") if name in RO.A_FAST else ("exact",):
            mine = [c for c in g if c["route_name"] == name and c["mode"] == mode and c["row0"] != RO.BIG]
            assert {c["row0"] for c in mine} == set(RO.OFFSETS) | {RO.CONTROL}, (name, mode)
            assert {c["row0"] & 3 for c in mine} == {0, 1, 2, 3} and {c["B"] for c in mine} == set(RO.A_BATCHES), (name, mode)
    for name in RO.A_UP:
        mine = [c for c in RO.cases("up") if c["route_name"] == name and c["row0"] != RO.BIG]
        assert {c["row0"] & 3 for c in mine} == {0, 1, 2, 3} and {c["B"] for c in mine} == set(RO.A_BATCHES), name
    assert {c["route"]["up"] for c in RO.cases("up")} == {"fused", "stream_real", "partial4", "partial"}
    assert {(c["route"]["up"], c["route"]["down"]) for c in g} == {("fused", "k2_stream"), ("stream_real", "k2_stream"), ("partial4", "k2_stream"),
                                                                  ("stream_real", "down_fused"), ("partial", "down_fused")}
    assert any(c["route"]["finish_groups"] for c in g) and any(c["opts"].get("k2s_rows") == 24 for c in g)
    assert sum(c["row0"] == RO.BIG for c in g) >= 1 and sum(c["row0"] == RO.BIG for c in RO.cases("up")) >= 1
    # group B: every route of cd_cases, both kinds, CD-2 on the routes with a streaming kernel; offsets 0, 3, 1, 2 mod 4
    assert [lo & 3 for lo, _ in RO.SHARDS] == [0, 3, 1, 2] and [hi - lo for lo, hi in RO.SHARDS] == [7, 14, 25, 20]
    for name, V, H, opts, groups in CC.ROUTES:
        mine = [c for c in RO.cases("shards") if c["route_name"] == name]
        want = {(kind, k) for kind in ("binary", "mixed") for k in ((1, 2) if RO.streaming(CC.route_of(V, H, opts, groups, 66)) else (1,))}
        assert {(c["data"], c["k"]) for c in mine} == want, name
    assert {c["route_name"] for c in RO.cases("step")} == set(RO.STEP_ROUTES) and {c["route_name"] for c in RO.cases("factors")} == set(RO.FACTOR_ROUTES)
    assert len(RO.cases("lean")) == 6 and {c["row0"] for c in RO.cases("lean")} == {1, 3}
    d = RO.cases("chain")
    assert {(c["call"], c["variant"], c["row0"]) for c in d} == set(itertools.product(RO.D_CALLS, RO.D_ROUTES, RO.D_OFFSETS))
    assert all(c["B"] == 27 and c["V"] == RC.CHAIN_V for c in d)


def test_pcd_cases_already_sweep_unaligned_replicas_without_a_group_and_the_new_case_adds_one():
    """pt_sweep draws replica r from row r M: pcd_cases has M = 5 x 3 replicas (`odd`), 6, 67 and 3 -- none with a softmax group."""
    import pcd_cases as Cs
    unaligned = {n: v for n, v in Cs.CASES.items() if v[2] % 4 and v[3] >= 2}
    assert Cs.CASES["odd"][2:4] == (5, 3) and set(unaligned) == {"odd", "h130", "rows67", "wide"}
    assert not any(v[4] for v in unaligned.values())
    pc = RO.pt_case()
    assert (pc["M"], pc["R"]) == (5, 3) and pc["groups"] and (pc["V"], pc["H"]) == Cs.CASES["groups"][:2]
    t = RO.pt_run(pc, pc["seed"])
    assert t["accs"].sum() > 0 and (t["tries"] - t["accs"]).sum() > 0, "the case never accepts, or never rejects, an exchange"


# ---- group A against float64 and the engine double -----------------------------------------------------------------------------------------
def _rbm(c, W=None):
    from imdbn.models import RBM
    W0, hb, vb = RC.params(c["V"], c["H"])
    r = RBM(c["V"], c["H"], 0.1, 1e-4, 0.5, softmax_groups=[tuple(g) for g in c["groups"]] or None)
    return P.set_params(r, "cpu", c.get("W", W0) if W is None else W, hb, vb)


@pytest.mark.parametrize("c", RO.cases("gibbs"), ids=IDS)
def test_gibbs_step_oracle_and_double_agree_with_float64_at_the_offset(c, oracle_runs, double):
    from imdbn import engine as E
    r_next, r_prob, r_h, r_hprob = RC.ref_gibbs(c)
    b = RC.prob_bound(1.0)
    rng = E.PhiloxRng(seed=c["seed"], row0=c["row0"])
    via = tuple(P.N(t) for t in double.gibbs_step(_rbm(c), P.T(RC.operand(c["operand"], c["B"], c["V"]), "cpu"), True, True, rng))
    assert rng.offset == RC.gibbs_draws(c)
    for v_next, v_prob, h, h_prob in (oracle_runs[c["id"]][0], via):
        assert np.abs(h_prob - r_hprob).max() <= b and np.abs(v_prob - r_prob).max() <= b
        assert np.array_equal(h, r_h) and np.array_equal(v_next, r_next)
    if c["row0"] == RO.BIG:      # the group index 2^30 fits the counter word: a row cut to 32 bits BEFORE the shift would draw offset 3's rows
        u = PhiloxStream(c["seed"], row0=RO.BIG).uniform((c["B"], c["H"]))
        assert not np.array_equal(u, PhiloxStream(c["seed"], row0=3).uniform((c["B"], c["H"])))
        assert np.array_equal(PhiloxStream(c["seed"], row0=2 ** 34 + 3).uniform((4, 5)), PhiloxStream(c["seed"], row0=3).uniform((4, 5)))
    if c["mode"] == "fast":
        assert c["operand"] == "binary" and np.array_equal(c["W"], RO.rne_bf16(RC.params(c["V"], c["H"])[0]))
        assert not (c["W"].view(np.uint32) & 0xFFFF).any() and np.abs(c["W"] - RC.params(c["V"], c["H"])[0]).max() > 0


@pytest.mark.parametrize("c", RO.cases("up"), ids=IDS)
def test_up_step_oracle_and_double_agree_with_float64_at_the_offset(c, oracle_runs, double):
    from imdbn import engine as E
    ref, ref_s = RC.ref_up(c)
    rng = E.PhiloxRng(seed=c["seed"], row0=c["row0"])
    p2, s2 = double.prop_up(_rbm(c), P.T(RC.operand(c["operand"], c["B"], c["V"]), "cpu"), T=1.0, sample=True, rng=rng)
    for p, s in (oracle_runs[c["id"]][0], (P.N(p2), P.N(s2))):
        assert np.abs(p - ref).max() <= RC.prob_bound(1.0) and np.array_equal(s, ref_s)


def test_offsets_change_the_draws_and_only_through_the_global_row():
    a = PhiloxStream(5, row0=0).uniform((12, 9))
    for row0 in RO.OFFSETS:
        assert np.array_equal(PhiloxStream(5, row0=row0).uniform((12 - row0, 9)), a[row0:])
        n = PhiloxStream(5, row0=0).normal((12, 9))
        assert np.array_equal(PhiloxStream(5, row0=row0).normal((12 - row0, 9)), n[row0:])
    assert not np.array_equal(PhiloxStream(5, row0=1).uniform((4, 9)), a[:4])


# ---- group B: the shards ---------------------------------------------------------------------------------------------------------------------
def _oracle_packed(s):
    return np.concatenate([(s["pos_assoc"].astype(F64) - s["neg_assoc"]).reshape(-1), s["pos_h_sum"].astype(F64) - s["neg_h_sum"],
                           s["data_sum"].astype(F64) - s["v_sum"], s["pos_h_sum"].astype(F64), [s["sq_err"].astype(F64).sum()]])


def _oracle_tol(want, B):
    """test_cd_routes_cpu.py's: the oracle sums pos and neg separately in fp32 (STATS_TOL on max(|.|, B)), squares fp32 elements."""
    tol = CC.STATS_TOL["rel"] * np.maximum(np.abs(want), B) + CC.STATS_TOL["atol"]
    tol[-1] = CC.STATS_TOL["rel"] * abs(want[-1]) + CC.STATS_TOL["atol"] + 1e-6 * abs(want[-1])
    return tol


@pytest.mark.parametrize("c", RO.cases("shards"), ids=IDS)
def test_shard_references_take_the_oracles_decisions_and_add_up_to_the_whole_batch(c, oracle_runs):
    res = oracle_runs[c["id"]][0]
    refs, whole = RO.ref_shards(c)
    for (lo, hi), ref, s in zip(RO.SHARDS + ((0, RO.B_ROWS),), refs + (whole,), res):
        assert np.array_equal(ref["v"], s["v"]), f"{c['id']} rows {lo}:{hi}: visible decisions differ from the oracle's"
        for (gs, ge), idx in zip(c["groups"], ref["picks"]):
            assert np.array_equal(idx, s["v"][:, gs:ge].argmax(1))
        want = CC.packed64(ref)
        assert (np.abs(_oracle_packed(s) - want) <= _oracle_tol(want, hi - lo)).all(), f"{c['id']} rows {lo}:{hi}"
    # what row0 promises: a shard at its offset takes the whole batch's decisions on its rows, so the statistics are linear in the shards
    assert np.array_equal(np.concatenate([r["v"] for r in refs]), whole["v"]) and np.array_equal(np.concatenate([r["h"] for r in refs]), whole["h"])
    total = sum(CC.packed64(r) for r in refs)
    assert np.abs(total - CC.packed64(whole)).max() <= 1e-9 * max(1.0, np.abs(CC.packed64(whole)).max())
    # and a shard keyed from row 0 instead would not
    lo, hi = RO.SHARDS[1]
    assert not np.array_equal(RO.ref_rows(c, lo, hi, row0=0)["h"], refs[1]["h"])


@pytest.mark.parametrize("c", [c for c in RO.cases("shards") if c["k"] == 1 and c["data"] == "mixed"], ids=IDS)
def test_double_cd_stats_shard_sum_is_the_whole_batch(c, double):
    from imdbn import engine as E
    x, st = RO.batch(c), CC.state(c["route_name"])
    r = _rbm(c, W=st["W"])
    parts = [P.N(double.cd_stats(r, P.T(x[lo:hi], "cpu"), c["k"], E.PhiloxRng(seed=c["seed"], row0=lo))).astype(F64) for lo, hi in RO.SHARDS]
    want = CC.packed64(RO.ref_shards(c)[1])
    got = sum(parts)[: want.size]
    assert (np.abs(got - want) <= _oracle_tol(want, RO.B_ROWS) + 3 * 2.0 ** -24 * np.abs(want)).all(), c["id"]


@pytest.mark.parametrize("c", RO.cases("step") + RO.cases("factors") + RO.cases("lean"), ids=IDS)
def test_single_pass_references_take_the_oracles_decisions(c, oracle_runs):
    res = oracle_runs[c["id"]][0]
    ref = RO.ref_rows(c, 0, 0, row0=c["row0"], x=RO.step_batch(c, 0) if c["kind"] == "step" else RO.rows(c))
    assert np.array_equal(ref["v"], res[0]["v"])
    want = CC.packed64(ref)
    assert (np.abs(_oracle_packed(res[0]) - want) <= _oracle_tol(want, c["B"])).all()
    assert len(res) == (RO.STEP_STEPS if c["kind"] == "step" else 1)
    if c["kind"] == "lean":      # the tape of group C: the very uniforms of the stream at the offset
        a, b = PhiloxStream(c["seed"], row0=c["row0"]), PhiloxStream(c["seed"], row0=c["row0"])
        assert np.array_equal(a.uniform((c["B"], c["H"])), b.uniform((c["B"], c["H"]))) and a.offset == b.offset == 1


# ---- group D -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RO.cases("chain"), ids=IDS)
def test_wide_chain_oracle_at_the_offset_differs_from_offset_zero(c, oracle_runs):
    (out, st, draws), bm, cm = oracle_runs[c["id"]]
    assert np.isfinite(np.asarray(out)).all() and draws > 0
    (base, _, draws0), _, _ = RC.run_oracle(dict(c, row0=0))
    assert draws0 == draws and not np.array_equal(np.asarray(out), np.asarray(base)), "the offset does not reach the chain's draws"


def test_reverse_chunks_at_their_offsets_are_the_single_chunk():
    """The twin run chunk by chunk at the chunks' offsets gives the logw of all engine rows in one chunk: the driver's promise."""
    import anneal_oracle as A
    for name in RO.REVERSE_NAMES:
        c = RO.reverse_case(name)
        chunks, _, _ = RO.reverse_run(c, c["seed"])
        x = np.repeat(c["rows"], RO.REVERSE_CHAINS, axis=0)
        one = A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], c["groups"], c["betas"], x, PhiloxStream(c["seed"]))[0]
        assert np.array_equal(chunks.reshape(-1), one) and RO.REVERSE_ROWS * RO.REVERSE_CHAINS <= 64
        assert [s * RO.REVERSE_CHAINS for s in range(0, RO.REVERSE_ROWS, RO.REVERSE_MAX_ROWS // RO.REVERSE_CHAINS)] == [0, 6, 12, 18]
