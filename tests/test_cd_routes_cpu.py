"""CPU: the case table of test_cd_routes_gpu.py (cd_cases.py) -- every seed is pinned with the margin the GPU comparison relies on, the
float64 reference takes the fp32 oracle's decisions and gives its statistics, the Python mirror of make_route reaches every value of
every CD-only field of Route, and every route meets every batch size, data kind, hint and CD depth."""
import numpy as np
import pytest

import cd_cases as CC

IDS = lambda c: c["id"]      # noqa: E731
F64 = np.float64


@pytest.fixture(scope="module")
def oracle_runs():
    """case id -> (oracle results per step, Bernoulli margin, categorical margin), each case run once."""
    return {c["id"]: CC.run_oracle(c) for c in CC.cases()}


def test_every_seed_keeps_the_margin_at_every_step(oracle_runs):
    for c in CC.cases():
        _, bm, cm = oracle_runs[c["id"]]
        assert bm >= CC.MARGIN and cm >= CC.MARGIN, f"{c['id']}: seed {c['seed']} leaves margins {bm:.2e} / {cm:.2e}: pin another (python tests/cd_cases.py)"
        assert c["seed"] >= 1


def test_seed_table_is_what_the_rule_prints():
    assert CC.pinned_seeds() == CC.SEEDS
    assert set(CC.SEEDS) <= {c["id"] for c in CC.cases()}, "SEEDS names a case that no longer exists"


def _check_against_oracle(cid, ref, s):
    V, H = ref["x"].shape[1], ref["hpos"].shape[1]
    assert np.array_equal(ref["v"], s["v"]), f"{cid}: {int((ref['v'] != s['v']).sum())} visible decisions differ from the oracle's"
    assert float(np.abs(ref["hpos"] - s["pos_h"]).max()) < 1e-5 and float(np.abs(ref["hneg"] - s["h_prob"]).max()) < 1e-5
    assert float(np.abs(ref["v_prob"] - s["v_prob"]).max()) < 1e-5
    got = np.concatenate([(s["pos_assoc"].astype(F64) - s["neg_assoc"]).reshape(-1), s["pos_h_sum"].astype(F64) - s["neg_h_sum"],
                          s["data_sum"].astype(F64) - s["v_sum"], s["pos_h_sum"].astype(F64), [s["sq_err"].astype(F64).sum()]])
    want = CC.packed64(ref)
    assert got.shape == want.shape == (V * H + 2 * H + V + 1,)
    # the oracle sums in fp32 (numpy's pairwise sums and BLAS): its own error next to float64 is that of update_cases.STATS_TOL
    # on pos and neg separately, i.e. on max(|pos|, |neg|) <= B, not on the difference
    B = ref["x"].shape[0]
    tol = CC.STATS_TOL["rel"] * np.maximum(np.abs(want), B) + CC.STATS_TOL["atol"]
    tol[-1] = CC.STATS_TOL["rel"] * abs(want[-1]) + CC.STATS_TOL["atol"] + 1e-6 * abs(want[-1])      # fp32 elements squared, then summed
    assert (np.abs(got - want) <= tol).all(), f"{cid}: statistics differ from the oracle's by {float((np.abs(got - want) / tol).max()):.2f} x tol"


@pytest.mark.parametrize("c", CC.cases("pass"), ids=IDS)
def test_reference_takes_the_oracles_decisions(c, oracle_runs):
    (s,), _, _ = oracle_runs[c["id"]]
    ref = CC.ref_cd(c)
    # the positive-phase sample: the oracle keeps only what follows from it, so recompute it from the oracle's P+ and the same draw
    u = CC.PhiloxStream(c["seed"]).uniform((c["B"], c["H"]))
    assert np.array_equal(ref["h"], (s["pos_h"] > u).astype(F64)), f"{c['id']}: hidden decisions differ from the oracle's"
    for (gs, ge), idx in zip(c["groups"], ref["picks"]):
        assert np.array_equal(idx, s["v"][:, gs:ge].argmax(1)) and (s["v"][:, gs:ge].sum(1) == 1).all(), f"{c['id']}: categorical picks"
    _check_against_oracle(c["id"], ref, s)


@pytest.mark.parametrize("c", CC.cases("seq", "stats"), ids=IDS)
def test_reference_takes_the_oracles_decisions_at_every_step_of_a_sequence(c, oracle_runs):
    res, _, _ = oracle_runs[c["id"]]
    st = CC.state(c["route_name"])
    for i, s in enumerate(res):
        _check_against_oracle(f"{c['id']} step {i}", CC.ref_seq_step(c, i, st, i * c["draws"]), s)


def test_route_mirror_reaches_every_value_of_every_cd_only_field():
    passes, seqs = CC.cases("pass"), CC.cases("seq")
    routes = [c["r"] for c in passes + seqs]
    for field in ("k2s_cd", "vbits", "neg_rm", "next_on_k1", "rides", "adaptive_ok", "adaptive_next", "prefetch", "k1s", "k1s_real", "up_fused"):
        assert {bool(r[field]) for r in routes} == {True, False}, f"no case has both values of {field}"
    steps = [s for c in seqs for s in c["steps"]]
    assert {s["expect_cd"]["next"] for s in steps} == set(CC.CARRIERS), "a carrier of the preparation is not reached"
    assert {s["expect_cd"]["adaptive"] for s in steps} == {True, False}
    assert {s["expect_cd"]["slot"] for s in steps} == {0, 1, 2}
    assert {s["form"] for s in steps} == {None, "one", "three", "item"}, "a slot form is not reached"
    # a slot of every form is consumed under every hint it can be prepared for
    for form, hint in (("one", "binary"), ("item", "unknown"), ("three", "unknown"), ("three", "real")):
        assert any(a["form"] == form and a["next_hint"] == hint and b["expect_cd"]["slot"] == a["next_slot"]
                   for c in seqs for a, b in zip(c["steps"], c["steps"][1:])), (form, hint)
    assert {c["expect_cd"]["pos_up"] for c in passes} == set(CC.UP_FAMILIES), "an up family never runs the positive phase"
    # the negative-phase K1 reads a sample: every family but stream_real, which ends a pass only as the forward of cd_step
    assert {c["expect_cd"]["last_up"] for c in passes} == {c["expect"]["up"] for c in passes} == set(CC.UP_FAMILIES) - {"stream_real"}
    fwd = {CC.expect_of(c["r"], c["hint"], forward=True)[0]["up"] for c in CC.one_per_route()}
    assert "stream_real" in fwd and fwd == {CC.data_up(c["r"], c["hint"]) for c in CC.one_per_route()}
    for key in ("first_down",):
        assert {c["expect_cd"][key] for c in passes} == set(CC.DOWN_FAMILIES)
    assert {(c["expect"]["down"], c["expect"]["down_epilogue"]) for c in passes} == {
        ("k2_stream", "lean"), ("k2_stream", "general"), ("down_fused", "lean")}      # down_fused is general only with a group, which takes k2_stream here
    assert {c["expect"]["finish_groups"] for c in passes} == {True, False}
    # the data operand: a bit plane read whole, per item, as bf16 terms; vis_rm[0] needed or not
    assert {(c["r"]["k1s"], c["hint"]) for c in passes} >= {(True, h) for h in CC.HINTS} | {(False, h) for h in CC.HINTS}
    # vbits from the tile height alone
    by = {c["route_name"]: c["r"] for c in passes}
    assert by["1040x36-no_bits-rows8"]["vbits"] and not by["1040x36-no_bits-rows12"]["vbits"]
    assert by["1040x36"]["k1s_ks"] == 5 and by["1040x36"]["adaptive_ok"] and not by["1100x12"]["adaptive_ok"]
    assert CC.smallest_non_adaptive(12) <= 1100 and CC.route_of(1576, 12)["adaptive_ok"] is False
    assert not CC.route_of(1437, 32)["adaptive_ok"] and not CC.route_of(2116, 28)["adaptive_ok"]      # the layers tools/stress_parity.py found


def test_ids_are_unique_and_every_route_meets_every_batch_kind_hint_and_depth():
    cs = CC.cases()
    assert len({c["id"] for c in cs}) == len(cs)
    passes = CC.cases("pass")
    assert 120 <= len(passes) <= 160, len(passes)
    for name, *_ in CC.ROUTES:
        mine = [c for c in passes if c["route_name"] == name]
        assert {c["B"] for c in mine} == set(CC.BATCHES), name
        assert {c["data"] for c in mine} == set(CC.KINDS), name
        assert {c["hint"] for c in mine} == set(CC.HINTS), name
        assert {c["k"] for c in mine} == set(CC.DEPTHS), name
        assert all(c["hint"] != "binary" or c["data"] == "binary" for c in mine)
        assert sum(c["kind"] == "seq" and c["route_name"] == name for c in cs) == (1 if mine[0]["groups"] else 2)
    assert {c["route_name"] for c in CC.one_per_route()} == {n for n, _, _, _, g in CC.ROUTES if not g}
