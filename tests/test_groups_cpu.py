"""CPU: the case table of test_groups_gpu.py (group_cases.py) is sound before any kernel is involved -- every drawing case's pinned
seed keeps the Bernoulli and categorical margins the exact comparison relies on, the float64 references agree with the fp32 oracle
within the bounds the GPU test uses (and take its decisions), every layout stays inside the engine's limits, every case fits the
size cap, every edge the table is built for is hit, and the comparison itself would notice a one-column slip of the groups or a
categorical taken from the wrong draw."""
import numpy as np
import pytest

import group_cases as GC
import route_cases as RC
from golden_utils import assert_close

F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731


@pytest.fixture(scope="module")
def oracle_runs():
    """case id -> (oracle result, Bernoulli margin, categorical margin), each drawing case run once."""
    return {c["id"]: GC.run_oracle(c) for c in GC.cases() if GC.has_draws(c)}


def test_every_pinned_seed_keeps_both_margins(oracle_runs):
    for c in GC.cases():
        if not GC.has_draws(c):
            continue
        _, bm, cm = oracle_runs[c["id"]]
        assert c["seed"] >= 1 and GC.margins_pass(c, bm, cm), \
            f"{c['id']}: seed {c['seed']} leaves margins {bm:.2e} / {cm:.2e} (needs {GC.MARGIN:.0e} / {GC.case_cat_margin(c):.2e}): pin another (python tests/group_cases.py)"
    assert set(GC.SEEDS) <= {c["id"] for c in GC.cases()}, "SEEDS names a case that no longer exists"
    # the threshold is width-aware, and never below the margin the narrow-group tables use
    assert GC.cat_margin(1) >= RC.MARGIN and GC.cat_margin(5) < GC.cat_margin(65) < GC.cat_margin(256) < 2.5e-5


def test_layouts_stay_inside_the_engines_limits_and_cases_inside_the_size_cap():
    cs = GC.cases()
    assert len({c["id"] for c in cs}) == len(cs)
    for c in cs:
        V, groups = c["V"], c["groups"]
        assert 1 <= len(groups) <= GC.MAX_GROUPS, c["id"]
        for i, (s, e) in enumerate(groups):
            assert 0 <= s < e <= V and e - s <= GC.GROUP_WMAX, c["id"]
            assert all(e <= s2 or e2 <= s for s2, e2 in groups[:i]), f"{c['id']}: overlapping groups"
        assert V * c["H"] * c["B"] <= GC.SIZE_CAP, c["id"]
        assert set(c["opts"]) <= set(GC.OPTION_DEFAULTS) and (c["kind"] == "sample" or c["route"]["finish_groups"] is True), c["id"]


def _crosses(groups, col):
    return any(s < col < e for s, e in groups)


def test_every_edge_of_the_table_is_hit():
    by_layout = {}
    for c in GC.cases():
        if c["kind"] != "sample":
            by_layout.setdefault((c["layout"], c["V"]), []).append(c)
    width = lambda name, V=1040: [e - s for s, e in GC.groups_of(name, V)]      # noqa: E731
    # the element loop of finish_groups (wd * 8 items over 256 threads) wraps first at 33; tails of the 8-wide row loops
    assert width("w33") == [33] and 33 * 8 > 256 >= 32 * 8 and 33 % 8 == 1
    assert width("w65") == [65] and 65 > 64 and 65 % 8 == 1
    assert width("w255") == [255] and 255 % 8 == 7 and width("w256") == [256] == [GC.GROUP_WMAX] and 256 % 8 == 0
    four = GC.groups_of("four", 1040)
    assert len(four) == 4 and four[0][0] == 0 and four[1][1] == four[2][0] and four[3] == (1039, 1040)
    assert _crosses(four, 64) and _crosses(four, 128) and four[2][1] - four[2][0] == 256
    mid = GC.groups_of("three-mid", 1040)
    assert len(mid) == 3 and all(e < 1040 for _, e in mid) and _crosses(mid, 1024)
    w4100, f4100 = GC.groups_of("w256", 4100), GC.groups_of("four", 4100)
    assert w4100[0][1] == 4100 and 4100 - 128 * (4100 // 128) == 4 and w4100[0][1] - w4100[0][0] == 256
    assert _crosses(f4100, 2048) and f4100[3] == (4099, 4100) and f4100[1][1] == f4100[2][0] and len(f4100) == 4
    # every layout on every route it fits
    kinds = lambda key: {(c["kind"], c["route"]["down"]) for c in by_layout[key]}      # noqa: E731
    for name in GC.NARROW:
        assert kinds((name, 1040)) >= {("down", "down_fused"), ("gibbs", "k2_stream"), ("gibbs", "down_fused")}, name
        downs = [c for c in by_layout[(name, 1040)] if c["kind"] == "down"]
        assert {c["H"] for c in downs} == {36, 37} and {c["T"] for c in downs} == set(GC.TEMPS), name
        g = [c for c in by_layout[(name, 1040)] if c["kind"] == "gibbs" and c["rng"] == "philox"]
        assert {(c["sample_h"], c["route"]["down"]) for c in g} == {(True, "k2_stream"), (True, "down_fused"), (False, "down_fused")}, name
    for name in GC.WIDE:
        want = {(k, r) for k in ("down", "gibbs") for r in ("down_chunks2", "down_chunks4", "down_tiled")}
        assert kinds((name, 4100)) == want, name
        assert {(c["route"]["down"], c["B"]) for c in by_layout[(name, 4100)]} == {("down_chunks2", 128), ("down_chunks4", 256), ("down_tiled", 128)}
    # group index 3 draws, trains and is replayed; the tape case has four groups
    assert any(len(c["groups"]) == 4 and c["kind"] == k for c in GC.cases() for k in ("gibbs",))
    tape = [c for c in GC.cases("gibbs") if c["rng"] == "tape"]
    assert len(tape) == 1 and len(tape[0]["groups"]) == 4
    train = GC.cases("train")
    assert {(c["layout"], c["B"], c["k"]) for c in train} == {(lay, B, k) for lay in ("w256", "four") for B in (33, 130) for k in (1, 2)}
    assert all(c["draws"] == 1 + c["k"] * (2 + len(c["groups"])) for c in train)
    assert {(c["rng"], c["B"]) for c in GC.cases("sample")} == {(r, B) for r in ("philox", "tape") for B in (1, 64, 65)}
    # the clamped mask splits the 65-wide group: its first half clamped, the rest free; the one falls on either side
    for c in GC.cases("chain"):
        vk, km, mu = GC.chain_inputs(c)
        (s, e), = c["groups"]
        assert e - s == 65 and km[:, s:s + 32].all() and not km[:, s + 32:e].any() and (mu is not None) == c["mu"]
        assert {int(x) for x in vk[:, s:e].sum(1)} == {0, 1} or c["B"] <= 32
    assert {c["call"] for c in GC.cases("chain")} == {"clamped-hv", "nmf-mu"}
    assert next(c for c in GC.cases("chain") if c["call"] == "clamped-hv")["kw"]["sample_v"] is True      # vmode 2


@pytest.mark.parametrize("c", [c for c in GC.cases("down") if c["V"] == 1040 or c["route"]["down"] == "down_tiled"], ids=IDS)
def test_down_reference_agrees_with_the_oracle_and_notices_a_shifted_layout(c):
    ref, raw = GC.ref_down(c)
    bound = GC.prob_bounds(ref, raw, c["T"], c["groups"])
    got, _, _ = GC.run_oracle(c)
    assert GC.worst_ratio(got, ref, bound) <= 1.0, c["id"]
    # every group one column off: the comparison must fail
    slipped, _ = GC.ref_down(c, GC.shifted(c["groups"], c["V"]))
    assert GC.worst_ratio(got, slipped, GC.prob_bounds(slipped, raw, c["T"], GC.shifted(c["groups"], c["V"]))) > 1.0, c["id"]
    assert GC.worst_ratio(got, slipped, bound) > 1.0, c["id"]


@pytest.mark.parametrize("c", GC.cases("gibbs"), ids=IDS)
def test_gibbs_reference_takes_the_oracles_decisions_and_notices_a_wrong_draw_index(c, oracle_runs):
    (o_next, o_prob, o_h, o_hprob), _, _ = oracle_runs[c["id"]]
    r_next, r_prob, r_h, r_hprob, raw = GC.ref_gibbs(c)
    assert GC.worst_ratio(o_hprob, r_hprob, RC.prob_bound(1.0)) <= 1.0
    assert GC.worst_ratio(o_prob, r_prob, GC.prob_bounds(r_prob, raw, 1.0, c["groups"])) <= 1.0, c["id"]
    assert np.array_equal(o_next, r_next), f"{c['id']}: {int((o_next != r_next).sum())} decisions differ from the oracle's"
    if c["sample_h"]:
        assert np.array_equal(o_h, r_h)
    if c["rng"] == "philox":      # group g's categorical from draw g instead of 1 + g: must not pass the exact comparison
        assert not np.array_equal(GC.ref_gibbs(c, cat_from_own_index=True)[0], o_next), c["id"]


@pytest.mark.parametrize("c", GC.cases("sample"), ids=IDS)
def test_sample_reference_takes_the_oracles_decisions_and_notices_a_wrong_draw_index(c, oracle_runs):
    got, _, _ = oracle_runs[c["id"]]
    assert np.array_equal(got, GC.ref_sample(c)), c["id"]
    if c["rng"] == "philox" and c["B"] > 1:
        assert not np.array_equal(GC.ref_sample(c, cat_from_own_index=True), got), c["id"]


@pytest.mark.parametrize("c", GC.cases("train"), ids=IDS)
def test_train_reference_agrees_with_the_oracle_step(c, oracle_runs):
    (loss, st, draws), _, _ = oracle_runs[c["id"]]
    ref, want = GC.ref_train(c)
    assert draws == c["draws"]
    assert abs(float(loss) - ref["sqerr"] / (c["B"] * c["V"])) <= 1e-5 * float(loss)
    for k in GC.UC.KEYS:
        assert_close(getattr(st, k), want[k], GC.UC.TOL["rel"], f"{c['id']}: {k}", atol=GC.UC.TOL["atol"])
    # a layout one column off gives another update: the comparison notices
    slipped = GC.CC.ref_pass(*RC.params(c["V"], c["H"]), GC.operand(c["operand"], c["B"], c["V"]), c["k"], GC.shifted(c["groups"], c["V"]),
                             GC.PhiloxStream(c["seed"]))
    assert not np.array_equal(slipped["v"], ref["v"]), c["id"]
