"""CPU-only: the case table of route_cases.py is sound before any kernel is involved.  Every pinned Philox seed keeps the oracle's
Bernoulli and categorical decisions away from rounding level, the oracle's fp32 numbers agree with the float64 references within the
bounds test_routes_gpu.py asserts on the device, the two references take the same decisions, and the table names every route."""
import numpy as np
import pytest

import route_cases as RC

IDS = lambda c: c["id"]      # noqa: E731


def _margins(c, bm, cm):
    assert bm >= RC.MARGIN, f"{c['id']}: Bernoulli margin {bm:.3e} < {RC.MARGIN}: pin another seed in route_cases.SEEDS"
    assert cm >= RC.MARGIN, f"{c['id']}: categorical margin {cm:.3e} < {RC.MARGIN}: pin another seed in route_cases.SEEDS"


@pytest.mark.parametrize("c", RC.cases("up"), ids=IDS)
def test_up_step_oracle_agrees_with_float64(c):
    (p, s), bm, cm = RC.run_oracle(c)
    _margins(c, bm, cm)
    ref, ref_s = RC.ref_up(c)
    d = np.abs(p - ref).max()
    assert d <= RC.prob_bound(c["T"]), (d, RC.prob_bound(c["T"]))
    if c["sample"]:
        assert np.isfinite(bm) and np.array_equal(s, ref_s)


@pytest.mark.parametrize("c", RC.cases("down"), ids=IDS)
def test_down_step_oracle_agrees_with_float64(c):
    got, bm, cm = RC.run_oracle(c)
    ref, raw = RC.ref_down(c)
    d = np.abs(got - ref).max()
    bound = RC.logit_bound(raw, c["T"]) if c["logits_only"] else RC.prob_bound(c["T"])
    assert d <= bound, (d, bound)
    for s, e in c["groups"]:
        if c["logits_only"]:      # the group columns stay raw logits: nowhere near a distribution
            assert np.abs(ref[:, s:e].sum(1) - 1).min() > 1e-3
        else:
            np.testing.assert_allclose(ref[:, s:e].sum(1), 1.0, atol=1e-12)


@pytest.mark.parametrize("c", RC.cases("gibbs"), ids=IDS)
def test_gibbs_step_oracle_agrees_with_float64(c):
    (v_next, v_prob, h, h_prob), bm, cm = RC.run_oracle(c)
    _margins(c, bm, cm)
    assert np.isfinite(bm) == bool(c["sample_h"] or c["sample_v"]) and np.isfinite(cm) == bool(c["sample_v"] and c["groups"])
    r_next, r_prob, r_h, r_hprob = RC.ref_gibbs(c)
    b = RC.prob_bound(1.0)
    assert np.abs(h_prob - r_hprob).max() <= b and np.abs(v_prob - r_prob).max() <= b
    if c["sample_h"]:
        assert np.array_equal(h, r_h)
    else:
        assert np.abs(h - r_h).max() <= b
    if c["sample_v"]:
        assert np.array_equal(v_next, r_next)
    else:
        assert np.abs(v_next - r_next).max() <= b


@pytest.mark.parametrize("c", RC.cases("chain"), ids=IDS)
def test_chain_seeds_keep_every_decision_clear_of_rounding(c):
    (out, st, draws), bm, cm = RC.run_oracle(c)
    _margins(c, bm, cm)
    assert np.isfinite(np.asarray(out)).all() and all(np.isfinite(getattr(st, k)).all() for k in ("W", "hid_bias", "vis_bias"))
    sampled = c["kw"].get("sample_h") or c["kw"].get("sample_v") or c["method"] == "conditional_gibbs_annealed"
    assert np.isfinite(bm) == bool(sampled), "the case samples nothing it should, or the other way round"
    assert draws > 0


def test_table_covers_every_route_both_epilogues_and_finish_groups():
    """Adding a route to prop() (native.ROUTE_UP / ROUTE_DOWN) without a case fails here."""
    from imdbn.engine import native
    assert tuple(native.ROUTE_UP) == RC.UP_ROUTES and tuple(native.ROUTE_DOWN) == RC.DOWN_ROUTES
    cs = RC.cases()
    single = [c for c in cs if c["kind"] != "chain"]      # every route by a single step against float64, not by a chain alone
    ups = {(c["route"]["up"], c["route"]["up_epilogue"]) for c in single if "up" in c["route"]}
    downs = {(c["route"]["down"], c["route"]["down_epilogue"], c["route"]["finish_groups"]) for c in single if "down" in c["route"]}
    assert {u for u, _ in ups} == set(RC.UP_ROUTES) and {d for d, _, _ in downs} == set(RC.DOWN_ROUTES)
    for r in RC.UP_ROUTES:
        # (the bit plane's general instantiation runs only inside the CD pass: route_cases.up_cases)
        assert (r, "lean") in ups and ((r, "general") in ups or r == "stream_bits"), r
    for r in RC.DOWN_ROUTES:
        # (k2_stream's lean instantiation likewise: every call that reaches it outside the CD pass writes a final state)
        assert ((r, "lean", False) in downs or r == "k2_stream") and (r, "general", False) in downs and (r, "general", True) in downs, r
    # every up route with every temperature; every operand kind and every batch on every prop_up route
    for r, V, H, _ in RC.UP_SHAPES:
        mine = [c for c in cs if c["kind"] == "up" and (c["route"]["up"], c["V"], c["H"]) == (r, V, H)]
        assert {c["T"] for c in mine if c["sample"]} == {c["T"] for c in mine if not c["sample"]} == set(RC.TEMPS)
        assert {c["operand"] for c in mine} == set(RC.OPERANDS) and {c["B"] for c in mine} == set(RC.BATCHES)
    # every down shape with every temperature x raw logits x group layout
    for r, V, H, B, _ in RC.DOWN_SHAPES:
        mine = [c for c in cs if c["kind"] == "down" and (c["route"]["down"], c["V"], c["H"], c["B"]) == (r, V, H, B)]
        assert len({(c["T"], c["logits_only"], c["groups"]) for c in mine}) == 3 * 2 * 3
    # the wide chains: every call on every route, both batches and both known sides per call and per route
    ch = RC.cases("chain")
    assert len(ch) == len(RC.CHAIN_CALLS) * len(RC.CHAIN_ROUTES)
    for key in ("call", "variant"):
        for val in {c[key] for c in ch}:
            mine = [c for c in ch if c[key] == val]
            assert {c["B"] for c in mine} == {27, 130} and {c["known"] for c in mine} == {"labels", "features"}, val
    assert all(max(c["V"], 1) * c["H"] * c["B"] <= 4100 * 72 * 256 for c in cs)


def test_categorical_margin_tracks_the_cumulative_sums_next_to_the_pick():
    import oracle.rbm_oracle as O
    from oracle.draws import CATEGORICAL_MARGIN, PhiloxStream
    O.reset_margin()
    assert CATEGORICAL_MARGIN["min"] == float("inf")
    p = np.full((64, 4), 0.25, np.float32)
    ps = PhiloxStream(3)
    u = PhiloxStream(3).uniform_silent((64, 1))[:, 0].astype(np.float64)
    idx = ps.categorical(p)
    assert np.array_equal(idx, np.minimum((u * 4).astype(int), 3))
    lo, hi = u - idx * 0.25, (idx + 1) * 0.25 - u        # distances to the cumulative sums on either side, row total 1
    want = min(min(l for l, i in zip(lo, idx) if i > 0), min(h for h, i in zip(hi, idx) if i < 3))
    assert abs(CATEGORICAL_MARGIN["min"] - want) < 1e-7
    O.reset_margin()
    assert CATEGORICAL_MARGIN["min"] == float("inf") and O.BERNOULLI_MARGIN["min"] == float("inf")
