"""CPU-only: the case table of signed_cases.py is sound before any kernel is involved.  The pm1 arrays have the tile arrangement the
table claims (recomputed with prep_operand's own two expressions), the float64 logits of every probability case stay within +-6, the
exact update cases satisfy the precondition their bit-for-bit comparison rests on, an fp32 emulation of the general update cases fits
update_cases.TOL with a factor 4 to spare, and every route appears with every kind it is listed with."""
import numpy as np
import pytest

import backprop_oracle as Bp
import pcd_oracle as P
import route_cases as RC
import signed_cases as SC
import update_cases as UC

F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731
PROP = SC.prop_cases()
EXACT, GENERAL, ALIASED = SC.exact_cases(), SC.general_cases(), SC.aliased_cases()


def _operand_shapes():
    """Every (B, N) at which a propagation case feeds an operand."""
    out = set()
    for c in PROP:
        up = c["kind"] in ("raw_up", "prob_up", "forward", "gibbs")
        out.add((c["B"], c["V"] if up else c["H"]))
    return sorted(out)


def test_every_route_appears_with_every_kind():
    assert len({c["id"] for c in PROP + EXACT + GENERAL + ALIASED}) == len(PROP) + len(EXACT) + len(GENERAL) + len(ALIASED)
    seen = {}
    for c in PROP:
        for side in ("up", "down"):
            if side in c["route"] and not (c["kind"] == "gibbs" and side == "up"):
                seen.setdefault(c["route"][side], set()).add(c["operand"])
    three = {"signed", "gauss", "pm1"}
    for route in ("fused", "stream_real", "partial4", "partial") + RC.DOWN_ROUTES:
        assert seen[route] >= three, (route, seen[route])
    assert seen["stream_bits"] == {"pm1_clean"}
    assert {r for r, *_ in RC.UP_SHAPES} | {r for r, *_ in RC.DOWN_SHAPES} | {"k2_stream", "stream_bits"} == set(seen)
    # every row of the two shape tables with its options, and 130 x 72 going down
    for route, V, H, opts in RC.UP_SHAPES:
        for kind in ("raw_up", "prob_up"):
            mine = [c for c in PROP if c["kind"] == kind and (c["V"], c["H"], c["opts"]) == (V, H, opts)]
            assert {c["operand"] for c in mine} == set(SC.KINDS), (kind, V, H)
            assert all(c["route"]["up"] == (route if kind == "prob_up" else SC.raw_up_route(route, H)) for c in mine)
        assert {c["B"] for c in PROP if c["kind"] in ("raw_up", "prob_up") and (c["V"], c["H"], c["opts"]) == (V, H, opts)} == set(RC.BATCHES)
    for route, V, H, B, opts in SC.DOWN_TABLE:
        for kind in ("raw_down", "logits_down", "prob_down"):
            mine = [c for c in PROP if c["kind"] == kind and (c["V"], c["H"], c["B"], c["opts"]) == (V, H, B, opts)]
            assert {c["operand"] for c in mine} == set(SC.KINDS) and all(c["route"]["down"] == route for c in mine), (kind, V, H, B)
    assert {T for c in PROP if c["kind"].startswith("prob") for T in [c["T"]]} == set(SC.PROB_TEMPS)
    # the update: every configuration of update_cases with signed, gauss and an exact signed kind; every phase; three and four passes
    for cfg in SC.ALL_CONFIGS:
        ex = [c for c in EXACT if c["config"] == cfg["name"]]
        ge = [c for c in GENERAL if c["config"] == cfg["name"]]
        assert len(ex) == 3 and {c["kinds"]["vpos"][0] for c in ge} == {"signed", "gauss"}, cfg["name"]
        assert all(c["expect"] == UC._expect(cfg) for c in ex + ge)
    assert {c["expect"] for c in EXACT + GENERAL} >= {(UC.UPDATE_GENERIC, 0), (UC.UPDATE_BIN, 1), (UC.UPDATE_BIN, 3)} | {(UC.UPDATE_PLANES, t) for t in (1, 2, 3, 5)}
    for group in (EXACT, GENERAL):
        assert {c["xa"] for c in group if c["xa"] is not None} == {0, 1, 2, 4, 8}
        assert sum(1 for c in group if c["pitch"]) >= 2
    for kind in ("signed", "gauss"):
        assert {c["B"] for c in GENERAL if c["kinds"]["vpos"][0] == kind} == set(UC.B_BATCHES), kind
    assert {c["B"] for c in EXACT} == {64, 128, 256}
    assert {(c["V"], c["H"], c["B"]) for c in ALIASED} == {(1040, 37, 33), (1040, 36, 130), (4100, 72, 128)}


@pytest.mark.parametrize("B,N", _operand_shapes())
def test_pm1_has_the_tile_arrangement_the_table_claims(B, N):
    x = SC.operand("pm1", B, N)
    assert x.dtype == F32 and set(np.unique(x)) <= {-1.0, 0.0, 1.0}
    negzero = (x == 0) & np.signbit(x)
    nonbin, bits = SC.tile_flags(x)
    assert np.array_equal(bits, (x == 1) | (x == -1)), "the bit plane (x != 0) is clear on -0.0 and set on -1"
    nty, ntx = nonbin.shape
    for ty in range(nty):
        for tx in range(ntx):
            t = x[8 * ty:8 * (ty + 1), 64 * tx:64 * (tx + 1)]
            assert negzero[8 * ty:8 * (ty + 1), 64 * tx:64 * (tx + 1)].any(), "every tile holds a -0.0, which the flag's test passes as binary"
            assert int((t == -1).sum()) == (1 if SC.tile_minus(ty, tx) else 0)
            assert nonbin[ty, tx] == SC.tile_minus(ty, tx), "a tile is non-binary exactly where it holds the -1"
            assert not (np.ascontiguousarray(t).view(np.uint32) & 0xFFFF).any(), "one-term throughout (FLAG_INEXACT clear)"
    assert nonbin[0, 0] and (x == 1).any()
    items = np.array([[nonbin[8 * iy:8 * (iy + 1), tx].any() for tx in range(ntx)] for iy in range(SC.cdiv(B, 64))])
    assert np.array_equal(items, np.array([[SC.item_dirty(iy, tx) for tx in range(ntx)] for iy in range(items.shape[0])]))
    if items.size >= 2:
        assert items.any() and not items.all(), "an all-{0, -0.0, 1} item of the adaptive preparation next to one that is not"
    clean = SC.operand("pm1_clean", B, N)
    assert not SC.tile_flags(clean)[0].any() and (np.signbit(clean) & (clean == 0)).any() and np.array_equal(np.abs(clean), np.abs(x))


def test_the_other_kinds_are_what_they_claim():
    s = SC.operand("signed", 130, 1040)
    assert abs(float(s.std()) - 0.3) < 0.01 and (s < 0).mean() > 0.45 and UC.n_terms(s) == 3
    g = SC.operand("gauss", 130, 1040)
    assert 15 < float(np.abs(g).max()) < 60 and (g < 0).mean() > 0.3 and UC.n_terms(g) == 3
    m = SC.operand("signed_mixed", 130, 1040)
    assert set(np.unique(m[:, :520])) == {0.0, 1.0} and (m[:, 520:] <= 0).all() and m[:, 520:].min() < -0.99
    assert np.array_equal(np.abs(m), RC.operand("mixed", 130, 1040))
    n = SC.exact_operand("dense", "narrow", True, 64, 40, "x")
    w = SC.exact_operand("sparse", "wide", True, 64, 40, "x")
    assert set(np.unique(np.abs(n))) == {0, 0.25, 0.5, 0.75, 1} and (n < 0).any() and (n > 0).any() and UC.n_terms(n) == 1
    assert np.array_equal(np.abs(w), UC.sparse("wide", 64, 40, "x")) and UC.n_terms(w) == 3
    nz = w != 0
    assert 0.3 < (w[nz] < 0).mean() < 0.7
    for t in UC.split3(w):      # the three terms of a negative value all carry its sign: every non-zero element has three non-zero terms
        assert np.array_equal(t != 0, nz) and (np.sign(t[nz]) == np.sign(w[nz])).all()


@pytest.mark.parametrize("c", [c for c in PROP if c["kind"] in ("prob_up", "prob_down", "forward", "gibbs")], ids=IDS)
def test_probability_cases_keep_their_logits_within_the_cap(c):
    """A saturated sigmoid would hide an error of the product: |float64 logits / T| <= 6 on every case, by an exact (power of two) scale."""
    up = c["kind"] != "prob_down"
    x = SC.prob_operand(c)
    s = SC.prob_scale(c["operand"], c["V"], c["H"], c["B"], up)
    assert np.log2(s) == np.floor(np.log2(s)) and np.array_equal(x.astype(F64), SC.operand(c["operand"], c["B"], x.shape[1]).astype(F64) * s)
    if c["operand"].startswith("pm1"):
        assert s == 1.0
    l = SC.logits64(x, c["V"], c["H"], up)[0] / c["T"]
    assert np.abs(l).max() <= SC.LOGIT_CAP, f"{c['id']}: |logits / T| reaches {np.abs(l).max():.3g}"
    assert np.abs(l).max() > 0.25, "the scale left nothing to see"


@pytest.mark.parametrize("c", EXACT, ids=IDS)
def test_exact_cases_make_every_partial_sum_an_fp32_number(c):
    """test_group_a_inputs_make_every_partial_sum_an_fp32_number on the signed inputs: all term products are multiples of q = 2^e and
    their ABSOLUTE values sum to less than 2^24 q per output element, so every partial sum in any order and with any signs is an fp32
    number and the float64 reference equals its fp32 rounding."""
    ops = SC.update_operands(c)
    for name, x in zip(("vpos", "hpos", "vneg", "hneg"), ops):
        form, kind, signed = c["kinds"][name]
        assert ((x != 0).sum(0) <= UC.SPARSE_ROWS).all() if form == "sparse" else ((x != 0).sum(0) > UC.SPARSE_ROWS).all()
        if form == "sparse":
            assert (x != 0).any(1).all(), f"{c['id']}: a batch row no column uses"
        assert (x < 0).any() == signed and UC.n_terms(x) == (3 if kind == "wide" else 1)
    signed = {k: v[2] for k, v in c["kinds"].items()}
    assert signed["vpos"] == signed["hpos"] and signed["vneg"] == signed["hneg"] and (signed["vpos"] or signed["vneg"])
    if c["mode"] == "fast":      # the bin body: one chunk, one-term operands in all four slots
        assert c["B"] == 64 and all(UC.n_terms(x) == 1 for x in ops) and c["expect"][0] == UC.UPDATE_BIN
    e, units = SC.exactness(ops)
    assert units < 2.0 ** 24, f"{c['id']}: sum of |term products| = {units:.3e} q (q = 2^{e})"
    assert c["B"] & (c["B"] - 1) == 0
    ref = SC.ref_exact(c)
    for k in UC.KEYS:
        assert np.array_equal(ref[k].astype(F32).astype(F64), ref[k]), f"{c['id']}: {k} is not an fp32 number"
    assert np.abs(ref["W"]).max() > 0 and (ref["W"] < 0).any() and np.array_equal(ref["W"], ref["W_m"])
    acc = np.zeros_like(ref["W"])
    for ch in UC.chunks(ops, c["B"]):
        acc = acc + UC.stats64([ch])["dW"] / c["B"]
        assert np.array_equal(acc.astype(F32).astype(F64), acc)
    assert np.array_equal(acc, ref["W_m"])


@pytest.mark.parametrize("c", GENERAL, ids=IDS)
def test_fp32_emulation_of_the_general_cases_fits_tol_with_a_factor_4_to_spare(c):
    """Before the GPU test relies on update_cases.TOL for signed sums (which cancel: the result is small against the sum of
    magnitudes): split3 terms accumulated in fp32 chunk by chunk stay within a quarter of it on these very inputs."""
    emu, ref = SC.emulate_general(c), SC.ref_general(c)
    worst = {k: SC.tol_fraction(emu[k], ref[k]) for k in UC.KEYS}
    print(f"{c['id']}: fraction of TOL used by the fp32 emulation: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 0.25, worst


@pytest.mark.parametrize("c", ALIASED, ids=IDS)
def test_aliased_cases_have_the_inputs_they_claim(c):
    io, l = SC.aliased_io(c), SC.aliased_layer(c["V"], c["H"])
    for k in ("x_v", "x_h"):
        assert io[k].min() >= 0 and io[k].max() <= 1
    assert (set(np.unique(io["x_v"])) == {0.0, 1.0}) == (c["xkind"] == "binary") and io["x_h"].min() >= 0.02 and io["x_h"].max() <= 0.98
    assert UC.n_terms(io["e_h"]) == 3 and UC.n_terms(io["e_v"]) == 3 and (io["e_h"] < 0).any() and (io["e_v"] < 0).any()
    up, dn = SC.ALIASED_FORMS[c["form"]]
    st = P.rbm_state(l, 0.05, 1e-4, 0.9)
    before = st.W.copy()
    out = Bp.backprop_step(st, (io["x_v"], io["e_h"]) if up else None, (io["x_h"], io["e_v"]) if dn else None, 0.05, 0.9, True)
    assert (out["err_v"] is not None) == up and (out["err_h"] is not None) == dn and not np.array_equal(st.W, before)
