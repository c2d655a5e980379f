"""CPU-only: the case table of update_cases.py is sound before any kernel is involved.  Ids are unique, every case names the update
kernel it expects, the block-map shapes reach all five branches of k3_block_map, the inputs of group A satisfy the exactness
condition their bit-for-bit comparison rests on, the float64 reference agrees with the fp32 numpy oracle, and the plane decoder
inverts a numpy encoding of the operand planes."""
import numpy as np
import pytest

import oracle.rbm_oracle as O
import update_cases as UC

F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731


def test_ids_are_unique_and_every_case_names_its_kernel():
    cs = UC.cases()
    assert len({c["id"] for c in cs}) == len(cs)
    for c in cs:
        kernel, tpb = c["expect"]
        assert kernel in (UC.UPDATE_GENERIC, UC.UPDATE_PLANES, UC.UPDATE_BIN, UC.UPDATE_RANKS), c["id"]
        assert (tpb == 0) == (kernel == UC.UPDATE_GENERIC) and tpb == (0 if c["generic"] else c["tpb"]), c["id"]
        assert tpb == c["opts"].get("k3_tpb", 0 if c["generic"] else 1), c["id"]
        assert set(c["opts"]) <= set(UC.OPTION_DEFAULTS), c["id"]
        assert c["entry"] in ("assoc_update", "cd_stats", "apply_factors", "train_epoch") and c["mode"] in ("exact", "fast"), c["id"]
        if kernel == UC.UPDATE_BIN:      # host_update.hpp: one chunk, MODE 0, one-term visible operands known to the host or the device
            assert c["B"] <= 64 and not c["opts"].get("no_update_bin") and (c["mode"] == "fast" or c["entry"] == "train_epoch"), c["id"]
        if kernel == UC.UPDATE_RANKS:
            assert c["entry"] == "apply_factors" and c["R"] >= c["opts"].get("min_rank_loop", 2) and not c["opts"].get("no_rank_loop"), c["id"]


def test_table_reaches_every_branch_of_the_block_map_and_every_route():
    cs = UC.cases()
    for g in ("A", "B"):      # all five xa values, by cases that compare with float64 on their own
        assert {c["xa"] for c in cs if c["group"] == g and c["xa"] is not None} == {0, 1, 2, 4, 8}, g
    assert UC.xa_of(256, 512, 1) == 4 and UC.xa_of(1024, 128, 1) == 1 and UC.xa_of(128, 1024, 1) == 8 and UC.xa_of(300, 132, 1) == 0
    assert UC.grid(700, 132, 5) == (2, 2) and UC.grid(300, 132, 1) == (2, 3) and UC.bias_rows(132) == 1 and UC.bias_rows(128) == 2
    a, b, c3 = UC.cases("A"), UC.cases("B"), UC.cases("C")
    # group A: every combination on every phase with every batch, on every configuration; P = 4 and P = 6 with more than one tile per block
    for cfg in UC.CONFIGS:
        mine = [c for c in a if c["id"].startswith(f"A-{cfg['name']}-") and c["mode"] == "exact"]
        assert len({(c["kinds"]["vpos"], c["kinds"]["hpos"], c["kinds"]["vneg"], c["kinds"]["hneg"]) for c in mine}) == 9, cfg["name"]
        assert {c["B"] for c in mine} >= {64, 128}, cfg["name"]
        if cfg["name"] != "130x36":
            assert {c["B"] for c in mine} == set(UC.A_BATCHES), cfg["name"]
    for tpb in (2, 3, 5):
        mine = [c for c in a if c["tpb"] == tpb and c["mode"] == "exact" and not c["generic"]]
        nap = {c["id"]: 1 if UC.n_terms(UC.operands(c)[0]) == 1 else 3 for c in mine}      # what the exactness map tells the kernel
        assert {nap[c["id"]] + 3 for c in mine} == {4, 6}, tpb
        assert {c["B"] for c in mine if nap[c["id"]] == 3} == {64, 128, 256}, tpb      # PASS 0 and 1 / 2 / 3 with P = 6
    assert any(c["generic"] and c["opts"].get("generic_k3") for c in a) and any(c["generic"] and c["H"] % 4 for c in a)
    fast = [c for c in a if c["mode"] == "fast"]
    assert {(c["B"], c["expect"][0]) for c in fast} == {(64, UC.UPDATE_BIN), (64, UC.UPDATE_PLANES), (128, UC.UPDATE_PLANES)}
    assert any(c["tpb"] > 1 for c in fast)                                           # assoc_update_planes<*, 1, *> with tpb > 1
    assert sum(1 for c in cs if c["pitch"]) >= 4 and {c["expect"][0] for c in cs if c["pitch"]} == {0, 1, 2, 3}      # the poisoned pitch once per family
    # group B: every batch and both operand kinds on every configuration, sparsity in half the cases
    for cfg in UC.CONFIGS:
        mine = [c for c in b if c["id"].startswith(f"B-{cfg['name']}-")]
        assert {c["B"] for c in mine} == set(UC.B_BATCHES) and {c["kinds"]["vpos"][1] for c in mine} == {"real", "mixed"}, cfg["name"]
    assert sum(c["sparsity"] for c in b) * 2 == len(b)
    # group C: MODE 1 with one and three launches at one and three tiles per block; every rank route on both shapes
    stats = [c for c in c3 if c["entry"] == "cd_stats"]
    assert {(c["B"], c["tpb"], c["data"]) for c in stats if c["mode"] == "exact"} == {(B, t, d) for B in (64, 130) for t in (1, 3) for d in ("binary", "mixed")}
    assert any(c["mode"] == "fast" for c in stats)
    ranks = [c for c in c3 if c["entry"] == "apply_factors"]
    assert any(c["tpb"] == 5 and c["expect"] == (UC.UPDATE_RANKS, 5) for c in ranks)                   # tile-wise by tiles per block > 4
    assert any(c["opts"].get("no_rank_acc") and c["expect"] == (UC.UPDATE_RANKS, 3) for c in ranks)   # ... and by option
    assert any(c["opts"].get("no_rank_loop") and c["expect"][0] == UC.UPDATE_PLANES and c["R"] == 3 for c in ranks)
    assert any(c["opts"].get("min_rank_loop") == 3 for c in ranks) and any(c["opts"].get("min_rank_loop") == 1 for c in ranks)
    assert {(c["R"], c["Bl"]) for c in ranks} >= {(1, 64), (2, 64), (3, 40)} and {c["mode"] for c in ranks} == {"exact", "fast"}
    assert {c["expect"][0] for c in c3 if c["entry"] == "train_epoch"} == {UC.UPDATE_BIN, UC.UPDATE_PLANES}


def test_operand_kinds_have_the_terms_they_claim():
    B, N = 64, 40
    assert UC.n_terms(UC.dense("binary", B, N, "x")) == 1 and UC.n_terms(UC.dense("narrow", B, N, "x")) == 1
    for kind, want in (("two-term", 2), ("wide", 3)):
        x = UC.sparse(kind, B, N, "x")
        terms = UC.split3(x)
        nz = x != 0
        assert (nz.sum(0) <= UC.SPARSE_ROWS).all() and nz.sum(0).min() == UC.SPARSE_ROWS
        for t in range(3):      # EVERY non-zero element needs exactly `want` terms
            assert np.array_equal(terms[t] != 0, nz if t < want else np.zeros_like(nz)), (kind, t)
        assert x.max() < 1 and (x[nz] >= 0.5).all()
    assert set(np.unique(UC.dense("narrow", B, N, "x"))) == {0, 0.25, 0.5, 0.75, 1}
    assert UC.n_terms(UC.dense("two-term", B, N, "x")) == 2 and (UC.dense("two-term", B, N, "x") != 0).all()
    x = UC.visible("mixed", 64, 300, 2, "x")
    cols = UC.mixed_columns(300, 2)
    assert cols.min() >= 128 and cols.max() < 256 and UC.n_terms(x[:, cols]) == 3 and UC.n_terms(np.delete(x, cols, axis=1)) == 1
    assert UC.mixed_columns(300, 3).min() >= 256 and UC.mixed_columns(300, 1).max() < 128
    assert UC.quantum_exp(np.array([0.75, 2.0, 0.0], F32)) == -2 and UC.quantum_exp(np.zeros(3, F32)) is None


@pytest.mark.parametrize("c", UC.cases("A"), ids=IDS)
def test_group_a_inputs_make_every_partial_sum_an_fp32_number(c):
    """The condition of the bit-for-bit comparison: all term products are multiples of q = 2^e and their absolute values sum to less
    than 2^24 q per output element; the float64 reference then equals its fp32 rounding.  A case that fails is repaired, never skipped."""
    ops = UC.operands(c)
    for (form, kind), x in zip((c["kinds"][k] for k in ("vpos", "hpos", "vneg", "hneg")), ops):
        if form == "sparse":
            assert ((x != 0).sum(0) <= UC.SPARSE_ROWS).all() and (x != 0).any(1).all(), f"{c['id']}: a batch row no column uses"
        else:
            assert ((x != 0).sum(0) > UC.SPARSE_ROWS).all()
        if c["mode"] == "fast":
            assert UC.n_terms(x) == 1, "FAST mode rounds operands to bf16"
    e, units = UC.exactness(c)
    assert units < 2.0 ** 24, f"{c['id']}: sum of |term products| = {units:.3e} q (q = 2^{e})"
    ref = UC.ref_a(c)
    for k in UC.KEYS:
        assert np.array_equal(ref[k].astype(F32).astype(F64), ref[k]), f"{c['id']}: {k} is not an fp32 number"
    assert np.abs(ref["W"]).max() > 0 and np.array_equal(ref["W"], ref["W_m"])
    # the same holds chunk by chunk (PASS 1 / 2 / 3 add d / n of one chunk each) and for the column sums of every 8-row group
    acc = np.zeros_like(ref["W"])
    for ch in UC.chunks(ops, c["B"]):
        acc = acc + UC.stats64([ch])["dW"] / c["B"]
        assert np.array_equal(acc.astype(F32).astype(F64), acc)
    assert np.array_equal(acc, ref["W_m"])


def _oracle_state(st, sparsity):
    o = O.RBMState.create(st["W"].copy(), 0.1, UC.B_WD, 0.5, sparsity=sparsity, sparsity_factor=UC.SPARSITY_TARGET,
                          hid_bias=st["hid_bias"].copy(), vis_bias=st["vis_bias"].copy())
    o.W_m, o.hb_m, o.vb_m = st["W_m"].copy(), st["hb_m"].copy(), st["vb_m"].copy()
    return o


def _oracle_stats(phases):
    cat = [np.concatenate([p[i] for p in phases]).astype(F32) for i in range(4)]
    vp, hp, vn, hn = cat
    return dict(pos_assoc=(vp.T @ hp).astype(F32), neg_assoc=(vn.T @ hn).astype(F32), pos_h_sum=hp.sum(0, dtype=F32),
                neg_h_sum=hn.sum(0, dtype=F32), data_sum=vp.sum(0, dtype=F32), v_sum=vn.sum(0, dtype=F32))


def _agrees(ref, o, what):
    for k in UC.KEYS:
        got, want = getattr(o, k).astype(F64), ref[k]
        d = np.abs(got - want).max()
        assert d <= 2e-5 * np.abs(want).max() + 2e-6, f"{what}: {k} differs from the oracle by {d:.3e}"


def test_float64_reference_agrees_with_the_oracle_on_one_case_per_group():
    """rbm.py:212-224 twice: ref_update (float64) against oracle.rbm_oracle.apply_cd_update (fp32)."""
    a = next(c for c in UC.cases("A") if c["id"].startswith("A-300x132-t3-two-two-both"))
    o = _oracle_state(UC.zero_params(a["V"], a["H"]), False)
    o.weight_decay = 0.0
    O.apply_cd_update(o, _oracle_stats([UC.operands(a)]), 1.0, 0.0, a["B"], False)
    _agrees(UC.ref_a(a), o, a["id"])
    for sp in (False, True):
        b = next(c for c in UC.cases("B") if c["B"] == 130 and c["sparsity"] == sp and c["V"] == 300)
        o = _oracle_state(UC.params(b["V"], b["H"]), sp)
        O.apply_cd_update(o, _oracle_stats([UC.operands(b)]), UC.B_LR, UC.B_MOM, b["B"], sp)
        _agrees(UC.ref_b(b), o, b["id"])
    # group C: the reference the GPU test builds from decoded planes, here from planes encoded in numpy (two rank blocks of 40 rows)
    c = next(c for c in UC.cases("C") if c["entry"] == "apply_factors" and c["R"] == 2 and c["Bl"] == 64 and c["V"] == 300)
    V, H, Bl, Bp = c["V"], c["H"], 40, 64
    g = np.random.Generator(np.random.PCG64(5))
    blocks, phases = [], []
    for rk in range(2):
        vp, hp, hn = UC.cd_data(c, rk)[:Bl], g.random((Bl, H), dtype=F32), g.random((Bl, H), dtype=F32)
        vn = (g.random((Bl, V), dtype=F32) > 0.5).astype(F32)
        blocks.append((vp, hp, vn, hn))
        phases.append((UC.decode_planes(UC.encode_planes(vp, Bp), V, Bl, Bp, 3), UC.decode_planes(UC.encode_planes(hp, Bp), H, Bl, Bp, 3),
                       UC.decode_planes(UC.encode_planes(vn, Bp, 1), V, Bl, Bp, 1),
                       UC.decode_planes(UC.encode_planes(hn, Bp, negate=True), H, Bl, Bp, 3, negated=True)))
    o = _oracle_state(UC.params(V, H), False)
    O.apply_cd_update(o, _oracle_stats(blocks), 0.1, 0.5, 2 * Bl, False)
    _agrees(UC.ref_update(UC.params(V, H), UC.stats64(phases), 0.1, 0.5, UC.C_WD, 2 * Bl), o, "decoded planes")


@pytest.mark.parametrize("B,Bp", [(64, 64), (40, 64), (130, 192)])
@pytest.mark.parametrize("negate", [False, True])
def test_plane_decoder_round_trips_an_encoded_buffer(B, Bp, negate):
    N = 37
    x = np.random.Generator(np.random.PCG64(B)).random((B, N), dtype=F32)
    x[:, ::3] = UC.dense("wide", B, N, "x")[:, ::3]
    buf = UC.encode_planes(x, Bp, 3, negate)
    assert buf.dtype == np.uint16 and buf.size == 3 * N * Bp
    planes = buf.reshape(3, N, Bp)
    assert not planes[:, :, B:].any() and planes[2].any()
    if negate:
        assert (planes[0][:, :B][x.T != 0] & 0x8000).all(), "the negated planes carry the sign bit"
    got = UC.decode_planes(buf.view(np.uint8), N, B, Bp, 3, negated=negate)      # raw bytes, as the device buffers come
    assert got.dtype == F64 and np.array_equal(got, x.astype(F64))
    one = UC.decode_planes(buf, N, B, Bp, 1, negated=negate)                        # the first term alone: the truncated bf16 value
    assert np.array_equal(one.astype(F32), UC.split3(x)[0])
    bad = buf.copy().reshape(3, N, Bp)
    if Bp > B:
        bad[0, 0, B] = 0x3F80
        with pytest.raises(AssertionError):
            UC.decode_planes(bad.reshape(-1), N, B, Bp, 3)
