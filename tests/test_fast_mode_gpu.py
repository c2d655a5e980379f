"""GPU: FAST mode (IMDBN_FAST_BF16: one bf16 term per weight and per operand, round to nearest even, fp32 accumulation) on every
propagation route, on the CD pass of every route, three cd_steps, a wide-layer chain, free_energy and the decode error, against the float64 twin of fast_cases.py (which has the table, the twin, the
staging rule for real-valued intermediates and the reasoning).  Every case asserts through HipEngine.last_route(), and for a CD
pass last_cd(), the kernels and epilogues it names, sets the mode as test_row_offset_gpu.py does and runs on a NaN-filled workspace.

The twin rounds operands and weights as the device must and takes every decision on the PhiloxStream draws (seeds pinned on the CPU
with a margin of 1e-6, test_fast_mode_cpu.py), so samples, sample planes and the one-term plane of the data are compared exactly;
probabilities within route_cases.prob_bound(T) = 5e-7 max(1, 1 / T); raw logits within route_cases.logit_bound; the packed
statistics within cd_cases.stats_bound.  A one-term plane of probabilities (hid_tr0 / hid_tr1) is held to

    |decoded - twin| <= prob_bound(1.0) + half a bf16 ulp of the twin's value

which is derived, not measured: the device's fp32 value is within prob_bound of the twin, and rounding it to the nearest bf16 moves
it by at most half an ulp.  test_fast_mode_cpu.py asserts that the FAST twin and the parity float64 reference are at least 20 bounds
apart on what each case compares, so none of these assertions holds for a kernel that runs parity arithmetic, truncates, or rounds
in another place.

Largest |device - twin| per compared quantity over the whole file on an MI355X, next to the bound of the element it was measured at
(every case prints its own figures with `-s`, the module prints this table at its end):

  p(h|v)    1.03e-07  (bound 7.14e-07, 0.14 of it)  fast-up-partial-1040x37-B7-T0.7-real
  p(v|h)    9.27e-08  (bound 5.00e-07, 0.19)        fast-gibbs-130x72-B66-mf
  logits    1.09e-07  (bound 2.02e-05, 0.01)        fast-down-down_fused-1040x36-B130-g0-T0.7-logits
  plane P+  1.95e-03  (bound 1.95e-03, 1.00)        fast-seq-stats-130x70-B33 step 0
  plane P-  1.95e-03  (bound 1.95e-03, 1.00)        fast-seq-stats-1040x36-no_bits-rows8-B33 step 4
  dW        4.59e-06  (bound 8.52e-05, 0.05)        fast-seq-stats-1040x36-B130 step 6
  dc        2.67e-05  (bound 9.74e-05, 0.27)        fast-cd-1040x36-no_adaptive-B130-k2-mixed-unknown
  db        1.69e-05  (bound 8.68e-05, 0.19)        fast-seq-stats-1040x36-B130 step 6
  hpos      1.83e-05  (bound 2.47e-04, 0.07)        fast-cd-1040x36-no_k2s-B130-k1-mixed-unknown
  sqerr     1.74e-03  (bound 6.80e-02, 0.03)        fast-seq-stats-1040x36-B130 step 0
  step W    7.84e-09  (2e-5 max|W| + 2e-6 = 5.46e-06)  fast-step-1040x36-B130-prefetch step 2   (the other five state tensors: <= 2e-8)
  F(v)      2.95e-06  (bound 1.63e-03, 0.00)        fast-free_energy-1040x36-B33
  sqerr/row 2.74e-13  (bound 5.10e-11, 0.01)        fast-prop_down_sqerr-1040x36-B33

Nothing is over its bound.  The planes sit AT theirs (2^-9 = half an ulp at p >= 0.5, a rounding that lands on a midpoint's side),
as a rounding bound must; the raw logits and dW are far below because the bounds are those of K = 2000 and of three-term planes,
kept as the project states them.

Every call runs on a NaN-filled workspace; options, the mode and the engine's prefetch record are restored after every case."""
import contextlib

import numpy as np
import pytest
import torch

import cd_cases as CC
import fast_cases as FC
import parity_cases as P
import route_cases as RC
import rowoffset_cases as RO
import test_cd_routes_gpu as TG
import test_routes_gpu as TR
import update_cases as UC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731
WORST = {}                   # quantity -> (largest |device - twin|, bound of that element, case)


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    from imdbn.engine import native
    E.set_engine_for_testing(None)
    eng = E.get_hip_engine()             # raises if the library is missing: no silent fallback
    cu, arch = eng.device_info()
    assert "gfx950" in arch, arch
    assert cu == CC.CUS, f"cd_cases.route_of mirrors the routes of a device with {CC.CUS} compute units, this one has {cu}"
    yield eng
    for k, v in dict(CC.OPTION_DEFAULTS, **RO.A_OPTION_DEFAULTS).items():
        eng.set_option(k, v)
    eng.mode = native.PARITY_F32
    eng._pf.clear()
    for what, (d, bound, cid) in WORST.items():
        print(f"[fast mode] {what:8s} {d:.2e}  (bound {bound:.2e}, {d / bound:.2f} of it)  {cid}")


@contextlib.contextmanager
def _fast(eng):
    from imdbn.engine import native
    mode = eng.mode
    try:
        eng.mode = native.FAST_BF16
        yield
    finally:
        eng.mode = mode
        eng._pf.clear()


def _within(got, ref, bound, what, cid):
    got = np.asarray(got, F64)
    assert np.isfinite(got).all(), f"{cid}: {what} is not finite"
    d = np.abs(got - ref)
    b = np.broadcast_to(np.asarray(bound, F64), d.shape)
    i = np.unravel_index(int(d.argmax()), d.shape) if d.ndim else ()
    if what not in WORST or float(d[i]) > WORST[what][0]:
        WORST[what] = (float(d[i]), float(b[i]), cid)
    print(f"{cid}: {what}: max|d| = {float(d[i]):.3e} (bound there {float(b[i]):.3e})")
    over = d > b
    j = np.unravel_index(int((d - b).argmax()), d.shape) if d.ndim else ()
    assert not over.any(), f"{cid}: {what}: {int(over.sum())} of {d.size} elements over the bound, worst |d| = {float(d[j]):.3e} at bound {float(b[j]):.3e}"


def _same(got, ref, what, cid):
    got = np.asarray(got, F64)
    bad = got != ref
    assert not bad.any(), f"{cid}: {int(bad.sum())} of {bad.size} {what} differ from the twin's decisions, rows {sorted(set(np.argwhere(bad)[:, 0]))[:8]}"


# ---- single propagations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.cases("up"), ids=IDS)
def test_up_step_matches_the_fast_twin_on_its_route(c, _native):
    from imdbn import engine as E
    r, v = TR._rbm(c), P.T(RC.operand(c["operand"], c["B"], c["V"]), DEV)
    rng = E.PhiloxRng(seed=c["seed"])
    with _fast(_native), TR._routed(_native, c):
        if c["kind"] == "forward":
            p, s = _native.forward(r, v, data_binary=True), None
        elif c["sample"]:
            p, s = _native.prop_up(r, v, T=c["T"], sample=True, rng=rng)
        else:
            p, s = _native.prop_up(r, v, T=c["T"]), None
        TR._assert_route(_native, c)
    ref, ref_s, _, _ = FC.twin_up(c)
    _within(P.N(p), ref, RC.prob_bound(c["T"]), "p(h|v)", c["id"])
    assert rng.offset == (1 if c["sample"] else 0)
    if c["sample"]:
        _same(P.N(s), ref_s, "hidden samples", c["id"])


@pytest.mark.parametrize("c", FC.cases("down"), ids=IDS)
def test_down_step_matches_the_fast_twin_on_its_route(c, _native):
    r, h = TR._rbm(c), P.T(RC.operand("real", c["B"], c["H"]), DEV)
    with _fast(_native), TR._routed(_native, c):
        out = P.N(_native.prop_down(r, h, T=c["T"], logits_only=bool(c["logits_only"])))
        TR._assert_route(_native, c)
    ref, raw, _ = FC.twin_down(c)
    if c["logits_only"]:      # every column, the softmax groups' included, stays a raw logit
        _within(out, ref, RC.logit_bound(raw, c["T"]), "logits", c["id"])
    else:
        _within(out, ref, RC.prob_bound(c["T"]), "p(v|h)", c["id"])


@pytest.mark.parametrize("c", FC.cases("gibbs"), ids=IDS)
def test_gibbs_step_matches_the_fast_twin_stage_by_stage(c, _native):
    """Sampled: the hidden sample reaches the K2 as a bit plane (or the one-term form), decisions exact.  Mean-field: K1's epilogue
    writes the one-term hid_rm from its fp32 h_prob; the twin of the K2 starts from the h_prob the device returned."""
    from imdbn import engine as E
    r, v = TR._rbm(c), P.T(RC.operand(c["operand"], c["B"], c["V"]), DEV)
    rng = E.PhiloxRng(seed=c["seed"])
    with _fast(_native), TR._routed(_native, c):
        v_next, v_prob, h, h_prob = (P.N(t) for t in _native.gibbs_step(r, v, c["sample_h"], c["sample_v"], rng))
        TR._assert_route(_native, c)
    t = FC.twin_gibbs(c, h_prob_device=None if c["sample_h"] else h_prob)
    b = RC.prob_bound(1.0)
    _within(h_prob, t["h_prob"], b, "p(h|v)", c["id"])
    if c["sample_h"]:
        _same(h, t["h"], "hidden samples", c["id"])
    else:
        assert np.array_equal(h, h_prob), f"{c['id']}: the mean-field h is not the h_prob of the same launch"
    _within(v_prob, t["v_prob"], b, "p(v|h)", c["id"])
    if c["sample_v"]:
        for s, e in c["groups"]:
            assert np.array_equal(v_next[:, s:e].argmax(1), t["v_next"][:, s:e].argmax(1)) and (v_next[:, s:e].sum(1) == 1).all(), f"{c['id']}: categorical picks"
        _same(v_next, t["v_next"], "visible samples", c["id"])
    else:
        _within(v_next, t["v_next"], b, "p(v|h)", c["id"])
    assert rng.offset == RC.gibbs_draws(c)


# ---- the CD pass ------------------------------------------------------------------------------------------------------------------------
def _check_planes(c, t, read, x, data_plane=True):
    """The operand planes and column sums a FAST pass leaves, against the twin; returns the device's one-term planes of P+ and P-
    (decode_planes asserts zero padding rows and no NaN)."""
    V, H, B, cid = c["V"], c["H"], c["B"], c["id"]
    Bp = (B + 63) // 64 * 64
    if data_plane:
        _same(UC.decode_planes(read("vis_tr0", V * Bp * 2), V, B, Bp, 1), t["x"], "elements of the data plane (rne_bf16 of the batch)", cid)
        TG._within(TG._colsum(read, "cs_vpos", V, Bp), x.astype(F64).sum(0), 1e-6 * B, f"{cid}: cs_vpos")
    _same(UC.decode_planes(read("vis_tr1", V * Bp * 2), V, B, Bp, 1), t["v"], "visible samples", cid)
    if c["r"]["vbits"]:
        _same(TG._bits(read("vis_bits1", (V + 63) // 64 * 8 * Bp), V, B, Bp), t["v"], "bits of vis_bits1", cid)
    hp = UC.decode_planes(read("hid_tr0", H * Bp * 2), H, B, Bp, 1)
    hn = UC.decode_planes(read("hid_tr1", H * Bp * 2), H, B, Bp, 1, negated=True)
    _within(hp, t["hpos"], CC.prob_bound(1.0) + FC.half_ulp_bf16(t["hpos"]), "plane P+", cid)
    _within(hn, t["hneg"], CC.prob_bound(1.0) + FC.half_ulp_bf16(t["hneg"]), "plane P-", cid)
    assert np.array_equal(RO.rne_bf16(hp.astype(F32)), hp.astype(F32)) and np.array_equal(RO.rne_bf16(hn.astype(F32)), hn.astype(F32))
    pb = B * CC.prob_bound(1.0) + 1e-6 * B
    TG._within(TG._colsum(read, "cs_hpos", H, Bp), t["hpos"].sum(0), pb, f"{cid}: cs_hpos")
    TG._within(TG._colsum(read, "cs_hneg", H, Bp), t["hneg"].sum(0), pb, f"{cid}: cs_hneg")
    TG._within(TG._colsum(read, "cs_vneg", V, Bp), t["v"].sum(0), 0.0, f"{cid}: cs_vneg")
    return hp, hn


def _check_packed(cid, V, H, B, packed, t, hp, hn):
    got, want = np.asarray(packed, F64)[: V * H + 2 * H + V + 1], FC.packed_twin(t, hp, hn)
    for name, sl in CC.packed_parts(V, H).items():
        _within(got[sl], want[sl], CC.stats_bound(B, want[sl]), name, cid)


@pytest.mark.parametrize("c", FC.cases("pass"), ids=IDS)
def test_cd_pass_matches_the_fast_twin_on_its_route(c, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    x = RC.operand(c["data"], B, V)
    t = FC.twin_cd(c)[0][0]
    rng = E.PhiloxRng(seed=c["seed"])
    with _fast(_native), TG._routed(_native, c):
        r = TG._rbm(c)
        packed = P.N(_native.cd_stats(r, P.T(x, DEV), c["k"], rng, data_binary=TG._hint_arg(c["hint"])))
        TG._assert_routes(_native, c["id"], c["expect"], c["expect_cd"])
        assert rng.offset == c["draws"]
        hp, hn = _check_planes(c, t, TG._reader(_native, c), x)
        _check_packed(c["id"], V, H, B, packed, t, hp, hn)


def _check_slot(c, s, read, nxt):
    """FAST mode prepares ONE plane of a hinted batch, whatever its form in parity mode: the nearest bf16 of every element."""
    V, B = c["V"], c["B"]
    Bp = (B + 63) // 64 * 64
    got = UC.decode_planes(read(f"pf_tr{s['next_slot']}", V * Bp * 2), V, B, Bp, 1)
    _same(got, RO.rne_bf16(nxt).astype(F64), f"elements of slot {s['next_slot']} (step {s['i']})", c["id"])


@pytest.mark.parametrize("c", FC.cases("seq"), ids=IDS)
def test_prefetched_sequence_matches_the_fast_twin_step_by_step(c, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    xs = FC.cd_batches(c)
    ts = [TG._tagged(x, s["hint"]) for x, s in zip(xs, c["steps"])]
    other = TG._tagged(np.roll(xs[3], 5, axis=0), "unknown")
    twins = FC.twin_cd(c)[0]
    rng = E.PhiloxRng(seed=c["seed"])
    with _fast(_native), TG._routed(_native, c):
        r = TG._rbm(c)
        for s in c["steps"]:
            i = s["i"]
            sc = dict(c, id=f"{c['id']} step {i}")
            hint = {"next": ts[i + 1] if i + 1 < len(ts) else None, "other": other, None: None}[s["nxt"]]
            packed = P.N(_native.cd_stats(r, ts[i], c["k"], rng, next_data=hint))
            TG._assert_routes(_native, sc["id"], s["expect"], s["expect_cd"])
            assert rng.offset == (i + 1) * c["draws"]
            read = TG._reader(_native, c)
            # (a step served from a slot reads its data planes there: the slot was checked when it was written)
            hp, hn = _check_planes(sc, twins[i], read, xs[i], data_plane=s["expect_cd"]["slot"] == 0)
            _check_packed(sc["id"], V, H, B, packed, twins[i], hp, hn)
            if s["next_slot"]:
                _check_slot(c, s, read, P.N(hint))
        assert not _native._pf


# ---- three consecutive cd_steps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.cases("step"), ids=IDS)
def test_three_cd_steps_match_the_fast_twin(c, _native):
    """The rule of test_cd_routes_gpu.py: parameters and momenta after every step within update_cases.TOL of the float64 update of
    the fp32 state the device held before it.  The twin of a step rounds THAT state's weights, and its dW multiplies the planes of
    P+ and P- the device left (the staging rule), each checked against the twin first."""
    from imdbn import engine as E
    from oracle.draws import PhiloxStream
    V, H, B = c["V"], c["H"], c["B"]
    xs = FC.cd_batches(c)
    ts = [TG._tagged(x, s["hint"]) for x, s in zip(xs, c["steps"])]
    ts.append(TG._tagged(CC.seq_batch("binary", B, V, len(xs)), "binary"))      # what the last step of the prefetch case hints
    rng = E.PhiloxRng(seed=c["seed"])
    st = CC.state(c["route_name"])
    with _fast(_native), TG._routed(_native, c):
        r = TG._rbm(c, step=True)
        for s in c["steps"]:
            i = s["i"]
            sc = dict(c, id=f"{c['id']} step {i}")
            m = FC.Margin()
            t = FC.twin_pass(FC.par_of(st["W"], st["hid_bias"], st["vis_bias"]), xs[i], c["k"], c["groups"], PhiloxStream(c["seed"], offset=i * c["draws"]), m)
            assert m.bern >= FC.MARGIN and m.cat >= FC.MARGIN, f"{sc['id']}: margins {m.bern:.2e} / {m.cat:.2e} on the device's state: replace the seed"
            loss = _native.cd_step(r, ts[i], CC.STEP_LR, CC.STEP_MOM, c["k"], rng, next_data=ts[i + 1] if s["nxt"] else None)
            TG._assert_routes(_native, sc["id"], s["expect"], s["expect_cd"])
            assert rng.offset == (i + 1) * c["draws"]
            got = TG._state(r)
            hp, hn = _check_planes(sc, t, TG._reader(_native, c), xs[i], data_plane=s["expect_cd"]["slot"] == 0)
            mean = t["sqerr"] / (B * V)
            assert abs(float(loss) - mean) <= 1e-5 * mean, (float(loss), mean)
            want = FC.step_update(st, FC.stats_twin(t, hp, hn), B)
            TG._close(sc["id"], got, want)
            for k in UC.KEYS:      # (the figures of the table; _close has asserted the project's rule, rel-Frobenius with an absolute floor)
                d = float(np.abs(got[k].astype(F64) - want[k]).max())
                if f"step {k}" not in WORST or d > WORST[f"step {k}"][0]:
                    WORST[f"step {k}"] = (d, UC.TOL["rel"] * float(np.abs(want[k]).max()) + UC.TOL["atol"], sc["id"])
            st = got      # the next step's reference starts from the fp32 state the device holds


# ---- the wide-layer chain, one launch per half step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.cases("chain"), ids=IDS)
def test_wide_chain_matches_the_fast_twin_step_by_step(c, _native):
    """Two sampled steps alone: the final sample equals the twin's.  Then all three, traced: every step's p(h|v) and p(v|h) against
    the twin, the mean-field step's K2 fed in the twin with the h_prob the device traced (its K1 wrote the one-term hid_rm from it)."""
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    r = TR._rbm(c)
    vk, km = P.T(RC.operand(c["operand"], B, V), DEV), torch.zeros(B, V, device=DEV)
    b = RC.prob_bound(1.0)
    with _fast(_native), TR._routed(_native, c):
        rng = E.PhiloxRng(seed=c["seed"])
        v2 = P.N(_native.chain(r, vk, km, c["steps"][:2], rng, init_uniform=False))
        assert _native.last_chain()["route"] == "per_launch" and rng.offset == 2 * (2 + len(c["groups"]))
        TR._assert_route(_native, dict(c, route=c["route_sampled"]))
        rng = E.PhiloxRng(seed=c["seed"])
        (final, tr, trh), = _native.chain_traced_vh(r, dict(v_known=vk, mask=km, steps=c["steps"], init_uniform=False, trace=(0, V, False), trace_h=(0, H)), None, rng)
        assert _native.last_chain()["route"] == "per_launch" and rng.offset == 2 * (2 + len(c["groups"]))
        TR._assert_route(_native, c)
    final, tr, trh = P.N(final), P.N(tr), P.N(trh)
    twin, _ = FC.twin_chain(c, h_prob_device=trh[2])
    _same(v2, twin[1]["v"], "visible samples after two sampled steps", c["id"])
    for i, t in enumerate(twin):
        _within(trh[i], t["h_prob"], b, "p(h|v)", f"{c['id']} step {i}")
        _within(tr[i], t["v_prob"], b, "p(v|h)", f"{c['id']} step {i}")
    assert np.array_equal(final, tr[2]), f"{c['id']}: the mean-field final state is not the traced p(v|h) of its step"


# ---- entries with an epilogue of their own behind a FAST propagation ------------------------------------------------------------------------
def test_free_energy_matches_the_fast_twin(_native):
    c = next(c for c in FC.cases() if c["kind"] == "free")
    r, x = TR._rbm(c), FC.midpoint_operand(c["B"], c["V"], c["H"])
    with _fast(_native), TR._routed(_native, c):
        F = P.N(_native.free_energy(r, P.T(x, DEV)))
        TR._assert_route(_native, c)
    want, bound, _ = FC.twin_free(c)
    _within(F, want, bound, "F(v)", c["id"])


def test_decode_error_matches_the_fast_twin(_native):
    c = next(c for c in FC.cases() if c["kind"] == "sqerr")
    r = TR._rbm(c)
    h, ref, want, bound, _ = FC.twin_sqerr(c)
    with _fast(_native), TR._routed(_native, c):
        got = P.N(_native.decode_sqerr([r], P.T(h, DEV), P.T(ref, DEV)))
        TR._assert_route(_native, c)
    _within(got, want, bound, "sqerr/row", c["id"])
