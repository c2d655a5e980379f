"""GPU: every sampling route at Philox row offsets that are not multiples of 4 (rowoffset_cases.py has the table, the mirror of
finish_lean and the reasoning).  Every case asserts through HipEngine.last_route(), and for a CD pass last_cd(), the kernels and the
epilogue the mirror derives for its offset and draw source.

The references take every decision on PhiloxStream(seed, row0=offset) as the device must (seeds pinned on the CPU with a margin of
1e-6, test_row_offset_cpu.py): samples, categorical picks and bit planes are compared exactly, probabilities within
route_cases.prob_bound(1.0) = 5e-7 of float64, packed statistics within cd_cases.stats_bound per part, parameters after an update
within update_cases.TOL.  The helpers are those of test_routes_gpu.py and test_cd_routes_gpu.py; every call runs on a NaN-filled
workspace.

What the shard sums are held to: the fp32 sum of the four shards' statistics against float64 of the whole batch within
stats_bound(66, .) + 3 * 2^-24 |ref| (rowoffset_cases.sum_bound), and against the device's own whole-batch pass as
test_stats_then_apply_equals_fused_update_for_multi_chunk_batches does (rel-Frobenius 2e-6 or every element within 2e-5).

Group C, lean against general on identical draws.  k1_stream's lean kernel adds the column sums of an 8-row group as
(r0 + r1 + r2 + r3) + (r4 + r5 + r6 + r7) (finish_lean4: two half-waves of four rows each), its general one and every other kernel
r0 .. r7 left to right.  Decisions, planes and dW are bit-equal whatever the epilogue; dc and hpos are bit-equal where the positive
phase is not k1_stream and held to update_cases.STATS_TOL where it is (the order was kept: the other order would put three more
dependent additions behind the cross-half shuffle of the last arriver's tail)."""
import contextlib

import numpy as np
import pytest
import torch

import cd_cases as CC
import parity_cases as P
import route_cases as RC
import rowoffset_cases as RO
import test_cd_routes_gpu as TG
import test_routes_gpu as TR
import update_cases as UC
from golden_utils import assert_close
from oracle.draws import PhiloxStream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731
REACHED = {}                 # instantiation the mirror derives -> a case that ran it (printed at the end of the module)


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
    for what, cid in sorted(REACHED.items()):
        print(f"[row offsets] {what}: {cid}")


@contextlib.contextmanager
def _mode(eng, c):
    from imdbn.engine import native
    mode = eng.mode
    try:
        eng.mode = native.FAST_BF16 if c.get("mode") == "fast" else native.PARITY_F32
        yield
    finally:
        eng.mode = mode


def _poison(eng, V, H, B):
    eng._workspace(torch.device(DEV), V, H, B).view(torch.float32).fill_(float("nan"))


def _rng(c, row0=None):
    from imdbn import engine as E
    return E.PhiloxRng(seed=c["seed"], row0=c["row0"] if row0 is None else row0)


# ---- group A ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RO.cases("gibbs"), ids=IDS)
def test_gibbs_step_matches_float64_at_the_offset(c, _native):
    V, H, B = c["V"], c["H"], c["B"]
    Bp = (B + 63) // 64 * 64
    r, v = TR._rbm(c), P.T(RC.operand(c["operand"], B, V), DEV)
    rng = _rng(c)
    with _mode(_native, c), TR._routed(_native, c):
        v_next, v_prob, h, h_prob = (P.N(t) for t in _native.gibbs_step(r, v, True, True, rng))
        TR._assert_route(_native, c)
        torch.cuda.synchronize()
        hbits = TG._bits(_native.debug_buffer(DEV, V, H, B, "hid_bits", (H + 63) // 64 * 8 * Bp).cpu().numpy(), H, B, Bp)
    r_next, r_prob, r_h, r_hprob = RC.ref_gibbs(c)      # (FAST: float64 on the bf16 weights the case carries)
    b = RC.prob_bound(1.0)
    TR._within(h_prob, r_hprob, b, f"{c['id']}: p(h|v)")
    assert np.array_equal(h, r_h), f"{c['id']}: {int((h != r_h).sum())} hidden samples differ from the reference's decisions, rows {sorted(set(np.argwhere(h != r_h)[:, 0]))[:8]}"
    assert np.array_equal(hbits, r_h), f"{c['id']}: the hidden bit plane does not hold the sample"
    TR._within(v_prob, r_prob, b, f"{c['id']}: p(v|h)")
    for s, e in c["groups"]:
        assert np.array_equal(v_next[:, s:e].argmax(1), r_next[:, s:e].argmax(1)) and (v_next[:, s:e].sum(1) == 1).all(), f"{c['id']}: categorical picks"
    assert np.array_equal(v_next, r_next), f"{c['id']}: {int((v_next != r_next).sum())} visible samples differ from the reference's decisions, rows {sorted(set(np.argwhere(v_next != r_next)[:, 0]))[:8]}"
    assert rng.offset == RC.gibbs_draws(c)


@pytest.mark.parametrize("c", RO.cases("up"), ids=IDS)
def test_sampled_up_step_matches_float64_at_the_offset(c, _native):
    r, v = TR._rbm(c), P.T(RC.operand(c["operand"], c["B"], c["V"]), DEV)
    rng = _rng(c)
    with TR._routed(_native, c):
        p, s = _native.prop_up(r, v, T=1.0, sample=True, rng=rng)
        TR._assert_route(_native, c)
    ref, ref_s = RC.ref_up(c)
    TR._within(P.N(p), ref, RC.prob_bound(1.0), f"{c['id']}: p(h|v)")
    assert rng.offset == 1
    assert np.array_equal(P.N(s), ref_s), f"{c['id']}: {int((P.N(s) != ref_s).sum())} hidden samples differ from the reference's decisions"


# ---- group B ---------------------------------------------------------------------------------------------------------------------------------
def _stats(eng, r, c, t, rng, **kw):
    return eng.cd_stats(r, t, c["k"], rng, **kw).clone()


def _note(c, sampling, row0, rider_ran):
    """Record which sampling k1_stream instantiation the mirror derives for a pass that ran (its carrier asserted through last_cd)."""
    for phase, fam, ep, rider in sampling:
        if fam in RC.STREAMS and ep == "general" and row0 & 3:
            REACHED.setdefault(f"k1_stream {fam} general{' + rider' if rider and rider_ran else ''} ({phase})", f"{c['id']} at row0 {row0}")


@pytest.mark.parametrize("c", RO.cases("shards"), ids=IDS)
def test_cd_pass_shard_by_shard_matches_float64_and_adds_up(c, _native):
    V, H = c["V"], c["H"]
    x = RO.batch(c)
    refs, whole = RO.ref_shards(c)
    n = V * H + 2 * H + V + 1
    with TG._routed(_native, c):
        r = TG._rbm(c)
        ts = [P.T(x[lo:hi], DEV) for lo, hi in RO.SHARDS]
        parts = []
        for i, (s, ref) in enumerate(zip(c["shards"], refs)):
            sc = dict(c, B=s["B"], r=s["r"], id=f"{c['id']} rows {s['lo']}:{s['hi']}")
            _poison(_native, V, H, s["B"])
            rng = _rng(c, s["lo"])
            packed = _stats(_native, r, c, ts[i], rng, data_binary=TG._hint_arg(c["hint"]), next_data=ts[i + 1] if i + 1 < len(ts) else None)
            TG._assert_routes(_native, sc["id"], s["expect"], s["expect_cd"])
            assert rng.offset == c["draws"]
            TG._check_planes(sc, ref, TG._reader(_native, sc), x[s["lo"]:s["hi"]])
            TG._check_packed(sc["id"], V, H, s["B"], packed, ref)
            _note(c, s["sampling"], s["lo"], False)
            if s["lo"] & 3 and s["expect"]["down"] == "k2_stream" and s["expect"]["down_epilogue"] == "general" and not s["r"]["neg_rm"] and not c["groups"]:
                REACHED.setdefault("k2_stream general by the offset alone", sc["id"])
            parts.append(packed)
        assert not _native._pf, "a hint of another shape was put on record"
        # the whole batch at offset 0, and the fp32 sum of the shards
        rng = _rng(c, 0)
        full = _stats(_native, r, c, P.T(x, DEV), rng, data_binary=TG._hint_arg(c["hint"]))
        TG._assert_routes(_native, c["id"], c["expect"], c["expect_cd"])
        TG._check_packed(f"{c['id']} whole", V, H, RO.B_ROWS, full, whole)
        total = P.N(parts[0] + parts[1] + parts[2] + parts[3])[:n]
        want, bad = CC.packed64(whole), []
        for name, sl in CC.packed_parts(V, H).items():
            d, bound = np.abs(total[sl].astype(F64) - want[sl]), RO.sum_bound(want[sl])
            print(f"{c['id']} shard sum {name}: max|d| {float(d.max()):.2e} (bound {float(bound.min()):.2e})")
            if (d > bound).any():
                bad.append(f"{name}: max|d| {float(d.max()):.3e} at bound {float(bound[d.argmax()]):.3e}")
        assert not bad, f"{c['id']}: shard sum against float64: " + "; ".join(bad)
        assert_close(total, P.N(full)[:n], 2e-6, f"{c['id']}: shard sum against the device's whole batch", atol=2e-5)
        # a hint of the batch's own shape at offset 7, and the hinted rows read from the slot at offset 21
        hd = c["hinted"]
        if hd:
            a, b, e = hd["rows"]
            hc = dict(c, B=hd["B"], r=hd["r"])
            _poison(_native, V, H, hd["B"])
            t0, t1 = P.T(x[a:b], DEV), TG._tagged(x[b:e], c["hint"])
            rng = _rng(c, a)
            p0 = _stats(_native, r, c, t0, rng, data_binary=TG._hint_arg(c["hint"]), next_data=t1)
            TG._assert_routes(_native, f"{c['id']} hinted rows {a}:{b}", *hd["first"])
            TG._check_packed(f"{c['id']} hinted rows {a}:{b}", V, H, hd["B"], p0, refs[1])
            TG._check_slot(hc, dict(i=0, next_slot=1, form=hd["form"]), TG._reader(_native, hc), x[b:e])
            _note(c, hd["sampling"], a, hd["first"][1]["next"] == "k1_stream")
            rng = _rng(c, b)
            p1 = _stats(_native, r, c, t1, rng)
            TG._assert_routes(_native, f"{c['id']} rows {b}:{e} from the slot", *hd["second"])
            TG._check_packed(f"{c['id']} rows {b}:{e} from the slot", V, H, hd["B"], p1, RO.ref_rows(c, b, e))
            assert not _native._pf


@pytest.mark.parametrize("c", RO.cases("step"), ids=IDS)
def test_three_cd_steps_at_offset_21_match_float64(c, _native):
    st = CC.state(c["route_name"])
    rng = _rng(c)
    with TG._routed(_native, c):
        r = TG._rbm(c, step=True)
        for i in range(RO.STEP_STEPS):
            x = RO.step_batch(c, i)
            ref = RO.ref_rows(c, 0, 0, row0=c["row0"], offset=i * c["draws"], st=st, x=x)
            loss = _native.cd_step(r, P.T(x, DEV), CC.STEP_LR, CC.STEP_MOM, c["k"], rng)
            TG._assert_routes(_native, f"{c['id']} step {i}", c["expect"], c["expect_cd"])
            assert rng.offset == (i + 1) * c["draws"]
            mean = ref["sqerr"] / (c["B"] * c["V"])
            assert abs(float(loss) - mean) <= 1e-5 * mean, (float(loss), mean)
            got = TG._state(r)
            TG._close(f"{c['id']} step {i}", got, TG._step_ref(c, st, ref))
            st = got      # the next step's reference starts from the fp32 state the device holds


@pytest.mark.parametrize("c", RO.cases("factors"), ids=IDS)
def test_cd_factors_block_at_offset_21_holds_the_references_decisions(c, _native):
    x = RO.rows(c)
    ref = RO.ref_rows(c, 0, 0, row0=c["row0"], x=x)
    with TG._routed(_native, c):
        r = TG._rbm(c)
        assert _native.factor_mode_ok(r, c["B"])
        rng = _rng(c)
        block = _native.cd_factors(r, P.T(x, DEV), c["k"], rng).clone()
        TG._assert_routes(_native, c["id"], c["expect"], c["expect_cd"])
        assert rng.offset == c["draws"]
        torch.cuda.synchronize()
        read, ws_read = TG._block_reader(_native, c, block), TG._reader(_native, c)
        # (the factor block carries the first term of vis_tr1 and no bit plane: vbits is checked on the workspace)
        TG._check_planes(c, ref, lambda name, nb: ws_read(name, nb) if name == "vis_bits1" else read(name, nb), x)


# ---- group C ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RO.cases("lean"), ids=IDS)
def test_lean_and_general_epilogues_agree_on_identical_draws(c, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    Bp = (B + 63) // 64 * 64
    x = RO.rows(c)
    ref = RO.ref_rows(c, 0, 0, row0=c["row0"], x=x)
    planes = [("vis_tr1", V * Bp * 2), ("hid_tr0", 3 * H * Bp * 2), ("hid_tr1", 3 * H * Bp * 2), ("hid_bits", (H + 63) // 64 * 8 * Bp)]
    if c["r"]["vbits"]:
        planes.append(("vis_bits1", (V + 63) // 64 * 8 * Bp))

    def run(rng, expect):
        _poison(_native, V, H, B)
        packed = _stats(_native, r, c, P.T(x, DEV), rng)
        TG._assert_routes(_native, c["id"], expect, c["expect_cd"])
        read = TG._reader(_native, c)
        TG._check_planes(c, ref, read, x)
        TG._check_packed(c["id"], V, H, B, packed, ref)
        return P.N(packed)[: V * H + 2 * H + V + 1], {name: read(name, nb).copy() for name, nb in planes}

    with TG._routed(_native, c):
        r = TG._rbm(c)
        gen, gp = run(_rng(c), c["expect"])
        lean, lp = run(E.ReplayRng(PhiloxStream(c["seed"], row0=c["row0"])), c["expect_tape"])
    for name, _ in planes:
        assert np.array_equal(gp[name], lp[name]), f"{c['id']}: {name} differs between the epilogues"
    parts = CC.packed_parts(V, H)
    assert np.array_equal(gen[parts["dW"]], lean[parts["dW"]]), f"{c['id']}: dW is not bit-equal"
    assert np.array_equal(gen[parts["db"]], lean[parts["db"]]), f"{c['id']}: db is not bit-equal"
    sq = float(lean[parts["sqerr"]][0])
    assert abs(float(gen[parts["sqerr"]][0]) - sq) <= 1e-5 * sq
    for name in ("dc", "hpos"):
        g, l = gen[parts[name]].astype(F64), lean[parts[name]].astype(F64)
        print(f"{c['id']}: {name} differs at {int((g != l).sum())} of {g.size} columns, max|d| {float(np.abs(g - l).max()):.3e}")
        if c["same_order"]:
            assert np.array_equal(g, l), f"{c['id']}: {name} is not bit-equal though both epilogues add eight rows per thread in row order"
        else:
            assert (np.abs(g - l) <= UC.STATS_TOL["rel"] * np.abs(l) + UC.STATS_TOL["atol"]).all(), f"{c['id']}: {name}"


# ---- group D ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RO.cases("chain"), ids=IDS)
def test_wide_chain_matches_oracle_at_the_offset(c, _native):
    from imdbn import engine as E
    (want, st, draws), _, _ = RO.run_oracle(c)
    r = TR._rbm(c)
    vk, km, mu = RC.chain_inputs(c)
    rng = _rng(c)
    with TR._routed(_native, c), E.use_rng(rng):
        r._mu_pull = {"mu_k": P.T(mu, DEV), "eta0": 0.15} if mu is not None else None
        got = P.N(getattr(r, c["method"])(P.T(vk, DEV), P.T(km, DEV), **c["kw"]))
        TR._assert_route(_native, c)
    assert rng.offset == draws and rng.row0 == c["row0"]
    assert np.isfinite(got).all()
    assert_close(got, want, 1e-4, f"{c['id']}: {c['method']}", atol=2e-6)


def test_pt_sweep_of_five_chains_by_three_replicas_with_a_softmax_group_is_the_twins(_native):
    from likelihood_gpu import dev, device_rbm
    pc = RO.pt_case()
    t = RO.pt_run(pc, pc["seed"])
    r, x, rng = device_rbm(pc), dev(pc["state"]), _rng(pc, 0)
    tries, accs = _native.pt_sweep(r, x, pc["betas"], pc["sweeps"], rng)
    torch.cuda.synchronize()
    assert rng.offset == pc["sweeps"] * (2 + len(pc["groups"]) + 1)
    off = np.argwhere(x.cpu().numpy() != t["state"])
    assert off.size == 0, f"{len(off)} state elements off the twin, rows {sorted(set(off[:, 0]))} (replica = row // {pc['M']})"
    assert tries.tolist() == t["tries"].tolist() and accs.tolist() == t["accs"].tolist()


@pytest.mark.parametrize("name", RO.REVERSE_NAMES)
def test_reverse_ais_chunks_of_three_chains_equal_one_chunk_and_the_twin(name, _native):
    from imdbn.utils import likelihood as LK
    from likelihood_gpu import base_bias, close, device_rbm
    c = RO.reverse_case(name)
    want, _, _ = RO.reverse_run(c, c["seed"])
    r, x = device_rbm(c), torch.from_numpy(c["rows"]).to(DEV)
    kw = dict(n_chains=RO.REVERSE_CHAINS, betas=c["betas"], base_vis_bias=base_bias(c), seed=c["seed"])
    one = LK.reverse_ais_log_likelihood(r, x, max_rows=4096, **kw)
    many = LK.reverse_ais_log_likelihood(r, x, max_rows=RO.REVERSE_MAX_ROWS, **kw)
    for k in ("ll", "ess", "logw"):
        assert torch.equal(one[k], many[k]), f"{name}: {k} depends on the chunking"
    # test_reverse_ais_gpu.py's tolerance: 2 H 1e-5 + 1e-9 |logw|
    close(many["logw"].cpu().numpy(), want, 2 * c["H"] * 1e-5 + 1e-9 * np.abs(want), f"{name}: logw against the twin at the chunk offsets")
