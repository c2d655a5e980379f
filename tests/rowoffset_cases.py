"""Cases shared by test_row_offset_cpu.py and test_row_offset_gpu.py: every sampling route at Philox row offsets that are not
multiples of 4 -- what a data-parallel shard, a replica of pt_sweep or a chunk of the reverse-AIS driver hands the kernels as `row0`.

The offset changes two things on the device.  Which Philox block an element comes from: four rows of a GLOBAL 4-row group share a
block of uniforms, two rows of a global pair a block of normals, and the fast paths of draw_uniform_rows / draw_normal_rows2
(csrc/common.hpp) apply only where row0 + b0 is aligned and the tile is whole.  And which epilogue the streaming kernels run:
finish_lean (csrc/host_prop.hpp) refuses the lean one to a launch that samples from Philox at row0 & 3 != 0.  finish_lean() below
restates that function term by term; epilogue() and expect_at() derive from it what HipEngine.last_route() / last_cd() must report
-- never copied from a run.

Offsets: 1, 2, 3, 5, 6 (every residue mod 4, both parities of the pair, both values of g0 & 2), 4 as the control that stays lean,
and 2^32 + 3 once per call family: the Philox counter word is (uint32_t)(global row >> 2), here 2^30, so the row must stay 64 bits
wide up to the shift -- cut to 32 bits before it, the device would draw the rows of offset 3.

  A   eng.gibbs_step and eng.prop_up(sample=True) on the shapes of route_cases, batches 1 (a row that is not the first of its
      group), 7 (a ragged only tile), 33 and 66 (second 64-row chunk at row0 + 64, ragged last tile), rotated so that every route meets
      every residue and every batch.  FAST mode (one bf16 weight term, round to nearest even) on 130 x 72 and 1040 x 36 with a 0/1
      operand, against float64 on the rounded weights.  Both propagations of a Gibbs step write a final state: the streaming kernels
      are general at every offset, which the mirror must say too.
  B   the CD pass shard by shard: a 66-row batch cut at 0, 7, 21, 46, 66 (offsets 0, 3, 1, 2 mod 4), every route of cd_cases.ROUTES,
      CD-1 everywhere and CD-2 on the routes with a streaming kernel.  Each shard is handed the following shard as next_data: the
      host accepts a hint only when it has the batch's own shape (HipEngine._prefetch_opts), so the mirror names carrier "none"
      there.  On the routes that prefetch, the 14 rows at offset 7 are run once more with the 14 rows behind them as a hint of their
      own shape, and those are then read from the slot at offset 21: the preparation rides, at CD-2, on the negative-phase
      k1_stream that samples (cd_phases: it == 0 && next_on_k1), which at row0 & 3 != 0 is the rider-plus-general instantiation.
      Three cd_step updates at offset 21, and the cd_factors block at offset 21.
  C   the same pass from Philox at offset r (general on the streams) and from a tape of the same uniforms (lean whatever the offset).
  D   callers that manufacture odd offsets: pt_sweep with 5 chains x 3 replicas and a softmax group (pcd_cases has M = 5, 6, 67, 3
      without one); the chunked reverse-AIS driver with 3 chains; wide-layer chains whose normals lose their pair alignment.

Every seed is pinned with the oracle alone, by the rule of route_cases / cd_cases: the first seed >= 1 at which the smallest
Bernoulli and categorical margins of the whole case -- all four shards, the whole batch and every step -- are at least MARGIN.
`python tests/rowoffset_cases.py` prints the table; test_row_offset_cpu.py asserts it."""
import functools

import numpy as np

import oracle.rbm_oracle as O
import cd_cases as CC
import route_cases as RC
import update_cases as UC
from oracle.draws import CATEGORICAL_MARGIN, PhiloxStream

F32, F64 = np.float32, np.float64
MARGIN = RC.MARGIN
OFFSETS = (1, 2, 3, 5, 6)
CONTROL = 4
BIG = 2 ** 32 + 3
A_OFFSETS = OFFSETS + (CONTROL,)
A_BATCHES = (1, 7, 33, 66)


# ---- the mirror of finish_lean ------------------------------------------------------------------------------------------------------------
def finish_lean(simple, vmode, out_final, rm_written, tape, row0):
    """csrc/host_prop.hpp finish_lean(), term by term: FinishArgs::simple; mean-field or a plain sample; no fp32 final state; no
    K16-blocked operand form written (rm_src && op.rm); and the draws -- none, a tape, or Philox from an aligned row."""
    return bool(simple and vmode in (0, 1) and not out_final and not rm_written and (vmode == 0 or tape or (row0 & 3) == 0))


def epilogue(route, simple, vmode, out_final, rm_written, tape, row0):
    """What last_route() reports for a launch: the streaming kernels pass finish_lean(), every other kernel branches on simple."""
    lean = finish_lean(simple, vmode, out_final, rm_written, tape, row0) if route in RC.STREAMS else simple
    return "lean" if lean else "general"


def expect_at(r, hint, row0, tape=False, next_hint=None, slot=0, forward=False):
    """cd_cases.expect_of with the draw source: (last_route() fields, last_cd() record) of a CD pass at global row `row0`.
    The last K2 samples (vmode 1) and writes vis_rm[1] where r["neg_rm"]; with a softmax group prop() gives it an fp32 final state.
    The last K1 is mean-field (the forward of cd_step too): no draw, so no offset reaches it."""
    route, cd = CC.expect_of(r, hint, next_hint, slot, forward)
    g = bool(r["groups"])
    route["down_epilogue"] = epilogue(route["down"], not g, 1, g, r["neg_rm"], tape, row0)
    route["up_epilogue"] = epilogue(route["up"], True, 0, False, False, tape, row0)
    return route, cd


def sampling_k1(r, hint, k, row0, tape=False, has_next=False):
    """The K1 launches of a CD-k pass that sample, as (phase, family, epilogue, carries the preparation): the positive phase and, with
    k >= 2, the negative-phase K1 of every iteration but the last.  Both write the one-term hid_rm unless their sample leaves as a bit
    plane (hid_bits_out: always, without no_bits).  last_route() does not see them -- the last K1 overwrites the record -- so this
    is what the launcher must have chosen by cd_phases and launch_k1_stream as written."""
    out = []
    rm = bool(r["opts"]["no_bits"])
    fam = CC.data_up(r, hint)
    out.append(("pos", fam, epilogue(fam, True, 1, False, rm, tape, row0), False))
    for it in range(k - 1):
        fam = CC.neg_up(r)
        out.append((f"neg{it}", fam, epilogue(fam, True, 1, False, rm, tape, row0), bool(has_next and it == 0 and r["next_on_k1"])))
    return out


def rne_bf16(x):
    """fp32 -> the nearest bf16 (ties to even) as fp32: csrc/common.hpp bf16_rne, the weights of FAST mode."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    out = u.astype(np.uint32).view(F32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fast_weights(V, H):
    return rne_bf16(RC.params(V, H)[0])


# ---- group A: single Gibbs steps and sampled up-steps ----------------------------------------------------------------------------------
A_ROUTES = [   # name, V, H, options, groups
    ("130x72", 130, 72, {}, ()),                               # fused / k2_stream
    ("1040x36", 1040, 36, {}, ()),                             # stream_real / k2_stream
    ("1040x36-no_k1s", 1040, 36, {"no_k1s": 1}, ()),           # partial4 + finish (finish_rows<2>)
    ("1040x36-no_k2s", 1040, 36, {"no_k2s": 1}, ()),           # bit-plane down_fused
    ("1040x36-no_bits", 1040, 36, {"no_bits": 1}, ()),         # bf16-form down_fused
    ("1040x37", 1040, 37, {}, ()),                             # scalar rows on both sides
    ("1040x36-group", 1040, 36, {}, ((1030, 1040),)),          # finish_groups; categorical draw keyed on row0
    ("1040x36-k2s24", 1040, 36, {"k2s_rows": 24}, ()),         # k2_stream, two MFMA tiles per block
]
A_FAST = ("130x72", "1040x36")
A_UP = ("130x72", "1040x36", "1040x36-no_k1s", "1040x37")      # one shape per up family a sampled prop_up can take here
A_OPTION_DEFAULTS = {"no_k1s": 0, "no_k2s": 0, "no_bits": 0, "k2s_rows": 0}


def _a_route(V, H, opts, groups):
    """(up family, down family) of a Gibbs step with a sampled h: the data are read as bf16 terms (no bit plane is prepared), the
    hidden sample leaves K1 as a bit plane unless no_bits."""
    r = CC.route_of(V, H, opts, groups)
    return CC.data_up(r, "real"), CC.cd_down(r)


def _gibbs(name, V, H, opts, groups, B, row0, mode):
    up, down = _a_route(V, H, opts, groups)
    g = bool(groups)
    c = dict(kind="gibbs", id=f"gibbs-{name}-B{B}-r{'big' if row0 == BIG else row0}{'-fast' if mode == 'fast' else ''}", route_name=name,
             V=V, H=H, B=B, row0=row0, mode=mode, sample_h=True, sample_v=True, groups=groups, opts=opts,
             operand="binary" if mode == "fast" else "mixed",
             # both propagations write a final state next to the probabilities; K1 also the one-term hid_rm unless a bit plane leaves
             route={"up": up, "up_epilogue": epilogue(up, True, 1, True, bool(opts.get("no_bits")), False, row0), "down": down,
                    "down_epilogue": epilogue(down, not g, 1, True, False, False, row0), "finish_groups": g})
    if mode == "fast":
        c["W"] = fast_weights(V, H)
    return c


def _up(name, V, H, opts, B, row0):
    up, _ = _a_route(V, H, opts, ())
    return dict(kind="up", id=f"up-{name}-B{B}-r{'big' if row0 == BIG else row0}", route_name=name, V=V, H=H, B=B, row0=row0, mode="exact",
                T=1.0, sample=True, operand="mixed", groups=(), opts=opts,
                route={"up": up, "up_epilogue": epilogue(up, True, 1, True, False, False, row0)})


def a_cases():
    out = []
    for ri, (name, V, H, opts, groups) in enumerate(A_ROUTES):
        for mode in ("exact", "fast") if name in A_FAST else ("exact",):
            for i, row0 in enumerate(A_OFFSETS):
                out.append(_gibbs(name, V, H, opts, groups, A_BATCHES[(i + ri + (mode == "fast")) % 4], row0, mode))
        if name in A_UP:
            for i, row0 in enumerate(A_OFFSETS):
                out.append(_up(name, V, H, opts, A_BATCHES[(i + ri + 2) % 4], row0))
    out.append(_gibbs("1040x36", 1040, 36, {}, (), 7, BIG, "exact"))
    out.append(_gibbs("130x72", 130, 72, {}, (), 33, BIG, "exact"))
    out.append(_up("1040x36", 1040, 36, {}, 33, BIG))
    return out


# ---- group B: the CD pass shard by shard ---------------------------------------------------------------------------------------------------
B_ROWS = 66
CUTS = (0, 7, 21, 46, 66)
SHARDS = tuple(zip(CUTS[:-1], CUTS[1:]))
HINTED = (7, 21, 35)          # rows [7, 21) hinted with rows [21, 35), which are then read from the slot at offset 21
STEP_ROW0, STEP_ROWS, STEP_STEPS = 21, 25, 3
STEP_ROUTES = ("1040x36", "1040x36-no_bits")
FACTOR_ROUTES = ("1040x36", "130x72")


def streaming(r):
    return bool(r["k1s"] or r["k2s_cd"])


def b_cases():
    out = []
    for ri, (name, V, H, opts, groups) in enumerate(CC.ROUTES):
        r66 = CC.route_of(V, H, opts, groups, B_ROWS)
        for kind in ("binary", "mixed"):
            for k in (1, 2) if streaming(r66) else (1,):
                hint = {"binary": ("binary", "unknown"), "mixed": ("unknown", "real")}[kind][(ri + k) % 2]
                shards = []
                for lo, hi in SHARDS:
                    r = CC.route_of(V, H, opts, groups, hi - lo)
                    route, cd = expect_at(r, hint, lo)      # the following shard has another shape: the host drops the hint
                    shards.append(dict(lo=lo, hi=hi, B=hi - lo, r=r, expect=route, expect_cd=cd, sampling=sampling_k1(r, hint, k, lo)))
                whole, whole_cd = expect_at(r66, hint, 0)
                c = dict(kind="shards", id=f"shards-{name}-{kind}-k{k}-{hint}", route_name=name, V=V, H=H, B=B_ROWS, k=k, data=kind, hint=hint,
                         opts=opts, groups=groups, r=r66, shards=shards, expect=whole, expect_cd=whole_cd, draws=1 + k * (2 + len(groups)),
                         hinted=None)
                if kind == "mixed" and k == (2 if streaming(r66) else 1) and r66["prefetch"]:
                    a, b, e = HINTED
                    r = CC.route_of(V, H, opts, groups, b - a)
                    first, first_cd = expect_at(r, hint, a, next_hint=hint)
                    second, second_cd = expect_at(r, hint, b, slot=1)
                    c["hinted"] = dict(rows=HINTED, B=b - a, r=r, first=(first, first_cd), second=(second, second_cd),
                                       form=CC.slot_form(r, hint), sampling=sampling_k1(r, hint, k, a, has_next=True))
                out.append(c)
    return out


def step_cases():
    out = []
    for name, V, H, opts, groups in CC.ROUTES:
        if name in STEP_ROUTES:
            r = CC.route_of(V, H, opts, groups, STEP_ROWS)
            route, cd = expect_at(r, "unknown", STEP_ROW0)
            out.append(dict(kind="step", id=f"step-{name}-r{STEP_ROW0}", route_name=name, V=V, H=H, B=STEP_ROWS, row0=STEP_ROW0, k=1,
                            data="mixed", hint="unknown", opts=opts, groups=groups, r=r, expect=route, expect_cd=cd, draws=3))
    return out


def factor_cases():
    out = []
    for name, V, H, opts, groups in CC.ROUTES:
        if name in FACTOR_ROUTES:
            r = CC.route_of(V, H, opts, groups, STEP_ROWS)
            route, cd = expect_at(r, "unknown", STEP_ROW0)
            out.append(dict(kind="factors", id=f"factors-{name}-r{STEP_ROW0}", route_name=name, V=V, H=H, B=STEP_ROWS, row0=STEP_ROW0, k=1,
                            data="mixed", hint="unknown", opts=opts, groups=groups, r=r, expect=route, expect_cd=cd, draws=3))
    return out


def batch(c):
    """The 66-row batch of a group B / C case (route_cases.operand)."""
    return CC.operand(c["data"], B_ROWS, c["V"])


def rows(c):
    """The rows a `step` / `factors` / `lean` case runs: STEP_ROWS (or its B) rows of the batch from its offset's shard on."""
    return batch(c)[STEP_ROW0:STEP_ROW0 + c["B"]] if c["kind"] in ("step", "factors") else batch(c)[:c["B"]]


def step_batch(c, i):
    x = np.roll(rows(c), i, axis=0).copy()
    x.setflags(write=False)
    return x


def ref_rows(c, lo, hi, row0=None, offset=0, st=None, x=None):
    """cd_cases.ref_pass of rows [lo, hi) of the case's batch, keyed from global row `row0` (lo where none is given)."""
    st = st or CC.state(c["route_name"])
    ps = PhiloxStream(c["seed"], offset=offset, row0=lo if row0 is None else row0)
    out = CC.ref_pass(st["W"], st["hid_bias"], st["vis_bias"], batch(c)[lo:hi] if x is None else x, c["k"], c["groups"], ps)
    assert ps.offset == offset + c["draws"]
    return out


@functools.lru_cache(maxsize=None)
def _ref_shards(cid):
    c = by_id(cid)
    return tuple(ref_rows(c, lo, hi) for lo, hi in SHARDS), ref_rows(c, 0, B_ROWS)


def ref_shards(c):
    """(ref_pass per shard at its offset, ref_pass of the whole batch at offset 0), computed once; read-only."""
    return _ref_shards(c["id"])


def sum_bound(ref_part):
    """|fp32 sum of the four shards' statistics - float64 of the whole batch|: stats_bound of 66 rows -- the per-shard bounds add up to
    no more, their row counts sum to 66 and their summation terms are taken on the shard's own smaller magnitudes -- plus the error of
    the three fp32 additions."""
    return CC.stats_bound(B_ROWS, ref_part) + 3 * 2.0 ** -24 * np.abs(ref_part)


# ---- group C: lean against general on identical draws ----------------------------------------------------------------------------------------
C_OFFSETS = (1, 3)
C_SHAPES = (("1040x36", 33, 2), ("1040x36", 66, 1), ("130x72", 33, 1))      # route, batch, CD depth


def c_cases():
    out = []
    for name, B, k in C_SHAPES:
        _, V, H, opts, groups = next(x for x in CC.ROUTES if x[0] == name)
        r = CC.route_of(V, H, opts, groups, B)
        for row0 in C_OFFSETS:
            philox, cd = expect_at(r, "unknown", row0)
            tape, cd_t = expect_at(r, "unknown", row0, tape=True)
            assert cd == cd_t
            out.append(dict(kind="lean", id=f"lean-{name}-B{B}-k{k}-r{row0}", route_name=name, V=V, H=H, B=B, k=k, row0=row0, data="mixed",
                            hint="unknown", opts=opts, groups=groups, r=r, expect=philox, expect_tape=tape, expect_cd=cd, draws=1 + 2 * k,
                            # the positive-phase K1 decides the bits of hpos / dc: k1_stream's lean kernel adds the column sums of an
                            # 8-row group as (r0 + r1 + r2 + r3) + (r4 + .. + r7) (finish_lean4), its general one left to right
                            same_order=CC.data_up(r, "unknown") not in RC.STREAMS))
    return out


# ---- group D: callers that manufacture odd offsets ----------------------------------------------------------------------------------------
D_CALLS = ("cg-hv", "nmf-mu", "cga")
D_ROUTES = ("default", "no_k1s")
D_OFFSETS = (3, 5)
D_BATCH = 27


def d_chain_cases():
    """The wide joint layer (route_cases.CHAIN_V, one launch per half step) at odd offsets: nmf-mu draws normals, which an odd offset
    takes off the pair alignment of draw_normal_rows2."""
    out = []
    for c in RC.cases("chain"):
        if c["call"] in D_CALLS and c["variant"] in D_ROUTES:
            for i, row0 in enumerate(D_OFFSETS):
                d = dict(c, id=f"{c['call']}-{c['variant']}-B{D_BATCH}-r{row0}", B=D_BATCH, row0=row0, known=("labels", "features")[i],
                         route_name=c["variant"], mode="exact")
                out.append(d)
    return out


# (V, H, M, R, groups, weight scale): pcd_cases' smallest shape with a softmax group, at 5 chains x 3 replicas -- replica offsets 5, 10
PT_GROUP = dict(name="groups-m5", V=26, H=40, M=5, R=3, groups=((20, 26),), scale=0.5, sweeps=2)
# the chunked reverse-AIS driver: 7 rows x 3 chains = 21 engine rows (<= 64: the propagations' slice count is that of one chunk either
# way); max_rows = 6 gives chunks of 2 rows starting at global rows 0, 6, 12, 18
REVERSE_NAMES = ("tiny_bA", "group")
REVERSE_CHAINS, REVERSE_ROWS, REVERSE_MAX_ROWS = 3, 7, 6


def reverse_case(name):
    """The anneal_cases.REVERSE case `name` with REVERSE_ROWS test rows of its own and the seed pinned here."""
    import anneal_cases as Cs
    c = dict(Cs.case(Cs.REVERSE, name))
    c["rows"] = Cs.start_rows(REVERSE_ROWS, c["V"], 8, c["groups"])
    c["seed"] = SEEDS.get(f"reverse-{name}", 1)
    return c


def reverse_run(c, seed):
    """The twin on the engine rows of every chunk at the chunk's offset: (logw [rows, chains], Bernoulli margin, categorical margin)."""
    import anneal_oracle as A
    M, per = REVERSE_CHAINS, max(1, REVERSE_MAX_ROWS // REVERSE_CHAINS)
    parts, bm, cm = [], float("inf"), float("inf")
    for s in range(0, REVERSE_ROWS, per):
        x = np.repeat(c["rows"][s:s + per], M, axis=0)
        logw, _, m, k = A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], c["groups"], c["betas"], x, PhiloxStream(seed, row0=s * M))
        parts.append(logw); bm = min(bm, m); cm = min(cm, k)
    return np.concatenate(parts).reshape(REVERSE_ROWS, M), bm, cm


def reverse_ok(bm, cm):
    import anneal_cases as Cs
    return bm >= Cs.MARGIN and cm >= Cs.CAT_MARGIN


def pt_case():
    """The dict pcd_cases.case builds, for PT_GROUP."""
    from anneal_cases import params, start_rows
    import pcd_cases as Cs
    p = PT_GROUP
    W, b, c, _ = params(p["V"], p["H"], 990, p["scale"])
    groups = [tuple(x) for x in p["groups"]]
    return dict(name=p["name"], V=p["V"], H=p["H"], M=p["M"], R=p["R"], groups=groups, W=W, b=b, c=c, seed=SEEDS.get("pt-groups-m5", 1),
                betas=np.asarray(Cs.LADDERS[p["R"]], F32), state=start_rows(p["R"] * p["M"], p["V"], 991, groups), sweeps=p["sweeps"])


def pt_run(c, seed):
    """The twin's sweeps on pt_case(): dict(state, tries, accs, bern, cat, exch)."""
    import pcd_oracle as T
    O.reset_margin()
    state, tries, accs, exch = T.pt_sweep(T.rbm_state(c), c["state"], c["betas"], c["sweeps"], PhiloxStream(seed))
    return dict(state=state, tries=tries, accs=accs, exch=exch, bern=O.BERNOULLI_MARGIN["min"], cat=CATEGORICAL_MARGIN["min"])


def pt_ok(c, t):
    import pcd_cases as Cs
    return t["bern"] > MARGIN and t["cat"] > MARGIN and t["exch"] > Cs.exchange_margin(c["H"])


# ---- the fp32 oracle (seed pinning, and the CPU test's comparison) ---------------------------------------------------------------------------
def _cd_oracle_state(c):
    return CC._oracle_state(c)


def run_oracle(c):
    """The case on the fp32 oracle with its seed: (results, smallest Bernoulli margin, smallest categorical margin).  `shards`: one
    cd_statistics per shard at its offset, then the whole batch at offset 0; `step`: STEP_STEPS updates; `lean` / `factors`: one pass."""
    O.reset_margin()
    k = c["kind"]
    if k == "gibbs":
        res = RC.oracle_gibbs(c)
    elif k == "up":
        res = RC.oracle_up(c)
    elif k == "chain":
        res = RC.oracle_chain(c)
    elif k == "shards":
        x = batch(c)
        res = [O.cd_statistics(_cd_oracle_state(c), x[lo:hi], c["k"], PhiloxStream(c["seed"], row0=lo)) for lo, hi in SHARDS]
        res.append(O.cd_statistics(_cd_oracle_state(c), x, c["k"], PhiloxStream(c["seed"])))
    elif k == "step":
        o, ps, res = _cd_oracle_state(c), PhiloxStream(c["seed"], row0=c["row0"]), []
        for i in range(STEP_STEPS):
            res.append(O.cd_statistics(o, step_batch(c, i), c["k"], ps))
            O.apply_cd_update(o, res[-1], CC.STEP_LR, CC.STEP_MOM, c["B"], True)
    else:
        assert k in ("lean", "factors"), k
        res = [O.cd_statistics(_cd_oracle_state(c), rows(c), c["k"], PhiloxStream(c["seed"], row0=c["row0"]))]
    return res, O.BERNOULLI_MARGIN["min"], CATEGORICAL_MARGIN["min"]


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
# Philox seed per case: the first seed >= 1 whose margins pass (printed by `python tests/rowoffset_cases.py`); cases not listed take 1
SEEDS = {
    "up-1040x36-B66-r6": 2,
    "gibbs-1040x36-no_k2s-B66-r6": 2,
    "gibbs-1040x36-k2s24-B66-r6": 2,
}


@functools.lru_cache(maxsize=None)
def _all():
    cs = a_cases() + b_cases() + step_cases() + factor_cases() + c_cases() + d_chain_cases()
    for c in cs:
        c["seed"] = SEEDS.get(c["id"], 1)
    assert len({c["id"] for c in cs}) == len(cs), "duplicate case id"
    return tuple(cs)


def cases(kind=None):
    return [c for c in _all() if kind is None or c["kind"] == kind]


def by_id(cid):
    return next(c for c in _all() if c["id"] == cid)


def pinned_seeds():
    """SEEDS as the rule gives it: per case the first seed >= 1 whose margins are at least MARGIN, listed where it is not 1."""
    out = {}
    for c in _all():
        keep = c["seed"]
        try:
            for seed in range(1, 200):
                c["seed"] = seed
                _, bm, cm = run_oracle(c)
                if bm >= MARGIN and cm >= MARGIN:
                    break
            else:
                raise SystemExit(f"no seed for {c['id']}")
        finally:
            c["seed"] = keep
        if seed != 1:
            out[c["id"]] = seed
    pc = pt_case()
    for seed in range(1, 200):
        if pt_ok(pc, pt_run(pc, seed)):
            break
    else:
        raise SystemExit("no seed for pt-groups-m5")
    if seed != 1:
        out["pt-groups-m5"] = seed
    for name in REVERSE_NAMES:
        rc = reverse_case(name)
        for seed in range(1, 200):
            if reverse_ok(*reverse_run(rc, seed)[1:]):
                break
        else:
            raise SystemExit(f"no seed for reverse-{name}")
        if seed != 1:
            out[f"reverse-{name}"] = seed
    return out


if __name__ == "__main__":      # pin the seeds: prints the SEEDS table
    print("SEEDS = {")
    for k, v in pinned_seeds().items():
        print(f'    "{k}": {v},')
    print("}")
