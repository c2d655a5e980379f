"""Cases shared by test_cd_routes_cpu.py and test_cd_routes_gpu.py: the CD pass (cd_phases / cd_prologue, csrc/engine.hip) on every
route make_route (csrc/host_layout.hpp) can give it, the next-batch prefetch included, against a float64 reference of rbm.py:199-209.

Each case names what HipEngine.last_route() (the LAST K2 with its epilogue and finish_groups, the final K1) and HipEngine.last_cd()
(positive-phase K1, first K2, last K1, carrier of the next batch's preparation, data slot, per-item preparation) must report after
the pass.  Both are derived here by route_of(), a Python mirror of make_route and of the choices prop() makes from it -- never copied
from a run.  The mirror assumes CUS compute units (the fused K2's rows per block and k1_stream's slices depend on the count); the GPU
tests assert the device has that many.

Parameters: W, biases from route_cases.params, momenta from update_cases.params.  Shapes (V x H), the smallest that cross each edge:

  130 x 72     gemm_up_fused with float4 rows, k2_stream as the CD K2; no k1_stream, so a next batch is prepared by a prep_operand
               launch of its own
  130 x 70     H % 4 != 0: scalar kernels on both sides, no prefetch: a hint is ignored
  1040 x 36    smallest Vpad > 1024: k1_stream (5 slices) and k2_stream; the negative K1 reads only the bit plane (no vis_rm[1]);
               the preparation rides on the negative-phase k1_stream
     no_bits            the fused K2 on the bf16 form; gemm_down_fused_next carries the preparation
     no_bits, down_rows 8 / 12    vbits true / false from the tile height alone (12: the negative K1 is the partial kernel)
     no_k2s             the fused K2 on the bit plane
     no_k1s             partial4 up; vis_rm[1] written and read
     no_k1s_real        real-valued data take the partial kernels, the bit planes k1_stream
     no_adaptive        unknown content read from the bf16 terms throughout;  k1s_force_na: bit planes on the bf16-capable instantiation
     group (1030, 1040) a softmax group turns vbits off; finish_groups and categorical draws
  1040 x 37    scalar rows at wide V: partial up, fused K2
  1100 x 12    adaptive_ok false (9 spans of the update kernel, 5 positive-phase blocks)

Batches 33 (ragged chunk), 64, 130 (three chunks, ragged last); CD-1 and CD-2; data kinds binary / real / mixed (route_cases.operand)
crossed with the caller's hint unknown / binary (0/1 data only) / real, rotated over the routes so that every route meets every
batch, kind, hint and depth (test_cd_routes_cpu.py asserts it).

Prefetch sequences (seq_cases): per route seven steps on one Philox stream --

  step  batch            hint for the next          data slot expected (where the route prefetches)
  0     binary, BINARY   step 1's batch             0
  1     mixed,  UNKNOWN  step 2's batch             1
  2     real,   REAL     step 3's batch             2
  3     binary, BINARY   a tensor that is NOT next  1
  4     binary, UNKNOWN  none                       0  (the prepared slot holds another batch)
  5     mixed,  UNKNOWN  step 6's batch             0
  6     real,   REAL     none                       1

Every Philox seed is pinned on the CPU with the fp32 oracle alone (`python tests/cd_cases.py` prints SEEDS): the first seed >= 1 for
which the oracle's smallest Bernoulli and categorical margins over the whole pass -- every step of a sequence -- are at least MARGIN.
test_cd_routes_cpu.py asserts that; a seed that fails is replaced, never skipped."""
import functools

import numpy as np

import oracle.rbm_oracle as O
import route_cases as RC
import update_cases as UC
from oracle.draws import CATEGORICAL_MARGIN, PhiloxStream
from route_cases import MARGIN, operand, prob_bound, probs64, sigmoid64      # noqa: F401  (re-exported for the tests)
from update_cases import STATS_TOL, TOL, decode_planes, split3               # noqa: F401

F32, F64 = np.float32, np.float64
CUS = 256                       # compute units the mirror assumes (MI355X)
K1S_MAX_KCHUNK = 3520           # csrc/kernels_stream.hpp
OPTION_DEFAULTS = {"no_bits": 0, "down_rows": 0, "no_k2s": 0, "no_k1s": 0, "no_k1s_real": 0, "no_adaptive": 0, "k1s_force_na": 0,
                   "no_prefetch": 0}
UP_FAMILIES = RC.UP_ROUTES
DOWN_FAMILIES = ("k2_stream", "down_fused")      # the other three need Vpad >= 4096 and a real-valued operand: never a CD pass here
CARRIERS = ("none", "own_launch", "fused_k2", "k1_stream")
STEP_LR, STEP_MOM, STEP_WD = 0.07, 0.6, 1e-3


def cdiv(a, b):
    return -(-a // b)


def rup(x, m):
    return cdiv(x, m) * m


# ---- the mirror of make_layout / make_route / prop() ----------------------------------------------------------------------------------
def route_of(V, H, opts=None, groups=(), B=64, cus=CUS):
    """The Route fields a CD pass depends on (csrc/host_layout.hpp make_route, on a contiguous 16-B aligned W), from the shape, the
    options, the softmax groups and the batch."""
    t = dict(OPTION_DEFAULTS, **(opts or {}))
    Bp, Vpad = rup(max(B, 1), 64), rup(V, 16)
    mb, Pn = Bp // 64, Bp // 8
    if t["down_rows"]:
        down_tr = t["down_rows"]
    else:      # plan_down_rows: the first of 32, 28, .. 16 with the fewest rows on the busiest CU
        down_tr = min(range(32, 12, -4), key=lambda tr: (cdiv(cdiv(V, tr), cus) * tr, -tr))
    k2s_tr = min(48, max(8, 8 * cdiv(V, 8 * cus)))
    tiles = cdiv(H, 32)
    ks = max(1, int(cus / (tiles * mb) + 0.5))
    ks = max(min(ks, max(1, Vpad // 192)), cdiv(Vpad, K1S_MAX_KCHUNK))
    kchunk = rup(cdiv(Vpad, ks), 64)
    k1s_ks = cdiv(Vpad, kchunk)
    r = dict(V=V, H=H, B=B, groups=tuple(groups), opts=t, down_tr=down_tr, k1s_ks=k1s_ks)
    r["vec4"] = H % 4 == 0 and H >= 4
    r["up_fused"] = Vpad <= 1024
    r["k1s"] = r["vec4"] and not t["no_k1s"] and not r["up_fused"]
    r["k1s_real"] = r["k1s"] and not t["no_k1s_real"]
    r["k2s"] = r["vec4"] and not t["no_k2s"]
    r["k2s_cd"] = r["k2s"] and not t["no_bits"]
    r["vbits"] = not groups and (r["k2s_cd"] or down_tr % 8 == 0)
    r["neg_rm"] = not (r["vbits"] and r["k1s"])
    r["prefetch"] = r["vec4"] and not t["no_prefetch"]
    r["next_on_k1"] = r["k2s_cd"] and r["vbits"] and r["k1s"]
    r["rides"] = (not r["k2s_cd"]) or r["next_on_k1"]
    tpb = max(1, cdiv(cdiv(H, 128) * cdiv(V, 128), cus))
    r["adaptive_ok"] = kchunk <= 2048 and 2 * tpb * Pn <= 256 and cdiv(cdiv(V, 128), tpb) <= tiles * k1s_ks
    r["adaptive_next"] = r["rides"] and not t["no_adaptive"] and r["k1s_real"] and r["adaptive_ok"]
    r["cd_k2_blocks"] = cdiv(Vpad, k2s_tr if r["k2s_cd"] else down_tr)
    return r


def _partial(r):
    return "partial4" if r["vec4"] else "partial"


def data_up(r, hint):
    """Family of the K1 that reads the data operand (positive phase; forward of cd_step) under the hint `unknown` / `binary` / `real`."""
    if r["up_fused"]:
        return "fused"
    if not r["k1s"]:
        return _partial(r)
    if hint == "binary":
        return "stream_bits"
    return "stream_real" if r["k1s_real"] else _partial(r)


def neg_up(r):
    """Family of the negative-phase K1: a sample, read as the bit plane where there is one, else (k1_stream takes no one-term bf16
    form of a sample) the partial kernels."""
    if r["up_fused"]:
        return "fused"
    return "stream_bits" if (r["k1s"] and r["vbits"]) else _partial(r)


def cd_down(r):
    return "k2_stream" if r["k2s_cd"] else "down_fused"


def down_epilogue(r):
    """k2_stream is lean when it writes the probabilities' sample as planes and bits only (no vis_rm[1], no group); the fused K2
    branches on FinishArgs::simple alone."""
    if cd_down(r) == "k2_stream":
        return "general" if (r["groups"] or r["neg_rm"]) else "lean"
    return "general" if r["groups"] else "lean"


def carrier(r, has_hint):
    if not (has_hint and r["prefetch"]):
        return "none"
    if not r["rides"]:
        return "own_launch"
    return "k1_stream" if r["next_on_k1"] else "fused_k2"


def slot_form(r, next_hint):
    """How a hinted batch sits in its slot: `one` bf16 plane, `three`, or `item` (one where the 64 x 64 item is all 0/1, else three)."""
    if r["k1s"] and next_hint == "binary":
        return "one"
    if r["k1s"] and next_hint == "unknown" and r["adaptive_next"]:
        return "item"
    return "three"


def expect_of(r, hint, next_hint=None, slot=0, forward=False):
    """(last_route() fields, last_cd() record) of one CD pass."""
    up_last = data_up(r, hint) if forward else neg_up(r)
    route = {"up": up_last, "up_epilogue": "lean", "down": cd_down(r), "down_epilogue": down_epilogue(r), "finish_groups": bool(r["groups"])}
    cd = {"pos_up": data_up(r, hint), "first_down": cd_down(r), "last_up": neg_up(r), "next": carrier(r, next_hint is not None),
          "slot": slot if r["prefetch"] else 0,
          "adaptive": carrier(r, next_hint is not None) != "none" and slot_form(r, next_hint) == "item"}
    return route, cd


def smallest_non_adaptive(H=12, B=64):
    """The smallest V > 1024 (k1_stream) at which adaptive_ok is false for this H: fewer positive-phase blocks than update spans."""
    for V in range(1025, 4096):
        if not route_of(V, H, B=B)["adaptive_ok"]:
            return V
    return None


# ---- the routes ---------------------------------------------------------------------------------------------------------------------
GROUP = ((1030, 1040),)
ROUTES = [   # name, V, H, options, groups
    ("130x72", 130, 72, {}, ()),
    ("130x70", 130, 70, {}, ()),
    ("1040x36", 1040, 36, {}, ()),
    ("1040x36-no_bits", 1040, 36, {"no_bits": 1}, ()),
    ("1040x36-no_bits-rows8", 1040, 36, {"no_bits": 1, "down_rows": 8}, ()),
    ("1040x36-no_bits-rows12", 1040, 36, {"no_bits": 1, "down_rows": 12}, ()),
    ("1040x36-no_k2s", 1040, 36, {"no_k2s": 1}, ()),
    ("1040x36-no_k1s", 1040, 36, {"no_k1s": 1}, ()),
    ("1040x36-no_k1s_real", 1040, 36, {"no_k1s_real": 1}, ()),
    ("1040x36-no_adaptive", 1040, 36, {"no_adaptive": 1}, ()),
    ("1040x36-force_na", 1040, 36, {"k1s_force_na": 1}, ()),
    ("1040x36-group", 1040, 36, {}, GROUP),
    ("1040x37", 1040, 37, {}, ()),
    ("1100x12", 1100, 12, {}, ()),
]
BATCHES = (33, 64, 130)
KINDS = ("binary", "real", "mixed")
HINTS = ("unknown", "binary", "real")
DEPTHS = (1, 2)
# (kind, hint): every kind under every hint it may carry (`binary` is asserted on 0/1 data only), then three more so that ten cases
# per route give every batch with both depths
COMBOS = [("binary", "unknown"), ("real", "real"), ("mixed", "unknown"), ("binary", "binary"), ("real", "unknown"), ("mixed", "real"),
          ("binary", "real"), ("mixed", "unknown"), ("binary", "binary"), ("real", "real")]


def state(name):
    """The fp32 start state of a route: W and biases of route_cases.params, momenta of update_cases.params."""
    _, V, H, _, _ = next(r for r in ROUTES if r[0] == name)
    W, hb, vb = RC.params(V, H)
    m = UC.params(V, H)
    return dict(W=W, hid_bias=hb, vis_bias=vb, W_m=m["W_m"], hb_m=m["hb_m"], vb_m=m["vb_m"])


def pass_cases():
    out = []
    for ri, (name, V, H, opts, groups) in enumerate(ROUTES):
        for i, (kind, hint) in enumerate(COMBOS):
            B, k = BATCHES[(i + ri) % 3], DEPTHS[(i // 3 + i + ri) % 2]
            r = route_of(V, H, opts, groups, B)
            route, cd = expect_of(r, hint)
            out.append(dict(kind="pass", id=f"cd-{name}-B{B}-k{k}-{kind}-{hint}", route_name=name, V=V, H=H, B=B, k=k, data=kind, hint=hint,
                            opts=opts, groups=groups, r=r, expect=route, expect_cd=cd, draws=1 + k * (2 + len(groups))))
    return out


# ---- prefetch sequences ----------------------------------------------------------------------------------------------------------------
SEQ = [   # kind, hint (= the tag the tensor carries), what the step hints: "next", "other" (a tensor that is not the next batch) or None
    ("binary", "binary", "next"), ("mixed", "unknown", "next"), ("real", "real", "next"), ("binary", "binary", "other"),
    ("binary", "unknown", None), ("mixed", "unknown", "next"), ("real", "real", None),
]
SEQ_BATCH = {"130x72": 64, "130x70": 33, "1040x36": 130, "1040x36-no_bits": 64, "1040x36-no_bits-rows8": 33, "1040x36-no_bits-rows12": 130,
             "1040x36-no_k2s": 33, "1040x36-no_k1s": 64, "1040x36-no_k1s_real": 130, "1040x36-no_adaptive": 64, "1040x36-force_na": 33,
             "1040x36-group": 64, "1040x37": 33, "1100x12": 130}


def seq_batch(kind, B, V, i):
    """The batch of step i: route_cases.operand with its rows rotated by i (every step a different tensor of the same column kinds)."""
    x = np.roll(operand(kind, B, V), i, axis=0).copy()
    x.setflags(write=False)
    return x


def seq_cases():
    """One sequence per route and entry: `stats` (cd_stats, fixed parameters) on every route, `step` (cd_step, the parameters move)
    on every route without a softmax group."""
    out = []
    for name, V, H, opts, groups in ROUTES:
        for entry in ("stats", "step"):
            if entry == "step" and groups:
                continue
            B = SEQ_BATCH[name]
            r = route_of(V, H, opts, groups, B)
            steps, slot, prepared = [], 0, None      # prepared: (step whose batch sits in a slot, slot, form)
            for i, (kind, hint, nxt) in enumerate(SEQ):
                data_slot = prepared[1] if (prepared and prepared[0] == i) else 0
                next_hint = None if nxt is None else (SEQ[i + 1][1] if nxt == "next" else "unknown")
                route, cd = expect_of(r, hint, next_hint, data_slot)
                next_slot = (2 if data_slot == 1 else 1) if (next_hint is not None and r["prefetch"]) else 0
                steps.append(dict(i=i, data=kind, hint=hint, nxt=nxt, next_hint=next_hint, expect=route, expect_cd=cd, next_slot=next_slot,
                                  form=slot_form(r, next_hint) if next_slot else None))
                prepared = (i + 1 if nxt == "next" else -1, next_slot, steps[-1]["form"]) if next_slot else None
            out.append(dict(kind="seq", id=f"seq-{entry}-{name}-B{B}", route_name=name, entry=entry, V=V, H=H, B=B, k=1, opts=opts, groups=groups,
                            r=r, steps=steps, draws=3 + len(groups)))
    return out


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------------
def ref_pass(W, hb, vb, x, k, groups, ps):
    """One CD-k pass of rbm.py:199-209 in float64 from fp32 parameters and the PhiloxStream `ps`, in sched_cd's draw order.  Returns
    dict(x, hpos, v, hneg: the update's operands; v_prob: the last one; h: the positive-phase sample; picks: the categorical picks of
    the last iteration; stats: update_cases.stats64 of the operands; sqerr: sum (x - v_prob)^2, whose mean is train_epoch's loss)."""
    B, V = x.shape
    H = W.shape[1]
    W64, hb64, vb64, x64 = (np.asarray(a, F64) for a in (W, hb, vb, x))
    hpos = sigmoid64(x64 @ W64 + hb64)
    h = h0 = (hpos > ps.uniform((B, H))).astype(F64)
    for _ in range(k):
        v_prob = probs64(h @ W64.T + vb64, 1.0, groups)
        v = (v_prob > ps.uniform((B, V))).astype(F64)
        picks = []
        for s, e in groups:
            idx = ps.categorical(np.clip(v_prob[:, s:e], 1e-8, 1.0).astype(F32))
            v[:, s:e] = 0.0
            v[np.arange(B), s + idx] = 1.0
            picks.append(idx)
        hneg = sigmoid64(v @ W64 + hb64)
        h = (hneg > ps.uniform((B, H))).astype(F64)      # the last draw is consumed and unused (rbm.py:208)
    return dict(x=x64, hpos=hpos, v=v, hneg=hneg, v_prob=v_prob, h=h0, picks=picks, stats=UC.stats64([(x64, hpos, v, hneg)]),
                sqerr=float(((x64 - v_prob) ** 2).sum()))


def packed64(ref):
    """The layout of imdbn_packed_delta_floats in float64: [dW][dc][db][sum P+][squared-error sum]."""
    s = ref["stats"]
    return np.concatenate([s["dW"].reshape(-1), s["hpos"] - s["hneg"], s["vpos"] - s["vneg"], s["hpos"], [ref["sqerr"]]])


def packed_parts(V, H):
    """name -> slice of the packed statistics."""
    n = V * H
    return {"dW": slice(0, n), "dc": slice(n, n + H), "db": slice(n + H, n + H + V), "hpos": slice(n + H + V, n + 2 * H + V),
            "sqerr": slice(n + 2 * H + V, n + 2 * H + V + 1)}


def stats_bound(B, ref_part):
    """|device - float64| per element of the packed statistics: the reference and the device share every decision, so the device's
    error is the fp32 error of P+ / P- (prob_bound(1.0) each, times another factor <= 1, B summands) plus the summation, for which
    update_cases.STATS_TOL stands (rel * |ref| + atol)."""
    return B * prob_bound(1.0) + STATS_TOL["rel"] * np.abs(ref_part) + STATS_TOL["atol"]


@functools.lru_cache(maxsize=None)
def _ref_cd(cid):
    c = by_id(cid)
    st = state(c["route_name"])
    ps = PhiloxStream(c["seed"])
    out = ref_pass(st["W"], st["hid_bias"], st["vis_bias"], operand(c["data"], c["B"], c["V"]), c["k"], c["groups"], ps)
    assert ps.offset == c["draws"]
    return out


def ref_cd(c):
    """ref_pass of a `pass` case (computed once, shared; treat as read-only)."""
    return _ref_cd(c["id"])


def ref_seq_step(c, i, st, offset):
    """ref_pass of step i of a sequence on the fp32 state `st`, from draw `offset` on."""
    ps = PhiloxStream(c["seed"], offset=offset)
    return ref_pass(st["W"], st["hid_bias"], st["vis_bias"], seq_batch(c["steps"][i]["data"], c["B"], c["V"], i), c["k"], c["groups"], ps)


# ---- the fp32 oracle (seed pinning, and the CPU test's comparison) -----------------------------------------------------------------------
def _oracle_state(c):
    st = state(c["route_name"])
    o = O.RBMState.create(st["W"], STEP_LR, STEP_WD, STEP_MOM, sparsity=True, sparsity_factor=UC.SPARSITY_TARGET,
                          softmax_groups=list(c["groups"]), hid_bias=st["hid_bias"], vis_bias=st["vis_bias"])
    o.W_m, o.hb_m, o.vb_m = st["W_m"].copy(), st["hb_m"].copy(), st["vb_m"].copy()
    return o


def run_oracle(c):
    """The case on the fp32 oracle with its seed: (list of cd_statistics results, smallest Bernoulli margin, smallest categorical
    margin).  A `step` sequence applies the update between the steps, as the device does."""
    O.reset_margin()
    o = _oracle_state(c)
    ps = PhiloxStream(c["seed"])
    if c["kind"] == "pass":
        res = [O.cd_statistics(o, operand(c["data"], c["B"], c["V"]), c["k"], ps)]
    else:
        res = []
        for i, s in enumerate(c["steps"]):
            res.append(O.cd_statistics(o, seq_batch(s["data"], c["B"], c["V"], i), c["k"], ps))
            if c["entry"] == "step":
                O.apply_cd_update(o, res[-1], STEP_LR, STEP_MOM, c["B"], True)
    return res, O.BERNOULLI_MARGIN["min"], CATEGORICAL_MARGIN["min"]


# ---- the table -----------------------------------------------------------------------------------------------------------------------
# Philox seed per case: the first seed >= 1 whose margins pass (printed by `python tests/cd_cases.py`); cases not listed take seed 1
SEEDS = {
    "cd-1040x36-no_bits-B130-k2-mixed-unknown": 3,
    "cd-1040x36-no_bits-B130-k2-mixed-real": 3,
    "cd-1040x36-no_bits-B130-k2-binary-binary": 6,
    "cd-1040x36-no_bits-rows8-B130-k2-real-real": 3,
    "cd-1040x36-no_bits-rows8-B130-k2-real-unknown": 3,
    "cd-1040x36-no_bits-rows8-B130-k2-mixed-unknown": 3,
    "cd-1040x36-no_bits-rows12-B130-k2-binary-unknown": 6,
    "cd-1040x36-no_bits-rows12-B64-k2-mixed-unknown": 3,
    "cd-1040x36-no_bits-rows12-B130-k2-binary-binary": 6,
    "cd-1040x36-no_bits-rows12-B64-k2-mixed-real": 3,
    "cd-1040x36-no_bits-rows12-B130-k2-binary-real": 6,
    "cd-1040x36-no_bits-rows12-B130-k2-real-real": 3,
    "cd-1040x36-no_k2s-B64-k2-real-real": 2,
    "cd-1040x36-no_k2s-B64-k2-real-unknown": 2,
    "cd-1040x36-no_k2s-B64-k2-mixed-unknown": 3,
    "cd-1040x36-no_k1s-B64-k2-real-real": 2,
    "cd-1040x36-no_adaptive-B130-k2-mixed-unknown": 3,
    "cd-1040x36-no_adaptive-B130-k2-mixed-real": 3,
    "cd-1040x36-no_adaptive-B130-k2-binary-binary": 6,
    "cd-1040x36-force_na-B130-k2-real-real": 3,
    "cd-1040x36-force_na-B130-k2-real-unknown": 3,
    "cd-1040x36-force_na-B130-k2-mixed-unknown": 3,
    "cd-1100x12-B130-k1-real-real": 2,
    "cd-1100x12-B130-k1-real-unknown": 2,
    "seq-stats-1040x36-B130": 3,
    "seq-step-1040x36-B130": 4,
    "seq-stats-1040x36-no_bits-B64": 4,
    "seq-step-1040x36-no_bits-B64": 2,
    "seq-stats-1040x36-no_bits-rows12-B130": 3,
    "seq-step-1040x36-no_bits-rows12-B130": 4,
    "seq-stats-1040x36-no_k1s-B64": 4,
    "seq-step-1040x36-no_k1s-B64": 2,
    "seq-stats-1040x36-no_k1s_real-B130": 3,
    "seq-step-1040x36-no_k1s_real-B130": 4,
    "seq-stats-1040x36-no_adaptive-B64": 4,
    "seq-step-1040x36-no_adaptive-B64": 2,
    "seq-stats-1040x37-B33": 2,
    "seq-stats-1100x12-B130": 3,
    "seq-step-1100x12-B130": 2,
}


@functools.lru_cache(maxsize=None)
def _all():
    cs = pass_cases() + seq_cases()
    for c in cs:
        c["seed"] = SEEDS.get(c["id"], 1)
    assert len({c["id"] for c in cs}) == len(cs), "duplicate case id"
    return tuple(cs)


def cases(kind=None, entry=None):
    return [c for c in _all() if (kind is None or c["kind"] == kind) and (entry is None or c.get("entry") == entry)]


def by_id(cid):
    return next(c for c in _all() if c["id"] == cid)


def one_per_route():
    """One `pass` case of every route without a softmax group (the cd_step tests), the i-th route taking its i-th case so that the
    kinds, hints, batches and depths rotate."""
    out = []
    for ri, (name, _, _, _, groups) in enumerate(ROUTES):
        if not groups:
            mine = [c for c in cases("pass") if c["route_name"] == name]
            out.append(mine[ri % len(mine)])
    return out


def pinned_seeds():
    """SEEDS as the rule gives it: for every case the first seed >= 1 whose margins are at least MARGIN, listed where it is not 1."""
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
    return out


if __name__ == "__main__":      # pin the seeds: prints the SEEDS table
    print("SEEDS = {")
    for k, v in pinned_seeds().items():
        print(f'    "{k}": {v},')
    print("}")
