"""Cases shared by test_fast_mode_cpu.py and test_fast_mode_gpu.py: FAST mode (IMDBN_FAST_BF16) on every propagation route and
on the CD pass of every route -- the `<1>` half of the instantiation tables of csrc/host_prop.hpp -- against a float64 twin.

FAST arithmetic: one bf16 term per weight and per operand, round to nearest even, fp32 accumulation.  The twin:

  logits = rne_bf16(x).astype(f64) @ rne_bf16(W).astype(f64) + bias (its fp32 value)
  then / max(1e-6, T), sigmoid and the softmax groups as route_cases.probs64

A bf16 x bf16 product has 16 significant bits and is exact in fp32, so the device differs from the twin by fp32 accumulation and the
fp32 epilogue only, exactly as in parity mode: the bounds are route_cases.prob_bound(T), route_cases.logit_bound and
cd_cases.stats_bound, unchanged.  The device is handed the fp32 parameters of route_cases.params and rounds them itself.

Staging of real-valued intermediates.  Where one kernel's epilogue writes a real-valued operand that the next kernel reads (the
mean-field h of gibbs_step with sample_h = 0; the one-term planes of P+ and P- the update kernel reads), the device rounds ITS fp32
value to bf16.  A float64 twin rounding its own value can land on the other side of a rounding midpoint, one bf16 ulp (2^-9 at
p = 0.5) away: far above any bound here.  So stage n is compared with the twin of stage n, and the twin of stage n + 1 starts from
what the device wrote for stage n (h_prob of gibbs_step; the decoded planes hid_tr0 / hid_tr1 for the statistics).  A one-term
plane itself is held to |decoded - twin| <= prob_bound + half a bf16 ulp of the twin's value (half_ulp_bf16): the device's fp32
value is within prob_bound of the twin and its rounding moves it by at most half an ulp.  Samples are 0/1 and need no hand-over;
caller operands are rounded from the same fp32 bits on both sides.

Cases (shapes, options and route mirrors are those of route_cases / cd_cases / rowoffset_cases, imported, never copied):

  up      every case of route_cases.cases("up") -- five families x TEMPS x sampled or not x real / binary / mixed, and the bit plane
          of forward(data_binary=True) -- plus ragged batches 7 and 66 on every family
  down    route_cases.DOWN_SHAPES and the 1089-wide joint layer with its 14-label group: every T, raw logits, no / one / two groups
  gibbs   rowoffset_cases.A_ROUTES with a `mixed` operand: sample_h = sample_v = 1 (bit plane -> k2_stream or the fused K2), and
          sample_h = sample_v = 0, where the epilogue-written one-term hid_rm feeds the K2 (staged)
  cd      cd_cases.cases("pass") re-run in FAST: four (data, hint) combinations per route of cd_cases.ROUTES, and the prefetch
          sequences of cd_cases.cases("seq", "stats") with their slot forms
  step    three consecutive cd_step updates on 1040 x 36 with every next batch prefetched, and on 1040 x 36 with its softmax group:
          parameters and momenta against the twin's update by the rule of test_cd_routes_gpu.py (update_cases.TOL, the next step's
          reference starting from the fp32 state the device holds)
  chain   the 1089-wide joint layer with its 14-label group, one launch per half step: two sampled steps compared exactly, then a
          mean-field step staged through the traced h_prob
  free    free_energy on an operand built beside the rounding midpoints (midpoint_operand), prop_down_sqerr against the parity
          reconstruction: the two entries that put an epilogue of their own behind a FAST propagation

Reach of the `<1>` instantiations (test_fast_mode_cpu.py asserts the table below against the case list): a caller tensor reaches the
fused K2 as a ONE-term operand only (prep() writes one term in FAST mode), so down_insts[0][*] is reached at operand kinds `bit
plane` and `one term`; its three-term and exactness-map kinds are not reachable in FAST mode through these entries.

Every Philox seed is pinned on the CPU with the twin alone (`python tests/fast_cases.py` prints SEEDS): the first seed >= 1 whose
smallest Bernoulli margin |p - u| and smallest categorical margin are at least MARGIN.  FAST logits differ from parity logits, so
the table is this file's own."""
import functools

import numpy as np

import cd_cases as CC
import route_cases as RC
import rowoffset_cases as RO
import update_cases as UC
from oracle.draws import CATEGORICAL_MARGIN, PhiloxStream
from rowoffset_cases import fast_weights, rne_bf16

F32, F64 = np.float32, np.float64
MARGIN = RC.MARGIN
DISCRIMINATION = 20.0          # the FAST twin and the parity reference differ by at least this many bounds somewhere in the output
RAGGED = (7, 66)


def half_ulp_bf16(y):
    """Half a unit in the last place of bf16 (8 significand bits) at |y|, elementwise: 2^(e - 8) for 2^e <= |y| < 2^(e + 1)."""
    _, e = np.frexp(np.abs(np.asarray(y, F64)))          # |y| = m 2^e, m in [0.5, 1)
    return np.where(np.asarray(y) == 0, 0.0, np.ldexp(1.0, e - 1 - 8))


def r64(x):
    return rne_bf16(x).astype(F64)


@functools.lru_cache(maxsize=None)
def params64(V, H):
    """(rne_bf16(W), hid_bias, vis_bias) as float64."""
    _, hb, vb = RC.params(V, H)
    return fast_weights(V, H).astype(F64), hb.astype(F64), vb.astype(F64)


def up_logits(V, H, x):
    W, hb, _ = params64(V, H)
    return r64(x) @ W + hb


def down_logits(V, H, h):
    W, _, vb = params64(V, H)
    return r64(h) @ W.T + vb


def exact_up_logits(V, H, x):
    W, hb, _ = RC.params(V, H)
    return np.asarray(x, F64) @ W.astype(F64) + hb.astype(F64)


def exact_down_logits(V, H, h):
    W, _, vb = RC.params(V, H)
    return np.asarray(h, F64) @ W.astype(F64).T + vb.astype(F64)


class Margin:
    """Smallest Bernoulli margin of the decisions taken through it; the categorical one is oracle.draws' own record."""
    def __init__(self):
        self.bern = float("inf")
        CATEGORICAL_MARGIN["min"] = float("inf")

    def decide(self, p, u):
        self.bern = min(self.bern, float(np.abs(p - u.astype(F64)).min()))
        return (p > u).astype(F64)

    @property
    def cat(self):
        return CATEGORICAL_MARGIN["min"]


def sample_visible(v_prob, groups, ps, m):
    """rbm.py:118-135 on the PhiloxStream: Bernoulli, then one categorical pick per group."""
    B = v_prob.shape[0]
    v = m.decide(v_prob, ps.uniform(v_prob.shape))
    picks = []
    for s, e in groups:
        idx = ps.categorical(np.clip(v_prob[:, s:e], 1e-8, 1.0).astype(F32))
        v[:, s:e] = 0.0
        v[np.arange(B), s + idx] = 1.0
        picks.append(idx)
    return v, picks


# ---- up -------------------------------------------------------------------------------------------------------------------------------
def up_cases():
    out = [dict(c, id="fast-" + c["id"], mode="fast") for c in RC.cases("up")]
    for i, (route, V, H, opts) in enumerate(RC.UP_SHAPES):      # ragged batches: one row short of two 4-row groups, two rows past a chunk
        for j, B in enumerate(RAGGED):
            T, sample, kind = RC.TEMPS[(i + j) % 3], bool((i + j) % 2), ("real", "mixed")[j]
            out.append(dict(kind="up", id=f"fast-up-{route}-{V}x{H}-B{B}-T{T}-{kind}{'-sample' if sample else ''}", V=V, H=H, B=B, T=T,
                            sample=sample, operand=kind, opts=opts, groups=(), mode="fast",
                            route={"up": route, "up_epilogue": RC._lean(route, T == 1.0, not sample)}))
    return out


def twin_up(c, seed=None):
    """(float64 probabilities, decisions or None, parity float64 probabilities, Margin)"""
    x = RC.operand(c["operand"], c["B"], c["V"])
    T = max(1e-6, c["T"])
    p = RC.sigmoid64(up_logits(c["V"], c["H"], x) / T)
    m = Margin()
    s = m.decide(p, PhiloxStream(c["seed"] if seed is None else seed).uniform(p.shape)) if c["sample"] else None
    return p, s, RC.sigmoid64(exact_up_logits(c["V"], c["H"], x) / T), m


# ---- down -----------------------------------------------------------------------------------------------------------------------------
DOWN_PICK = ((0, 1.0, 0), (1, 0.7, 0), (2, 3.0, 0), (0, 0.7, 1), (1, 3.0, 1), (2, 1.0, 1))      # (groups index, T, logits_only)
JOINT = ("down_fused", RC.CHAIN_V, 36, 33, {})


def down_cases():
    out = []
    for route, V, H, B, opts in RC.DOWN_SHAPES + [JOINT]:
        gs = RC.down_groups(V) if V != RC.CHAIN_V else [(), RC.CHAIN_GROUPS, RC.CHAIN_GROUPS]
        for gi, T, lo in DOWN_PICK:
            groups = gs[gi]
            out.append(dict(kind="down", id=f"fast-down-{route}-{V}x{H}-B{B}-g{gi}-T{T}{'-logits' if lo else ''}", V=V, H=H, B=B, T=T,
                            logits_only=lo, groups=groups, opts=opts, mode="fast", operand="real",
                            route={"down": route, "down_epilogue": RC._lean(route, T == 1.0 and not groups and not lo, True),
                                   "finish_groups": bool(groups) and not lo}))
    return out


def twin_down(c):
    """(float64 reference, un-tempered float64 logits, the parity reference)"""
    h = RC.operand("real", c["B"], c["H"])
    T = max(1e-6, c["T"])
    l, le = down_logits(c["V"], c["H"], h), exact_down_logits(c["V"], c["H"], h)
    if c["logits_only"]:
        return l / T, l, le / T
    return RC.probs64(l, c["T"], c["groups"]), l, RC.probs64(le, c["T"], c["groups"])


# ---- Gibbs steps ------------------------------------------------------------------------------------------------------------------------
GIBBS_ROUTES = RO.A_ROUTES + [("1040x36-k2s40", 1040, 36, {"k2s_rows": 40}, ())]      # + k2_stream with three MFMA tiles per block


def gibbs_cases():
    out = []
    for ri, (name, V, H, opts, groups) in enumerate(GIBBS_ROUTES):
        g = bool(groups)
        for sampled in (True, False):
            B = (66, 33, 7, 130)[(ri + sampled) % 4]
            c = RO._gibbs(name, V, H, opts, groups, B, 0, "fast")
            del c["W"]
            c.update(id=f"fast-gibbs-{name}-B{B}-{'hv' if sampled else 'mf'}", operand="mixed", sample_h=sampled, sample_v=sampled)
            if not sampled:      # mean-field: no draw; K1 writes the one-term hid_rm, which the fused K2 reads (no bit plane)
                up = c["route"]["up"]
                c["route"] = {"up": up, "up_epilogue": RO.epilogue(up, True, 0, True, True, False, 0), "down": "down_fused",
                              "down_epilogue": RO.epilogue("down_fused", not g, 0, True, False, False, 0), "finish_groups": g}
            out.append(c)
    return out


def twin_gibbs(c, h_prob_device=None, seed=None):
    """dict(h_prob, h, v_prob, v_next, exact_h_prob, exact_v_prob, m).  Mean-field: the K2's operand is the device's fp32 h_prob
    (`h_prob_device`; the twin's own where None: the CPU test's discrimination figure only)."""
    V, H, B = c["V"], c["H"], c["B"]
    x = RC.operand(c["operand"], B, V)
    ps, m = PhiloxStream(c["seed"] if seed is None else seed), Margin()
    h_prob = RC.sigmoid64(up_logits(V, H, x))
    e_hprob = RC.sigmoid64(exact_up_logits(V, H, x))
    if c["sample_h"]:
        h = m.decide(h_prob, ps.uniform((B, H)))
        h_in = e_in = h
    else:
        h = h_prob
        h_in = h_prob if h_prob_device is None else np.asarray(h_prob_device, F32)
        e_in = e_hprob
    v_prob = RC.probs64(down_logits(V, H, h_in), 1.0, c["groups"])
    e_vprob = RC.probs64(exact_down_logits(V, H, e_in), 1.0, c["groups"])
    v_next = sample_visible(v_prob, c["groups"], ps, m)[0] if c["sample_v"] else v_prob
    assert ps.offset == RC.gibbs_draws(c)
    return dict(h_prob=h_prob, h=h, v_prob=v_prob, v_next=v_next, exact_h_prob=e_hprob, exact_v_prob=e_vprob, m=m)


# ---- the CD pass ------------------------------------------------------------------------------------------------------------------------
CD_COMBOS = (("binary", "binary"), ("real", "real"), ("mixed", "unknown"), ("real", "unknown"))


def cd_cases():
    """Per route of cd_cases.ROUTES the first `pass` case of each combination in CD_COMBOS, re-run in FAST mode; and every `stats`
    prefetch sequence."""
    out = []
    for name, *_ in CC.ROUTES:
        mine = [c for c in CC.cases("pass") if c["route_name"] == name]
        for kind, hint in CD_COMBOS:
            c = next(c for c in mine if (c["data"], c["hint"]) == (kind, hint))
            out.append(dict(c, id="fast-" + c["id"], mode="fast"))
    for c in CC.cases("seq", "stats"):
        out.append(dict(c, id="fast-" + c["id"], mode="fast"))
    return out


def par_of(W, hb, vb):
    """(rne_bf16(W), hid_bias, vis_bias, W) as float64 from fp32 parameters: what a FAST pass and its parity counterpart multiply."""
    return r64(W), np.asarray(hb, F64), np.asarray(vb, F64), np.asarray(W, F64)


@functools.lru_cache(maxsize=None)
def par(V, H):
    return par_of(*RC.params(V, H))


def twin_pass(pr, x, k, groups, ps, m):
    """cd_cases.ref_pass in FAST arithmetic on the parameters `pr` (par_of): dict(x: the rounded data; hpos, hneg, v_prob: float64
    probabilities; h, v: decisions; exact_hpos, exact_hneg: the parity float64 P+ and, on the same sample, P-; sqerr, vpos: from
    the UNrounded data, which the squared error and the bias sums read)."""
    W, hb, vb, We = pr
    B = x.shape[0]
    hpos = RC.sigmoid64(r64(x) @ W + hb)
    h = h0 = m.decide(hpos, ps.uniform((B, W.shape[1])))
    for _ in range(k):
        v_prob = RC.probs64(h @ W.T + vb, 1.0, groups)
        v, _ = sample_visible(v_prob, groups, ps, m)
        hneg = RC.sigmoid64(v @ W + hb)
        h = m.decide(hneg, ps.uniform((B, W.shape[1])))      # the last draw is consumed and unused (rbm.py:208)
    x64 = np.asarray(x, F64)
    return dict(x=r64(x), x_exact=x64, hpos=hpos, hneg=hneg, v=v, v_prob=v_prob, h=h0, exact_hpos=RC.sigmoid64(x64 @ We + hb),
                exact_hneg=RC.sigmoid64(v @ We + hb), sqerr=float(((x64 - v_prob) ** 2).sum()), vpos=x64.sum(0))


def stats_twin(t, hpos_plane, hneg_plane):
    """update_cases.stats64 of a FAST pass: dW from the one-term operands the update kernel read -- the rounded data, the planes of
    P+ and P- handed in (on the device: its own, by the staging rule), the sample; the bias sums from the fp32 values the
    epilogues add up, i.e. the unrounded probabilities and the unrounded data."""
    s = UC.stats64([(t["x"], hpos_plane, t["v"], hneg_plane)])
    s.update(hpos=t["hpos"].sum(0), hneg=t["hneg"].sum(0), vpos=t["vpos"])
    return s


def packed_twin(t, hpos_plane, hneg_plane):
    """cd_cases.packed64's layout for a FAST pass, from stats_twin."""
    s = stats_twin(t, hpos_plane, hneg_plane)
    return np.concatenate([s["dW"].reshape(-1), s["hpos"] - s["hneg"], s["vpos"] - s["vneg"], s["hpos"], [t["sqerr"]]])


def parity_dW(t):
    """dW of the same decisions from unrounded operands: what the FAST statistics must be told apart from."""
    return t["x_exact"].T @ t["exact_hpos"] - t["v"].T @ t["exact_hneg"]


def cd_batches(c):
    if c["kind"] == "pass":
        return [RC.operand(c["data"], c["B"], c["V"])]
    if c["kind"] == "step" and c["steps"][0]["nxt"] is None:      # (no roll: every step another kind of data)
        return [RC.operand(s["data"], c["B"], c["V"]) for s in c["steps"]]
    return [CC.seq_batch(s["data"], c["B"], c["V"], s["i"]) for s in c["steps"]]


def twin_cd(c, seed=None):
    """(twin_pass per step, Margin over all of them) on one PhiloxStream, as the device consumes it."""
    ps, m = PhiloxStream(c["seed"] if seed is None else seed), Margin()
    out = [twin_pass(par(c["V"], c["H"]), x, c["k"], c["groups"], ps, m) for x in cd_batches(c)]
    assert ps.offset == c["draws"] * len(out)
    return out, m


# ---- three consecutive cd_steps -----------------------------------------------------------------------------------------------------------
STEPS = 3


def step_cases():
    """Three cd_step updates on two routes: 1040 x 36 with every step hinting the next batch (the first three steps of cd_cases'
    `step` sequence: slots 0 -> 1 -> 2), and 1040 x 36 with its softmax group (no hint: mixed, real, binary data)."""
    c = CC.by_id("seq-step-1040x36-B130")
    out = [dict(c, id="fast-step-1040x36-B130-prefetch", kind="step", mode="fast", steps=c["steps"][:STEPS])]
    name, V, H, opts, groups = next(r for r in CC.ROUTES if r[0] == "1040x36-group")
    B = 64
    r = CC.route_of(V, H, opts, groups, B)
    steps = []
    for i, (kind, hint) in enumerate((("mixed", "unknown"), ("real", "real"), ("binary", "binary"))):
        route, cd = CC.expect_of(r, hint)
        steps.append(dict(i=i, data=kind, hint=hint, nxt=None, next_hint=None, expect=route, expect_cd=cd, next_slot=0, form=None))
    out.append(dict(kind="step", id=f"fast-step-{name}-B{B}", route_name=name, entry="step", mode="fast", V=V, H=H, B=B, k=1, opts=opts,
                    groups=groups, r=r, steps=steps, draws=3 + len(groups)))
    return out


def step_update(st, s, B):
    """rbm.py:212-224 on the state `st` from the statistics `s` with the scalars of the cd_step tests (float64 state)."""
    return UC.ref_update(st, s, CC.STEP_LR, CC.STEP_MOM, CC.STEP_WD, B, sparsity=True)


def twin_steps(c, seed=None):
    """The CPU twin of a `step` case, the state moving by its OWN update between the steps (each plane the twin's own rounding;
    on the device the reference restarts from the state and planes the device holds): (twin_pass per step, Margin)."""
    ps, m = PhiloxStream(c["seed"] if seed is None else seed), Margin()
    st, out = CC.state(c["route_name"]), []
    for x in cd_batches(c):
        t = twin_pass(par_of(st["W"], st["hid_bias"], st["vis_bias"]), x, c["k"], c["groups"], ps, m)
        new = step_update(st, stats_twin(t, r64(t["hpos"].astype(F32)), r64(t["hneg"].astype(F32))), c["B"])
        st = {k: v.astype(F32) for k, v in new.items()}
        out.append(t)
    return out, m


# ---- one wide-layer chain, one launch per half step ------------------------------------------------------------------------------------------
CHAIN = dict(kind="chain", id="fast-chain-1089x36-B33-hv-hv-mf", mode="fast", V=RC.CHAIN_V, H=36, B=33, groups=RC.CHAIN_GROUPS,
             opts={"no_chain_kernel": 1}, operand="mixed",
             steps=[dict(T=1.0, sigma=0.0, eta=0.0, sample_h=1, vmode=1, clamp=0), dict(T=1.0, sigma=0.0, eta=0.0, sample_h=1, vmode=1, clamp=0),
                    dict(T=1.0, sigma=0.0, eta=0.0, sample_h=0, vmode=0, clamp=0)],
             # the last pair of the two sampled steps (bit plane -> k2_stream) and of all three (mean-field: the one-term hid_rm -> fused K2)
             # (rowoffset_cases.epilogue = the mirror of finish_lean: a sampled h leaves as a bit plane and nothing else is written -> lean;
             #  the mean-field K1 writes the one-term hid_rm -> general; every K2 here has the group)
             route_sampled={"up": "stream_real", "up_epilogue": RO.epilogue("stream_real", True, 1, False, False, False, 0), "down": "k2_stream",
                            "down_epilogue": RO.epilogue("k2_stream", False, 1, True, True, False, 0), "finish_groups": True},
             route={"up": "stream_real", "up_epilogue": RO.epilogue("stream_real", True, 0, False, True, False, 0), "down": "down_fused",
                    "down_epilogue": RO.epilogue("down_fused", False, 0, True, True, False, 0), "finish_groups": True})


def chain_cases():
    return [dict(CHAIN)]


def twin_chain(c, h_prob_device=None, seed=None):
    """The chain from v0 = the `mixed` operand (init_uniform = False, nothing clamped): per step dict(h_prob, v_prob, v, exact_h_prob),
    the sampled steps decided on the PhiloxStream, the mean-field step's K2 fed with `h_prob_device` (the twin's own where None)."""
    V, H, B = c["V"], c["H"], c["B"]
    W, hb, vb, We = par(V, H)
    ps, m = PhiloxStream(c["seed"] if seed is None else seed), Margin()
    v, ve, out = RC.operand(c["operand"], B, V), None, []
    for s in c["steps"]:
        h_prob = RC.sigmoid64(r64(v) @ W + hb)
        e_hprob = RC.sigmoid64(np.asarray(v, F64) @ We + hb)
        if s["sample_h"]:
            h = m.decide(h_prob, ps.uniform((B, H)))
        else:
            h = h_prob if h_prob_device is None else np.asarray(h_prob_device, F32)
        v_prob = RC.probs64(r64(h) @ W.T + vb, 1.0, c["groups"])
        v = sample_visible(v_prob, c["groups"], ps, m)[0] if s["vmode"] else v_prob
        out.append(dict(h_prob=h_prob, exact_h_prob=e_hprob, v_prob=v_prob, v=v))
    return out, m


# ---- free energy and the decode error -----------------------------------------------------------------------------------------------------------
FREE = dict(kind="free", id="fast-free_energy-1040x36-B33", mode="fast", V=1040, H=36, B=33, opts={}, groups=(),
            route={"up": "partial4", "up_epilogue": "general"})      # raw logits: never k1_stream (Route::up)
SQERR = dict(kind="sqerr", id="fast-prop_down_sqerr-1040x36-B33", mode="fast", V=1040, H=36, B=33, opts={}, groups=(),
             route={"down": "down_fused", "down_epilogue": "lean"})


def midpoint_operand(B, V, H):
    """[B, V] fp32 in [0.5, 1): every element 1/64 of a bf16 ulp beside a rounding midpoint, on the side that makes round-to-nearest
    move it with the sign of its weight row's sum.  The free energy adds H logits, whose FAST-against-parity differences have
    random signs and cancel on an ordinary operand; here they add up, so the case tells the modes apart by far more than the
    worst-case bound -- and truncation, or rounding the wrong way, is wrong by the whole of it."""
    W = RC.params(V, H)[0]
    base = (RC.operand("real", B, V).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32) * F32(0.5) + F32(0.5)      # bf16 values in [0.5, 1)
    base = (base.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
    up = W.astype(F64).sum(1) < 0                      # F falls with the logits: push them up where the weights are negative ... down
    x = base + F32(2.0 ** -8) * np.where(up, F32(0.5 + 2.0 ** -6), F32(0.5 - 2.0 ** -6))[None, :].astype(F32)
    x = x.astype(F32)
    x.setflags(write=False)
    return x


def free_energy64(l, v, vb):
    """F(v) = -v . b - sum_j softplus(l_j) from float64 logits (energy_utils.py:19-28)."""
    return -(np.asarray(v, F64) @ vb) - np.logaddexp(0.0, l).sum(1)


def twin_free(c):
    """(FAST twin F, bound per row, parity F).  The bound: every logit within route_cases.logit_bound, a softplus slope of at most 1,
    so H of them; plus the fp32 reduction of free_energy_rows -- per thread cdiv(V, 256) + cdiv(H, 256) additions, 8 tree levels,
    and 4 ulp for expf / log1pf and the product -- on the sum of the magnitudes."""
    V, H, B = c["V"], c["H"], c["B"]
    x = midpoint_operand(B, V, H)
    W, hb, vb, We = par(V, H)
    l, le = r64(x) @ W + hb, np.asarray(x, F64) @ We + hb
    mag = np.abs(np.asarray(x, F64) * vb).sum(1) + np.logaddexp(0.0, l).sum(1)
    bound = H * RC.logit_bound(l, 1.0) + (-(-V // 256) + -(-H // 256) + 8 + 4) * 2.0 ** -24 * mag
    return free_energy64(l, x, vb), bound, free_energy64(le, x, vb)


def twin_sqerr(c):
    """(h, ref, FAST twin of mean_c (p(v|h)_c - ref_c)^2, bound per row, the parity value).  ref = the fp32 PARITY reconstruction:
    the compared quantity is then the squared FAST-against-parity difference itself.  The bound: p within prob_bound of the twin,
    so each square moves by at most (2 |p - ref| + prob_bound) prob_bound; plus row_sqerr's fp32 reduction (cdiv(V, 256)
    additions per thread, 8 tree levels, 3 roundings for the difference, the square and the division)."""
    V, H, B = c["V"], c["H"], c["B"]
    h = RC.operand("real", B, H)
    W, _, vb, We = par(V, H)
    p = RC.sigmoid64(r64(h) @ W.T + vb)
    ref = RC.sigmoid64(np.asarray(h, F64) @ We.T + vb).astype(F32)
    d = np.abs(p - ref.astype(F64))
    pb = RC.prob_bound(1.0)
    mse = (d ** 2).mean(1)
    bound = ((2 * d + pb) * pb).mean(1) + (-(-V // 256) + 8 + 3) * 2.0 ** -24 * mse
    pe = RC.sigmoid64(np.asarray(h, F64) @ We.T + vb)
    return h, ref, mse, bound, ((pe - ref.astype(F64)) ** 2).mean(1)


# ---- the instantiations the table must reach -----------------------------------------------------------------------------------------------
def reached(c):
    """The `<1>` instantiations of csrc/host_prop.hpp a case runs, as (kernel, detail...) tuples derived from its route mirror."""
    out = set()
    if c["kind"] in ("up", "forward"):
        r = c["route"]
        gen = r["up_epilogue"] == "general"
        out.add({"fused": ("gemm_up_fused<1>",), "partial4": ("gemm_up4_partial<1>",), "partial": ("gemm_up_partial<1>",),
                 "stream_bits": ("k1_stream<1>", 0, False, gen), "stream_real": ("k1_stream<1>", 1, False, gen)}[r["up"]])
    elif c["kind"] == "down":
        out.add({"down_fused": ("gemm_down_fused<1>", c["H"] % 4 == 0, "one term"), "down_chunks2": ("down_chunk_insts[0]", 2),
                 "down_chunks4": ("down_chunk_insts[0]", 4), "down_tiled": ("gemm_down_tiled<1>",)}[c["route"]["down"]])
    elif c["kind"] == "gibbs":
        r = c["route"]
        if r["down"] == "k2_stream":
            out.add(("k2_stream<1>", -(-(c["opts"].get("k2s_rows", 0) or 8) // 16), r["down_epilogue"] == "general"))      # (k2s_tr = 8 at V <= 2048)
        else:
            bits = c["sample_h"] and not c["opts"].get("no_bits")
            out.add(("gemm_down_fused<1>", c["H"] % 4 == 0, "bit plane" if bits else "one term"))
    elif c["kind"] in ("chain", "free", "sqerr"):
        pass      # (instantiations the single propagations already reach)
    else:
        r = c["r"]
        steps = c["steps"] if c["kind"] in ("seq", "step") else [dict(expect=c["expect"], expect_cd=c["expect_cd"])]
        for s in steps:
            e, cd = s["expect"], s["expect_cd"]
            has_next = cd["next"] != "none"
            if cd["next"] == "fused_k2":
                out.add(("down_next_insts[0]", not r["opts"]["no_bits"]))
            # the K1 launches: the sampling ones as rowoffset_cases.sampling_k1 derives them, then the last (mean-field, lean), which
            # at CD-1 is the launch of iteration 0 and carries the rider
            k1 = [(fam, ep == "general", rider) for _, fam, ep, rider in RO.sampling_k1(r, s.get("hint", c.get("hint")), c["k"], 0, has_next=has_next)]
            k1.append((cd["last_up"], False, bool(has_next and c["k"] == 1 and r["next_on_k1"])))
            for fam, gen, rider in k1:
                if fam in ("stream_bits", "stream_real"):
                    na = 0 if fam == "stream_bits" and (rider or not r["opts"]["k1s_force_na"]) else 1
                    out.add(("k1_stream<1>", na, rider, gen))
            if e["down"] == "k2_stream":
                out.add(("k2_stream<1>", 1, e["down_epilogue"] == "general"))
    return out


REQUIRED = (
    [("gemm_up_fused<1>",), ("gemm_up4_partial<1>",), ("gemm_up_partial<1>",), ("gemm_down_tiled<1>",),
     ("down_chunk_insts[0]", 2), ("down_chunk_insts[0]", 4), ("down_next_insts[0]", False), ("down_next_insts[0]", True)]
    + [("k1_stream<1>", na, False, gen) for na in (0, 1) for gen in (False, True)]
    # (the rider with the GENERAL epilogue runs only where the negative-phase K1 of a CD-2 pass samples at a Philox row offset that
    #  is no multiple of 4 -- test_row_offset_gpu.py's hinted shards, parity mode; at offset 0 the rider is lean)
    + [("k1_stream<1>", 0, True, False)]
    # (k2_stream with 2 / 3 MFMA tiles per block needs the k2s_rows knob, which a Gibbs step honours and writes a final state: general)
    + [("k2_stream<1>", 1, gen) for gen in (False, True)] + [("k2_stream<1>", 2, True), ("k2_stream<1>", 3, True)]
    + [("gemm_down_fused<1>", vec4, kind) for vec4 in (False, True) for kind in ("bit plane", "one term")])


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
# Philox seed per case that draws: the first seed >= 1 whose margins pass (printed by `python tests/fast_cases.py`); others take 1
SEEDS = {
    "fast-cd-130x70-B33-k2-mixed-unknown": 2,
    "fast-cd-1040x36-B64-k1-mixed-unknown": 3,
    "fast-cd-1040x36-no_bits-rows12-B64-k2-mixed-unknown": 3,
    "fast-cd-1040x36-no_k1s_real-B64-k1-mixed-unknown": 3,
    "fast-cd-1040x36-group-B64-k2-mixed-unknown": 3,
    "fast-seq-stats-1040x36-B130": 9,
    "fast-seq-stats-1040x36-no_bits-B64": 4,
    "fast-seq-stats-1040x36-no_bits-rows12-B130": 9,
    "fast-seq-stats-1040x36-no_k1s-B64": 4,
    "fast-seq-stats-1040x36-no_k1s_real-B130": 9,
    "fast-seq-stats-1040x36-no_adaptive-B64": 4,
    "fast-seq-stats-1040x36-group-B64": 3,
    "fast-seq-stats-1100x12-B130": 7,
    "fast-step-1040x36-B130-prefetch": 7,
    "fast-step-1040x36-group-B64": 3,
}


def has_draws(c):
    return c["kind"] in ("pass", "seq", "step", "chain") or (c["kind"] == "gibbs" and c["sample_h"]) or bool(c.get("sample"))


def margins(c, seed=None):
    """(smallest Bernoulli margin, smallest categorical margin) of the case's twin at `seed` (the case's own where None)."""
    if c["kind"] in ("pass", "seq"):
        m = twin_cd(c, seed)[1]
    elif c["kind"] == "step":
        m = twin_steps(c, seed)[1]
    elif c["kind"] == "chain":
        m = twin_chain(c, seed=seed)[1]
    elif c["kind"] == "gibbs":
        m = twin_gibbs(c, seed=seed)["m"]
    else:
        m = twin_up(c, seed)[3]
    return m.bern, m.cat


@functools.lru_cache(maxsize=None)
def _all():
    cs = up_cases() + down_cases() + gibbs_cases() + cd_cases() + step_cases() + chain_cases() + [dict(FREE), dict(SQERR)]
    for c in cs:
        c["seed"] = SEEDS.get(c["id"], 1)
    assert len({c["id"] for c in cs}) == len(cs), "duplicate case id"
    return tuple(cs)


def cases(kind=None):
    return [c for c in _all() if kind is None or c["kind"] == kind or (kind == "up" and c["kind"] == "forward")]


def pinned_seeds():
    out = {}
    for c in _all():
        if not has_draws(c):
            continue
        for seed in range(1, 200):
            bm, cm = margins(c, seed)
            if bm >= MARGIN and cm >= MARGIN:
                break
        else:
            raise SystemExit(f"no seed for {c['id']}")
        if seed != 1:
            out[c["id"]] = seed
    return out


if __name__ == "__main__":      # pin the seeds: prints the SEEDS table
    print("SEEDS = {")
    for k, v in pinned_seeds().items():
        print(f'    "{k}": {v},')
    print("}")
