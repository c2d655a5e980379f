"""Cases shared by test_groups_cpu.py and test_groups_gpu.py: softmax groups up to the engine's limits -- four per visible layer
(IMDBN_MAX_GROUPS), each up to 256 columns wide (GROUP_WMAX) -- on every down route of prop() (csrc/host_prop.hpp) behind which
finish_groups (csrc/kernels_ew.hpp) runs, against float64.  Parameters, operands and the float64 pieces are route_cases.py's.

Layouts (LAYOUTS; V = 1040 or 4100), each the smallest that reaches its edge:

  w33         (V-33, V)     first width at which finish_groups' element loop (it < wd * 8, 256 threads) wraps; wd % 8 = 1
  w65         (V-65, V)     past a wave and past one 64-column tile; a tail of 1 in the 8-wide row loops
  w255, w256  the limit and one below: a scalar tail of 7, and none; 16 K blocks, 4 (5) epilogue tiles, 8 wraps of the element loop
  four        (0, 5) (60, 133) (133, 389) (1039, 1040): a group at column 0; two groups sharing a boundary; one crossing columns 64
              and 128; a 256-wide group in slot 2; a width-1 group in slot 3 at the last column
  three-mid   (100, 140) (500, 533) (1000, 1030): none touching the end of the layer, one crossing column 1024 (the last 128-row
              tile boundary before Vpad)
  w256 at V = 4100   (3844, 4100): ends with the layer, in the 128-row tile that holds 4 real rows
  four at V = 4100   (0, 5) (1847, 1920) (1920, 2176) (4099, 4100): the 256-wide group crosses row 2048

Calls, each asserting its route through HipEngine.last_route(), "finish_groups": True included:

  down     prop_down (probabilities) at the three TEMPS: down_fused with float4 rows (1040 x 36, B = 130) and scalar rows (1040 x 37,
           B = 33); down_chunks2 / down_chunks4 / down_tiled at 4100 x 72 with the batches and options of route_cases.DOWN_SHAPES
  gibbs    gibbs_step(sample_v=True) on Philox draws: k2_stream (sampled h), down_fused from the bit plane (no_k2s) and from the
           mean-field operand at 1040 x 36; the three 4100-column routes with a mean-field h at B = 128 / 256.  plan_down
           (csrc/host_prop.hpp) keeps a K2 off the chunked and tiled kernels only when it must also write the K16-blocked operand
           form (rm_src with op.rm); gibbs_step's K2 asks for none, so a mean-field h does reach them and they are covered here
           with samples as well as by `down`.  The step takes the Bernoulli tensor at draw 1 (0 with a mean-field h) and group g's
           categorical at the draw after it + 1 + g; the draws consumed are asserted (route_cases.gibbs_draws)
  tape     the `four` layout once through ReplayRng: the categorical tape is read at cat_tape + g * B
  train    RBM.train_epoch with CD = 1 and 2 on w256 and four, 1040 x 36, B = 33 and 130: the operand forms and column sums that
           finish_groups rewrites feed the weight update, the group loss slots enter the loss; against cd_cases.ref_pass and
           update_cases.ref_update within update_cases.TOL, the loss as test_cd_routes_gpu.py compares it
  chain    train_epoch_clamped as the `clamped-hv` call of route_cases.CHAIN_CALLS (vmode 2) and noisy_meanfield_annealed with the
           mu-pull, on w65 with a mask that clamps the first half of the group (and of the features) and leaves the rest free;
           compared with the oracle as test_routes_gpu.py compares its chains
  sample   sample_visible (categorical_rows) on a [B, V] probability tensor, `four`, B = 1, 64, 65, Philox and tape

Bounds.  Sigmoid columns: route_cases.prob_bound(T).  Softmax columns, from the logit bound d = route_cases.logit_bound(raw, T):
p_j = e_j / Z with e_j = exp(l_j - max).  Logits off by at most d move every e_j by a factor within exp(+-d) (the shift of the
maximum included: it cancels in the quotient) and Z, a sum of such terms, by a factor within exp(+-d); the quotient moves by a
factor within exp(+-2 d), and since the p_j still sum to one the movement of p_j is at most p_j (1 - p_j) (exp(2 d) - 1) [as
chain_cases.group_bound].  expf (1 ulp), the ordered fp32 sum of w terms and the division add p_j (w + 4) u, u = 2^-24:

  |p_j - float64| <= p_j (1 - p_j) expm1(2 d) + p_j (w + 4) u                                                   (softmax_bound)

Categorical decisions must equal the reference's with no exception, so every drawing case's Philox seed is pinned on the CPU with
the fp32 oracle alone (`python tests/group_cases.py` prints SEEDS): the first seed >= 1 whose smallest Bernoulli margin is at
least route_cases.MARGIN and whose smallest categorical margin (oracle.draws.CATEGORICAL_MARGIN, relative to the row total) is at
least cat_margin(width of the widest group).  A pick is the first j with cum_j > u_draw * total, so what must not move is
cum_j / total next to u_draw; the threshold bounds how far that quotient can lie apart between two left-to-right fp32 cumulative
sums of w clamped probabilities (the device's and the oracle's) that are each a softmax of logits within d0 of float64:
  inputs   an error of the row sum Z is common to every p_j of the row and cancels in cum_j / total; what remains per column is the
           factor exp(+-2 d0) of the logits and expf, the subtraction of the maximum and the division (4 u): each side moves the
           quotient by at most expm1(2 d0) + 4 u (the clamp to [1e-8, 1] is 1-Lipschitz; a clamped entry of the mask is the same
           number on both sides).  d0 = 4 prob_bound(T) is the logit error that prob_bound already presumes of the same GEMM (a
           sigmoid's slope is at most 1/4) -- the absolute bound of test_products_are_fp32_exact, not logit_bound's relative term
  sums     the prefix and the total of each side round once per addition, by at most u times a partial sum <= total.  The worst
           case (every rounding at half an ulp, all in one direction, 4 w u = 6.1e-5 at w = 256) is NOT what is used: a pick lands
           in an interval of relative length p_j ~ 1 / w, so a margin m fails a pick with probability 2 m w, and at 4 w u no seed
           exists for the 260 picks of a CD-2 pass at B = 130, w = 256 (0.97^260).  The threshold takes the roundings as w
           independent errors uniform in +-u: standard deviation u sqrt(w / 3) per sum, six of them, four sums added linearly

  cat_margin(w) = 2 (expm1(2 d0) + 4 u) + 24 u sqrt(w / 3)           (2.2e-5 at w = 256, 1.0e-5 at w = 5)

A pick that differs on the device where this margin holds is reported as a failure, never forgiven.  A seed that fails the margins
is replaced in the table, never skipped."""
import functools

import numpy as np

import cd_cases as CC
import oracle.rbm_oracle as O
import route_cases as RC
import update_cases as UC
from oracle.draws import CATEGORICAL_MARGIN, DrawStream, PhiloxStream
from route_cases import MARGIN, TEMPS, logit_bound, operand, params, prob_bound, probs64      # noqa: F401  (re-exported for the tests)

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
MAX_GROUPS, GROUP_WMAX = 4, 256                      # include/imdbn_engine.h IMDBN_MAX_GROUPS, csrc/kernels_ew.hpp GROUP_WMAX
SIZE_CAP = 4100 * 72 * 256                           # V * H * B of the largest case
TRAIN_EPOCH, MAX_EPOCHS = 1, 10
SEED_SEARCH = 3000                                   # seeds the pinning tries: a 256-row batch with a 256-wide group passes about one seed in 150
OPTION_DEFAULTS = {"no_k2s": 0, "no_down_tiled": 0}


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
def _end(w):
    return lambda V: ((V - w, V),)


LAYOUTS = {   # name -> V -> groups
    "w33": _end(33), "w65": _end(65), "w255": _end(255), "w256": _end(256),
    "four": lambda V: ((0, 5), (60, 133), (133, 389), (V - 1, V)) if V == 1040 else ((0, 5), (1847, 1920), (1920, 2176), (V - 1, V)),
    "three-mid": lambda V: ((100, 140), (500, 533), (1000, 1030)),
}
NARROW = ("w33", "w65", "w255", "w256", "four", "three-mid")      # at V = 1040
WIDE = ("w256", "four")                                             # at V = 4100


def groups_of(layout, V):
    return LAYOUTS[layout](V)


def shifted(groups, V):
    """Every group moved by one column: to the right, or to the left where it ends with the layer."""
    return tuple((s + 1, e + 1) if e < V else (s - 1, e - 1) for s, e in groups)


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
def softmax_bound(p, w, d):
    return p * (1.0 - p) * np.expm1(2.0 * d) + p * (w + 4) * U


def prob_bounds(p, raw, T, groups):
    """[B, V] bound on |device - float64| of the probabilities `p` (float64) of the un-tempered float64 logits `raw`."""
    b = np.full(p.shape, prob_bound(T))
    d = logit_bound(raw, T)
    for s, e in groups:
        b[:, s:e] = softmax_bound(p[:, s:e], e - s, d)
    return b


def worst_ratio(got, ref, bound):
    """Largest |got - ref| / bound (inf where got is not finite): the comparison passes when it is at most 1."""
    got = np.asarray(got, F64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bound).max())


def cat_margin(w, T=1.0):
    """The smallest categorical margin (relative to the row total) a pinned seed must keep for a group `w` wide (module docstring)."""
    d0 = 4 * prob_bound(T)
    return float(2 * (np.expm1(2 * d0) + 4 * U) + 24 * U * np.sqrt(w / 3.0))


def case_cat_margin(c):
    return cat_margin(max(e - s for s, e in c["groups"]))


# ---- prop_down ----------------------------------------------------------------------------------------------------------------------
DOWN_SHAPES = [   # route, V, H, B, options, layouts
    ("down_fused", 1040, 36, 130, {}, NARROW),                      # float4 rows, three row blocks of finish_groups, the last ragged
    ("down_fused", 1040, 37, 33, {}, NARROW),                       # scalar rows
    ("down_chunks2", 4100, 72, 128, {"no_down_tiled": 1}, WIDE),
    ("down_chunks4", 4100, 72, 256, {"no_down_tiled": 1}, WIDE),
    ("down_tiled", 4100, 72, 128, {}, WIDE),
]


def down_cases():
    out = []
    for route, V, H, B, opts, layouts in DOWN_SHAPES:
        for name in layouts:
            for T in TEMPS:
                out.append(dict(kind="down", id=f"down-{route}-{V}x{H}-B{B}-{name}-T{T}", V=V, H=H, B=B, T=T, logits_only=0, layout=name,
                                groups=groups_of(name, V), opts=opts,
                                route={"down": route, "down_epilogue": "general", "finish_groups": True}))
    return out


def ref_down(c, groups=None):
    """(float64 probabilities, un-tempered float64 logits); `groups`: another layout than the case's (the slip check)."""
    raw = RC._down_logits64(c["V"], c["H"], c["B"])
    return probs64(raw, c["T"], c["groups"] if groups is None else groups), raw


# ---- gibbs_step -----------------------------------------------------------------------------------------------------------------------
GIBBS_ROUTES = [   # name, V, H, batches, sample_h, options, up, down, layouts
    ("k2s", 1040, 36, (33, 130), True, {}, "stream_real", "k2_stream", NARROW),
    ("bits", 1040, 36, (130, 33), True, {"no_k2s": 1}, "stream_real", "down_fused", NARROW),
    ("mf", 1040, 36, (33, 130), False, {}, "stream_real", "down_fused", NARROW),
    ("chunks2", 4100, 72, (128,), False, {"no_down_tiled": 1}, "stream_real", "down_chunks2", WIDE),
    ("chunks4", 4100, 72, (256,), False, {"no_down_tiled": 1}, "stream_real", "down_chunks4", WIDE),
    ("tiled", 4100, 72, (128,), False, {}, "stream_real", "down_tiled", WIDE),
]


def gibbs_cases():
    out = []
    for name, V, H, batches, sample_h, opts, up, down, layouts in GIBBS_ROUTES:
        for i, lay in enumerate(layouts):
            B = batches[i % len(batches)]
            out.append(dict(kind="gibbs", id=f"gibbs-{name}-{V}x{H}-B{B}-{lay}", V=V, H=H, B=B, sample_h=sample_h, sample_v=True, layout=lay,
                            groups=groups_of(lay, V), opts=opts, operand="mixed", rng="philox",
                            route={"up": up, "up_epilogue": "general", "down": down, "down_epilogue": "general", "finish_groups": True}))
    k2s = next(c for c in out if c["layout"] == "four" and c["route"]["down"] == "k2_stream")
    out.append(dict(k2s, id=f"gibbs-tape-k2s-1040x36-B{k2s['B']}-four", rng="tape"))      # the same call from a replay tape
    return out


class Tape:
    """Uniforms of a DrawStream; categorical indices of a seeded generator (a replayed index is simply a given), remembered in `cats`."""

    def __init__(self, seed):
        self.s, self.g, self.cats = DrawStream(seed), np.random.Generator(np.random.PCG64(seed + 1)), []

    def uniform(self, shape): return self.s.uniform(shape)
    def normal(self, shape): return self.s.normal(shape)

    def categorical(self, p):
        self.cats.append(self.g.integers(0, p.shape[1], p.shape[0]))
        return self.cats[-1]


def source(c):
    return PhiloxStream(c["seed"]) if c["rng"] == "philox" else Tape(c["seed"])


def ref_gibbs(c, cat_from_own_index=False):
    """float64 (v_next, v_prob, h, h_prob, un-tempered visible logits) with the decisions taken on the case's draws.
    `cat_from_own_index`: the slip check -- group g's categorical from draw g of the visible sample instead of 1 + g."""
    V, H, B = c["V"], c["H"], c["B"]
    W, hb, vb = params(V, H)
    ps = source(c)
    h_prob = RC.sigmoid64(RC._up_logits64(V, H, c["operand"], B))
    h = (h_prob > ps.uniform((B, H))).astype(F64) if c["sample_h"] else h_prob
    raw = RC._down64(W, vb, h)
    v_prob = probs64(raw, 1.0, c["groups"])
    base = getattr(ps, "offset", 0)
    v_next = (v_prob > ps.uniform((B, V))).astype(F64)
    for g, (s, e) in enumerate(c["groups"]):
        p = np.clip(v_prob[:, s:e], 1e-8, 1.0).astype(F32)
        if cat_from_own_index:
            idx = PhiloxStream(c["seed"], offset=base + g).categorical(p)
        else:
            idx = ps.categorical(p)
        v_next[:, s:e] = 0.0
        v_next[np.arange(B), s + idx] = 1.0
    if c["rng"] == "philox" and not cat_from_own_index:
        assert ps.offset == RC.gibbs_draws(c)
    return v_next, v_prob, h, h_prob, raw


def oracle_gibbs(c):
    st = RC.state(c["V"], c["H"], c["groups"])
    if c["rng"] == "philox":
        src = PhiloxStream(c["seed"])
    else:      # the oracle replays recorded indices: record the Tape's
        t = Tape(c["seed"])
        src = DrawStream(c["seed"], cat=[t.categorical(np.zeros((c["B"], e - s), F32)) for s, e in c["groups"]])
    return O.gibbs_step(st, operand(c["operand"], c["B"], c["V"]), src, c["sample_h"], c["sample_v"])


# ---- train_epoch ------------------------------------------------------------------------------------------------------------------------
def train_cases():
    out = []
    for lay in ("w256", "four"):
        for B in (33, 130):
            for k in (1, 2):
                V, H = 1040, 36
                groups = groups_of(lay, V)
                r = CC.route_of(V, H, {}, groups, B)
                route, _ = CC.expect_of(r, "unknown")
                out.append(dict(kind="train", id=f"train-{V}x{H}-B{B}-k{k}-{lay}", V=V, H=H, B=B, k=k, layout=lay, groups=groups, opts={},
                                operand="mixed", rng="philox", route=route, draws=1 + k * (2 + len(groups))))
    return out


def train_scalars(c):
    """(lr, momentum, weight decay) of the update: RBM(lr 0.1, dynamic, momentum 0.5) at epoch TRAIN_EPOCH (rbm.py:194-195)."""
    return 0.1 / (1 + 0.01 * TRAIN_EPOCH), 0.5, 1e-4


def train_state(c):
    W, hb, vb = params(c["V"], c["H"])
    return dict(W=W, hid_bias=hb, vis_bias=vb, W_m=np.zeros_like(W), hb_m=np.zeros_like(hb), vb_m=np.zeros_like(vb))


@functools.lru_cache(maxsize=None)
def _ref_train(cid):
    c = by_id(cid)
    st = train_state(c)
    ps = PhiloxStream(c["seed"])
    ref = CC.ref_pass(st["W"], st["hid_bias"], st["vis_bias"], operand(c["operand"], c["B"], c["V"]), c["k"], c["groups"], ps)
    assert ps.offset == c["draws"]
    lr, mom, wd = train_scalars(c)
    return ref, UC.ref_update(st, ref["stats"], lr, mom, wd, c["B"])


def ref_train(c):
    """(cd_cases.ref_pass of the case, float64 state after the update); computed once, shared, read-only."""
    return _ref_train(c["id"])


def oracle_train(c):
    st = RC.state(c["V"], c["H"], c["groups"])
    ps = PhiloxStream(c["seed"])
    loss = O.train_epoch(st, operand(c["operand"], c["B"], c["V"]), TRAIN_EPOCH, c["k"], ps)
    return loss, st, ps.offset


# ---- clamped chains ---------------------------------------------------------------------------------------------------------------------
CHAIN_CALLS = [c for c in RC.CHAIN_CALLS if c[0] in ("clamped-hv", "nmf-mu")]


def chain_cases():
    out = []
    V, H, lay = 1040, 36, "w65"
    groups = groups_of(lay, V)
    for cname, method, kw in CHAIN_CALLS:
        B = {"clamped-hv": 130, "nmf-mu": 27}[cname]      # 130 rows: the one of a row's label falls in the clamped half or in the free one
        clamped = method == "train_epoch_clamped"
        out.append(dict(kind="chain", id=f"chain-{cname}-{V}x{H}-B{B}-{lay}", V=V, H=H, B=B, layout=lay, groups=groups, opts={}, call=cname,
                        method=method, kw=kw, mu=cname == "nmf-mu", rng="philox",
                        route={"up": "stream_real", "up_epilogue": "lean" if clamped else "general",
                               "down": "k2_stream" if clamped else "down_fused", "down_epilogue": "general", "finish_groups": True}))
    return out


def chain_inputs(c):
    """(v_known, known_mask, mu or None): the first half of the features and of the softmax group is clamped, the rest is free; the
    label of row b is b % w, so the clamped half holds the one in some rows and only zeros in the others."""
    B, V = c["B"], c["V"]
    (s, e), = c["groups"]
    w, half = e - s, s + (e - s) // 2
    g = np.random.Generator(np.random.PCG64(31 * B + c["H"]))
    z = g.random((B, s), dtype=F32)
    mu = g.random((B, s), dtype=F32)
    vk = np.zeros((B, V), F32); km = np.zeros((B, V), F32)
    vk[:, : s // 2] = z[:, : s // 2]; km[:, : s // 2] = 1
    y = np.eye(w, dtype=F32)[np.arange(B) % w]
    vk[:, s:half] = y[:, : half - s]; km[:, s:half] = 1
    return vk, km, (mu if c["mu"] else None)


def oracle_chain(c):
    """(final state or loss, oracle state after the call, draws consumed)"""
    st = RC.state(c["V"], c["H"], c["groups"])
    vk, km, mu = chain_inputs(c)
    ps = PhiloxStream(c["seed"])
    if mu is not None:
        st.mu_pull = {"mu_k": mu, "eta0": 0.15}
    if c["method"] == "train_epoch_clamped":
        out = O.train_epoch_clamped(st, vk, km, RC.CLAMPED_EPOCH, ps, **c["kw"])
    else:
        out = getattr(O, c["method"])(st, vk, km, ps, **c["kw"])
    st.mu_pull = None
    return out, st, ps.offset


# ---- sample_visible -----------------------------------------------------------------------------------------------------------------------
def sample_cases():
    V, H, lay = 1040, 36, "four"
    return [dict(kind="sample", id=f"sample-{rng}-{V}-B{B}-{lay}", V=V, H=H, B=B, layout=lay, groups=groups_of(lay, V), opts={}, rng=rng)
            for rng in ("philox", "tape") for B in (1, 64, 65)]


def sample_input(c):
    """[B, V] fp32 probabilities: the float64 reference of the layout's visible probabilities at T = 1, rounded."""
    return probs64(RC._down_logits64(c["V"], c["H"], c["B"]), 1.0, c["groups"]).astype(F32)


def ref_sample(c, cat_from_own_index=False):
    """The decisions on the fp32 input itself (nothing is propagated: the comparison 1[p > u] is exact on both sides)."""
    p, B = sample_input(c), c["B"]
    ps = source(c)
    v = (p > ps.uniform(p.shape)).astype(F32)
    for g, (s, e) in enumerate(c["groups"]):
        q = np.clip(p[:, s:e], F32(1e-8), F32(1.0)).astype(F32)
        idx = PhiloxStream(c["seed"], offset=g).categorical(q) if cat_from_own_index else ps.categorical(q)
        v[:, s:e] = 0.0
        v[np.arange(B), s + idx] = 1.0
    return v


def oracle_sample(c):
    st = RC.state(c["V"], c["H"], c["groups"])
    if c["rng"] == "philox":
        src = PhiloxStream(c["seed"])
    else:
        t = Tape(c["seed"])
        src = DrawStream(c["seed"], cat=[t.categorical(np.zeros((c["B"], e - s), F32)) for s, e in c["groups"]])
    return O.sample_visible(st, sample_input(c), src)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
# seed per drawing case: the first seed >= 1 whose margins pass (printed by `python tests/group_cases.py`); cases not listed take seed 1
SEEDS = {
    "gibbs-k2s-1040x36-B130-w65": 2,
    "gibbs-k2s-1040x36-B33-w255": 3,
    "gibbs-k2s-1040x36-B130-w256": 17,
    "gibbs-k2s-1040x36-B33-four": 3,
    "gibbs-bits-1040x36-B33-w256": 3,
    "gibbs-bits-1040x36-B130-four": 18,
    "gibbs-bits-1040x36-B33-three-mid": 3,
    "gibbs-mf-1040x36-B130-w65": 3,
    "gibbs-chunks2-4100x72-B128-four": 9,
    "gibbs-chunks4-4100x72-B256-w256": 514,
    "gibbs-chunks4-4100x72-B256-four": 578,
    "gibbs-tiled-4100x72-B128-four": 9,
    "gibbs-tape-k2s-1040x36-B33-four": 2,
    "train-1040x36-B33-k1-w256": 3,
    "train-1040x36-B33-k2-w256": 3,
    "train-1040x36-B130-k1-w256": 17,
    "train-1040x36-B130-k2-w256": 26,
    "train-1040x36-B33-k1-four": 3,
    "train-1040x36-B33-k2-four": 3,
    "train-1040x36-B130-k1-four": 18,
    "train-1040x36-B130-k2-four": 23,
    "sample-philox-1040-B64-four": 11,
    "sample-tape-1040-B65-four": 2,
}


def has_draws(c):
    return c["kind"] != "down"


def run_oracle(c):
    """The case on the fp32 oracle with its seed: (result, smallest Bernoulli margin, smallest categorical margin)."""
    O.reset_margin()
    res = {"down": lambda c: O.visible_probs(RC.state(c["V"], c["H"], c["groups"]), operand("real", c["B"], c["H"]), c["T"]),
           "gibbs": oracle_gibbs, "train": oracle_train, "chain": oracle_chain, "sample": oracle_sample}[c["kind"]](c)
    return res, O.BERNOULLI_MARGIN["min"], CATEGORICAL_MARGIN["min"]


def margins_pass(c, bm, cm):
    """A replayed index is a given: a tape case has no categorical margin to keep."""
    return bm >= MARGIN and (c["rng"] == "tape" or cm >= case_cat_margin(c))


@functools.lru_cache(maxsize=None)
def _all():
    cs = down_cases() + gibbs_cases() + train_cases() + chain_cases() + sample_cases()
    for c in cs:
        c["seed"] = SEEDS.get(c["id"], 1)
    assert len({c["id"] for c in cs}) == len(cs), "duplicate case id"
    return tuple(cs)


def cases(kind=None):
    return [c for c in _all() if kind is None or c["kind"] == kind]


def by_id(cid):
    return next(c for c in _all() if c["id"] == cid)


def pinned_seeds():
    """SEEDS as the rule gives it: for every drawing case the first seed >= 1 whose margins pass, listed where it is not 1."""
    out = {}
    for c in _all():
        if not has_draws(c):
            continue
        keep = c["seed"]
        try:
            for seed in range(1, SEED_SEARCH):
                c["seed"] = seed
                _, bm, cm = run_oracle(c)
                if margins_pass(c, bm, cm):
                    break
            else:
                raise SystemExit(f"no seed for {c['id']}")
        finally:
            c["seed"] = keep
        if seed != 1:
            out[c["id"]] = seed
            print(f'    "{c["id"]}": {seed},', flush=True)
    return out


if __name__ == "__main__":      # pin the seeds: prints the SEEDS table
    print("SEEDS = {")
    pinned_seeds()      # prints every entry as it is found
    print("}")
