"""Cases shared by test_signed_operands_cpu.py and test_signed_operands_gpu.py: SIGNED operands, and operands far outside [0, 1], on
every propagation route of prop() (csrc/host_prop.hpp) and every route of the weight update (csrc/host_update.hpp), against float64.
route_cases.py and update_cases.py feed values in [0, 1] only; backprop_step, delta_step, the centered and the Gaussian RBM and the
label-gradient paths push error rows, -p, v - mu and v / sigma^2 through the same prep_operand -> prop() -> launch_assoc path.

Operand kinds (fixed PCG64 generators, fp32):
  signed        N(0, 0.3^2): error rows
  gauss         per column (offset + scale N(0, 1)) / exp(logvar), offset in (-1, 1), scale in (0.3, 3), logvar in (-1, 1): |x| reaches ~25
  pm1           {-1, -0.0, 0, 1} laid out by the 8-row x 64-column tiles of the exactness map (PrepArgs::flag): every tile holds a -0.0;
                the 64 x 64 items of the adaptive preparation alternate like a chess board between "clean" (all tiles {0, -0.0, 1}:
                binary by the flag's own test x == 0 || x == 1) and "dirty" (every other 8-row tile holds ONE -1 among 0 / 1 values:
                one-term but not binary); item (0, 0) is dirty.  `pm1_clean`: the same with every -1 replaced by 1
  signed_mixed  route_cases' `mixed` with the real-valued half negated
  signed narrow / signed wide   update_cases' `narrow` and `wide` times a sign per element (exact kinds of the update)

Propagation.  Every row of route_cases.UP_SHAPES / DOWN_SHAPES with its options, 130 x 72 added going down, all kinds on each:
  raw       backprop_step(apply=False) with the layer input at the constant 0.5 (x (1 - x) = 0.25 exactly): a quarter of the bias-free
            product, held element by element to 0.25 (N + 16) 2^-23 sum |e| |W| (test_backprop_gpu._err_close); the run on negated
            error rows is held to the same bound against the negated reference (it is not the negated bits on any route: the sum
            inside a bf16 MFMA is not sign-symmetric, test_signed_operands_gpu.py); a NaN-filled and a zero-filled workspace must
            give the same bits; no parameter moves
  logits    prop_down(logits_only=True): the same bound with |bias| added to the magnitude sum
  prob      prop_up / prop_down at T in {1, 0.7} within route_cases.prob_bound(T); every kind but pm1 is scaled by a power of two so
            that the float64 logits / T stay within +-6 (pm1 stays within it unscaled)
  forward   forward(data_binary=True) of pm1_clean on stream_bits: bit-equal to the batch with -0.0 replaced by +0.0
  gibbs     gibbs_step(sample_h=True) at 130 x 72: k2_stream.  Its operand is a bit plane by construction (hid_bits of a sampled h), so a
            signed value reaches it only through the K1 in front: p(h|v) against float64, h against the Philox draw wherever
            |p - u| > MARGIN, and p(v|h) against float64 OF THE DEVICE'S h (no seed is pinned)
A propagation with logits_only never takes k1_stream (Route::up): the raw form of the stream_real rows runs partial4, and stream_real
itself is reached by the prob cases.  raw_up_route() states that rule; each case asserts HipEngine.last_route().

  route \\ kind     signed  gauss  pm1  signed_mixed
  fused            raw prob  raw prob  raw prob  raw prob
  stream_real      prob      prob      prob      prob
  stream_bits      -         -         forward (pm1_clean)   -
  partial4         raw prob  raw prob  raw prob  raw prob
  partial          raw prob  raw prob  raw prob  raw prob
  down_fused       raw logits prob on all four (float4 / scalar rows, one block per (tile, chunk), 130 x 72)
  down_chunks2     raw logits prob on all four
  down_chunks4     raw logits prob on all four
  down_tiled       raw logits prob on all four (B = 128 and 192)
  k2_stream        gibbs on all four (behind a fused K1 that reads the signed operand)

Update (eng.assoc_update, all four slots signed; each case asserts imdbn_debug_last_update).  Configurations: update_cases.CONFIGS
(300 x 132 at 1, 2, 3 tiles per block; 700 x 132 at 1, 2, 3, 5; 128 x 128; 130 x 36; the xa = 2, 4, 1, 8 shapes; 300 x 45 and
generic_k3 = 1: the generic kernel) and 1100 x 260 on the NaN-poisoned pitch 288, planes and generic.
  exact     group A's construction (row-sparse side, W = W_m = 0, lr 1, n a power of two) with `signed wide` x `signed narrow` and
            `signed narrow` x `signed wide`, the signs on the positive phase, the negative phase and both: BIT-EQUAL to float64
  bin       the two-plane body (assoc_update_bin): one chunk, one-term `signed narrow` operands in all four slots.  assoc_update
            reaches it only where the negative visible operand has ONE plane, which is HT = 1 (update_cases' `A-fast` cases); the
            inputs are bf16-exact, so that mode rounds nothing
  general   `signed` x `signed` and `gauss` visible x `signed` hidden, lr 0.07, momentum 0.6, weight decay 1e-3, B in {40, 64, 130,
            256}: float64 within update_cases.TOL.  An fp32 numpy emulation of the same sum (split3 terms, fp32 accumulation chunk
            by chunk) fits TOL with a factor 4 to spare on every case (test_signed_operands_cpu.py; worst measured: 0.007 of TOL)
  aliased   backprop_step(apply=True) up-only, down-only and both against backprop_oracle at 1040 x 37 B = 33, 1040 x 36 B = 130
            (also with a 0/1 x_v: an all-binary exactness map next to signed three-term error slots) and 4100 x 72 B = 128
The rank kernels (assoc_update_planes_ranks) read the factor blocks of a CD pass, which draws: k3_tpb = 5 through assoc_update runs
assoc_update_planes at five tiles per block, as update_cases has it.

  route \\ kind          signed  gauss  signed narrow / wide
  planes t1 t2 t3 t5    general general exact
  planes xa 1 2 4 8     general general exact
  generic (shape, opt)  general general exact
  pitch 288 + NaN       general general exact (planes and generic)
  bin                   -       -       bin (signed narrow)
  3 and 4 passes        B = 130, 256 general; B = 128, 256 exact"""
import functools

import numpy as np

import route_cases as RC
import update_cases as UC

F32, F64 = np.float32, np.float64
KINDS = ("signed", "gauss", "pm1", "signed_mixed")
_KIND_ID = {"signed": 1, "gauss": 2, "pm1": 3, "signed_mixed": 4, "uniform": 5, "binary": 6}
LOGIT_CAP = 6.0
PROB_TEMPS = (1.0, 0.7)
TILE_ROWS, TILE_COLS, ITEM_ROWS = 8, 64, 64         # PrepArgs::flag tiles; items of the adaptive preparation (prep_item_process)
cdiv = UC.cdiv


def _gen(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def item_dirty(iy, tx):
    """The 64 x 64 item (row block iy, column tile tx) of a pm1 array holds -1 somewhere."""
    return (iy + tx) % 2 == 0


def tile_minus(ty, tx):
    """The 8 x 64 tile (ty, tx) of a pm1 array holds exactly one -1."""
    return item_dirty(ty // (ITEM_ROWS // TILE_ROWS), tx) and ty % 2 == 0


def _pm1(g, B, N):
    x = (g.random((B, N), dtype=F32) > 0.6).astype(F32)
    x[(g.random((B, N), dtype=F32) < 0.2) & (x == 0)] = F32(-0.0)
    for ty in range(cdiv(B, TILE_ROWS)):
        for tx in range(cdiv(N, TILE_COLS)):
            r0, c0 = TILE_ROWS * ty, TILE_COLS * tx
            h, w = min(TILE_ROWS, B - r0), min(TILE_COLS, N - c0)
            assert h * w >= 2, (B, N)
            k = (3 * ty + 5 * tx) % (h * w)
            x[r0 + k // w, c0 + k % w] = F32(-0.0)
            if tile_minus(ty, tx):
                k = (k + 1 + (ty + tx) % (h * w - 1)) % (h * w)      # another element of the tile
                x[r0 + k // w, c0 + k % w] = F32(-1.0)
    return x


@functools.lru_cache(maxsize=None)
def operand(kind, B, N, tag=0):
    """[B, N] fp32 of a kind above; `uniform` in (0.02, 0.98) and `binary` 0/1 are the layer inputs of the aliased cases."""
    g = _gen(_KIND_ID[kind.replace("_clean", "")], B, N, tag)
    if kind == "signed":
        x = g.standard_normal((B, N), dtype=F32) * F32(0.3)
    elif kind == "gauss":
        off, sc, lv = g.uniform(-1.0, 1.0, N), g.uniform(0.3, 3.0, N), g.uniform(-1.0, 1.0, N)
        x = ((off + sc * g.standard_normal((B, N))) / np.exp(lv)).astype(F32)
    elif kind == "pm1":
        x = _pm1(g, B, N)
    elif kind == "pm1_clean":
        x = operand("pm1", B, N, tag).copy()
        x[x == -1] = 1
    elif kind == "signed_mixed":
        x = RC.operand("mixed", B, N).copy()
        x[:, N // 2:] *= F32(-1)
    elif kind == "uniform":
        x = g.uniform(0.02, 0.98, (B, N)).astype(F32)
    else:
        assert kind == "binary", kind
        x = (g.random((B, N), dtype=F32) > 0.6).astype(F32)
    x.setflags(write=False)
    return x


def tile_flags(x):
    """(nonbinary [tiles y, tiles x], bits [B, N]) with the two expressions of prep_operand: a tile is non-binary when some element
    has x != 0 && x != 1; the bit plane holds x != 0."""
    B, N = x.shape
    nb = (x != 0) & (x != 1)
    out = np.zeros((cdiv(B, TILE_ROWS), cdiv(N, TILE_COLS)), bool)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            out[ty, tx] = nb[TILE_ROWS * ty:TILE_ROWS * (ty + 1), TILE_COLS * tx:TILE_COLS * (tx + 1)].any()
    return out, x != 0


# ---- propagation: references --------------------------------------------------------------------------------------------------------
def logits64(x, V, H, up, bias=True):
    """(float64 logits of x through the case parameters, the magnitude sum sum |x| |W| (+ |bias|) alongside)."""
    W, hb, vb = RC.params(V, H)
    W64 = W.astype(F64) if up else W.astype(F64).T
    b = (hb if up else vb).astype(F64) if bias else 0.0
    x64 = np.asarray(x, F64)
    return x64 @ W64 + b, np.abs(x64) @ np.abs(W64) + np.abs(b)


@functools.lru_cache(maxsize=None)
def prob_scale(kind, V, H, B, up):
    """The power of two that brings the float64 logits / T of the kind's operand within +-LOGIT_CAP at every T of PROB_TEMPS (1: none
    needed).  pm1 is never scaled: test_signed_operands_cpu.py asserts that it needs none."""
    x = operand(kind, B, V if up else H)
    worst = float(np.abs(logits64(x, V, H, up)[0]).max()) / min(PROB_TEMPS)
    if worst <= 0.95 * LOGIT_CAP or kind.startswith("pm1"):
        return 1.0
    return float(2.0 ** np.floor(np.log2(0.95 * LOGIT_CAP / worst)))


def prob_operand(c):
    """The operand of a prob / forward / gibbs case, scaled (exactly: a power of two)."""
    up = c["kind"] != "prob_down"
    x = operand(c["operand"], c["B"], c["V"] if up else c["H"])
    return (x * F32(prob_scale(c["operand"], c["V"], c["H"], c["B"], up))).astype(F32)


def raw_input(c):
    """(error rows fed, up: they are sent UP through W).  raw_down: the up pair (x_v, e_h), e_h goes down; raw_up: the down pair."""
    up = c["kind"] == "raw_up"
    return operand(c["operand"], c["B"], c["V"] if up else c["H"]), up


def ref_raw(c):
    """(float64 quarter of the bias-free product, quarter of the magnitude sum, the summed dimension N)."""
    e, up = raw_input(c)
    l, mag = logits64(e, c["V"], c["H"], up, bias=False)
    return 0.25 * l, 0.25 * mag, (c["V"] if up else c["H"])


def err_tol(mag, N):
    """test_backprop_gpu._err_close's bound: (N + 16) 2^-23 times the magnitude sum."""
    return (N + 16) * 2.0 ** -23 * mag


# ---- propagation: cases ---------------------------------------------------------------------------------------------------------------
DOWN_TABLE = list(RC.DOWN_SHAPES) + [("down_fused", 130, 72, 33, {}), ("down_fused", 130, 72, 130, {})]


def raw_up_route(route, H):
    """Route::up with logits_only: gemm_up_fused where the shape allows it, else the split-K kernels, never k1_stream."""
    return route if route == "fused" else ("partial4" if H % 4 == 0 else "partial")


def prop_cases():
    out = []
    for si, (route, V, H, opts) in enumerate(RC.UP_SHAPES):
        for ki, kind in enumerate(KINDS):
            B = RC.BATCHES[(si + ki) % 3]
            out.append(dict(kind="raw_up", id=f"raw_up-{route}-{V}x{H}-B{B}-{kind}", V=V, H=H, B=B, operand=kind, opts=opts,
                            route={"up": raw_up_route(route, H), "up_epilogue": "general"}))
            for ti, T in enumerate(PROB_TEMPS):
                B = RC.BATCHES[(si + ki + ti + 1) % 3]
                out.append(dict(kind="prob_up", id=f"prob_up-{route}-{V}x{H}-B{B}-T{T}-{kind}", V=V, H=H, B=B, T=T, operand=kind, opts=opts,
                                route={"up": route, "up_epilogue": RC._lean(route, T == 1.0, True)}))
    for route, V, H, B, opts in DOWN_TABLE:
        for kind in KINDS:
            general = {"down": route, "down_epilogue": "general", "finish_groups": False}
            out.append(dict(kind="raw_down", id=f"raw_down-{route}-{V}x{H}-B{B}-{kind}", V=V, H=H, B=B, operand=kind, opts=opts, route=general))
            out.append(dict(kind="logits_down", id=f"logits_down-{route}-{V}x{H}-B{B}-{kind}", V=V, H=H, B=B, T=1.0, operand=kind, opts=opts,
                            route=general))
            for T in PROB_TEMPS:
                out.append(dict(kind="prob_down", id=f"prob_down-{route}-{V}x{H}-B{B}-T{T}-{kind}", V=V, H=H, B=B, T=T, operand=kind, opts=opts,
                                route={"down": route, "down_epilogue": RC._lean(route, T == 1.0, True), "finish_groups": False}))
    for B in (33, 130):
        out.append(dict(kind="forward", id=f"forward-stream_bits-1040x36-B{B}-pm1_clean", V=1040, H=36, B=B, T=1.0, operand="pm1_clean",
                        opts={}, route={"up": "stream_bits", "up_epilogue": "lean"}))
    for ki, kind in enumerate(KINDS):
        for B in (33, 130):
            out.append(dict(kind="gibbs", id=f"gibbs-k2_stream-130x72-B{B}-{kind}", V=130, H=72, B=B, T=1.0, operand=kind, opts={}, seed=3 + ki,
                            route={"up": "fused", "up_epilogue": "lean", "down": "k2_stream", "down_epilogue": "general",
                                   "finish_groups": False}))
    assert len({c["id"] for c in out}) == len(out)
    return out


# ---- update: operands -------------------------------------------------------------------------------------------------------------------
def _signs(shape, *key):
    return np.where(_gen(7, *key).random(shape) < 0.5, F32(-1), F32(1)).astype(F32)


@functools.lru_cache(maxsize=None)
def exact_operand(form, kind, signed, B, N, name):
    """update_cases' dense / sparse operand of `kind`, times a fixed sign per element where `signed` (0 then becomes -0.0 in places)."""
    x = {"dense": UC.dense, "sparse": UC.sparse}[form](kind, B, N, name)
    if signed:
        x = (x * _signs(x.shape, B, N, sum(map(ord, name + kind)))).astype(F32)
        x.setflags(write=False)
    return x


def update_operands(c):
    """(vpos, hpos, vneg, hneg) fp32 of an update case."""
    B, V, H = c["B"], c["V"], c["H"]
    out = []
    for name, N in (("vpos", V), ("hpos", H), ("vneg", V), ("hneg", H)):
        k = c["kinds"][name]
        out.append(exact_operand(*k, B, N, name) if len(k) == 3 else operand(k[0], B, N, sum(map(ord, name))))
    return out


def exactness(ops):
    """update_cases.exactness on given operands: (q exponent, largest sum over both phases of |term products| of one output element
    in units of q = 2^e).  Signs change nothing: partial sums stay multiples of q and are bounded by the magnitude sum."""
    vp, hp, vn, hn = ops
    tv, th = [UC.split3(vp), UC.split3(vn)], [UC.split3(hp), UC.split3(hn)]
    qv = min(e for e in (UC.quantum_exp(t) for ph in tv for t in ph) if e is not None)
    qh = min(e for e in (UC.quantum_exp(t) for ph in th for t in ph) if e is not None)
    total = sum(sum(np.abs(t.astype(F64)) for t in tv[ph]).T @ sum(np.abs(t.astype(F64)) for t in th[ph]) for ph in range(2))
    return qv + qh, float(total.max()) / 2.0 ** (qv + qh)


# ---- update: cases -------------------------------------------------------------------------------------------------------------------
ALL_CONFIGS = UC.CONFIGS + [UC.PITCHED, UC.PITCHED_GENERIC]
COMBOS = {     # name: (visible form, visible kind, hidden form, hidden kind), both signed
    "swideV-snarrowH": ("sparse", "wide", "dense", "narrow"),
    "snarrowV-swideH": ("dense", "narrow", "sparse", "wide"),
}
PLAIN = {"swideV-snarrowH": UC._plain("wideV-narrowH"), "snarrowV-swideH": UC._plain("binaryV-wideH")}      # the unsigned phase


def _phase(combo, carries):
    vf, vk, hf, hk = COMBOS[combo] if carries else PLAIN[combo]
    return (vf, vk, carries), (hf, hk, carries)


def exact_cases():
    out = []
    for ci, cfg in enumerate(ALL_CONFIGS):
        for pi, phase in enumerate(UC.PHASES):
            combo = list(COMBOS)[(ci + pi) % 2]
            B = UC.A_BATCHES[(ci + pi) % 3]
            if COMBOS[combo][2] == "sparse" and not UC.covers_every_row(B, cfg["H"]):
                B = 128
            vp, hp = _phase(combo, phase in ("pos", "both"))
            vn, hn = _phase(combo, phase in ("neg", "both"))
            out.append(UC._base(cfg, id=f"exact-{cfg['name']}-{combo}-{phase}-B{B}", group="exact", entry="assoc_update", B=B, config=cfg["name"],
                                expect=UC._expect(cfg), kinds=dict(vpos=vp, hpos=hp, vneg=vn, hneg=hn)))
    for cfg in (UC.CONFIGS[0], UC.CONFIGS[2], UC.CONFIGS[5], UC.PITCHED):
        k = ("dense", "narrow", True)
        out.append(UC._base(cfg, id=f"bin-{cfg['name']}-B64", group="exact", entry="assoc_update", B=64, mode="fast", config="bin",
                            expect=(UC.UPDATE_BIN, cfg["tpb"]), kinds=dict(vpos=k, hpos=k, vneg=k, hneg=k)))
    return out


def general_cases():
    out = []
    for ci, cfg in enumerate(ALL_CONFIGS):
        for k, vkind in enumerate(("signed", "gauss")):
            B = UC.B_BATCHES[(ci + 2 * k + ci // 4) % 4]
            out.append(UC._base(cfg, id=f"general-{cfg['name']}-B{B}-{vkind}", group="general", entry="assoc_update", B=B, config=cfg["name"],
                                expect=UC._expect(cfg), sparsity=False,
                                kinds=dict(vpos=(vkind,), hpos=("signed",), vneg=(vkind,), hneg=("signed",))))
    return out


def ref_exact(c):
    return UC.ref_update(UC.zero_params(c["V"], c["H"]), UC.stats64([update_operands(c)]), 1.0, 0.0, 0.0, c["B"])


def ref_general(c):
    return UC.ref_update(UC.params(c["V"], c["H"]), UC.stats64([update_operands(c)]), UC.B_LR, UC.B_MOM, UC.B_WD, c["B"])


def emulate_general(c):
    """The update of a general case in fp32 numpy: the nine term products of split3 per phase, accumulated in fp32 chunk by chunk (the
    order of the host's launches), then the momentum / decay arithmetic in fp32.  What ANY fp32 kernel of this sum may be off by."""
    st, ops = UC.params(c["V"], c["H"]), update_operands(c)
    lr, mom, wd, n = F32(UC.B_LR), F32(UC.B_MOM), F32(UC.B_WD), F32(c["B"])
    acc = np.zeros((c["V"], c["H"]), F32)
    sums = [np.zeros(a.shape[1], F32) for a in ops]
    for ch in UC.chunks(ops, c["B"]):
        for v, h, sign in ((ch[0], ch[1], F32(1)), (ch[2], ch[3], F32(-1))):
            for a in UC.split3(v):
                for b in UC.split3(h):
                    acc += sign * (a.T @ b)
        for s, a in zip(sums, ch):
            s += a.sum(0, dtype=F32)
    W_m = mom * st["W_m"] + lr * (acc / n - wd * st["W"])
    hb_m = mom * st["hb_m"] + lr * (sums[1] - sums[3]) / n
    vb_m = mom * st["vb_m"] + lr * (sums[0] - sums[2]) / n
    return dict(W=st["W"] + W_m, hid_bias=st["hid_bias"] + hb_m, vis_bias=st["vis_bias"] + vb_m, W_m=W_m, hb_m=hb_m, vb_m=vb_m)


def tol_fraction(got, ref, tol=UC.TOL):
    """How much of the tolerance (golden_utils.assert_close: relative Frobenius OR all elements within atol) a result uses: <= 1 passes."""
    d = np.asarray(got, F64) - ref
    n = float(np.linalg.norm(ref))
    rel = float(np.linalg.norm(d)) / n if n > 0 else float(np.linalg.norm(d))
    return min(rel / tol["rel"], float(np.abs(d).max()) / tol["atol"])


# ---- aliased slots: backprop_step(apply=True) at route-edge layers -------------------------------------------------------------------------
ALIASED = [   # name, V, H, B, kind of x_v, down route (e_h going down), update expected
    ("1040x37-B33", 1040, 37, 33, "uniform", "down_fused", (UC.UPDATE_GENERIC, 0)),
    ("1040x36-B130", 1040, 36, 130, "uniform", "down_fused", (UC.UPDATE_PLANES, 1)),
    ("1040x36-B130-binary", 1040, 36, 130, "binary", "down_fused", (UC.UPDATE_PLANES, 1)),
    ("4100x72-B128", 4100, 72, 128, "uniform", "down_tiled", (UC.UPDATE_PLANES, 1)),
]
ALIASED_FORMS = {"up": (True, False), "down": (False, True), "both": (True, True)}


def aliased_cases():
    out = []
    for name, V, H, B, xkind, down, expect in ALIASED:
        for form in (ALIASED_FORMS if xkind == "uniform" else ("up", "both")):
            up, dn = ALIASED_FORMS[form]
            route = {}
            if up:
                route.update({"down": down, "down_epilogue": "general", "finish_groups": False})
            if dn:
                route.update({"up": raw_up_route("partial", H), "up_epilogue": "general"})
            out.append(dict(id=f"aliased-{name}-{form}", V=V, H=H, B=B, xkind=xkind, form=form, route=route, expect=expect, opts={}))
    return out


@functools.lru_cache(maxsize=None)
def aliased_layer(V, H):
    """The layer as a pcd_cases-style dict: route_cases' parameters with small non-zero momenta."""
    W, hb, vb = RC.params(V, H)
    g = _gen(8, V, H)
    return dict(W=W, b=vb, c=hb, groups=[], W_m=(g.standard_normal((V, H)) * 0.01).astype(F32),
                hb_m=(g.standard_normal(H) * 0.01).astype(F32), vb_m=(g.standard_normal(V) * 0.01).astype(F32))


def aliased_io(c):
    """dict(x_v, e_h, x_h, e_v): inputs uniform in (0.02, 0.98) (x_v 0/1 where the case says so), errors `signed`."""
    V, H, B = c["V"], c["H"], c["B"]
    return dict(x_v=operand(c["xkind"], B, V, 1), e_h=operand("signed", B, H, 2), x_h=operand("uniform", B, H, 3), e_v=operand("signed", B, V, 4))
