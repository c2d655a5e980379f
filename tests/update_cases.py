"""Cases shared by test_update_routes_cpu.py and test_update_routes_gpu.py: the weight / bias update (K3, csrc/kernels_gemm.hpp and
csrc/host_update.hpp) on every kernel route, each case naming the update it must launch as imdbn_debug_last_update reports it
(the kernel code IMDBN_UPDATE_* and the visible tiles per block), against a float64 reference of rbm.py:209-224.

Shapes are the smallest that cross the edge a route depends on (V x H; `tN` = the option k3_tpb = N, else the host picks the tiles
per block: 1 on every device with more CUs than the shape has tiles):

  300 x 132    three visible tiles, the last partial (rows 256..299); two column stripes, the second 4 columns wide; one fused
               bias row.  t2: groups of 2 and 1 tiles; t3: one group of three (both register sets, set A reused)
  700 x 132    six tiles.  t2 / t3: even groups; t5: groups of 5 and 1, and tiles per block > 4 is what makes the host take the
               tile-wise rank kernel (assoc_update_planes_ranks<HT, false>)
  128 x 128    one tile, one stripe; two fused bias rows (k3_bias_rows)
  130 x 36     H < 128: one partial stripe, second tile two rows high
  300 x 45     H % 4 != 0: the generic kernel (assoc_update + bias_update) by shape
  300 x 132 with generic_k3 = 1: the generic kernel by option, on aligned rows
  1024 x 132, 256 x 512, 1024 x 128, 128 x 1024: the branches xa = 2 (two slots per XCD), 4, 1, 8 of k3_block_map (every other grid
               above takes xa = 0);
               xa_of() derives the branch from the grid (ceil(H / 128), ceil(ceil(V / 128) / tiles per block))
  1100 x 260 on a forced row pitch of 288 floats, the padding of W and W_m poisoned with NaN: one case per kernel family

Batches: 64 (one chunk, n a power of two), 40 (zero rows in the chunk; the division branch of the epilogue), 130 (three launches,
PASS 1, 2, 3, ragged last chunk), 256 (four launches: two middle passes).

Operand kinds: `binary` 0/1; `narrow` {0, 1/4, 1/2, 3/4, 1} (bf16-exact: one term); `two-term` a / 1024 with 512 <= a < 1024 whose
low two bits are not both zero; `wide` a / 2^18 with 2^17 <= a < 2^18 and non-zero bits in all three bf16 terms of the truncation
split (csrc/common.hpp split3); `real` uniform fp32; `mixed` 0/1 with real-valued columns only in the LAST tile of the first
block's tile range, so that the exactness map makes that block take three positive terms and its neighbour one.

Group A (exact inputs, bit-equal to float64).  Through HipEngine.assoc_update with W = W_m = 0, zero biases and momenta, lr = 1,
momentum 0, weight decay 0, no sparsity, B in {64, 128, 256}.  One side of every phase is row-sparse -- every feature column is
non-zero in at most 6 batch rows, rows (j + k * ceil(B / 6)) mod B of column j, so the rows rotate with the column and every batch
row of every chunk is used by some column -- and the other side is dense: visible `wide` x hidden `narrow`, visible `binary` x
hidden `wide`, `two-term` x `two-term` (the (1, 1) cross product), each on the positive phase, on the negative phase and on both;
a phase that does not carry the combination has a row-sparse `binary` operand on the same side and a dense `narrow` (`binary`) one on
the other.  The positive visible operand then has one term (P = 1 + 3 = 4 planes per tile: assoc_update always passes three negative
planes in exact mode) or three (P = 6).  Every term product is a multiple of one power of two q and, per output element, the sum of
|term products| over both phases and all chunks is below 2^24 q: every partial sum in any order is an fp32 number, d / n is exact
(n a power of two), and so W_m, W, the bias momenta and the biases computed in float64 ARE fp32 numbers, which the device must
return bit for bit.  What cannot be made exact this way are the products of a second or third term with a third term (2^-8 * 2^-16
below the leading product: no room in 24 bits next to six rows): a kernel that dropped only those would pass group A; group B
bounds them at the project's tolerance.  FAST mode (HT = 1) rounds operands to bf16, so it gets `binary` and `narrow` inputs only.

Group B (general arithmetic): the same shapes and tilings with W ~ N(0, 1) / sqrt(V), non-zero momenta and biases, lr = 0.07,
momentum 0.6, weight decay 1e-3, sparsity in half the cases, `real` and `mixed` operands, B in {40, 64, 130, 256}; float64 within
the tolerance of test_assoc_update_alone_matches_oracle (TOL) on all six state tensors.

Group C (routes only a CD pass reaches): cd_stats (MODE 1), cd_factors + apply_factors (the rank kernels) and one CD-1 train_epoch
on the bin and planes routes.  The float64 reference is computed from the operand planes the update kernel read (decode_planes), so
no Philox seed has to be pinned."""
import functools
import itertools

import numpy as np

F32, F64 = np.float32, np.float64
UPDATE_GENERIC, UPDATE_PLANES, UPDATE_BIN, UPDATE_RANKS = 0, 1, 2, 3      # include/imdbn_engine.h IMDBN_UPDATE_*
OPTION_DEFAULTS = {"k3_tpb": 0, "no_update_bin": 0, "generic_k3": 0, "no_rank_acc": 0, "no_rank_loop": 0, "min_rank_loop": 2}
TOL = dict(rel=2e-5, atol=2e-6)            # test_assoc_update_alone_matches_oracle
STATS_TOL = dict(rel=2e-6, atol=2e-5)      # test_stats_then_apply_equals_fused_update_for_multi_chunk_batches
KEYS = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")
SPARSE_ROWS = 6
SPARSITY_TARGET = 0.1


def cdiv(a, b):
    return -(-a // b)


# ---- what the host and the kernels derive from a shape (csrc/host_update.hpp, k3_block_map) ------------------------------------------
def grid(V, H, tpb):
    """(hidden stripes, blocks per stripe) of the streaming update kernels, without the bias rows."""
    return cdiv(H, 128), cdiv(cdiv(V, 128), tpb)


def xa_of(V, H, tpb):
    """The branch of k3_block_map this grid takes: 0 (identity) or the hidden stripes per XCD."""
    nbx, nby = grid(V, H, tpb)
    if nbx % 2 == 0 and nby % 4 == 0:
        return 2
    if nbx % 4 == 0 and nby % 2 == 0:
        return 4
    if nby % 8 == 0:
        return 1
    if nbx % 8 == 0:
        return 8
    return 0


def bias_rows(H):
    return 1 if cdiv(H, 128) >= 2 else 2


# ---- bf16 terms -------------------------------------------------------------------------------------------------------------------
def _trunc16(x):
    return (np.ascontiguousarray(x, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def split3(x):
    """csrc/common.hpp split3 in numpy: three bf16-exact fp32 arrays with hi + mid + lo == x exactly (truncation)."""
    x = np.ascontiguousarray(x, F32)
    hi = _trunc16(x)
    r = x - hi
    mid = _trunc16(r)
    lo = r - mid
    assert np.array_equal(_trunc16(lo), lo) and np.array_equal((hi.astype(F64) + mid) + lo, x.astype(F64))
    return hi, mid, lo


def n_terms(x):
    """Number of leading non-zero bf16 terms the operand needs (1, 2 or 3)."""
    _, mid, lo = split3(x)
    return 3 if lo.any() else (2 if mid.any() else 1)


def quantum_exp(x):
    """e such that every element of the fp32 array x is a multiple of 2^e (the largest such e); None for an all-zero array."""
    b = np.ascontiguousarray(x, F32).view(np.uint32)[np.asarray(x) != 0]
    if b.size == 0:
        return None
    ex = ((b >> 23) & 0xFF).astype(np.int64)
    assert (ex > 0).all(), "denormal"
    mant = ((b & 0x7FFFFF) | 0x800000).astype(np.int64)
    tz = np.zeros_like(mant)
    for k in range(24):
        tz = np.where((mant & ((1 << (k + 1)) - 1)) == 0, k + 1, tz)
    return int((ex - 150 + tz).min())


def encode_planes(x, Bp, terms=3, negate=False):
    """[B, N] fp32 -> the operand planes tr[term][feature][Bp] as uint16 (bf16 bits), rows B..Bp zero: what prep / finish write."""
    B, N = x.shape
    out = np.zeros((terms, N, Bp), np.uint16)
    for t, part in enumerate(split3(-x if negate else x)[:terms]):
        out[t, :, :B] = (part.view(np.uint32) >> 16).astype(np.uint16).T
    return out.reshape(-1)


def decode_planes(buf, N, B, Bp, terms, negated=False):
    """The operand the update kernel read: planes tr[term][feature][Bp] (bf16 bits, any integer dtype or raw bytes), the terms summed
    in float64 -> [B, N].  `negated`: the producer stored the planes negated (hid_tr1)."""
    u = np.ascontiguousarray(buf).view(np.uint16)[: terms * N * Bp].reshape(terms, N, Bp)
    f = (u.astype(np.uint32) << 16).view(F32).astype(F64).sum(axis=0)
    assert np.isfinite(f).all() and not f[:, B:].any(), "the padding rows of an operand plane are not zero"
    return (-f if negated else f)[:, :B].T.copy()


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return np.random.Generator(np.random.PCG64(abs(hash(key)) % (1 << 63)))


def _values(kind, g, shape):
    if kind == "binary":
        return (g.random(shape, dtype=F32) > 0.5).astype(F32)
    if kind == "narrow":
        return (g.integers(0, 5, shape) / 4).astype(F32)
    if kind == "two-term":
        a = 512 + g.integers(0, 512, shape)
        a = np.where(a & 3, a, a | 1 + (a >> 2 & 1))            # low two bits not both zero
        return (a / 1024).astype(F32)
    if kind == "wide":      # 8 + 8 + 2 bits: the top bit of each term set, so the truncation split has three non-zero terms
        a = (1 << 17) | (g.integers(0, 128, shape) << 10) | (1 << 9) | (g.integers(0, 128, shape) << 2) | (g.integers(0, 2, shape) << 1) | 1
        return (a / (1 << 18)).astype(F32)
    assert kind == "real", kind
    return g.random(shape, dtype=F32)


def sparse_rows(B, j):
    """The batch rows in which column j of a row-sparse operand is non-zero."""
    return [(j + k * cdiv(B, SPARSE_ROWS)) % B for k in range(SPARSE_ROWS)]


@functools.lru_cache(maxsize=None)
def dense(kind, B, N, tag):
    x = _values(kind, _gen(1, B, N, sum(map(ord, tag + kind))), (B, N))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sparse(kind, B, N, tag):
    g = _gen(2, B, N, sum(map(ord, tag + kind)))
    x = np.zeros((B, N), F32)
    for j in range(N):
        rows = sparse_rows(B, j)
        x[rows, j] = 1.0 if kind == "binary" else _values(kind, g, len(rows))
    x.setflags(write=False)
    return x


def covers_every_row(B, N):
    return len({r for j in range(N) for r in sparse_rows(B, j)}) == B


def mixed_columns(V, tpb):
    """Every fifth column of the last tile of the first block's tile range."""
    last = min(tpb, cdiv(V, 128)) - 1
    return np.arange(128 * last, min(128 * (last + 1), V), 5)


@functools.lru_cache(maxsize=None)
def visible(kind, B, V, tpb, tag):
    """[B, V] `binary`, `real`, or `mixed` for blocks of `tpb` tiles."""
    g = _gen(3, B, V, tpb, sum(map(ord, tag + kind)))
    if kind == "real":
        x = g.random((B, V), dtype=F32)
    else:
        x = (g.random((B, V), dtype=F32) > 0.7).astype(F32)
        if kind == "mixed":
            cols = mixed_columns(V, tpb)
            x[:, cols] = g.random((B, len(cols)), dtype=F32)
        else:
            assert kind == "binary", kind
    x.setflags(write=False)
    return x


# ---- parameters and the float64 reference -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def params(V, H):
    """Group B / C start state: W ~ N(0, 1) / sqrt(V), biases ~ 0.1 N(0, 1), momenta ~ 0.01 N(0, 1)."""
    g = _gen(4, V, H)
    st = dict(W=g.standard_normal((V, H), dtype=F32) / F32(np.sqrt(V)), hid_bias=g.standard_normal(H, dtype=F32) * F32(0.1),
              vis_bias=g.standard_normal(V, dtype=F32) * F32(0.1), W_m=g.standard_normal((V, H), dtype=F32) * F32(0.01),
              hb_m=g.standard_normal(H, dtype=F32) * F32(0.01), vb_m=g.standard_normal(V, dtype=F32) * F32(0.01))
    for a in st.values():
        a.setflags(write=False)
    return st


def zero_params(V, H):
    return dict(W=np.zeros((V, H), F32), hid_bias=np.zeros(H, F32), vis_bias=np.zeros(V, F32), W_m=np.zeros((V, H), F32),
                hb_m=np.zeros(H, F32), vb_m=np.zeros(V, F32))


def stats64(phases):
    """The statistics of rbm.py:209-211 in float64 from a list of (vpos, hpos, vneg, hneg) row blocks (chunks / ranks are summed)."""
    s = None
    for vp, hp, vn, hn in phases:
        vp, hp, vn, hn = (np.asarray(a, F64) for a in (vp, hp, vn, hn))
        t = dict(dW=vp.T @ hp - vn.T @ hn, hpos=hp.sum(0), hneg=hn.sum(0), vpos=vp.sum(0), vneg=vn.sum(0))
        s = t if s is None else {k: s[k] + t[k] for k in s}
    return s


def ref_update(st, s, lr, mom, wd, n, sparsity=False, target=SPARSITY_TARGET):
    """rbm.py:212-224 in float64 from the statistics `s` (stats64) on the state `st` (fp32 arrays); the scalars are the fp32 numbers
    the engine receives.  Returns the new state as float64 arrays."""
    lr, mom, wd, target, n = (F64(F32(x)) for x in (lr, mom, wd, target, n))
    o = {k: np.asarray(v, F64) for k, v in st.items()}
    W_m = mom * o["W_m"] + lr * (s["dW"] / n - wd * o["W"])
    hb_m = mom * o["hb_m"] + lr * (s["hpos"] - s["hneg"]) / n
    if sparsity:
        hb_m = hb_m - lr * (s["hpos"] / n - target)
    vb_m = mom * o["vb_m"] + lr * (s["vpos"] - s["vneg"]) / n
    return dict(W=o["W"] + W_m, hid_bias=o["hid_bias"] + hb_m, vis_bias=o["vis_bias"] + vb_m, W_m=W_m, hb_m=hb_m, vb_m=vb_m)


# ---- the configurations: shape, tiles per block, options, forced pitch ------------------------------------------------------------------
def _cfg(V, H, tpb=None, opts=None, pitch=0, generic=False):
    name = f"{V}x{H}" + (f"-t{tpb}" if tpb else "") + ("-generic_k3" if opts else "") + (f"-p{pitch}" if pitch else "")
    o = dict(opts or {})
    if tpb:
        o["k3_tpb"] = tpb
    return dict(name=name, V=V, H=H, tpb=tpb or 1, opts=o, pitch=pitch, generic=generic or bool(opts))


CONFIGS = ([_cfg(300, 132, t) for t in (None, 2, 3)] + [_cfg(700, 132, t) for t in (None, 2, 3, 5)] +
           [_cfg(128, 128), _cfg(130, 36), _cfg(1024, 132), _cfg(256, 512), _cfg(1024, 128), _cfg(128, 1024),
            _cfg(300, 45, generic=True), _cfg(300, 132, opts={"generic_k3": 1})])
PITCHED = _cfg(1100, 260, pitch=288)
PITCHED_GENERIC = _cfg(1100, 260, opts={"generic_k3": 1}, pitch=288)


def _expect(cfg, kernel=UPDATE_PLANES):
    return (UPDATE_GENERIC, 0) if cfg["generic"] else (kernel, cfg["tpb"])


def _base(cfg, **kw):
    c = dict(V=cfg["V"], H=cfg["H"], tpb=cfg["tpb"], opts=dict(cfg["opts"]), pitch=cfg["pitch"], generic=cfg["generic"], mode="exact")
    c.update(kw)
    c["xa"] = None if c["expect"][0] == UPDATE_GENERIC else xa_of(c["V"], c["H"], c["tpb"])
    return c


# ---- group A ----------------------------------------------------------------------------------------------------------------------
COMBOS = {     # name: (visible form, visible kind, hidden form, hidden kind)
    "wideV-narrowH": ("sparse", "wide", "dense", "narrow"),
    "binaryV-wideH": ("dense", "binary", "sparse", "wide"),
    "two-two": ("sparse", "two-term", "dense", "two-term"),
}
PHASES = ("pos", "neg", "both")
A_BATCHES = (64, 128, 256)


def _plain(combo):
    """The phase that does not carry the combination: `binary` where the combination is row-sparse, `narrow` / `binary` where dense."""
    vf, _, hf, _ = COMBOS[combo]
    return (vf, "binary", hf, "binary" if hf == "sparse" else "narrow")


def _a_case(cfg, combo, phase, B, tag=""):
    if COMBOS[combo][2] == "sparse" and not covers_every_row(B, cfg["H"]):      # 36 hidden columns x 6 rows < 256
        B = 128
    pos = COMBOS[combo] if phase in ("pos", "both") else _plain(combo)
    neg = COMBOS[combo] if phase in ("neg", "both") else _plain(combo)
    return _base(cfg, id=f"A-{cfg['name']}-{combo}-{phase}-B{B}{tag}", group="A", entry="assoc_update", B=B, expect=_expect(cfg),
                 kinds=dict(vpos=pos[:2], hpos=pos[2:], vneg=neg[:2], hneg=neg[2:]))


def _fast_case(cfg, B, old, group="A"):
    opts = dict(cfg["opts"], **({"no_update_bin": 1} if old else {}))
    kernel = UPDATE_BIN if (B == 64 and not old) else UPDATE_PLANES
    kinds = dict(vpos=("dense", "binary"), hpos=("dense", "narrow"), vneg=("dense", "narrow"), hneg=("dense", "narrow"))
    return _base(cfg, id=f"A-fast-{cfg['name']}-B{B}{'-no_update_bin' if old else ''}", group="A", entry="assoc_update", B=B, mode="fast",
                 opts=opts, expect=(kernel, cfg["tpb"]), kinds=kinds)


def group_a():
    out = []
    for cfg in CONFIGS:
        for i, (combo, phase) in enumerate(itertools.product(COMBOS, PHASES)):
            out.append(_a_case(cfg, combo, phase, A_BATCHES[(i + i // 3) % 3]))      # every combination and every phase with every batch
    for cfg in (CONFIGS[2], CONFIGS[6]):      # planes 4 and 5 all non-zero (P = 6, `wide` on both phases) also with one and two launches
        out += [_a_case(cfg, "wideV-narrowH", "both", B) for B in (64, 128)]
    out.append(_a_case(PITCHED, "two-two", "both", 128))
    out.append(_a_case(PITCHED_GENERIC, "wideV-narrowH", "both", 128))
    for cfg in (CONFIGS[0], CONFIGS[2], CONFIGS[5], PITCHED):
        out += [_fast_case(cfg, 64, False), _fast_case(cfg, 64, True), _fast_case(cfg, 128, False)]
    return out


def operands(c):
    """(vpos, hpos, vneg, hneg) fp32 of a group A or B case."""
    B, V, H = c["B"], c["V"], c["H"]
    out = []
    for name, N in (("vpos", V), ("hpos", H), ("vneg", V), ("hneg", H)):
        form, kind = c["kinds"][name]
        if form == "visible":
            out.append(visible(kind, B, V, c["tpb"], name))
        else:
            out.append({"dense": dense, "sparse": sparse}[form](kind, B, N, name))
    return out


def chunks(ops, B):
    """The operands cut into the 64-row chunks the host launches one by one."""
    return [tuple(a[b0:b0 + 64] for a in ops) for b0 in range(0, B, 64)]


def exactness(c):
    """(q exponent, largest sum over both phases and all chunks of |term products| of one output element, in units of q) on the
    truncation split of the case's inputs."""
    vp, hp, vn, hn = operands(c)
    tv = [split3(vp), split3(vn)]
    th = [split3(hp), split3(hn)]
    qv = min(e for e in (quantum_exp(t) for ph in tv for t in ph) if e is not None)
    qh = min(e for e in (quantum_exp(t) for ph in th for t in ph) if e is not None)
    total = np.zeros((c["V"], c["H"]), F64)
    for ph in range(2):
        av = sum(np.abs(t.astype(F64)) for t in tv[ph])
        ah = sum(np.abs(t.astype(F64)) for t in th[ph])
        total += av.T @ ah           # = sum over all (visible term, hidden term) pairs of |products|
    return qv + qh, float(total.max()) / 2.0 ** (qv + qh)


def ref_a(c):
    return ref_update(zero_params(c["V"], c["H"]), stats64([operands(c)]), 1.0, 0.0, 0.0, c["B"])


# ---- group B ----------------------------------------------------------------------------------------------------------------------
B_BATCHES = (40, 64, 130, 256)
B_LR, B_MOM, B_WD = 0.07, 0.6, 1e-3


def group_b():
    out = []
    for ci, cfg in enumerate(CONFIGS + [PITCHED, PITCHED_GENERIC]):
        for k, B in enumerate(B_BATCHES):
            kind = ("real", "mixed")[(k + ci) % 2]
            sp = bool((k + ci // 2) % 2)
            kinds = dict(vpos=("visible", kind), hpos=("dense", "real"), vneg=("visible", kind), hneg=("dense", "real"))
            out.append(_base(cfg, id=f"B-{cfg['name']}-B{B}-{kind}{'-sparsity' if sp else ''}", group="B", entry="assoc_update", B=B,
                             expect=_expect(cfg), kinds=kinds, sparsity=sp))
    return out


def ref_b(c):
    return ref_update(params(c["V"], c["H"]), stats64([operands(c)]), B_LR, B_MOM, B_WD, c["B"], c["sparsity"])


# ---- group C ----------------------------------------------------------------------------------------------------------------------
C_WD = 1e-3
RANK_ROUTES = [   # name, tiles per block, options, ranks (None: R from the case), kernel
    ("acc", None, {}, None, UPDATE_RANKS),                              # assoc_update_planes_ranks<HT, true>
    ("acc", 3, {}, None, UPDATE_RANKS),
    ("tilewise", 3, {"no_rank_acc": 1}, None, UPDATE_RANKS),            # assoc_update_planes_ranks<HT, false> by option
    ("tilewise", 5, {}, None, UPDATE_RANKS),                            # ... and by tiles per block > 4 (700 x 132 only)
    ("no_rank_loop", 3, {"no_rank_loop": 1}, None, UPDATE_PLANES),      # one launch per rank: PASS 1, (2,) 3
    ("min_rank_loop3", 3, {"min_rank_loop": 3}, 2, UPDATE_PLANES),      # two ranks below the threshold: PASS 1, 3
    ("one_rank", 3, {}, 1, UPDATE_PLANES),                              # the plain kernel, PASS 0
    ("min_rank_loop1", 3, {"min_rank_loop": 1}, 1, UPDATE_RANKS),       # the rank kernel on a single block
]
RANK_VARIANTS = [(2, 64, "binary", "exact"), (3, 40, "mixed", "exact"), (2, 64, "mixed", "fast"), (3, 40, "binary", "fast")]


def group_c():
    out = []
    for B, tpb, kind in itertools.product((64, 130), (None, 3), ("binary", "mixed")):
        cfg = _cfg(300, 132, tpb)
        out.append(_base(cfg, id=f"C-stats-{cfg['name']}-B{B}-{kind}", group="C", entry="cd_stats", B=B, data=kind, expect=_expect(cfg)))
    cfg = _cfg(300, 132, 3)
    out.append(_base(cfg, id="C-stats-fast-300x132-t3-B130-binary", group="C", entry="cd_stats", B=130, data="binary", mode="fast",
                     expect=_expect(cfg)))
    for V, (name, tpb, opts, ranks, kernel) in itertools.product((300, 700), RANK_ROUTES):
        if tpb == 5 and V != 700:
            continue
        cfg = _cfg(V, 132, tpb)
        for R, Bl, kind, mode in RANK_VARIANTS:
            R = ranks or R
            out.append(_base(cfg, id=f"C-ranks-{cfg['name']}-{name}-R{R}x{Bl}-{kind}-{mode}", group="C", entry="apply_factors", R=R, Bl=Bl,
                             B=R * Bl, data=kind, mode=mode, opts=dict(cfg["opts"], **opts), expect=(kernel, cfg["tpb"]),
                             mixed_rank=min(1, R - 1)))
    cfg = _cfg(1100, 260, pitch=288)
    out.append(_base(cfg, id="C-ranks-1100x260-p288-acc-R2x64-binary-exact", group="C", entry="apply_factors", R=2, Bl=64, B=128,
                     data="binary", expect=(UPDATE_RANKS, 1), mixed_rank=1))
    cfg = _cfg(300, 132, 3)
    for kind, old in itertools.product(("binary", "mixed"), (False, True)):
        out.append(_base(cfg, id=f"C-cd1-300x132-t3-{'planes' if old else 'bin'}-{kind}", group="C", entry="train_epoch", B=64, data=kind,
                         opts=dict(cfg["opts"], **({"no_update_bin": 1} if old else {})),
                         expect=(UPDATE_PLANES if old else UPDATE_BIN, 3)))
    return out


def cd_data(c, rank=None):
    """The batch of a group C case (of one rank: Bl rows; `mixed` only in the rank c["mixed_rank"])."""
    if rank is None:
        return visible(c["data"], c["B"], c["V"], c["tpb"], "data")
    kind = c["data"] if (c["data"] != "mixed" or rank == c["mixed_rank"]) else "binary"
    return visible(kind, c["Bl"], c["V"], c["tpb"], f"rank{rank}")


# ---- the table --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _all():
    cs = group_a() + group_b() + group_c()
    assert len({c["id"] for c in cs}) == len(cs), "duplicate case id"
    return tuple(cs)


def cases(group=None, entry=None):
    return [c for c in _all() if (group is None or c["group"] == group) and (entry is None or c["entry"] == entry)]


if __name__ == "__main__":
    for c in _all():
        print(c["id"], c["expect"], "xa", c["xa"], c["opts"])
