"""Cases shared by test_chain_kernel_cpu.py and test_chain_kernel_gpu.py: the row-parallel chain kernel (k4_chain / k4_split_planes,
csrc/kernels_chain.hpp) and its host routing (chain_kernel_ok / launch_k4 / run_chain / run_chain_pair, csrc/engine.hip) on every
path, each case naming the record it must leave in imdbn_debug_last_chain (route, rows per block, blocks, records of chain 0),
against a float64 reference of every half step.

All chains run through HipEngine.chain_traced_vh with the full windows trace = (0, V, baseline) and trace_h = (0, H), so every half
step is observable.  The reference goes step by step (`walk`, an extension of bimodal_logging_oracle.check_recorded_chain): the
float64 value of a half step is computed from the state the device recorded entering it, the next state is rebuilt in fp32 from the
recorded probabilities and the same draws, and the rebuilt final state must equal the returned one bit for bit.  Draws come from a
tape (DrawStream; categorical indices given) or from oracle.draws.PhiloxStream (with the case's row0); under Philox the categorical
index of a softmax group is rebuilt with PhiloxStream.categorical from the recorded fp32 probabilities of the group (they are
recorded after the mu-pull), mixed with the clamp for vmode 2 and clipped to [1e-8, 1] in fp32: the kernel's numbers in the kernel's
order, so no decision can differ.

Decoded terms.  The kernel multiplies encodings of its operands (k4_terms): PARITY hi = fp16(x), lo = fp16(x - fp32(hi)), the lo
term of a sampled 0/1 hidden state dropped; FAST one bf16, round to nearest even.  `terms` restates that in numpy and the float64
reference multiplies the decoded weights by the decoded entering activations, so what separates the device from it is fp32
accumulation and the fp32 epilogue only.  Chains that run one launch per half step read fp32 operands as three exact bf16 terms
(split3): their reference multiplies the undecoded numbers.

Bounds (`half_step`, `prob_bound`, `group_bound`), derived, never fitted.  With u = 2^-24:
  logit    an accumulator of k4_gemm adds K * NA products (NA activation terms; fp16 x fp16 products are exact in fp32) and the NW
           accumulators are added after: at most n = K * NA + NW additions, each rounding a partial sum whose magnitude is at most
           S = sum |a_k w_k| over all term products:  |dx| <= n u S   (at most 9 K additions of split3 products per launch)
  epilogue + bias, x / T, z * sigma and the sum round once each: 5 u max(|x|, 1) covers them; z differs from the numpy Box-Muller twin by
           logf / cosf / sqrtf of at most 1 / 2 / 0.5 ulp on the device and 1 ulp each in numpy on |z| <= r <= sqrt(-2 ln 2^-24) =
           5.77:  |dz| <= 8 u r  (NORMAL_ERR), times sigma
  sigmoid  slope <= 1/4; expf (1 ulp), 1 + e and the division:  4 u  (SIGMOID_ERR)
  softmax  logits off by at most D (the largest bound in the group, plus u |x - max| of the subtraction) move p_j by at most
           p_j (1 - p_j) (exp(2 D) - 1)  [p~_j - p_j = p_j (1 - p_j) (e^dj - m) / Z, m a mean of the other e^di, Z >= e^-D]; expf, the ordered sum of g terms and the division add p_j (g + 4) u
  mu-pull  (1 - eta) p + eta mu: |1 - eta| times the bound of p, plus 3 u
Weights are drawn small enough for that bound to stay inside the project's chain tolerance (TOL = 1e-5 on probabilities, the TOL of
test_bimodal_logging_gpu.py): test_chain_kernel_cpu.py asserts bound + |decoded reference - plain float64 reference| <= TOL for
every PARITY case.

Shapes, batches and schedules are the smallest that reach an edge; the groups of the table are the items of the list in `GROUPS`.
A batch written ("cu", m, a) is m * CU count + a rows, resolved with the count the device reports."""
import functools
import zlib

import numpy as np

from oracle.draws import DrawStream, PhiloxStream

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TOL = 1e-5                                    # test_bimodal_logging_gpu.py TOL: the project's chain tolerance on probabilities
NORMAL_ERR = 8 * U * 5.77
SIGMOID_ERR = 4 * U
CHAIN_PER_LAUNCH, CHAIN_KERNEL, CHAIN_KERNEL_PAIR = 0, 1, 2      # include/imdbn_engine.h IMDBN_CHAIN_*
OPTION_DEFAULTS = {"chain_rows": 0, "no_chain_kernel": 0, "no_chain_pair": 0}
GROUPS = ("rows", "auto", "fast", "geometry", "gemm", "lds", "steps", "pitch", "wide")
NOMINAL_CU = 256                               # what the CPU tests resolve ("cu", m, a) batches with

# ---- what the host derives from a call (csrc/engine.hip chain_kernel_ok, run_chain_pair, launch_k4) ---------------------------------
K4_ROWS, K4_LDS_BYTES, CHAIN_MAX_STEPS, GROUP_WMAX, PLANES_MAX = 16, 152 * 1024, 256, 256, 1024


def rup(x, m):
    return (x + m - 1) // m * m


def cdiv(a, b):
    return -(-a // b)


def lds_bytes(V, H, gw, mode):
    """The byte count of chain_kernel_ok: activation terms, fp32 stage, group logits + row stats, group noise drawn ahead."""
    nt = 2 if mode == "parity" else 1
    return (nt * K4_ROWS * ((rup(V, 32) + 8) + (rup(H, 32) + 8)) * 2 + K4_ROWS * (rup(max(V, H), 16) + 1) * 4
            + K4_ROWS * (gw + 1) * 4 + K4_ROWS * 16 + (K4_ROWS // 2) * gw * 2 * 4)


def kernel_ok(V, H, groups, mode, n_recs, opts=None):
    opts = opts or {}
    if opts.get("no_chain_kernel") or V > PLANES_MAX or H > PLANES_MAX or n_recs < 2 or n_recs > CHAIN_MAX_STEPS:
        return False
    if len(groups) > 1:
        return False
    gw = groups[0][1] - groups[0][0] if groups else 0
    return gw <= GROUP_WMAX and lds_bytes(V, H, gw, mode) <= K4_LDS_BYTES


def rows_rule(B, chains, cu, forced=0):
    bt = B * chains
    return forced if forced > 0 else (2 if bt <= 2 * cu else (4 if bt <= 4 * cu else (8 if bt <= 8 * cu else 16)))


def n_recs(ch):
    return ch["n"] + (1 if ch["base"] else 0)


def batch(c, cu=NOMINAL_CU):
    B = c["B"]
    return B[1] * cu + B[2] if isinstance(B, tuple) else B


def expected(c, cu=NOMINAL_CU):
    """(route, rows per block, blocks, records of chain 0) the call must leave in imdbn_debug_last_chain."""
    B, chs, o = batch(c, cu), c["chains"], c["opts"]
    ok = [kernel_ok(c["V"], c["H"], c["groups"], c["mode"], n_recs(ch), o) for ch in chs]
    if len(chs) == 2 and all(ok) and n_recs(chs[0]) + n_recs(chs[1]) <= CHAIN_MAX_STEPS and not o.get("no_chain_pair"):
        rows = rows_rule(B, 2, cu, o.get("chain_rows", 0))
        return (CHAIN_KERNEL_PAIR, rows, 2 * cdiv(B, rows), n_recs(chs[0]))
    if not ok[-1]:                              # the record describes the last chain run
        return (CHAIN_PER_LAUNCH, 0, 0, n_recs(chs[0]))
    rows = rows_rule(B, 1, cu, o.get("chain_rows", 0))
    return (CHAIN_KERNEL, rows, cdiv(B, rows), n_recs(chs[0]))


def on_kernel(c, i, cu=NOMINAL_CU):
    """Whether chain i of the case runs on the chain kernel (its reference then multiplies decoded terms)."""
    return kernel_ok(c["V"], c["H"], c["groups"], c["mode"], n_recs(c["chains"][i]), c["opts"])


# ---- k4_terms in numpy ------------------------------------------------------------------------------------------------------------
def terms(x, enc, exact1=False):
    """The terms the kernel multiplies for the fp32 array x, as fp32 arrays whose float64 sum is the decoded value.  enc "parity":
    hi = fp16(x), lo = fp16(x - fp32(hi)) (`exact1`: x is a sampled 0/1 state, lo is dropped); "fast": bf16_rne(x); "none": x."""
    x = np.ascontiguousarray(x, F32)
    if enc == "none":
        return [x]
    if enc == "fast":
        u = x.view(np.uint32).astype(np.uint64)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
        return [(r & 0xFFFFFFFF).astype(np.uint32).view(F32)]
    assert enc == "parity", enc
    hi = x.astype(np.float16)
    lo = (x - hi.astype(F32)).astype(np.float16)
    return [hi.astype(F32)] if exact1 else [hi.astype(F32), lo.astype(F32)]


def term_error(x, enc):
    """|x - decoded| and its stated bound: PARITY 2^-22 |x| (two 11-bit significands), or 2^-25 where lo is an fp16 subnormal
    (quantum 2^-24); FAST 2^-8 |x| (half an ulp of an 8-bit significand)."""
    d = np.abs(np.asarray(x, F64) - sum(t.astype(F64) for t in terms(x, enc)))
    return d, (np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -25) if enc == "parity" else 2.0 ** -8 * np.abs(np.asarray(x, F64)))


def _sum64(ts):
    return sum(t.astype(F64) for t in ts)


def _abs64(ts):
    return sum(np.abs(t.astype(F64)) for t in ts)


# ---- one half step: float64 value and bound -----------------------------------------------------------------------------------------
def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def half_step(a_terms, w_terms, bias, T, sigma, z, down, enc):
    """(float64 logits after temperature and noise, their bound) of act @ W (`down`: act @ W^T) + bias from operand terms."""
    A, W = _sum64(a_terms), _sum64(w_terms)
    Aa, Wa = _abs64(a_terms), _abs64(w_terms)
    K = A.shape[1]
    x = A @ (W.T if down else W) + bias
    S = Aa @ (Wa.T if down else Wa)
    n = 9 * K if enc == "none" else K * len(a_terms) + len(w_terms)
    Tm = max(1e-6, T)
    x, d = x / Tm, n * U * S / Tm
    if sigma > 0:
        x = x + z.astype(F64) * sigma
        d = d + sigma * NORMAL_ERR
    return x, d + 5 * U * np.maximum(np.abs(x), 1.0)


def prob_bound(d):
    return d / 4 + SIGMOID_ERR


def group_bound(x, d, p):
    g = x.shape[1]
    D = d.max(1, keepdims=True) + U * np.abs(x - x.max(1, keepdims=True)).max(1, keepdims=True)
    return p * (1 - p) * np.expm1(2 * D) + p * (g + 4) * U


def softmax(x):
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


# ---- draws --------------------------------------------------------------------------------------------------------------------------
class Tape:
    """Uniforms and normals of a DrawStream, categorical indices of a seeded generator (a replayed index is simply a given)."""

    def __init__(self, seed):
        self.s, self.g = DrawStream(seed), np.random.Generator(np.random.PCG64(seed + 1))

    def uniform(self, shape): return self.s.uniform(shape)
    def normal(self, shape): return self.s.normal(shape)
    def categorical(self, p): return self.g.integers(0, p.shape[1], p.shape[0])


def source(c):
    return PhiloxStream(c["seed"], row0=c["row0"]) if c["rng"] == "philox" else Tape(c["seed"])


def _step_draws(src, st, B, V, H, groups, philox):
    """The draws of one step in the engine's order (imdbn.engine.rng.sched_chain).  A Philox categorical is a stream positioned at the
    draw, to be evaluated once the probabilities are known."""
    d = {}
    if st["sigma"] > 0:
        d["nh"] = np.asarray(src.normal((B, H)), F32)
    if st["sample_h"]:
        d["uh"] = np.asarray(src.uniform((B, H)), F32)
    if st["sigma"] > 0:
        d["nv"] = np.asarray(src.normal((B, V)), F32)
    if st["vmode"] != 0:
        d["uv"] = np.asarray(src.uniform((B, V)), F32)
        d["cat"] = []
        for s, e in groups:
            if philox:
                d["cat"].append(PhiloxStream(src.seed, offset=src.offset, row0=src.row0))
                src.offset += 1
            else:
                d["cat"].append(np.asarray(src.categorical(np.zeros((B, e - s), F32)), np.int64))
    return d


# ---- the step-by-step walk ------------------------------------------------------------------------------------------------------------
def walk(c, prob, i, src, enc, rec=None):
    """Chain i of case c on the problem `prob`, step by step.  `rec` = (vis [T (+1), B, V], hid [T, B, H], final [B, V]) fp32 as the
    device recorded them; None: the fp32 rounding of the reference stands in for the record (the CPU tests).  `enc`: how the chain's
    operands are encoded ("parity" / "fast" on the chain kernel, "none" one launch per half step).  Returns a dict: `ratio_h` /
    `ratio_v` the largest |recorded - float64| / bound, `err` the largest |recorded - float64|, `bound` the largest bound, `plain`
    the largest bound + |decoded reference - float64 of the undecoded operands|, `final_equal`, `rebuilt` the fp32 final state,
    `vis` / `hid` the references rounded to fp32."""
    ch = c["chains"][i]
    W, hb, vb = prob["W"], prob["hb"].astype(F64), prob["vb"].astype(F64)
    vk, km, mu = prob["vk"], prob["mask"][i], prob["mu"]
    B, V = vk.shape
    H = W.shape[1]
    groups, philox = c["groups"], c["rng"] == "philox"
    wt = terms(W, enc)
    free = np.ones(V, bool)
    for s, e in groups:
        free[s:e] = False
    one = F32(1)
    mix = lambda x: x * (one - km) + vk * km      # noqa: E731  (fp32, in the kernel's order)
    v = (vk * km + (one - km) * np.asarray(src.uniform((B, V)), F32)) if ch["init_uniform"] else vk.copy()
    out = dict(ratio_h=0.0, ratio_v=0.0, err=0.0, bound=0.0, plain=0.0)
    vis_ref, hid_ref = [], []

    def note(which, got, ref, bound, ref_plain):
        e = np.abs(got.astype(F64) - ref)
        out["ratio_" + which] = max(out["ratio_" + which], float((e / bound).max()))
        out["err"], out["bound"] = max(out["err"], float(e.max())), max(out["bound"], float(bound.max()))
        out["plain"] = max(out["plain"], float((bound + np.abs(ref - ref_plain)).max()))

    def v_prob(a_terms, w_terms, e_, st, d, extra=None):
        x, dx = half_step(a_terms, w_terms, vb, st["T"], st["sigma"], d.get("nv"), True, e_)
        if extra is not None:
            dx = dx + extra
        p, b = sigmoid(x), prob_bound(dx)
        for s, e in groups:
            p[:, s:e] = softmax(x[:, s:e])
            b[:, s:e] = group_bound(x[:, s:e], dx[:, s:e], p[:, s:e])
        if mu is not None and st["eta"] != 0.0:
            Dz, eta = mu.shape[1], F32(st["eta"])
            keep = F64(one - eta)
            p[:, :Dz] = keep * p[:, :Dz] + F64(eta) * mu.astype(F64)
            b[:, :Dz] = abs(keep) * b[:, :Dz] + 3 * U
        return p, b

    def h_prob(a_terms, w_terms, e_, st, d):
        x, dx = half_step(a_terms, w_terms, hb, st["T"], st["sigma"], d.get("nh"), False, e_)
        return sigmoid(x), prob_bound(dx)

    plain_w = [W]
    steps = ch["steps"]
    b0 = 1 if ch["base"] else 0
    if ch["base"]:      # observe-only record: p(v | p(h | v0)) at T = 1, no draws; its hidden probabilities are not recorded
        assert enc != "fast", "a bf16 neighbour of p(h) is 2^-8 away: the table has no FAST baseline"
        st0 = dict(T=1.0, sigma=0.0, eta=0.0)
        ph, bh = h_prob(terms(v, enc), wt, enc, st0, {})
        php, _ = h_prob([v], plain_w, "none", st0, {})
        # the device's fp32 p(h) is within bh of ph: the visible logits move by at most |W| bh (and by the encoding of a neighbour)
        extra = (bh + 2.0 ** -21) @ _abs64(wt).T
        pv, bv = v_prob(terms(ph.astype(F32), enc), wt, enc, st0, {}, extra)
        pvp, _ = v_prob([php.astype(F32)], plain_w, "none", st0, {})
        got = rec[0][0] if rec else pv.astype(F32)
        note("v", got, pv, bv, pvp)
        vis_ref.append(pv.astype(F32))
    for t, st in enumerate(steps):
        d = _step_draws(src, st, B, V, H, groups, philox)
        ph, bh = h_prob(terms(v, enc), wt, enc, st, d)
        php, _ = h_prob([v], plain_w, "none", st, d)
        hid_t = rec[1][t] if rec else ph.astype(F32)
        note("h", hid_t, ph, bh, php)
        hid_ref.append(ph.astype(F32))
        h = (hid_t > d["uh"]).astype(F32) if st["sample_h"] else hid_t
        pv, bv = v_prob(terms(h, enc, exact1=bool(st["sample_h"])), wt, enc, st, d)
        pvp, _ = v_prob([h], plain_w, "none", st, d)
        vis_t = rec[0][t + b0] if rec else pv.astype(F32)
        note("v", vis_t, pv, bv, pvp)
        vis_ref.append(pv.astype(F32))
        # the next state in fp32, from the recorded probabilities and the same draws
        p32 = np.asarray(vis_t, F32)
        if st["vmode"] == 0:
            v = mix(p32) if st["clamp"] else p32.copy()
        else:
            srcp = mix(p32) if (st["vmode"] == 2 and st["clamp"]) else p32
            s = (srcp > d["uv"]).astype(F32)
            for (a, b), cat in zip(groups, d["cat"]):
                idx = cat.categorical(np.minimum(np.maximum(srcp[:, a:b], F32(1e-8)), one)) if philox else cat
                s[:, a:b] = np.eye(b - a, dtype=F32)[idx]
            v = mix(s) if (st["vmode"] == 1 and st["clamp"]) else s
        v = np.asarray(v, F32)
    out["rebuilt"] = v
    out["final_equal"] = bool(np.array_equal(v, np.asarray(rec[2], F32))) if rec else True
    out["vis"], out["hid"] = vis_ref, hid_ref
    return out


# ---- problems ---------------------------------------------------------------------------------------------------------------------------
def weight_scale(V, H, enc="parity"):
    """Standard deviation of the weights: at most 0.4 (the small shapes of test_bimodal_logging_gpu.py), and small enough that the
    accumulation bound n u S / (4 T) of a mean-field half step -- n = 2 K additions on the kernel, 9 K per launch, S ~ 0.4 K s
    (activations ~ 0.5, E|w| = 0.8 s), T >= 0.7 -- stays near 2e-6 (twice that through a softmax), inside TOL with room for the epilogue terms."""
    K = max(V, H)
    n = 9 if enc == "none" else 2
    return min(0.4, 2e-6 * 4 * 0.7 / (n * K * U * 0.4 * K))


@functools.lru_cache(maxsize=None)
def _problem(key, V, H, B, Dz, scale):
    g = np.random.Generator(np.random.PCG64(zlib.crc32(key.encode())))
    p = dict(W=(g.standard_normal((V, H)) * scale).astype(F32), hb=(g.standard_normal(H) * 0.5).astype(F32),
             vb=(g.standard_normal(V) * 0.5).astype(F32), vk=g.random((B, V), dtype=F32),
             mask=[(g.random((B, V)) < 0.5).astype(F32), (g.random((B, V)) < 0.5).astype(F32)],
             mu=g.random((B, Dz), dtype=F32) if Dz else None)
    for a in [p["W"], p["hb"], p["vb"], p["vk"], *p["mask"]] + ([p["mu"]] if Dz else []):
        a.setflags(write=False)
    return p


def problem(c, cu=NOMINAL_CU):
    """W ~ N(0, s^2) (weight_scale), biases ~ N(0, 1/4), v_known uniform in [0, 1), element-wise 0/1 masks (one per chain of a pair:
    every column, softmax-group columns included, is clamped in some rows and free in others), mu uniform [B, Dz]."""
    enc = "parity" if all(on_kernel(c, i) for i in range(len(c["chains"]))) else "none"
    return _problem(c["id"], c["V"], c["H"], batch(c, cu), c["Dz"] or 0, weight_scale(c["V"], c["H"], enc))


# ---- schedules --------------------------------------------------------------------------------------------------------------------------
def _st(T=1.0, sigma=0.0, eta=0.0, sample_h=False, vmode=0, clamp=True):
    return dict(T=float(F32(T)), sigma=float(F32(sigma)), eta=float(F32(eta)), sample_h=bool(sample_h), vmode=int(vmode), clamp=bool(clamp))


TEMPS = (1.0, 0.7, 1.3)


def schedule(kind, n, eta=0.0):
    """`meanfield` (two activation terms both ways), `sampled` (sampled h: the one-term GEMM; sampled v re-clamped), `noisy` (T, noise,
    alternating h sampling, vmode 0 / 1), `vmode2`, and `mix`: every combination a few steps reach -- h sampled on odd steps, vmode
    step % 3, clamp on the first three steps of every six, noise on steps with step % 3 != 1, temperatures 1 / 0.7 / 1.3, the mu-pull throughout."""
    if kind == "meanfield":
        return [_st(eta=eta) for _ in range(n)]
    if kind == "sampled":
        return [_st(sample_h=True, vmode=1, eta=eta) for _ in range(n)]
    if kind == "vmode2":
        return [_st(T=0.7, vmode=2, clamp=(i % 2 == 0), sample_h=(i % 2 == 1), eta=eta) for i in range(n)]
    if kind == "noisy":
        return [_st(T=0.7, sigma=0.3, sample_h=(i % 2 == 0), vmode=(1 if i % 3 == 0 else 0), eta=eta) for i in range(n)]
    assert kind == "mix", kind
    return [_st(T=TEMPS[i % 3], sigma=(0.3 if i % 3 != 1 else 0.0), eta=eta, sample_h=(i % 2 == 1), vmode=i % 3, clamp=(i // 3 % 2 == 0))
            for i in range(n)]


KINDS = ("meanfield", "sampled", "vmode2", "noisy", "mix")


def _chain(kind, n, base=False, init_uniform=True, eta=0.0):
    return dict(kind=kind, n=n, base=bool(base), init_uniform=bool(init_uniform), steps=schedule(kind, n, eta))


def _case(group, name, V, H, B, chains, groups=(), mode="parity", rng="philox", row0=0, seed=11, Dz=None, opts=None, pitch=0,
          strided=False, **tags):
    eta = 0.3 if Dz else 0.0
    chs = [_chain(eta=eta, **ch) if isinstance(ch, dict) else _chain(ch[0], ch[1], eta=eta) for ch in chains]
    c = dict(id=f"{group}-{name}", group=group, V=V, H=H, B=B, chains=chs, groups=[tuple(g) for g in groups], mode=mode, rng=rng,
             row0=row0, seed=seed, Dz=Dz, opts=dict(opts or {}), pitch=pitch, strided=strided)
    c.update(tags)
    return c


ROWS = (1, 2, 3, 4, 5, 8, 15, 16)
SMALL, JOINT = (36, 24, ()), (150, 48, ((140, 150),))


def _rows_batch(rows):
    """Partial last block; at least three blocks and an odd-start block for odd rows; one row at rows 2."""
    return 1 if rows == 2 else (2 * rows + max(1, rows // 2) if rows % 2 else rows + max(1, rows // 2))


def group_rows():
    out = []
    for (V, H, groups), rows in ((s, r) for s in (SMALL, JOINT) for r in ROWS):
        B = _rows_batch(rows)
        tag = f"{V}x{H}-r{rows}"
        out.append(_case("rows", f"{tag}-B{B}-mix", V, H, B, [("mix", 6)], groups, opts={"chain_rows": rows}, rows=rows))
        out.append(_case("rows", f"{tag}-B{B}-pair-noisy-sampled", V, H, B, [("noisy", 4), ("sampled", 3)], groups, opts={"chain_rows": rows},
                         rows=rows, seed=12))
    for rows in (3, 4):
        V, H, groups = JOINT
        out.append(_case("rows", f"{V}x{H}-r{rows}-B11-row0_3-mix", V, H, 11, [("mix", 6)], groups, row0=3, opts={"chain_rows": rows},
                         rows=rows, seed=13))
    return out


def group_auto():
    V, H, _ = SMALL
    out = [_case("auto", f"single-{m}c+{a}", V, H, ("cu", m, a), [("mix", 2)], seed=14 + m + a) for m in (2, 4, 8) for a in (0, 1)]
    out += [_case("auto", f"pair-c+{a}", V, H, ("cu", 1, a), [("mix", 2), ("sampled", 2)], seed=17 + a) for a in (0, 1)]
    return out


PRODUCTION = (532, 256, ((500, 532),))


def group_fast():
    out = []
    for (V, H, groups), kind, rows, pair in ((s, k, r, p) for s in (SMALL, JOINT, PRODUCTION) for k in KINDS for r in (2, 16) for p in (0, 1)):
        if (V, H) == PRODUCTION[:2] and (rows == 16) != (pair == 1) and kind not in ("mix", "meanfield"):
            continue                            # the production shape: every kind at rows 2 single and rows 16 pair; mix and mean-field on all four
        B = 5 if rows == 2 else 19
        chains = [(kind, 4), (KINDS[(KINDS.index(kind) + 1) % len(KINDS)], 3)] if pair else [(kind, 4)]
        out.append(_case("fast", f"{V}x{H}-{kind}-r{rows}-{'pair' if pair else 'single'}", V, H, B, chains, groups, mode="fast",
                         opts={"chain_rows": rows}, rows=rows, seed=21, Dz=(V - 20 if kind == "mix" else None)))
    return out


def group_geometry():
    out = []
    V, H = 150, 48
    for w in (1, 3, 8, 13, 16, 32):
        for where, s in (("end", V - w), ("start", 0), ("middle", 64 - w // 2)):
            for rows, rng in ((2, "philox"), (3, "philox"), (2, "tape")):
                if rng == "tape" and where != "end" and w not in (13, 32):
                    continue
                # the mu-pull ends before the group, inside it, or at V
                Dz = {"end": s + (w + 1) // 2, "start": V, "middle": s - 7}[where] if w > 1 else {"end": V, "start": 1, "middle": s}[where]
                out.append(_case("geometry", f"{V}x{H}-w{w}-{where}-r{rows}-{rng}", V, H, 7, [("mix", 6)], [(s, s + w)], rng=rng,
                                 opts={"chain_rows": rows}, rows=rows, Dz=Dz, seed=31 + w, width=w, where=where))
    for rng in ("philox", "tape"):
        out.append(_case("geometry", f"300x48-w256-middle-r3-{rng}", 300, 48, 7, [("mix", 6)], [(20, 276)], rng=rng, opts={"chain_rows": 3},
                         rows=3, Dz=150, seed=41, width=256, where="middle"))
    out.append(_case("geometry", "300x48-w256-end-r2-pair", 300, 48, 5, [("mix", 6), ("vmode2", 4)], [(44, 300)], opts={"chain_rows": 2},
                     rows=2, Dz=300, seed=42, width=256, where="end"))
    return out


GEMM_SHAPES = ((24, 36), (32, 16), (64, 128), (128, 64), (144, 40), (272, 40), (532, 256))


def group_gemm():
    out = []
    for V, H in GEMM_SHAPES:
        groups = PRODUCTION[2] if (V, H) == PRODUCTION[:2] else ()
        for kind in ("meanfield", "sampled"):
            out.append(_case("gemm", f"{V}x{H}-{kind}", V, H, 5, [(kind, 3)], groups, seed=51))
        out.append(_case("gemm", f"{V}x{H}-pair-mix", V, H, 5, [("mix", 3), ("meanfield", 2)], groups, seed=52))
    return out


LDS_ADMITTED = ((1024, 352, (), "parity"), (1024, 352, ((1019, 1024),), "parity"), (1024, 1024, (), "fast"))
LDS_REJECTED = ((1024, 384, (), "parity"), (1024, 352, ((1018, 1024),), "parity"), (1025, 24, (), "parity"), (36, 1025, (), "parity"))


def group_lds():
    # three steps: noise (every draw helper, gz), a sampled step (the one-term GEMM) and a vmode 2 step: every LDS array is written
    out = []
    for V, H, groups, mode in LDS_ADMITTED + LDS_REJECTED:
        gw = groups[0][1] - groups[0][0] if groups else 0
        out.append(_case("lds", f"{V}x{H}-g{gw}-{mode}", V, H, 3, [("mix", 3)], groups, mode=mode, seed=61, admitted=(V, H, groups, mode) in LDS_ADMITTED))
    return out


def group_steps():
    V, H, _ = SMALL
    one = lambda name, chains, **kw: _case("steps", name, V, H, 3, chains, seed=71, **kw)      # noqa: E731
    out = [one(f"n{n}", [("sampled" if n > 64 else "mix", n)]) for n in (1, 2, 32, 33, 64, 65, 256, 257)]
    out += [one("n256-baseline", [dict(kind="sampled", n=256, base=True)]), one("n255-baseline", [dict(kind="sampled", n=255, base=True)]),
            _case("steps", "two-groups", V, H, 3, [("mix", 4)], [(20, 26), (30, 36)], seed=72),
            _case("steps", "two-groups-tape", V, H, 3, [("mix", 4)], [(20, 26), (30, 36)], rng="tape", seed=72),
            one("pair-128+128", [("sampled", 128), ("meanfield", 128)]), one("pair-128+129", [("sampled", 128), ("meanfield", 129)]),
            one("pair-33+7", [("mix", 33), ("mix", 7)]),
            one("pair-no_chain_pair", [("mix", 5), ("sampled", 4)], opts={"no_chain_pair": 1}),
            one("no_chain_kernel", [("mix", 5)], opts={"no_chain_kernel": 1}),
            one("pair-no_chain_kernel", [("mix", 5), ("sampled", 4)], opts={"no_chain_kernel": 1}),
            one("no-init-uniform", [dict(kind="mix", n=5, init_uniform=False)]),
            one("pair-no-init-uniform-b", [("mix", 4), dict(kind="noisy", n=4, init_uniform=False)]),
            one("pair-baseline-a", [dict(kind="mix", n=4, base=True), ("sampled", 4)]),
            one("pair-baseline-b", [("mix", 4), dict(kind="sampled", n=4, base=True)]),
            one("pair-1+4", [("mix", 1), ("mix", 4)])]
    return out


def group_pitch():
    V, H, groups = JOINT
    # HipEngine passes the row stride of v_known / mask (one stride for both) and of mu through (hip_engine._f32c keeps a column
    # slice with unit inner stride as it is), so the strided case reaches the kernel's ldk / ldmu
    return [_case("pitch", "150x48-p64-nan-padding", V, H, 5, [("mix", 6), ("noisy", 4)], groups, Dz=145, pitch=64, seed=81),
            _case("pitch", "150x48-strided-inputs", V, H, 5, [("mix", 6), ("vmode2", 4)], groups, Dz=145, strided=True, seed=82)]


def lds_edge(gw, H=48, mode="parity"):
    """(largest V the kernel admits with one group `gw` wide at this H, the first it rejects), from kernel_ok alone."""
    ok = [V for V in range(gw, PLANES_MAX + 1) if kernel_ok(V, H, ((V - gw, V),), mode, 3)]
    return ok[-1], next(V for V in range(ok[-1] + 1, PLANES_MAX + 2) if not kernel_ok(V, H, ((V - gw, V),), mode, 3))


WIDE_SHAPES = ((150, 48, ((117, 150),)), (300, 48, ((44, 300),)))      # JOINT with a group of 33; widened for one of 256


def group_wide():
    """One group of 33 (the first width past a wave's 32 lanes of logits per row pair) and of 256 (GROUP_WMAX): the group logits
    glog[row * GW + j], the noise drawn ahead gz[(gp * gwd + gc) * 2] and their 8-wide loops beyond gwd = 32; the two gw terms of
    chain_kernel_ok's LDS sum at the admission edge of a 256-wide group."""
    out = []
    for V, H, groups in WIDE_SHAPES:
        w = groups[0][1] - groups[0][0]
        for kind in ("mix", "noisy", "vmode2"):
            for rows in (2, 16):
                B = 5 if rows == 2 else 19
                out.append(_case("wide", f"{V}x{H}-w{w}-{kind}-r{rows}", V, H, B, [(kind, 6 if kind == "mix" else 4)], groups,
                                 opts={"chain_rows": rows}, rows=rows, Dz=(V - w - 7 if kind == "mix" else None), seed=91 + w, width=w))
        out.append(_case("wide", f"{V}x{H}-w{w}-r2-pair", V, H, 5, [("mix", 6), ("vmode2", 4)], groups, opts={"chain_rows": 2}, rows=2,
                         seed=92 + w, width=w))
    for V, admitted in zip(lds_edge(GROUP_WMAX), (True, False)):
        out.append(_case("wide", f"lds-{V}x48-g{GROUP_WMAX}", V, 48, 3, [("mix", 3)], ((V - GROUP_WMAX, V),), seed=93, width=GROUP_WMAX,
                         admitted=admitted))
    return out


@functools.lru_cache(maxsize=None)
def _all():
    cs = (group_rows() + group_auto() + group_fast() + group_geometry() + group_gemm() + group_lds() + group_steps() + group_pitch()
          + group_wide())
    assert len({c["id"] for c in cs}) == len(cs), "duplicate case id"
    return tuple(cs)


def cases(group=None):
    return [c for c in _all() if group is None or c["group"] == group]


def encoding(c, i):
    """How chain i's operands are encoded where it runs: the kernel's terms, or none (one launch per half step, PARITY: exact)."""
    if on_kernel(c, i):
        return c["mode"]
    assert c["mode"] == "parity", "the table runs FAST chains on the kernel only"
    return "none"


if __name__ == "__main__":
    for c in _all():
        print(c["id"], expected(c), [(ch["kind"], n_recs(ch)) for ch in c["chains"]], c["opts"])
