"""Cases shared by test_trace_scans_cpu.py and test_trace_scans_gpu.py: the convergence-tracing family of DESIGN section 10 at the
shapes where its kernels can go wrong (DESIGN section 39 has the table and the figures).

A  Partial trace windows of chain_traced / chain_traced_vh (k4_chain's `col >= c0 && col < c1` with the base pointer moved back by c0,
   trace_copy on the route of one launch per half step, htr_t0 under a baseline slot).  test_chain_kernel_gpu.py holds the FULL
   windows to float64, so a partial window only has to equal columns [c0, c1) of the full window of the same call under the same
   seed, bit for bit; final states and the RNG offset must be those of the untraced call.  One RBM, 83 x 45 (no multiple of 16)
   with the softmax group [70, 79) inside V; batches 1, 5, 67; the `mix` schedule of chain_cases.py (sampled h and v, noise,
   temperatures) at 4 steps, so a chain has 4 or 5 records and the kernel route applies.

B  trace_code_scan against float64.  beta = 0 copies: z_new has the input's bits.  On the 2^-6 grid every d = z - z_prev is a
   multiple of 2^-6 of magnitude at most 1, every d * d a multiple of 2^-12 at most 1, and a sum of at most 130 of them is below
   2^8: a multiple of 2^-12 below 2^12 fits the 24-bit significand, so every partial sum is exact in any order and only the square
   root rounds: dz lies within one ulp of float32(sqrt(exact sum)).  Real values and beta > 0: the rule of test_tap_gpu.py -- the
   fp32 twin trace_oracle.code_scan_f32 is measured against float64 over these same cases, the kernel gets four times its worst
   figure per quantity (z_new elementwise absolute, dz relative) and width Dz, capped by the 1e-4 parity bound of DESIGN
   section 5 (`code_scan_bounds`).  The float64 reference takes beta as the fp32 number the entry receives.

C  trace_patience_scan: dyadic inputs and thresholds, both sides decide in double, every output equal.  `PLANTS` names the planted
   rows; a plant that does not fit T or the patience is left out of that case and the CPU test asserts where each must be present.
   As the rule is written a step that improves resets the counter before it is tested, so a stop and an improvement cannot share a
   step: the plant `improve_at_stop` puts an improvement on the very step at which the counter would have run out, and the oracle's
   answer (no stop there) is what the kernel must give.  With best = +inf nothing finite fails to improve, so the only rows that
   stop at t = patience are those whose mse is NaN or +inf from the start.

D  imdbn_rbm_prop_down_sqerr / HipEngine.decode_sqerr against float64.  Weights ~ N(0, 1) / sqrt(H): the fan-in of the down
   direction is H, so the logits have the spread under which route_cases.prob_bound was established.  Bound, derived:
   let d = prob_bound(1.0), p the float64 probabilities, p + e the device's, |e| <= d.  In exact arithmetic
       mean((p + e - r)^2) - mean((p - r)^2) = mean(2 e (p - r)) + mean(e^2),   so   |.| <= 2 d mean|p - r| + d^2.
   The fp32 evaluation of the mean adds, relative to the mean of non-negative terms: at most ceil(V / 256) - 1 < V / 256 additions
   per thread, 8 levels of the tree, the square and the division: (V / 256 + 10) 2^-24 mse.  (The subtraction x - r rounds too:
   2 * 2^-24 mse <= 2 * 2^-24 mean|p - r|, charged to the first term, where d = 5e-7 was stated for K = 2000 and these K <= 132.)
   Under a second layer the bottom layer's operand is itself off by at most d per element: its logits move by at most
   d * max_v sum_h |W[v, h]| and its probabilities by a quarter of that, so d_stack = d (1 + max_v sum_h |W[v, h]| / 4).

E  One odd-shaped panel, both directions, against trace_oracle.StackOracle: image stack [67, 33, 21], joint (21 + 5) x 19, B = 9,
   T = 12, z_class_mean; curves within the tolerances of test_full_size_panel_against_the_oracle, steps and pred equal on every
   row whose oracle margin exceeds 1e-5, at most B // 4 rows excused; the seed is the first for which the oracle alone meets that
   and, in both directions, stops some row and does not stop every row at the same step."""
import functools
import zlib

import numpy as np

import chain_cases as CC
import route_cases as RC
import trace_oracle as TO

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
PARITY = 1e-4


def _gen(key):
    return np.random.Generator(np.random.PCG64(zlib.crc32(key.encode())))


# ---- A: windows -------------------------------------------------------------------------------------------------------------------------
WIN_V, WIN_H, WIN_GROUP = 83, 45, (70, 79)
WIN_BATCHES = (1, 5, 67)
WIN_STEPS = 4
WIN_SEED = 2024
VIS_WINDOWS = ((0, 1), (82, 83), (37, 38), (3, 70), (70, 79), (72, 77), (0, 83))
HID_WINDOWS = ((0, 1), (44, 45), (17, 18), (3, 40), (0, 45))
RAW_VIS, RAW_HID = (3, 70), (3, 40)           # the windows that go under the wrapper


def window_calls():
    """(trace or None, trace_h or None) of every single-chain call: each visible window with and without the baseline slot, the hidden
    windows dealt round over them (so each occurs under a baseline, where htr_t0 = 1, and without), and each hidden window alone."""
    out, k = [], 0
    for base in (0, 1):
        for c0, c1 in VIS_WINDOWS:
            out.append(((c0, c1, base), HID_WINDOWS[k % len(HID_WINDOWS)] if k % 3 != 2 else None))
            k += 1
    out += [(None, w) for w in HID_WINDOWS]
    return out


def window_pairs():
    """Pairs of chains with different windows: (chain a's (trace, trace_h), chain b's)."""
    return [(((3, 70, 1), None), (None, (3, 40))),                       # a visible window only, b hidden only
            (((70, 79, 0), (0, 1)), ((72, 77, 1), (44, 45))),
            (((0, 1, 1), (3, 40)), ((82, 83, 0), (17, 18)))]


@functools.lru_cache(maxsize=None)
def window_problem(B):
    g = _gen(f"windows-{B}")
    p = dict(W=(g.standard_normal((WIN_V, WIN_H)) * 0.3).astype(F32), hb=(g.standard_normal(WIN_H) * 0.5).astype(F32),
             vb=(g.standard_normal(WIN_V) * 0.5).astype(F32), vk=g.random((B, WIN_V), dtype=F32),
             mask=[(g.random((B, WIN_V)) < 0.5).astype(F32), (g.random((B, WIN_V)) < 0.5).astype(F32)])
    return p


def window_steps(chain=0):
    return CC.schedule("mix", WIN_STEPS) if chain == 0 else CC.schedule("sampled", WIN_STEPS - 1)


def window_route(no_chain_kernel, pair):
    """The route name imdbn_debug_last_chain must report (chain_cases.kernel_ok: small planes, one group, 3 to 5 records)."""
    recs = WIN_STEPS - 1
    ok = CC.kernel_ok(WIN_V, WIN_H, [WIN_GROUP], "parity", recs, {"no_chain_kernel": no_chain_kernel})
    return "per_launch" if not ok else ("kernel_pair" if pair else "kernel")


# ---- B: code scan -----------------------------------------------------------------------------------------------------------------------
CODE_DZ, CODE_B, CODE_T, CODE_BETA = (1, 63, 64, 65, 130), (1, 4, 5, 9), (1, 6), (0.0, 0.3, 1.0)


def code_cases():
    """Every (Dz, B, T, beta); beta = 0 on the 2^-6 grid and on real values, beta > 0 on real values.  B = 5 passes the trace as a
    view of a NaN-filled [T, B, Dz + 3] parent (and z_init as a view of a NaN-filled [B, Dz + 3] one)."""
    out = []
    for Dz in CODE_DZ:
        for B in CODE_B:
            for T in CODE_T:
                for beta in CODE_BETA:
                    for data in (("grid", "real") if beta == 0.0 else ("real",)):
                        out.append(dict(id=f"code-Dz{Dz}-B{B}-T{T}-beta{beta}-{data}", Dz=Dz, B=B, T=T, beta=float(F32(beta)), data=data,
                                        strided=(B == 5)))
    return out


@functools.lru_cache(maxsize=None)
def _code_inputs(cid, Dz, B, T, data):
    g = _gen(cid)
    if data == "grid":
        zs, z0 = g.integers(0, 65, (T, B, Dz)).astype(F32) / 64, g.integers(0, 65, (B, Dz)).astype(F32) / 64
    else:
        zs, z0 = g.random((T, B, Dz), dtype=F32), g.random((B, Dz), dtype=F32)
    zs.setflags(write=False); z0.setflags(write=False)
    return zs, z0


def code_inputs(c):
    return _code_inputs(c["id"], c["Dz"], c["B"], c["T"], c["data"])


@functools.lru_cache(maxsize=None)
def code_ref(cid):
    c = next(c for c in code_cases() if c["id"] == cid)
    zs, z0 = code_inputs(c)
    return TO.code_scan(zs.astype(F64), z0.astype(F64), c["beta"])


def code_errors(c, zn, dz):
    """(largest |z_new - float64|, largest |dz - float64| / float64) of an fp32 result."""
    zr, dr = code_ref(c["id"])
    return float(np.abs(zn.astype(F64) - zr).max()), float((np.abs(dz.astype(F64) - dr) / dr).max())


@functools.lru_cache(maxsize=None)
def code_scan_twin_worst(Dz):
    """The twin's worst error against float64 over the real-valued cases of this width: (z_new absolute, dz relative).  Per width,
    because at Dz = 1 the relative error of dz = |z - z_prev| is that of one difference, which can be small against its operands'
    rounding (cancellation), while a sum over many columns never is."""
    wz = wd = 0.0
    for c in code_cases():
        if c["data"] == "real" and c["Dz"] == Dz:
            zs, z0 = code_inputs(c)
            ez, ed = code_errors(c, *TO.code_scan_f32(zs, z0, c["beta"]))
            wz, wd = max(wz, ez), max(wd, ed)
    return wz, wd


def code_scan_bounds(Dz):
    """(z_new absolute, dz relative) at this width: four times the twin's worst figure, capped by the parity bound."""
    wz, wd = code_scan_twin_worst(Dz)
    return min(4 * wz, PARITY), min(4 * wd, PARITY)


# ---- C: patience scan -------------------------------------------------------------------------------------------------------------------
PAT_B, PAT_T, PAT_P = (1, 63, 64, 65, 130), (1, 2, 7), (1, 3)
EPS_Z, MSE_TOL = 2.0 ** -10, 2.0 ** -10
SMALL, BIG = 2.0 ** -12, 2.0 ** -8               # dz below / above eps_z
PLANTS = ("stop_at_patience", "stop_at_T", "never", "dz_equals_eps", "late_reset", "exact_tol", "all_nan", "inf_inside",
          "improve_at_stop")


def plant(name, T, P):
    """(dz row, mse row, expected steps, expected best) of a planted row, or None where it does not fit T and the patience."""
    lo, inf, nan = np.full(T, SMALL), np.inf, np.nan
    if name == "stop_at_patience":               # nothing ever improves on +inf
        return (lo, np.full(T, inf), P, inf) if T >= P else None
    if name == "all_nan":
        return (lo, np.full(T, nan), P, inf) if T >= P else None
    if name == "stop_at_T":                      # improves through step T - P, flat after
        if T - P < 1:
            return None
        m = np.array([0.5 - 2 * MSE_TOL * min(t, T - P - 1) for t in range(T)])
        return lo, m, T, m[-1]
    if name == "never":
        return np.full(T, BIG), np.full(T, 0.5), T + 1, 0.5
    if name == "dz_equals_eps":                  # not below: the counter never starts
        return np.full(T, EPS_Z), np.full(T, 0.5), T + 1, 0.5
    if name == "late_reset":                     # the counter at P - 2, an improvement at step P, then P flat steps
        if P < 2 or T < 2 * P:
            return None
        m = np.array([0.5] * (P - 1) + [0.25] * (T - P + 1))
        return lo, m, 2 * P, 0.25
    if name == "exact_tol":                      # m = best - mse_tol: m + 1e-12 < best - mse_tol is false in double
        if T < P + 1:
            return None
        m = np.array([0.5] + [0.5 - MSE_TOL] * (T - 1))
        return lo, m, P + 1, 0.5
    if name == "inf_inside":
        if T < 2:
            return None
        m = np.array([0.5, inf] + [0.25, inf] * T)[:T]      # +inf never improves: it counts like a flat step
        steps, best = {(2, 1): (2, 0.5), (7, 1): (2, 0.5), (2, 3): (3, 0.5), (7, 3): (6, 0.25)}[(T, P)]
        return lo, m, steps, best
    assert name == "improve_at_stop", name        # counter at P - 1, then an improvement on the step it would have run out
    if T < P + 1:
        return None
    m = np.array([0.5] * P + [0.25] * (T - P))
    return lo, m, (2 * P + 1 if 2 * P + 1 <= T else T + 1), 0.25


def patience_cases():
    return [dict(id=f"patience-B{B}-T{T}-p{P}", B=B, T=T, P=P) for B in PAT_B for T in PAT_T for P in PAT_P]


@functools.lru_cache(maxsize=None)
def _patience_inputs(B, T, P):
    g = _gen(f"patience-{B}-{T}-{P}")
    dz = g.choice([SMALL, SMALL, EPS_Z, BIG], (B, T))
    mse = g.integers(0, 1024, (B, T)) / 1024.0
    mse[g.random((B, T)) < 0.05] = np.nan
    mse[g.random((B, T)) < 0.05] = np.inf
    fits = [n for n in PLANTS if plant(n, T, P) is not None]
    rows = {}
    for i, n in enumerate(fits):                 # B = 1 takes the plant its (T, P) index names; larger batches take them all
        b = 0 if B == 1 else i
        if B == 1 and i != (T + P) % len(fits):
            continue
        dz[b], mse[b] = plant(n, T, P)[:2]
        rows[n] = b
    return dz.astype(F32), mse.astype(F32), rows


def patience_inputs(c):
    """(dz, mse) fp32 [B, T] -- every value dyadic, NaN or +inf -- and {plant name: row}."""
    return _patience_inputs(c["B"], c["T"], c["P"])


def patience_ref(c):
    dz, mse, _ = patience_inputs(c)
    steps, best, _ = TO.patience_scan(dz.astype(F64), mse.astype(F64), EPS_Z, MSE_TOL, c["P"])
    return steps, best


# ---- D: decode error --------------------------------------------------------------------------------------------------------------------
DEC_V, DEC_H, DEC_B = (5, 255, 256, 257, 700), (33, 64, 132), (1, 5, 67, 130)
REF_ROWS = ("none", "perm", "repeat")


@functools.lru_cache(maxsize=None)
def layer(V, H):
    """(W [V, H], hb, vb) fp32: W ~ N(0, 1) / sqrt(H), biases ~ 0.1 N(0, 1)."""
    g = _gen(f"decode-layer-{V}x{H}")
    return ((g.standard_normal((V, H)) / np.sqrt(H)).astype(F32), (g.standard_normal(H) * 0.1).astype(F32),
            (g.standard_normal(V) * 0.1).astype(F32))


def decode_cases():
    """Every bottom layer V x H, with the batches, the two kinds of h, the three kinds of ref_row and plain / strided operands dealt
    round so that each value meets several shapes; then the two-layer stacks."""
    out, k = [], 0
    for V in DEC_V:
        for H in DEC_H:
            for kind in ("binary", "real"):
                B, rr = DEC_B[k % 4], REF_ROWS[(k // 2) % 3]
                out.append(dict(id=f"decode-{V}x{H}-B{B}-{kind}-{rr}{'-strided' if k % 2 else ''}", sizes=(V, H), B=B, kind=kind,
                                ref_row=rr, strided=bool(k % 2)))
                k += 1
    for sizes, B, kind, rr, st in (((257, 33, 21), 67, "real", "repeat", True), ((700, 132, 64), 130, "binary", "perm", False),
                                   ((5, 64, 33), 5, "real", "none", False)):
        out.append(dict(id=f"decode-{'x'.join(map(str, sizes))}-B{B}-{kind}-{rr}{'-strided' if st else ''}", sizes=sizes, B=B, kind=kind,
                        ref_row=rr, strided=st))
    return out


def decode_layers(c):
    s = c["sizes"]
    return [layer(s[i], s[i + 1]) for i in range(len(s) - 1)]


@functools.lru_cache(maxsize=None)
def _decode_inputs(cid, n, Dz, V, kind, rr):
    g = _gen(cid)
    z = g.random((n, Dz), dtype=F32)
    if kind == "binary":
        z = (z > 0.6).astype(F32)
    if rr == "repeat":                           # n = T * R rows against R references, as the tracing does with arange(R).repeat(T)
        R = max(1, n // 4)
        rows = np.resize(np.arange(R), n).astype(np.int32)
    elif rr == "perm":
        R, rows = n, g.permutation(n).astype(np.int32)
    else:
        R, rows = n, None
    ref = np.where(g.random((R, V)) < 0.5, (g.random((R, V)) < 0.3).astype(F32), g.random((R, V), dtype=F32)).astype(F32)
    return z, ref, rows


def decode_inputs(c):
    """(z [B, top], ref [R, V], ref_row int32 [B] or None, every entry in [0, R))."""
    s = c["sizes"]
    return _decode_inputs(c["id"], c["B"], s[-1], s[0], c["kind"], c["ref_row"])


def decode_ref(c, z=None, ref=None, rows=None):
    """(float64 mse [B], its bound [B]) of the case (or of the given operands on the case's layers)."""
    if z is None:
        z, ref, rows = decode_inputs(c)
    L = decode_layers(c)
    l64 = [(W.astype(F64), vb.astype(F64)) for W, _, vb in L]
    p = TO.decode_probs(l64, z)
    r = ref.astype(F64)[rows if rows is not None else np.arange(len(z))]
    mse = ((p - r) ** 2).mean(1)
    d = RC.prob_bound(1.0)
    if len(L) > 1:
        d = d * (1 + float(np.abs(l64[0][0]).sum(1).max()) / 4)
    V = c["sizes"][0]
    return mse, 2 * d * np.abs(p - r).mean(1) + d * d + (V / 256 + 10) * U * mse


def decode_twin(c):
    """The fp32 twin: decode in fp32 numpy, then trace_oracle.row_sqerr_f32."""
    z, ref, rows = decode_inputs(c)
    cur = z
    for W, _, vb in reversed(decode_layers(c)):
        cur = (F32(1) / (F32(1) + np.exp(-((cur @ W.T).astype(F32) + vb)))).astype(F32)
    return TO.row_sqerr_f32(cur, ref[rows if rows is not None else np.arange(len(z))])


# ---- E: the odd-shaped panel ------------------------------------------------------------------------------------------------------------
PANEL_SIZES, PANEL_DZ, PANEL_K, PANEL_JH, PANEL_B, PANEL_T = (67, 33, 21), 21, 5, 19, 9, 12
PANEL_MARGIN = 1e-5
PANEL_SEED = 4                                   # panel_seed(): pinned by test_trace_scans_cpu.py


@functools.lru_cache(maxsize=None)
def panel(seed):
    """(weights dict, X [B, 67] 0/1, Y one-hot [B, K], class indices) of the panel drawn from `seed`."""
    g = np.random.Generator(np.random.PCG64(1000 + seed))
    s, Dz, K = PANEL_SIZES, PANEL_DZ, PANEL_K
    w = {}
    for i in range(2):
        w[f"img{i}_W"] = (g.standard_normal((s[i], s[i + 1])) * (2.0 / np.sqrt(s[i]))).astype(F32)
        w[f"img{i}_hid_bias"] = (g.standard_normal(s[i + 1]) * 0.5).astype(F32)
        w[f"img{i}_vis_bias"] = (g.standard_normal(s[i]) * 0.5).astype(F32)
    w["joint_W"] = (g.standard_normal((Dz + K, PANEL_JH)) * 0.3).astype(F32)
    w["joint_hid_bias"] = (g.standard_normal(PANEL_JH) * 0.2).astype(F32)
    w["joint_vis_bias"] = np.concatenate([g.standard_normal(Dz) * 0.2, g.standard_normal(K) * 1.5]).astype(F32)
    w["z_class_mean"] = g.random((K, Dz), dtype=F32)
    yi = np.arange(PANEL_B) % K
    X = (g.random((PANEL_B, s[0])) < 0.3).astype(F32)
    return w, X, np.eye(K, dtype=F32)[yi], yi


@functools.lru_cache(maxsize=None)
def panel_oracle(seed):
    """(img2txt (curves, steps, pred, margin), txt2img dict) of StackOracle, the initial uniforms from the Philox twin."""
    from oracle.draws import PhiloxStream
    w, X, Y, yi = panel(seed)
    o = TO.StackOracle(w, PANEL_DZ, PANEL_K)
    u = PhiloxStream(seed).uniform((PANEL_B, PANEL_DZ + PANEL_K)).astype(F64)
    return o.img2txt(X, u, PANEL_T, gt=yi), o.txt2img(X, Y, PANEL_T)


def panel_ok(seed):
    (_, s1, _, m1), t = panel_oracle(seed)
    s2, m2 = t["steps"], t["margin"]
    excused = int((m1 <= PANEL_MARGIN).sum() + (m2 <= PANEL_MARGIN).sum())
    mixed = all((s <= PANEL_T).any() and len(set(s.tolist())) >= 2 for s in (s1, s2))
    return excused <= PANEL_B // 4 and mixed


def panel_seed(limit=200):
    return next(s for s in range(limit) if panel_ok(s))


if __name__ == "__main__":
    for Dz in CODE_DZ:
        print(f"code scan Dz {Dz}: twin's worst (z_new abs, dz rel)", code_scan_twin_worst(Dz), "bounds", code_scan_bounds(Dz))
    print("panel seed", panel_seed())
