"""Cases shared by test_exchange_cpu.py and test_exchange_gpu.py: what a data-parallel step runs (RBM.train_epoch with dp.active()),
one process, the ranks emulated by copies, against float64 and against a numpy twin of the wire codec.

  factors path    cd_factors_wire -> all-gather -> apply_wire; building blocks pack_factors, unpack_factors, apply_factors_wire
  all-reduce      cd_stats / clamped_stats -> all-reduce (an fp32 sum) -> apply_delta: more than 64 rows per rank, H % 4 != 0,
                  softmax groups, or dp.enable(mode="allreduce")

The factor block (csrc/host_layout.hpp make_layout; every piece padded to 256 B; Bp = 64 ceil(B / 64), P = Bp / 8, Vpad = 16 ceil(V / 16)):

  flags      P * ceil(Vpad / 64) * 4      exactness map of the data (NOT ceil(V / 64): 300 -> Vpad 304 -> 5 words per row group)
  hid_tr0/1  3 * H * Bp * 2 each          hidden planes tr[term][feature][Bp] bf16, the negative ones negated
  cs_hpos, cs_hneg  P * H * 4 each;  cs_vpos, cs_vneg  P * V * 4 each      column-sum partials per 8 rows
  loss_part  (max(ceil(max(V, H) / 64) * P, (ceil(V / 8) + 2) * Bp / 64) + 4 * Bp / 64) * 4      (4 = IMDBN_MAX_GROUPS)
  ---- head_bytes = f_vpos: everything above travels verbatim
  vis_tr0    3 * V * Bp * 2               the data, three bf16 terms
  vis_tr1    V * Bp * 2                   the negative visible sample: its first plane only is inside the block

The compact (wire) block (csrc/engine.hip wire_layout; up = round up to 256):

  [0, head_bytes)                        the head, byte for byte
  c_vneg = head_bytes                    bit plane of vis_tr1, V * Bp / 8 bytes, up
  c_vpos = c_vneg + up(V * Bp / 8)       binary promise: bit plane of the FIRST plane of vis_tr0; else the three planes, up(3 V Bp 2)
  c_bad  = c_vpos + that                 trailer of 256 B: word 0 the `bad` mark, word 1 the pack epoch; bad when the two agree
  compact_bytes = c_bad + 256

The codec (csrc/kernels_ew.hpp, comment above pack8_bf16): byte i of a bit plane <-> the bf16 elements 8 i .. 8 i + 7 of the plane
[feature][Bp], element j in bit j, 1.0 = 0x3F80, 0.0 = 0; any other element raises `bad`.  pack_plane / unpack_plane below are that
statement in numpy and nothing else: the independent reference of the device codec (a bit order swapped inside unpack only is
invisible to tests that feed the update what went through the same pack / unpack pair).

Shapes (update_cases.py has the reasons a route depends on them; here what the wire layout adds):
  300 x 132    Vpad = 304 != V, last tile partial, n_flags from ceil(Vpad / 64) = 5; V * Bp / 8 = 2400 is no multiple of 256
  130 x 36     H < 128; head regions all need padding
  128 x 128    every plane and column-sum region a multiple of 256: no padding between them
  700 x 132 with k3_tpb = 5: the tile-wise rank kernel
  1100 x 260 on a pitch of 288 floats, the padding of W and W_m NaN: Vpad = 1104 > 1024, so the CD pass takes the streaming K1 and a
               prefetched 0/1 batch the compact slot form
  rows per rank 1 (Bp - 1 zero rows: the padding rows of every plane byte), 40 (division branch of the epilogue; 24 zero rows),
  64 (a full chunk: the last byte of a plane holds real rows); 1, 2 and 3 ranks (1 rank: the plain update kernel, PASS 0)

All-reduce group:
  300 x 45              H % 4 != 0: the generic statistics kernel + bias_update(pack_tail); apply_delta<false>
  1100 x 260 p288       apply_delta<true> with ldw != H: packed rows H apart, W rows 288 apart
  2100 x 8, 8 x 1100    V >> H and H >> V: the bias tail.  8 x 1100 gets the constructor's own pitch, 1152
  3 x 260               the grid rule grid.x >= ceil(max(V, H) / 256).  ceil(max(V, H) / 256) exceeds ceil(V H / 4 / 256) only if
                        min(V, H) < 4 (grid_rule_binds() below); H >= 4 on the float4 path, so V <= 3: neither 2100 x 8 (9 against 17
                        blocks) nor 8 x 1100 (5 against 9) does.  3 x 260 is the smallest H % 4 == 0 at V = 3 for which it does (2
                        against 1).  Only apply_delta runs at this shape, on statistics drawn on the host: no CD pass is needed to
                        test an element-wise kernel, and none of the suite's CD passes has so few visible units
  104 x 40, softmax group (96, 104): the smallest joint shape of parity_cases (case_joint_small); groups force the all-reduce path
  300 x 132             a factors-path shape taken to the all-reduce path by its rows per rank (104, 96), FAST mode; and, at 64 rows,
                        with `packed` a view one float into a larger buffer: the launcher must fall back to the scalar kernel
  batches 40, 64, 130, 200 in 2 or 3 shards on multiples of 8; sparsity on and off

References: update_cases.ref_update (rbm.py:212-224 in float64) on update_cases.stats64 of the operand planes the ORIGINAL cd_factors
blocks / the workspace hold; the tail of the packed buffer (dc = sum hpos - sum hneg, db = sum vpos - sum vneg, sum P+) from the same.
Tolerances: update_cases.TOL, update_cases.STATS_TOL and the 1e-5 loss tolerance of test_parity_gpu.py, nothing else."""
import functools

import numpy as np

import update_cases as UC

F32, F64 = np.float32, np.float64
MAX_GROUPS = 4                     # include/imdbn_engine.h IMDBN_MAX_GROUPS
ONE_BF16 = 0x3F80
LR, MOM, WD = 0.07, 0.6, 1e-3
cdiv = UC.cdiv


def up(x):
    return cdiv(x, 256) * 256


# ---- layouts (host_layout.hpp make_layout, engine.hip wire_layout), offsets relative to the start of the block ----------------------------
def block_layout(V, H, B):
    Bp = cdiv(max(B, 1), 64) * 64
    P, Vpad = Bp // 8, cdiv(V, 16) * 16
    n_loss = max(cdiv(max(V, H), 64) * P, (cdiv(V, 8) + 2) * (Bp // 64)) + MAX_GROUPS * (Bp // 64)
    sizes = [("flags", P * cdiv(Vpad, 64) * 4), ("hid_tr0", 3 * H * Bp * 2), ("hid_tr1", 3 * H * Bp * 2), ("cs_hpos", P * H * 4),
             ("cs_hneg", P * H * 4), ("cs_vpos", P * V * 4), ("cs_vneg", P * V * 4), ("loss_part", n_loss * 4),
             ("vis_tr0", 3 * V * Bp * 2), ("vis_tr1", V * Bp * 2)]
    L, off = dict(Bp=Bp, P=P, Vpad=Vpad, size={}), 0
    for name, n in sizes:
        L[name] = off
        L["size"][name] = n
        off += up(n)
    L["fb_bytes"] = off
    return L


def wire_layout(V, H, B, binary):
    L = block_layout(V, H, B)
    nb = V * L["Bp"] // 8
    w = dict(Bp=L["Bp"], nb=nb, head_bytes=L["vis_tr0"], f_vpos=L["vis_tr0"], f_vneg=L["vis_tr1"], f_cs_hpos=L["cs_hpos"],
             f_flags=L["flags"], n_flags=L["size"]["flags"], f_cs_vpos=L["cs_vpos"], n_cs_vpos=L["size"]["cs_vpos"])
    w["c_vneg"] = w["head_bytes"]
    w["c_vpos"] = w["c_vneg"] + up(nb)
    w["c_bad"] = w["c_vpos"] + (up(nb) if binary else up(3 * V * L["Bp"] * 2))
    w["compact_bytes"] = w["c_bad"] + 256
    return w


def factor_mode_ok(H, pitch, Bl, groups=()):
    """HipEngine.factor_mode_ok / engine.hip factor_mode_ok without the pointer alignment (torch allocations are 256-B aligned)."""
    return 1 <= Bl <= 64 and H % 4 == 0 and H >= 4 and (pitch or H) % 4 == 0 and not groups


def grid_rule_binds(V, H):
    """engine.hip imdbn_rbm_apply_delta on float4 rows: is grid.x set by ceil(max(V, H) / 256), not by the weight items?"""
    return cdiv(max(V, H), 256) > min(cdiv(V * H // 4, 256), 8192)


# ---- the codec twin ---------------------------------------------------------------------------------------------------------------------
def pack_plane(plane):
    """bf16 plane (uint16, a multiple of 8 elements) -> (bit-plane bytes, bad): element 8 i + j in bit j of byte i; bad when any element
    is neither 0 nor 0x3F80."""
    e = np.ascontiguousarray(plane, np.uint16).reshape(-1, 8)
    byte = ((e != 0).astype(np.uint16) << np.arange(8, dtype=np.uint16)).sum(axis=1).astype(np.uint8)
    return byte, bool(((e != 0) & (e != ONE_BF16)).any())


def unpack_plane(byte):
    b = np.ascontiguousarray(byte, np.uint8).astype(np.uint16)
    return (((b[:, None] >> np.arange(8, dtype=np.uint16)) & 1) * np.uint16(ONE_BF16)).astype(np.uint16).reshape(-1)


def bad_elements(plane):
    e = np.ascontiguousarray(plane, np.uint16).reshape(-1)
    return np.flatnonzero((e != 0) & (e != ONE_BF16))


def expand(compact, V, H, B, binary):
    """One compact block (host bytes) -> the full block unpack_factors must produce, by the twin; bytes unpack leaves alone are 0xFF,
    and so are the second and third data plane under a binary promise (the exactness map says "one term": nobody reads them)."""
    L, w = block_layout(V, H, B), wire_layout(V, H, B, binary)
    full = np.full(L["fb_bytes"], 0xFF, np.uint8)
    full[: w["head_bytes"]] = compact[: w["head_bytes"]]
    n = V * w["Bp"] * 2
    full[w["f_vneg"]: w["f_vneg"] + n] = unpack_plane(compact[w["c_vneg"]: w["c_vneg"] + w["nb"]]).view(np.uint8)
    if binary:
        full[w["f_vpos"]: w["f_vpos"] + n] = unpack_plane(compact[w["c_vpos"]: w["c_vpos"] + w["nb"]]).view(np.uint8)
    else:
        full[w["f_vpos"]: w["f_vpos"] + 3 * n] = compact[w["c_vpos"]: w["c_vpos"] + 3 * n]
    return full


def with_zero_terms(full, V, H, B):
    """`expand` of a binary block with the two unread data planes as zeros: what update_gpu.phases decodes."""
    L = block_layout(V, H, B)
    n = V * L["Bp"] * 2
    out = full.copy()
    out[L["vis_tr0"] + n: L["vis_tr0"] + 3 * n] = 0
    return out


# ---- the tail of the packed statistics ------------------------------------------------------------------------------------------------------
def tail64(s):
    """[dc | db | sum P+] of the packed buffer from stats64's sums."""
    return dict(dc=s["hpos"] - s["hneg"], db=s["vpos"] - s["vneg"], sp=s["hpos"])


def split_packed(packed, V, H):
    p = np.asarray(packed)
    t = p[V * H:]
    return dict(dW=p[: V * H].reshape(V, H), dc=t[:H], db=t[H:H + V], sp=t[H + V:2 * H + V], sqerr=t[2 * H + V])


def shards(B, n):
    """Row ranges of `n` shards on multiples of 8 (test_stats_then_apply_equals_fused_update_for_multi_chunk_batches)."""
    step = (B // n + 7) // 8 * 8
    cuts = [min(i * step, B) for i in range(n)] + [B]
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:])]


# ---- the tables -------------------------------------------------------------------------------------------------------------------------
def _shape(V, H, tpb=None, pitch=0):
    o = {"k3_tpb": tpb} if tpb else {}
    return dict(V=V, H=H, tpb=tpb or 1, opts=o, pitch=pitch, name=f"{V}x{H}" + (f"-t{tpb}" if tpb else "") + (f"-p{pitch}" if pitch else ""))


S300, S130, S128, S700 = _shape(300, 132), _shape(130, 36), _shape(128, 128), _shape(700, 132, 5)
S1100 = _shape(1100, 260, pitch=288)


def _w(sh, R, Bl, data, binary, mode="exact"):
    kernel = UC.UPDATE_RANKS if R >= 2 else UC.UPDATE_PLANES        # apply_factors: one block runs the plain kernel, PASS 0
    return dict(sh, id=f"W-{sh['name']}-R{R}x{Bl}-{data}-{'bits' if binary else 'planes'}-{mode}", group="W", entry="apply_wire", R=R,
                Bl=Bl, B=R * Bl, data=data, binary=binary, mode=mode, opts=dict(sh["opts"]), expect=(kernel, sh["tpb"]),
                mixed_rank=min(1, R - 1))


def wire_cases():
    return [_w(S300, 2, 64, "binary", True), _w(S300, 3, 40, "mixed", False), _w(S300, 1, 1, "binary", True),
            _w(S300, 2, 1, "binary", False, "fast"), _w(S130, 2, 40, "binary", True, "fast"), _w(S130, 3, 64, "mixed", False),
            _w(S128, 2, 64, "binary", True), _w(S128, 3, 1, "mixed", False), _w(S700, 2, 40, "binary", True),
            _w(S700, 3, 64, "mixed", False, "fast"), _w(S1100, 2, 64, "binary", True), _w(S1100, 3, 40, "mixed", False)]


def fused_cases():
    """W3: cd_factors_wire over two ranks and three steps; `hint`: next_data is passed; `prefetch`: the route takes it (the slot)."""
    out = []
    for sh, binary, hint, opts in ((S1100, True, True, {}), (S300, False, True, {}), (S300, True, False, {}),
                                   (S300, True, True, {"no_prefetch": 1})):
        c = _w(sh, 2, 40, "binary" if binary else "mixed", binary)
        c.update(id=f"F-{sh['name']}-{'bits' if binary else 'planes'}-{'hint' if hint else 'nohint'}{'-no_prefetch' if opts else ''}",
                 group="F", entry="cd_factors_wire", hint=hint, prefetch=hint and not opts, opts=dict(c["opts"], **opts), steps=3)
        out.append(c)
    return out


def broken_cases():
    """W4: one 0.5 in 0/1 data under a binary promise: (rank, batch row, visible column) of the planted element."""
    out = []
    for sh, R, Bl, where in ((S300, 2, 40, "first"), (S300, 2, 64, "last"), (S130, 3, 40, "last"), (S300, 3, 40, "last_rank")):
        c = _w(sh, R, Bl, "binary", True)
        V = sh["V"]
        plant = {"first": (0, 3, 0), "last": (0, Bl - 1, V - 1), "last_rank": (R - 1, Bl // 2, V // 2)}[where]
        c.update(id=f"K-{sh['name']}-R{R}x{Bl}-{where}", group="K", entry="broken_promise", where=where, plant=plant)
        out.append(c)
    return out


def plant_index(c):
    """Index of the planted element in the data plane [V][Bp] of its rank."""
    _, row, col = c["plant"]
    return col * (cdiv(c["Bl"], 64) * 64) + row


def _d(sh, B, n, data, sparsity, why, mode="exact", entry="cd_stats", groups=(), generic=False, **kw):
    name = f"D-{entry}-{sh['name']}-B{B}s{n}-{data}{'-sparsity' if sparsity else ''}{'-fast' if mode == 'fast' else ''}"
    c = dict(sh, id=name + "".join(f"-{k}" for k in kw), group="D", entry=entry, B=B, n_shards=n, data=data, sparsity=sparsity, why=why,
             mode=mode, groups=tuple(groups), opts=dict(sh["opts"]), expect=(UC.UPDATE_GENERIC, 0) if generic else (UC.UPDATE_PLANES, sh["tpb"]),
             misaligned=False, synthetic=False)
    c.update(kw)
    return c


S45, S2100, S8, S3, SJ = _shape(300, 45), _shape(2100, 8), _shape(8, 1100, pitch=1152), _shape(3, 260), _shape(104, 40)
JOINT_GROUPS = ((96, 104),)


def delta_cases():
    """All-reduce group.  `why`: what keeps the case off the factors path ("H%4", "rows", "groups"; "mode": nothing, dp.enable(mode=
    "allreduce") chose it)."""
    return [_d(S45, 40, 2, "binary", True, "H%4", generic=True), _d(S45, 130, 3, "mixed", False, "H%4", generic=True),
            _d(S1100, 64, 2, "binary", True, "mode"), _d(S1100, 200, 2, "mixed", False, "rows"),
            _d(S2100, 40, 2, "binary", True, "mode"), _d(S8, 64, 2, "real", False, "mode"),
            _d(SJ, 130, 3, "binary", False, "groups", groups=JOINT_GROUPS), _d(SJ, 40, 2, "binary", True, "groups", mode="fast", groups=JOINT_GROUPS),
            _d(SJ, 40, 2, "binary", False, "groups", entry="clamped_stats", groups=JOINT_GROUPS),
            _d(S300, 200, 2, "mixed", True, "rows", mode="fast"), _d(S300, 64, 2, "binary", True, "mode", misaligned=True),
            _d(S3, 64, 1, "real", True, "mode", synthetic=True)]


def stats_cases():
    """D1: the statistics and their tail, on the joint shape (cd_stats exact and FAST, clamped_stats), the generic kernel and V >> H."""
    want = {"D-cd_stats-104x40-B130s3-binary", "D-cd_stats-104x40-B40s2-binary-sparsity-fast", "D-clamped_stats-104x40-B40s2-binary",
            "D-cd_stats-300x45-B40s2-binary-sparsity", "D-cd_stats-2100x8-B40s2-binary-sparsity"}
    out = [c for c in delta_cases() if c["id"] in want]
    assert len(out) == len(want)
    return out


def apply_cases():
    return [c for c in delta_cases() if c["entry"] == "cd_stats"]


@functools.lru_cache(maxsize=None)
def _all():
    cs = wire_cases() + fused_cases() + broken_cases() + delta_cases()
    assert len({c["id"] for c in cs}) == len(cs), "duplicate case id"
    return tuple(cs)


def cases(group=None):
    return [c for c in _all() if group is None or c["group"] == group]


# ---- data -------------------------------------------------------------------------------------------------------------------------------
def rank_data(c, rank, step=0):
    """Rows of one rank (update_cases.cd_data; later steps of a fused case: fresh 0/1 batches), the planted element set where the case
    has one."""
    if step:
        x = UC.visible("binary", c["Bl"], c["V"], c["tpb"], f"rank{rank}-step{step}")
    else:
        x = UC.cd_data(c, rank)
    if c.get("plant") and c["plant"][0] == rank:
        x = x.copy()
        x[c["plant"][1], c["plant"][2]] = 0.5
    return x


@functools.lru_cache(maxsize=None)
def _batch(cid):
    c = next(c for c in _all() if c["id"] == cid)
    x = UC.visible(c["data"], c["B"], c["V"], c["tpb"], "data").copy()
    for s, e in c["groups"]:                     # a joint batch: [code | one-hot label]
        x[:, s:e] = np.eye(e - s, dtype=F32)[np.arange(c["B"]) % (e - s)]
    x.setflags(write=False)
    return x


def batch(c):
    return _batch(c["id"])


def clamped_inputs(c):
    """(v_known, mask) of a clamped case: the label columns of the batch known, everything else free."""
    x = batch(c)
    vk, km = np.zeros_like(x), np.zeros_like(x)
    for s, e in c["groups"]:
        vk[:, s:e] = x[:, s:e]
        km[:, s:e] = 1
    return vk, km


def synthetic_stats(c):
    """Un-normalised statistics drawn on the host for a case that runs apply_delta alone: (packed fp32 buffer without padding, the
    float64 sums ref_update takes)."""
    V, H, B = c["V"], c["H"], c["B"]
    g = UC._gen(9, V, H, B)
    dW = (g.standard_normal((V, H), dtype=F32) * F32(B / 8)).astype(F32)
    hpos, hneg = g.random(H, dtype=F32) * F32(B), g.random(H, dtype=F32) * F32(B)
    vpos, vneg = g.random(V, dtype=F32) * F32(B), g.random(V, dtype=F32) * F32(B)
    dc, db = (hpos - hneg).astype(F32), (vpos - vneg).astype(F32)
    sqerr = F32(0.25 * B * V)
    packed = np.concatenate([dW.ravel(), dc, db, hpos, [sqerr]]).astype(F32)
    z = np.zeros
    s = dict(dW=dW.astype(F64), hpos=hpos.astype(F64), hneg=hpos.astype(F64) - dc.astype(F64), vpos=db.astype(F64), vneg=z(V, F64))
    return packed, s


if __name__ == "__main__":
    for c in _all():
        print(c["id"], c["expect"], c["opts"])
