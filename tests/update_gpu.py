"""GPU helpers shared by test_update_routes_gpu.py and test_exchange_gpu.py (a plain module: no tests, no fixtures): an RBM on a forced
row pitch with poisoned padding, the options of a case, the NaN-filled workspace, and the float64 statistics of the operand planes a
CD pass left behind (update_cases.py has the reasoning)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import parity_cases as P
import update_cases as UC
from golden_utils import assert_close

DEV = "cuda:0"
F32, F64 = np.float32, np.float64


def last_update():
    from imdbn.engine import native
    rec = (C.c_int * 2)()
    native.check(native.lib().imdbn_debug_last_update(rec), "imdbn_debug_last_update")
    return rec[0], rec[1]


def assert_update(c):
    got = last_update()
    assert got == tuple(c["expect"]), f"{c['id']}: launched update kernel {got[0]} with {got[1]} tiles per block, the case names {c['expect']}"


@contextlib.contextmanager
def routed(eng, c):
    """The case's options and engine mode for the duration of the calls."""
    from imdbn.engine import native
    mode = eng.mode
    try:
        for k, v in c["opts"].items():
            eng.set_option(k, v)
        eng.mode = native.FAST_BF16 if c["mode"] == "fast" else native.PARITY_F32
        yield
    finally:
        eng.mode = mode
        for k in c["opts"]:
            eng.set_option(k, UC.OPTION_DEFAULTS[k])


def poison_ws(eng, V, H, B):
    eng._workspace(torch.device(DEV), V, H, B).view(torch.float32).fill_(float("nan"))


def padded(r):
    V, _ = r.W.shape
    pitch = r.W.stride(0)
    return torch.as_strided(r.W.data, (V, pitch), (pitch, 1)), torch.as_strided(r.W_m, (V, pitch), (pitch, 1)), pitch


def rbm(c, st, wd, sparsity=False, groups=None):
    """RBM from the constructor (row pitch forced and its padding poisoned with NaN where the case says so), state `st` set in place."""
    from imdbn.models import RBM
    V, H = c["V"], c["H"]
    with pytest.MonkeyPatch.context() as mp:
        if c["pitch"]:
            mp.setenv("IMDBN_ROW_PITCH_ABS", str(c["pitch"]))
        r = RBM(V, H, 0.1, wd, 0.5, sparsity=sparsity, sparsity_factor=UC.SPARSITY_TARGET, softmax_groups=groups).to(DEV)
    Wb, Mb, pitch = padded(r)
    assert pitch == (c["pitch"] or H) and r.W_m.stride(0) == pitch and r.W_m.data_ptr() != r.W.data_ptr(), pitch
    if pitch > H:
        Wb[:, H:] = float("nan")
        Mb[:, H:] = float("nan")
    r.W.data.copy_(P.T(st["W"], DEV)); r.W_m.copy_(P.T(st["W_m"], DEV))
    r.hid_bias.data.copy_(P.T(st["hid_bias"], DEV)); r.vis_bias.data.copy_(P.T(st["vis_bias"], DEV))
    r.hb_m.copy_(P.T(st["hb_m"], DEV)); r.vb_m.copy_(P.T(st["vb_m"], DEV))
    assert r.W.stride(0) == pitch
    return r


def state(r):
    torch.cuda.synchronize()
    Wb, Mb, pitch = padded(r)
    H = r.W.shape[1]
    if pitch > H:
        assert torch.isnan(Wb[:, H:]).all() and torch.isnan(Mb[:, H:]).all(), "a kernel wrote into the row padding"
    out = {k: P.N(getattr(r, k)) for k in UC.KEYS}
    for k, v in out.items():
        assert np.isfinite(v).all(), f"{k} is not finite"
    return out


def close(c, got, ref, tol=UC.TOL, what=""):
    worst = {k: float(np.abs(got[k].astype(F64) - ref[k]).max()) for k in UC.KEYS}
    print(f"{c['id']}{what}: max|d| " + "  ".join(f"{k} {d:.3e}" for k, d in worst.items()))
    for k in UC.KEYS:
        assert_close(got[k], ref[k], tol["rel"], f"{c['id']}{what}: {k}", atol=tol["atol"])


# ---- from the operand planes the kernel read ------------------------------------------------------------------------------------------
def ws_offset(eng, V, H, B, name):
    off = C.c_size_t(0)
    eng._call("imdbn_debug_ws_offset", int(V), int(H), int(B), name.encode(), C.byref(off))
    return int(off.value)


def phases(c, B, read):
    """(vpos, hpos, vneg, hneg) in float64 from the planes vis_tr0, hid_tr0, vis_tr1, hid_tr1 (tr[term][feature][Bp] bf16, hid_tr1
    stored negated); `read(name, nbytes)` returns the bytes of a buffer.  The terms the update kernel reads: three of the data and of
    the hidden probabilities (one in FAST mode), one of the negative visible sample."""
    V, H, Bp = c["V"], c["H"], (B + 63) // 64 * 64
    t = 1 if c["mode"] == "fast" else 3
    return (UC.decode_planes(read("vis_tr0", t * V * Bp * 2), V, B, Bp, t), UC.decode_planes(read("hid_tr0", t * H * Bp * 2), H, B, Bp, t),
            UC.decode_planes(read("vis_tr1", V * Bp * 2), V, B, Bp, 1), UC.decode_planes(read("hid_tr1", t * H * Bp * 2), H, B, Bp, t, negated=True))


def colsum(read, name, N, B):
    """A column sum the bias update reads: the per-8-row partials [Bp / 8][N] fp32, summed in float64."""
    Pn = (B + 63) // 64 * 8
    return read(name, Pn * N * 4).view(F32).reshape(Pn, N).astype(F64).sum(0)


def stats(c, blocks, rows=None):
    """float64 statistics of the row blocks [(phases, read)].  In FAST mode the first plane alone is a bf16 rounding of the operand,
    while the bias update reads column sums of the fp32 values: those sums are then taken from the device's partials.  `rows`: the
    rows of each block (default: the case's rows per rank, or its batch)."""
    s = UC.stats64([ph for ph, _ in blocks])
    if c["mode"] == "fast":
        rows = rows if rows is not None else [c.get("Bl", c["B"])] * len(blocks)
        s["hpos"] = sum(colsum(read, "cs_hpos", c["H"], n) for (_, read), n in zip(blocks, rows))
        s["hneg"] = sum(colsum(read, "cs_hneg", c["H"], n) for (_, read), n in zip(blocks, rows))
        s["vpos"] = sum(colsum(read, "cs_vpos", c["V"], n) for (_, read), n in zip(blocks, rows))
    return s


def ws_reader(eng, c, B):
    torch.cuda.synchronize()
    return lambda name, nbytes: eng.debug_buffer(DEV, c["V"], c["H"], B, name, nbytes).cpu().numpy()


def block_reader(eng, c, Bl, host_block):
    """`read` of phases / colsum on a host copy of one factor block of `Bl` rows."""
    fb, _ = eng.factor_block(c["V"], c["H"], Bl)

    def read(name, nbytes):
        off = ws_offset(eng, c["V"], c["H"], Bl, name) - fb
        return host_block[off:off + nbytes].copy()
    return read
