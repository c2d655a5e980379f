"""GPU: the weight / bias update (K3) on every kernel route against float64, each case asserting through imdbn_debug_last_update
that it launched the kernel and the tiles per block it names (update_cases.py has the table, the shapes and the reasoning).

  A  exact inputs through HipEngine.assoc_update: all six state tensors BIT-EQUAL to the float64 reference (signed zeros aside)
  B  real-valued and mixed inputs, non-trivial state and hyper-parameters: float64 within rel 2e-5 / atol 2e-6
  C  the routes only a CD pass reaches -- statistics into `delta` (cd_stats), the rank kernels (cd_factors + apply_factors) and a
     CD-1 train_epoch on the bin and planes routes -- against float64 computed from the operand planes the kernel read

Every call runs on a NaN-filled workspace; the options of a case are reset in a `finally`."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import parity_cases as P
import update_cases as UC
from golden_utils import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    eng = E.get_hip_engine()             # raises if the library is missing: no silent fallback
    cu, arch = eng.device_info()
    assert "gfx950" in arch, arch
    assert cu >= 16, "the automatic tiles per block of the table's shapes is 1 only with more CUs than tiles"
    yield eng
    for k, v in UC.OPTION_DEFAULTS.items():
        eng.set_option(k, v)


def _last_update():
    from imdbn.engine import native
    rec = (C.c_int * 2)()
    native.check(native.lib().imdbn_debug_last_update(rec), "imdbn_debug_last_update")
    return rec[0], rec[1]


def _assert_update(c):
    got = _last_update()
    assert got == tuple(c["expect"]), f"{c['id']}: launched update kernel {got[0]} with {got[1]} tiles per block, the case names {c['expect']}"


@contextlib.contextmanager
def _routed(eng, c):
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


def _poison_ws(eng, V, H, B):
    eng._workspace(torch.device(DEV), V, H, B).view(torch.float32).fill_(float("nan"))


def _padded(r):
    V, _ = r.W.shape
    pitch = r.W.stride(0)
    return torch.as_strided(r.W.data, (V, pitch), (pitch, 1)), torch.as_strided(r.W_m, (V, pitch), (pitch, 1)), pitch


def _rbm(c, st, wd, sparsity=False):
    """RBM from the constructor (row pitch forced and its padding poisoned with NaN where the case says so), state `st` set in place."""
    from imdbn.models import RBM
    V, H = c["V"], c["H"]
    with pytest.MonkeyPatch.context() as mp:
        if c["pitch"]:
            mp.setenv("IMDBN_ROW_PITCH_ABS", str(c["pitch"]))
        r = RBM(V, H, 0.1, wd, 0.5, sparsity=sparsity, sparsity_factor=UC.SPARSITY_TARGET).to(DEV)
    Wb, Mb, pitch = _padded(r)
    assert pitch == (c["pitch"] or H) and r.W_m.stride(0) == pitch and r.W_m.data_ptr() != r.W.data_ptr(), pitch
    if pitch > H:
        Wb[:, H:] = float("nan")
        Mb[:, H:] = float("nan")
    r.W.data.copy_(P.T(st["W"], DEV)); r.W_m.copy_(P.T(st["W_m"], DEV))
    r.hid_bias.data.copy_(P.T(st["hid_bias"], DEV)); r.vis_bias.data.copy_(P.T(st["vis_bias"], DEV))
    r.hb_m.copy_(P.T(st["hb_m"], DEV)); r.vb_m.copy_(P.T(st["vb_m"], DEV))
    assert r.W.stride(0) == pitch
    return r


def _state(r):
    torch.cuda.synchronize()
    Wb, Mb, pitch = _padded(r)
    H = r.W.shape[1]
    if pitch > H:
        assert torch.isnan(Wb[:, H:]).all() and torch.isnan(Mb[:, H:]).all(), "a kernel wrote into the row padding"
    out = {k: P.N(getattr(r, k)) for k in UC.KEYS}
    for k, v in out.items():
        assert np.isfinite(v).all(), f"{k} is not finite"
    return out


def _close(c, got, ref, tol=UC.TOL):
    worst = {k: float(np.abs(got[k].astype(F64) - ref[k]).max()) for k in UC.KEYS}
    print(f"{c['id']}: max|d| " + "  ".join(f"{k} {d:.3e}" for k, d in worst.items()))
    for k in UC.KEYS:
        assert_close(got[k], ref[k], tol["rel"], f"{c['id']}: {k}", atol=tol["atol"])


# ---- A: exact inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", UC.cases("A"), ids=IDS)
def test_exact_inputs_give_the_float64_update_bit_for_bit(c, _native):
    ops = [P.T(x, DEV) for x in UC.operands(c)]
    ref = UC.ref_a(c)
    with _routed(_native, c):
        r = _rbm(c, UC.zero_params(c["V"], c["H"]), 0.0)
        _poison_ws(_native, c["V"], c["H"], c["B"])
        _native.assoc_update(r, *ops, 1.0, 0.0)
        _assert_update(c)
        got = _state(r)
    for k in UC.KEYS:
        want = ref[k].astype(F32)
        if not np.array_equal(got[k], want):
            bad = np.argwhere(got[k] != want)
            i = tuple(bad[0])
            raise AssertionError(f"{c['id']}: {k} differs from float64 at {len(bad)} of {want.size} elements, first {i}: got {got[k][i]!r}, "
                                 f"want {want[i]!r} (difference {float(got[k][i]) - float(want[i]):.3e}); rows {sorted(set(bad[:, 0]))[:8]}")


# ---- B: general arithmetic --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", UC.cases("B"), ids=IDS)
def test_update_matches_float64_on_its_route(c, _native):
    ops = [P.T(x, DEV) for x in UC.operands(c)]
    with _routed(_native, c):
        r = _rbm(c, UC.params(c["V"], c["H"]), UC.B_WD, c["sparsity"])
        _poison_ws(_native, c["V"], c["H"], c["B"])
        _native.assoc_update(r, *ops, UC.B_LR, UC.B_MOM)
        _assert_update(c)
        got = _state(r)
    _close(c, got, UC.ref_b(c))


# ---- C: from the operand planes the kernel read ---------------------------------------------------------------------------------------
def _ws_offset(eng, V, H, B, name):
    off = C.c_size_t(0)
    eng._call("imdbn_debug_ws_offset", int(V), int(H), int(B), name.encode(), C.byref(off))
    return int(off.value)


def _phases(c, B, read):
    """(vpos, hpos, vneg, hneg) in float64 from the planes vis_tr0, hid_tr0, vis_tr1, hid_tr1 (tr[term][feature][Bp] bf16, hid_tr1
    stored negated); `read(name, nbytes)` returns the bytes of a buffer.  The terms the update kernel reads: three of the data and of
    the hidden probabilities (one in FAST mode), one of the negative visible sample."""
    V, H, Bp = c["V"], c["H"], (B + 63) // 64 * 64
    t = 1 if c["mode"] == "fast" else 3
    return (UC.decode_planes(read("vis_tr0", t * V * Bp * 2), V, B, Bp, t), UC.decode_planes(read("hid_tr0", t * H * Bp * 2), H, B, Bp, t),
            UC.decode_planes(read("vis_tr1", V * Bp * 2), V, B, Bp, 1), UC.decode_planes(read("hid_tr1", t * H * Bp * 2), H, B, Bp, t, negated=True))


def _colsum(read, name, N, B):
    """A column sum the bias update reads: the per-8-row partials [Bp / 8][N] fp32, summed in float64."""
    Pn = (B + 63) // 64 * 8
    return read(name, Pn * N * 4).view(F32).reshape(Pn, N).astype(F64).sum(0)


def _stats(c, blocks):
    """float64 statistics of the row blocks [(phases, read)].  In FAST mode the first plane alone is a bf16 rounding of the operand,
    while the bias update reads column sums of the fp32 values: those sums are then taken from the device's partials."""
    s = UC.stats64([ph for ph, _ in blocks])
    if c["mode"] == "fast":
        rows = c.get("Bl", c["B"])
        s["hpos"] = sum(_colsum(read, "cs_hpos", c["H"], rows) for _, read in blocks)
        s["hneg"] = sum(_colsum(read, "cs_hneg", c["H"], rows) for _, read in blocks)
        s["vpos"] = sum(_colsum(read, "cs_vpos", c["V"], rows) for _, read in blocks)
    return s


def _ws_reader(eng, c, B):
    torch.cuda.synchronize()
    return lambda name, nbytes: eng.debug_buffer(DEV, c["V"], c["H"], B, name, nbytes).cpu().numpy()


def _tagless(x):
    return P.T(x, DEV)


@pytest.mark.parametrize("c", UC.cases("C", "cd_stats"), ids=IDS)
def test_statistics_match_float64_of_the_planes(c, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    st = UC.params(V, H)
    with _routed(_native, c):
        r = _rbm(c, st, UC.C_WD)
        _poison_ws(_native, V, H, B)
        packed = _native.cd_stats(r, _tagless(UC.cd_data(c)), 1, E.PhiloxRng(seed=7))
        _assert_update(c)
        got = P.N(packed)[: V * H].reshape(V, H)
        vp, hp, vn, hn = _phases(c, B, _ws_reader(_native, c, B))
        after = _state(r)
    assert np.array_equal(vp.astype(F32), UC.cd_data(c)) or c["mode"] == "fast", "vis_tr0 does not hold the batch"
    want = vp.T @ hp - vn.T @ hn
    print(f"{c['id']}: max|d| {float(np.abs(got - want).max()):.3e} of max {float(np.abs(want).max()):.3e}")
    assert_close(got, want, UC.STATS_TOL["rel"], f"{c['id']}: statistics", atol=UC.STATS_TOL["atol"])
    for k in UC.KEYS:
        assert np.array_equal(after[k], st[k]), f"{c['id']}: the statistics pass changed {k}"


@pytest.mark.parametrize("c", UC.cases("C", "apply_factors"), ids=IDS)
def test_rank_update_matches_float64_of_the_gathered_planes(c, _native):
    from imdbn import engine as E
    V, H, R, Bl = c["V"], c["H"], c["R"], c["Bl"]
    st = UC.params(V, H)
    lr, mom = 0.07, 0.6
    with _routed(_native, c):
        r = _rbm(c, st, UC.C_WD)
        assert _native.factor_mode_ok(r, Bl)
        gathered = _native.gather_buffer(r, Bl, R)
        _poison_ws(_native, V, H, Bl)
        for rk in range(R):
            gathered[rk].copy_(_native.cd_factors(r, _tagless(UC.cd_data(c, rk)), 1, E.PhiloxRng(seed=11, row0=rk * Bl)))
        _native.apply_factors(r, gathered, Bl, R * Bl, lr, mom)
        _assert_update(c)
        got = _state(r)
        fb, _ = _native.factor_block(V, H, Bl)
        host = gathered.cpu().numpy()
        blocks = []
        for rk in range(R):
            def read(name, nbytes, rk=rk):
                off = _ws_offset(_native, V, H, Bl, name) - fb
                return host[rk, off:off + nbytes].copy()
            blocks.append((_phases(c, Bl, read), read))
    if c["mode"] == "exact":
        for rk in range(R):
            assert np.array_equal(blocks[rk][0][0].astype(F32), UC.cd_data(c, rk)), f"rank {rk}: vis_tr0 does not hold the batch"
    _close(c, got, UC.ref_update(st, _stats(c, blocks), lr, mom, UC.C_WD, R * Bl))


@pytest.mark.parametrize("c", UC.cases("C", "train_epoch"), ids=IDS)
def test_cd1_step_matches_float64_of_the_planes(c, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    st = UC.params(V, H)
    with _routed(_native, c):
        r = _rbm(c, st, UC.C_WD)
        lr, mom = r._lr_mom(0)
        _poison_ws(_native, V, H, B)
        with E.use_rng(E.PhiloxRng(seed=13)):
            loss = r.train_epoch(_tagless(UC.cd_data(c)), 0, 10, CD=1)
        _assert_update(c)
        got = _state(r)
        read = _ws_reader(_native, c, B)
        ph = _phases(c, B, read)
    assert np.isfinite(float(loss)) and np.array_equal(ph[0].astype(F32), UC.cd_data(c))
    _close(c, got, UC.ref_update(st, _stats(c, [(ph, read)]), lr, mom, UC.C_WD, B))
