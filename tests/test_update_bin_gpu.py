"""The two-plane weight-update kernel of a 0/1 batch (assoc_update_bin) against the kernel it replaces on that route.

`no_update_bin` forces the old route (assoc_update_planes<0, HT, 0>).  Both run the same MFMAs in the same order on the same
fragments and the same epilogue arithmetic, so every comparison here is BIT FOR BIT.  A batch that is not one-term (mixed or
real-valued columns) enters the new kernel too (the host does not know) and must leave through the old body.  Every run asserts
which kernel it launched and with how many visible tiles per block (imdbn_debug_last_update).

What is new in the kernel -- the two alternating slice buffers, the slice request ahead of the epilogue stores, the counted wait
that leaves those stores in flight, the 24 + 8 prefetch -- only runs in a block that takes MORE THAN ONE tile.  The host picks
tiles_per_block = ceil(tiles / CUs), which is 1 for every small shape on a 256-CU device, so the cases that matter force it with
the `k3_tpb` option (tiles per block in brackets; groups = tiles of the blocks of one column stripe):
  300 x 132  [3]   one group of three tiles, the last partial (rows 256..299); two column stripes, the second 4 columns wide;
                   both slice buffers used, buffer 0 reused
  128 x 128  [3]   a single tile in a block that could take three: the prologue's slices only, no next tile is ever requested
  1100 x 260 [4]   nine tiles, the last partial (rows 1024..1099): groups 4, 4, 1 -- a last group with an odd count
  1100 x 260 [7]   groups 7, 2 -- a last group with an even count, and seven tiles through the two buffers
             1100 x 260 on a padded row pitch (288 floats) whose padding is poisoned with NaN and must stay untouched
and the same shapes as the host picks it (one tile per block on the devices this suite runs on: the prologue path alone).
Batch 64, and 40 (zero rows in the 64-row chunk; 40 is no power of two: the division branch of the epilogue).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle.rbm_oracle as O
import parity_cases as P
from golden_utils import assert_close, gpu_cd_samples
from oracle.draws import PhiloxStream

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda:0"
STATE = P.KEYS
UPDATE_PLANES, UPDATE_BIN = 1, 2      # include/imdbn_engine.h IMDBN_UPDATE_*
# (V, H, forced tiles per block or None = as the host picks it)
SHAPES = [(300, 132, None), (128, 128, None), (1100, 260, None), (300, 132, 3), (128, 128, 3), (1100, 260, 4), (1100, 260, 7)]


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    eng = E.get_hip_engine()
    yield eng
    eng.set_option("no_update_bin", 0)
    eng.set_option("k3_tpb", 0)


def _last_update():
    """(kernel, visible tiles per block) of the last weight update this thread launched."""
    from imdbn.engine import native
    rec = (C.c_int * 2)()
    native.check(native.lib().imdbn_debug_last_update(rec), "imdbn_debug_last_update")
    return rec[0], rec[1]


def _padded(r):
    V, H = r.W.shape
    pitch = r.W.stride(0)
    return (torch.as_strided(r.W.data, (V, pitch), (pitch, 1)), torch.as_strided(r.W_m, (V, pitch), (pitch, 1)), pitch)


PITCH = {260: 288}      # hidden width -> forced row pitch (the constructor pads 132, 128 and 260 columns to nothing by itself)


def _make(V, H, W0):
    """RBM from the constructor (W / W_m row-padded where PITCH says so, the padding poisoned with NaN), parameters set in place."""
    from imdbn.models import RBM
    with pytest.MonkeyPatch.context() as mp:
        if H in PITCH:
            mp.setenv("IMDBN_ROW_PITCH_ABS", str(PITCH[H]))
        r = RBM(V, H, 0.1, 1e-4, 0.5, dynamic_lr=True, final_momentum=0.95).to(DEV)
    Wb, Mb, pitch = _padded(r)
    assert pitch == PITCH.get(H, H) and r.W_m.stride(0) == pitch and r.W_m.data_ptr() != r.W.data_ptr(), pitch
    if pitch > H:
        Wb[:, H:] = float("nan")
        Mb[:, H:] = float("nan")
    r.W.data.copy_(P.T(W0, DEV))
    r.W_m.zero_()
    r.hid_bias.data.zero_(); r.vis_bias.data.zero_(); r.hb_m.zero_(); r.vb_m.zero_()
    assert r.W.stride(0) == pitch
    return r


def _padding_untouched(r):
    Wb, Mb, _ = _padded(r)
    H = r.W.shape[1]
    assert Wb.shape[1] == H or (torch.isnan(Wb[:, H:]).all() and torch.isnan(Mb[:, H:]).all()), "a kernel wrote into the row padding"
    for k in STATE:
        assert torch.isfinite(getattr(r, k)).all(), f"NaN leaked from the row padding into {k}"


def _data(kind, B, V, n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(n):
        if kind == "real":
            X = g.random((B, V), dtype=F32)
        else:
            X = (g.random((B, V), dtype=F32) > 0.8).astype(F32)
            if kind == "mixed":                      # a few real-valued columns, in the first and in the last visible tile
                for c in (3, 70, V - 2):
                    X[:, c] = g.random(B, dtype=F32)
        out.append(X)
    return out


def _run(eng, old_route, V, H, W0, xs, seed, prefetch, tpb=None, tag=False, fast=False):
    """The state and the loss after every update of the batches `xs`, on the old or the new route; `tpb` forces the tiles per
    block, `tag` marks the batches as 0/1 for the engine, `fast` runs the single-term arithmetic (HT = 1, host-known term count)."""
    from imdbn import engine as E
    from imdbn.engine import native
    eng.set_option("no_update_bin", 1 if old_route else 0)
    eng.set_option("k3_tpb", tpb or 0)
    mode = eng.mode
    try:
        if fast:
            eng.mode = native.FAST_BF16
        r = _make(V, H, W0)
        ts = [P.T(x, DEV) for x in xs]
        if tag:
            for t in ts:
                t._imdbn_binary = True
        snaps = []
        with E.use_rng(E.PhiloxRng(seed=seed)):
            for i, t in enumerate(ts):
                nxt = ts[i + 1] if prefetch and i + 1 < len(ts) else None
                loss = r.train_epoch(t, 0, 10, CD=1, next_data=nxt)
                kernel, got_tpb = _last_update()
                assert kernel == (UPDATE_PLANES if old_route else UPDATE_BIN), (kernel, old_route)
                assert got_tpb == tpb if tpb else got_tpb >= 1, (got_tpb, tpb)
                snaps.append((float(loss), {k: getattr(r, k).detach().clone() for k in STATE}))
        torch.cuda.synchronize()
        _padding_untouched(r)
        return snaps
    finally:
        eng.mode = mode
        eng.set_option("no_update_bin", 0)
        eng.set_option("k3_tpb", 0)


def _both(eng, V, H, tpb, xs, seed, prefetch=False, **kw):
    W0 = _W0(V, H)
    new = _run(eng, False, V, H, W0, xs, seed, prefetch, tpb, **kw)
    old = _run(eng, True, V, H, W0, xs, seed, prefetch, tpb, **kw)
    _assert_same(new, old, f"{V}x{H} tiles per block {tpb} {kw}")
    return new, W0


def _assert_same(new, old, what):
    assert len(new) == len(old)
    for i, ((ln, sn), (lo, so)) in enumerate(zip(new, old)):
        assert ln == lo, f"{what}: loss of update {i}: {ln!r} != {lo!r}"
        for k in STATE:
            if not torch.equal(sn[k], so[k]):
                d = (sn[k] != so[k]).nonzero()
                raise AssertionError(f"{what}: {k} differs after update {i} at {d.shape[0]} elements, first {d[0].tolist()}")


def _W0(V, H, seed=5):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.standard_normal((V, H), dtype=F32) / F32(np.sqrt(V))).astype(F32)


@pytest.mark.parametrize("B", [64, 40])
@pytest.mark.parametrize("V,H,tpb", SHAPES)
def test_binary_batch_equals_the_old_route_bit_for_bit(_native, V, H, tpb, B):
    new, W0 = _both(_native, V, H, tpb, _data("binary", B, V, 2, seed=11), seed=31)
    assert not torch.equal(new[0][1]["W"], P.T(W0, DEV)), "the update did nothing"


@pytest.mark.parametrize("kind", ["mixed", "real"])
def test_a_batch_that_is_not_one_term_leaves_through_the_old_body(_native, kind):
    _both(_native, 300, 132, 3, _data(kind, 64, 300, 2, seed=12), seed=32)


@pytest.mark.parametrize("V,H,tpb", [(300, 132, 3), (1100, 260, 4)])
def test_ten_consecutive_prefetched_updates_equal_the_old_route(_native, V, H, tpb):
    _both(_native, V, H, tpb, _data("binary", 64, V, 10, seed=13), seed=33, prefetch=True)


@pytest.mark.parametrize("kw", [{"tag": True}, {"fast": True}], ids=["tagged", "fast"])
def test_tagged_batches_and_the_single_term_arithmetic(_native, kw):
    """Batches the caller marked as 0/1, and FAST mode: there the host knows the term count (vpos_terms = 1) and HT = 1 runs."""
    _both(_native, 300, 132, 3, _data("binary", 40, 300, 3, seed=15), seed=35, prefetch=True, **kw)


def test_binary_update_against_the_oracle(_native):
    """One Philox update on the new route, three tiles per block, against the numpy oracle at the suite's tolerance
    (test_layouts_gpu.py)."""
    from imdbn import engine as E
    V, H, B = 300, 132, 64
    W0 = _W0(V, H)
    X = _data("binary", B, V, 1, seed=14)[0]
    st = O.RBMState.create(W0, 0.1, 1e-4, 0.5, dynamic_lr=True, final_momentum=0.95)
    _native.set_option("k3_tpb", 3)
    try:
        r = _make(V, H, W0)
        with E.use_rng(E.PhiloxRng(seed=21)):
            loss = r.train_epoch(P.T(X, DEV), 0, 10, CD=1)
        assert _last_update() == (UPDATE_BIN, 3)
    finally:
        _native.set_option("k3_tpb", 0)
    h_gpu, v_gpu = gpu_cd_samples(_native, DEV, V, H, B)
    O.set_tie_break([h_gpu, v_gpu, None], tol=2e-6)
    try:
        want = O.train_epoch(st, X, 0, 1, PhiloxStream(21))
        assert O.TIE_BREAK["used"] <= 6, dict(O.TIE_BREAK, queue=None)
    finally:
        O.set_tie_break(None)
    assert_close(float(loss), want, 1e-5, "loss")
    for k in STATE:
        assert_close(P.N(getattr(r, k)), getattr(st, k), 1e-4, k, atol=2e-6)
    _padding_untouched(r)
