"""GPU: imdbn_cross_metrics against its numpy twin on given p (no chains), accumulation over calls and bit-for-bit repeats, invalid
arguments, ``iMDBN._log_snapshots`` against the reference's recording (snapshots_small.npz, the recorded draws replayed) and
``iMDBN.evaluate`` against the twin fed the outputs of ``_cross_reconstruct`` run by hand.

Decisions (pred, rank, confusion, counts) compare the same fp32 numbers on both sides, so they must be equal exactly, on every row.
Tolerances: ce_sum 1e-5 relative (F_REL of test_energy_trace_gpu.py), p_pred / p_true 1e-6 absolute against the twin on the same p
and 1e-5 absolute (P_TOL) against the reference's recording, snap/image_mse 1e-4 relative (the single-RBM tolerance of
test_parity_gpu.py), text_ce / image_mse of evaluate 1e-5 relative."""
import numpy as np
import pytest
import torch

import cross_eval_oracle as CO
from cross_eval_cases import Run, Tape, small_model as _small_model
from golden_utils import Fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_TOL = 1e-5
F_REL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    yield E.get_hip_engine()


@pytest.fixture(scope="module")
def fx():
    return Fixture("snapshots_small.npz")


@pytest.fixture(scope="module")
def small(fx):
    return _small_model(fx, DEV, n_rows=21)


def _rel(a, b, tol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b) / np.abs(b)
    print(f"{what}: max relative error {err.max():.3g} (tolerance {tol:g})")
    assert err.max() <= tol, f"{what}: {err.max():.3g} > {tol:g}"


def _random_p(g, B, K):
    """Rows of independent sigmoids (what the label slice of a mean-field chain holds), a few of them nearly one-hot."""
    p = (1.0 / (1.0 + np.exp(-2.5 * g.standard_normal((B, K))))).astype(np.float32)
    p[::5] = (p[::5] ** 6).astype(np.float32)
    return p


def _host(o):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _check(o, m, tag, with_mse=True):
    """Engine result `o` (host arrays) against the twin `m`: decisions exact on every row, the sums to their tolerances."""
    for k in ("pred", "gt", "rank"):
        assert np.array_equal(o[k], m[k]), f"{tag} {k}: rows {np.nonzero(o[k] != m[k])[0][:8]}"
    assert np.array_equal(o["confusion"], m["confusion"]), f"{tag} confusion"
    assert np.array_equal(o["acc"][[0, 1, 2, 5, 6, 7]], m["acc"][[0, 1, 2, 5, 6, 7]]), (tag, o["acc"], m["acc"])
    assert np.array_equal(o["class_sums"][:, :2], m["class_sums"][:, :2]), f"{tag} class counts"
    _rel(o["acc"][3], m["acc"][3], F_REL, f"{tag} ce_sum")
    for k in ("p_pred", "p_true"):
        err = np.abs(o[k].astype(np.float64) - m[k])
        print(f"{tag} {k}: max error {err.max():.3g} (tolerance 1e-6)")
        assert err.max() <= 1e-6
    if with_mse:
        _rel(o["acc"][4], m["acc"][4], F_REL, f"{tag} mse_sum")
        seen = m["class_sums"][:, 0] > 0
        _rel(o["class_sums"][seen, 2], m["class_sums"][seen, 2], F_REL, f"{tag} class sums of row_mse")
        assert (o["class_sums"][~seen] == 0).all()


SHAPES = [(1, 2, 3), (5, 3, 3), (9, 2, 3), (67, 65, 3), (33, 256, 3), (256, 32, 3), (4100, 10, 2)]


@pytest.mark.parametrize("B,K,topk", SHAPES, ids=lambda v: str(v))
def test_kernel_against_the_twin(B, K, topk, _native):
    """(9, 2) with topk = 3 > K; (67, 65) one past a wave; (33, 256) four slots per lane; (4100, 10): more rows than one pass of the
    1024-block grid (every wave takes a second row)."""
    g = np.random.Generator(np.random.PCG64(1000 * B + K))
    p = _random_p(g, B, K)
    gt = g.integers(0, K, B).astype(np.int32)
    rm = g.random(B, dtype=np.float32)
    tp, trm = torch.from_numpy(p).to(DEV), torch.from_numpy(rm).to(DEV)
    m = CO.metrics(p, gt=gt, row_mse=rm, npix=100, topk=topk)
    a = _host(_native.cross_metrics(tp, gt=torch.from_numpy(gt).to(DEV), row_mse=trm, npix=100, topk=topk))
    _check(a, m, f"B={B} K={K} gt")
    # the same truth as one-hot rows: identical results, bit for bit
    y = torch.from_numpy(np.eye(K, dtype=np.float32)[gt]).to(DEV)
    b = _host(_native.cross_metrics(tp, y=y, row_mse=trm, npix=100, topk=topk))
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"B={B} K={K}: {k} differs between gt and y"


def test_tail_view_of_a_wider_buffer(_native):
    """(64, 32) read as v[:, 37:] of a [64, 69] buffer whose other columns are NaN: a base aligned to 4 bytes only, ldp != K."""
    g = np.random.Generator(np.random.PCG64(5))
    p = _random_p(g, 64, 32)
    gt = g.integers(0, 32, 64).astype(np.int32)
    big = torch.full((64, 69), float("nan"), device=DEV)
    big[:, 37:] = torch.from_numpy(p).to(DEV)
    view = big[:, 37:]
    assert view.data_ptr() % 16 == 4 and view.stride(0) == 69
    ybig = torch.full((64, 45), float("nan"), device=DEV)
    ybig[:, 13:] = torch.from_numpy(np.eye(32, dtype=np.float32)[gt]).to(DEV)
    o = _host(_native.cross_metrics(view, y=ybig[:, 13:]))
    _check(o, CO.metrics(p, gt=gt), "tail view", with_mse=False)
    assert o["acc"][4] == 0 and (o["class_sums"][:, 2] == 0).all()


def test_tie_rule(_native):
    """The top two equal (the lower index predicts); the true label tied with a lower and a higher index (rank counts the lower)."""
    K = 70
    p = np.full((6, K), 0.25, np.float32)
    p[0, [3, 68]] = 0.9                      # top two equal, across two slots of a lane pair
    p[1, [64, 65]] = 0.9                     # top two equal in the second slot
    p[2, [10, 20, 30]] = 0.5                 # the truth (20) tied with a lower and a higher index
    p[3] = 0.5                               # everything ties
    p[4, 69] = 0.7; p[4, 5] = 0.7            # the truth is the LOWER of a tied top pair
    p[5, 0] = 0.1                            # the truth is the only value below the rest
    gt = np.array([68, 65, 20, 69, 5, 0], np.int32)
    o = _host(_native.cross_metrics(torch.from_numpy(p).to(DEV), gt=torch.from_numpy(gt).to(DEV), topk=2))
    assert o["pred"].tolist() == [3, 64, 10, 0, 5, 1]
    assert o["rank"].tolist() == [1, 1, 1, 69, 0, 69]
    assert o["acc"][:3].tolist() == [6, 1, 4]
    _check(o, CO.metrics(p, gt=gt, topk=2), "ties", with_mse=False)


def test_clamps(_native):
    """Rows holding exact 0, exact 1 and values below 1e-6: p_pred / p_true clamp to [1e-9, 1], the BCE to [1e-6, 1 - 1e-6]."""
    p = np.array([[0.0, 1.0, 1e-8, 0.5], [1.0, 0.0, 0.0, 0.0], [1e-10, 1e-7, 1e-12, 0.0], [0.0, 0.0, 0.0, 0.0]], np.float32)
    gt = np.array([0, 0, 2, 3], np.int32)
    o = _host(_native.cross_metrics(torch.from_numpy(p).to(DEV), gt=torch.from_numpy(gt).to(DEV)))
    m = CO.metrics(p, gt=gt)
    _check(o, m, "clamps", with_mse=False)
    assert o["p_true"].tolist() == [np.float32(1e-9), 1.0, np.float32(1e-9), np.float32(1e-9)]
    assert o["p_pred"].tolist() == [1.0, 1.0, np.float32(1e-7), np.float32(1e-9)]
    # row 1 is a perfect prediction: its BCE is 4 x -log(1 - 1e-6) in fp32 terms, about 4e-6; row 0's true label costs -log(1e-6)
    assert abs(m["ce_rows"][1] - 4 * -np.log(np.float64(np.float32(1.0 - 1e-6)))) < 1e-9
    assert np.isfinite(o["acc"][3])


def test_absent_class_gives_nan(small, _native):
    """A class without rows: zero counts from the kernel, NaN (not 0) from evaluate()."""
    g = np.random.Generator(np.random.PCG64(9))
    p = _random_p(g, 40, 6)
    gt = g.integers(0, 5, 40).astype(np.int32)                  # class 5 never occurs
    o = _host(_native.cross_metrics(torch.from_numpy(p).to(DEV), gt=torch.from_numpy(gt).to(DEV), row_mse=torch.rand(40, device=DEV)))
    assert (o["class_sums"][5] == 0).all() and (o["confusion"][5] == 0).all() and (o["class_sums"][:5, 0] > 0).all()
    r = small.evaluate(seed=2, max_batches=1)                   # 8 rows of 8 classes: some class is absent
    absent = r["per_class_n"] == 0
    assert absent.any() and not absent.all()
    assert np.isnan(r["per_class_acc"][absent]).all() and np.isnan(r["per_class_image_mse"][absent]).all()
    assert np.isfinite(r["per_class_acc"][~absent]).all() and np.isfinite(r["per_class_image_mse"][~absent]).all()


def _poisoned(n, dtype, fill):
    """A buffer of n elements inside 64 elements of padding on each side, the padding holding `fill`."""
    big = torch.full((n + 128,), fill, dtype=dtype, device=DEV)
    return big, big[64:64 + n]


def test_accumulation_determinism_and_padding(_native):
    from imdbn.engine import native as N
    import ctypes as C
    g = np.random.Generator(np.random.PCG64(77))
    B, K = 256, 32
    p = _random_p(g, B, K)
    gt = g.integers(0, K, B).astype(np.int32)
    rm = g.random(B, dtype=np.float32)
    tp, tg, trm = torch.from_numpy(p).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(rm).to(DEV)
    one = _host(_native.cross_metrics(tp, gt=tg, row_mse=trm, npix=7))

    def three_calls():
        acc = torch.zeros(8, dtype=torch.float64, device=DEV)
        conf = torch.zeros(K, K, dtype=torch.int64, device=DEV)
        cls = torch.zeros(K, 3, dtype=torch.float64, device=DEV)
        for s, e in ((0, 100), (100, 200), (200, 256)):
            o = _native.cross_metrics(tp[s:e], gt=tg[s:e], row_mse=trm[s:e], npix=7, acc=acc, confusion=conf, class_sums=cls)
            assert o["acc"] is acc and o["confusion"] is conf and o["class_sums"] is cls
        torch.cuda.synchronize()
        return acc.cpu().numpy(), conf.cpu().numpy(), cls.cpu().numpy()

    a1, c1, s1 = three_calls()
    assert np.array_equal(a1[[0, 1, 2, 5, 6, 7]], one["acc"][[0, 1, 2, 5, 6, 7]]) and np.array_equal(c1, one["confusion"])
    assert np.array_equal(s1[:, :2], one["class_sums"][:, :2])
    _rel(a1[3], one["acc"][3], 1e-12, "ce_sum: 3 calls vs 1")
    _rel(a1[4], one["acc"][4], 1e-12, "mse_sum: 3 calls vs 1")
    a2, c2, s2 = three_calls()
    assert a1.tobytes() == a2.tobytes() and c1.tobytes() == c2.tobytes() and s1.tobytes() == s2.tobytes(), "two runs differ in a bit"
    again = _host(_native.cross_metrics(tp, gt=tg, row_mse=trm, npix=7))
    for k in one:
        assert one[k].tobytes() == again[k].tobytes(), f"{k}: two single calls differ in a bit"

    # NaN / sentinel padding around every output buffer is untouched (the raw entry: the buffers are the caller's)
    nan = float("nan")
    bufs = {"pred": _poisoned(B, torch.int32, -77), "gt": _poisoned(B, torch.int32, -77), "p_pred": _poisoned(B, torch.float32, nan),
            "p_true": _poisoned(B, torch.float32, nan), "rank": _poisoned(B, torch.int32, -77), "acc": _poisoned(8, torch.float64, nan),
            "confusion": _poisoned(K * K, torch.int64, -77), "class_sums": _poisoned(K * 3, torch.float64, nan)}
    for k in ("acc", "confusion", "class_sums"):
        bufs[k][1].zero_()
    out = N.CrossMetricsOut()
    for k, (_, inner) in bufs.items():
        setattr(out, k, inner.data_ptr())
    ws = torch.empty(4 * B + 256 + (128 << 10), dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rc = N.lib().imdbn_cross_metrics(C.c_void_p(tp.data_ptr()), K, B, K, None, 0, C.c_void_p(tg.data_ptr()), C.c_void_p(trm.data_ptr()), 7, 3,
                                     C.byref(out), C.c_void_p(ws.data_ptr()), ws.numel(), st)
    assert rc == 0
    torch.cuda.synchronize()
    for k, (big, inner) in bufs.items():
        pad = torch.cat([big[:64], big[64 + inner.numel():]])
        assert (torch.isnan(pad).all() if pad.is_floating_point() else (pad == -77).all()), f"the padding around {k} was written"
        assert np.array_equal(inner.cpu().numpy().reshape(one[k].shape), one[k]), k


def test_invalid_arguments_raise(_native):
    from imdbn.engine import EngineError
    g = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(EngineError, match="K = 1 "):
        _native.cross_metrics(torch.rand(4, 1, device=DEV), gt=g)
    with pytest.raises(EngineError, match="K = 257"):
        _native.cross_metrics(torch.rand(4, 257, device=DEV), gt=g)
    p = torch.rand(4, 8, device=DEV)
    with pytest.raises(EngineError, match="both"):
        _native.cross_metrics(p, y=torch.rand(4, 8, device=DEV), gt=g)
    with pytest.raises(EngineError, match="neither"):
        _native.cross_metrics(p)
    with pytest.raises(EngineError, match="topk = 0"):
        _native.cross_metrics(p, gt=g, topk=0)
    # an out-of-range gt entry raises nothing: the row is skipped and counted
    gt = torch.tensor([1, 8, 3, 0], dtype=torch.int32, device=DEV)
    o = _host(_native.cross_metrics(p, gt=gt, row_mse=torch.ones(4, device=DEV)))
    m = CO.metrics(p.cpu().numpy(), gt=gt.cpu().numpy(), row_mse=np.ones(4, np.float32))
    assert o["acc"][5] == 1 and o["acc"][0] == 3 and int(o["confusion"].sum()) == 3 and o["acc"][4] == 3
    assert o["rank"][1] == -1 and np.isnan(o["p_true"][1]) and o["gt"][1] == 8
    assert np.array_equal(o["rank"], m["rank"]) and np.array_equal(o["confusion"], m["confusion"])
    _rel(o["acc"][3], m["acc"][3], F_REL, "ce_sum with a skipped row")


def test_snapshot_against_the_reference(fx, small):
    from imdbn import engine as E
    m = small
    assert torch.equal(m.validation_images.cpu(), torch.from_numpy(fx["imgs"]))
    m.wandb_run = Run()
    tape = Tape(fx)
    try:
        with E.use_rng(E.ReplayRng(tape)):
            s = m._log_snapshots(fx.meta["epoch"], fx.meta["num"])
        run = m.wandb_run
    finally:
        m.wandb_run = None
    assert tape.done(), "not every recorded draw was consumed"
    assert list(s) == ["snap/image_mse", "confusion", "table", "pred", "gt"]
    assert np.array_equal(s["pred"], fx["cm_preds"]) and np.array_equal(s["gt"], fx["cm_y_true"])          # all 8 rows
    want = np.zeros((8, 8), np.int64)
    np.add.at(want, (fx["cm_y_true"], fx["cm_preds"]), 1)
    assert np.array_equal(s["confusion"], want) and s["confusion"].dtype == np.int64
    assert [row[:3] for row in s["table"]] == fx["table_int"].tolist() and all(len(row) == 5 for row in s["table"])
    err = np.abs(np.array([row[3:5] for row in s["table"]]) - fx["table_p"])
    print(f"p_pred / p_true vs the recording: max error {err.max():.3g} (tolerance {P_TOL:g})")
    assert err.max() <= P_TOL
    _rel(s["snap/image_mse"], fx["snap_image_mse"], 1e-4, "snap/image_mse")
    assert run.logged == [{"snap/image_mse": s["snap/image_mse"], "epoch": fx.meta["epoch"]}]


def _by_hand(m, seed, n_batches=3):
    """The per-batch outputs of _cross_reconstruct under PhiloxRng(seed), in evaluate()'s order; the draws they made."""
    from imdbn import engine as E
    from imdbn.utils import batches, rows_on_device
    out = []
    with E.use_rng(E.PhiloxRng(seed)) as rng:
        for b, (img, y) in enumerate(batches(m.val_loader)):
            if b >= n_batches:
                break
            img = rows_on_device(img, m.device)
            y = y.to(m.device).float()
            rec, p_y = m._cross_reconstruct(m.image_idbn.represent(img), y, steps=m.cross_steps)
            out.append((rec.cpu().numpy(), p_y.cpu().numpy(), img.cpu().numpy(), y.cpu().numpy()))
        return out, rng.offset


def test_evaluate_against_the_twin(small):
    from imdbn import engine as E
    from imdbn.utils import cross_eval as CE
    m = small
    assert [len(b[0]) for b in m.val_loader] == [8, 8, 5]
    hand, n_draws = _by_hand(m, 11)
    want = CO.evaluate(hand)
    E.manual_seed(123)
    E.get_rng().advance(17)
    r = m.evaluate(seed=11)
    assert E.get_rng().offset == 17, "evaluate(seed=...) moved the caller's draw counter"
    assert r["n"] == want["n"] == 21 and r["skipped"] == 0
    for k in ("pred", "gt", "rank", "confusion", "per_class_n"):
        assert np.array_equal(r[k], want[k]), k
    assert r["text_top1"] == want["text_top1"] and r["text_top3"] == want["text_top3"]
    assert np.array_equal(r["per_class_acc"], want["per_class_acc"], equal_nan=True)
    _rel(r["text_ce"], want["text_ce"], 1e-5, "text_ce")
    _rel(r["image_mse"], want["image_mse"], 1e-5, "image_mse")
    seen = want["per_class_n"] > 0
    _rel(r["per_class_image_mse"][seen], want["per_class_image_mse"][seen], 1e-5, "per-class image mse")
    assert np.abs(r["p_pred"] - want["p_pred"]).max() <= 1e-6 and np.abs(r["p_true"] - want["p_true"]).max() <= 1e-6
    assert r["confusion"].dtype == np.int64 and r["confusion"].shape == (8, 8)
    # no seed: the ambient source advances by the draws of three _cross_reconstruct calls
    m.evaluate()
    assert E.get_rng().offset == 17 + n_draws and n_draws > 0
    # max_batches
    two = m.evaluate(seed=11, max_batches=2)
    assert two["n"] == 16 and np.array_equal(two["pred"], r["pred"][:16]) and np.array_equal(two["confusion"], CO.evaluate(hand[:2])["confusion"])
    # the two routes to the per-row image error
    img, y = torch.from_numpy(hand[0][2]).to(DEV), torch.from_numpy(hand[0][3]).to(DEV)
    z = m.image_idbn.represent(img)
    assert CE.fused_decode_ok(m)
    with E.use_rng(E.PhiloxRng(11)):
        a, pa = CE.row_image_error(m, z, y, img, m.cross_steps, fused=True)
    with E.use_rng(E.PhiloxRng(11)):
        b, pb = CE.row_image_error(m, z, y, img, m.cross_steps, fused=False)
    assert torch.equal(pa, pb)
    _rel(a.sum().item(), b.sum().item(), 1e-5, "image error: prop_down_sqerr vs decoded rows")
    _rel(a.cpu().numpy(), CO.row_mse(hand[0][0], hand[0][2]), 1e-5, "row_mse vs the twin")
    # a wandb_run gets the four scalars
    m.wandb_run = Run()
    try:
        r2 = m.evaluate(seed=11)
        assert m.wandb_run.logged == [{"eval/" + k: r2[k] for k in ("text_top1", "text_top3", "text_ce", "image_mse")}]
        assert r2["text_ce"] == r["text_ce"] and r2["image_mse"] == r["image_mse"]            # bit-for-bit repeat
    finally:
        m.wandb_run = None
