"""GPU: imdbn_unit_moments (csrc/kernels_tuning.hpp) against the numpy moments of tests/tuning_oracle.py, and
``iDBN.unit_tuning`` end to end.

Exact cases: activations in {0, 1} and small-integer regressors make every sum an integer below 2^53 whatever its order, so all seven
accumulators must equal the oracle bit for bit.  Real-valued cases: every product is exact in double on both sides, so two summation
orders of the same m terms t differ by at most 2 m 2^-53 sum|t| (each order is within (m - 1) 2^-53 sum|t| of the true sum to first
order); that bound is derived, not measured, and the largest observed fraction of it is printed."""
import ctypes as C

import numpy as np
import pytest
import torch

import tuning_cases as Cs
import tuning_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOAT_KEYS = ("cls_sum", "cls_sumsq", "xa", "aa", "xx")


@pytest.fixture(scope="module", autouse=True)
def eng():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    yield E.get_hip_engine()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(eng, act, cls, K, x, acc=None):
    return eng.unit_moments(_dev(act) if isinstance(act, np.ndarray) else act, _dev(cls), K, _dev(x), acc)


def _host(o):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _assert_bits(got, want, what=""):
    for k in TO.KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes() or np.array_equal(g, w, equal_nan=True), (what, k)


def _assert_bound(got, want, act, cls, K, x, what):
    """|got - want| <= 2 m 2^-53 sum|t| per entry; counts exact.  Returns the largest observed fraction of the bound."""
    absm, terms, worst = TO.abs_moments(act, cls, K, x), TO.term_counts(want), 0.0
    for k in ("cls_count", "rows"):
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in FLOAT_KEYS:
        bound = 2.0 * terms[k] * 2.0 ** -53 * absm[k]
        err = np.abs(got[k] - want[k])
        assert (err <= bound).all(), (what, k, float(err.max()))
        frac = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
        worst = max(worst, float(frac.max()) if frac.size else 0.0)
    print(f"{what}: largest |error| / bound = {worst:.3g}")
    return worst


# ---- 1. exact cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,K,R", Cs.SHAPES)
def test_exact_shapes_are_bit_equal(eng, B, H, K, R):
    act, cls, x = Cs.make(B, H, K, R)
    _assert_bits(_host(_run(eng, act, cls, K, x)), TO.unit_moments(act, cls, K, x))


@pytest.mark.parametrize("layout", Cs.LAYOUTS)
def test_exact_layouts_are_bit_equal(eng, layout):
    B, H, K, R = Cs.LAYOUT_SHAPE
    act, cls, x = Cs.make(B, H, K, R, layout)
    want = TO.unit_moments(act, cls, K, x)
    got = _host(_run(eng, act, cls, K, x))
    _assert_bits(got, want, layout)
    skipped = {"skip_one": 1, "skip_all": B, "nan_regressor": 2}.get(layout, 0)
    assert got["rows"].tolist() == [B - skipped, skipped]
    if layout == "skip_all":                                           # only rows[1] changes
        assert all(not got[k].any() for k in TO.KEYS[:-1])


def test_all_rows_skipped_leaves_earlier_sums_alone(eng):
    B, H, K, R = Cs.LAYOUT_SHAPE
    act, cls, x = Cs.make(B, H, K, R)
    acc = _run(eng, act, cls, K, x)
    before = _host(acc)
    act2, cls2, x2 = Cs.make(B, H, K, R, "skip_all", seed=1)
    after = _host(_run(eng, act2, cls2, K, x2, acc))
    for k in TO.KEYS[:-1]:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert after["rows"].tolist() == [B, B]


# ---- 2. real-valued cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,K,R", Cs.SHAPES)
def test_real_valued_shapes_stay_within_the_sum_bound(eng, B, H, K, R):
    act, cls, x = Cs.make(B, H, K, R, exact=False)
    _assert_bound(_host(_run(eng, act, cls, K, x)), TO.unit_moments(act, cls, K, x), act, cls, K, x, f"B={B} H={H} K={K} R={R}")


# ---- 3. layout ------------------------------------------------------------------------------------------------------------------------
def test_a_column_offset_view_in_a_nan_parent_gives_the_contiguous_bits(eng):
    B, H, K, R = 300, 65, 33, 3
    act, cls, x = Cs.make(B, H, K, R, exact=False)
    want = _host(_run(eng, act, cls, K, x))
    parent = torch.full((B, H + 12), float("nan"), device=DEV)
    view = parent[:, 5:5 + H]
    view.copy_(_dev(act))
    assert view.stride() == (H + 12, 1) and not view.is_contiguous()
    got = _host(_run(eng, view, cls, K, x))
    for k in TO.KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert all(np.isfinite(got[k]).all() for k in FLOAT_KEYS)          # nothing beyond column H was read
    assert torch.isnan(parent[:, :5]).all() and torch.isnan(parent[:, 5 + H:]).all() and torch.equal(view, _dev(act))


def test_a_nan_activation_poisons_its_own_column_only(eng):
    B, H, K, R = 300, 200, 33, 3
    act, cls, x = Cs.make(B, H, K, R, exact=False)
    clean = _host(_run(eng, act, cls, K, x))
    j = 64
    act[17, j] = np.nan
    got = _host(_run(eng, act, cls, K, x))
    keep = np.arange(H) != j
    for k in ("cls_sum", "cls_sumsq", "xa"):
        assert got[k][:, keep].tobytes() == clean[k][:, keep].tobytes(), k
        assert np.isnan(got[k][:, j]).any()
    assert got["aa"][keep].tobytes() == clean["aa"][keep].tobytes() and np.isnan(got["aa"][j])
    assert np.isnan(got["cls_sum"][:, j]).sum() == 1 and np.isnan(got["xa"][:, j]).all()      # one class of that column, every regressor
    for k in ("xx", "cls_count", "rows"):
        assert got[k].tobytes() == clean[k].tobytes(), k


def test_workspace_contents_and_repeats_do_not_matter(eng):
    B, H, K, R = 4099, 200, 2, 3
    act, cls, x = Cs.make(B, H, K, R, exact=False)
    first = _host(_run(eng, act, cls, K, x))
    again = _host(_run(eng, act, cls, K, x))
    key = ("unit_moments", torch.device(DEV), torch.cuda.current_stream(DEV).cuda_stream)
    ws = eng._ws[key]
    ws.fill_(0xFF)                                                      # every double and float a NaN, every int32 -1
    poisoned = _host(_run(eng, act, cls, K, x))
    assert eng._ws[key] is ws
    for k in TO.KEYS:
        assert again[k].tobytes() == first[k].tobytes() and poisoned[k].tobytes() == first[k].tobytes(), k


@pytest.mark.parametrize("exact", [True, False])
def test_two_halves_equal_the_whole(eng, exact):
    B, H, K, R = 4099, 65, 33, 3
    act, cls, x = Cs.make(B, H, K, R, exact=exact)
    whole = _host(_run(eng, act, cls, K, x))
    h = 2048
    acc = _run(eng, act[:h], cls[:h], K, x[:h])
    halves = _host(_run(eng, act[h:], cls[h:], K, x[h:], acc))
    if exact:
        _assert_bits(halves, whole)
    else:
        _assert_bound(halves, whole, act, cls, K, x, "two halves against the whole")


def test_acc_of_another_shape_is_refused(eng):
    from imdbn.engine import EngineError
    act, cls, x = Cs.make(64, 64, 2, 3)
    acc = _run(eng, act, cls, 2, x)
    for bad in (dict(K=3), dict(x=x[:, :2])):
        with pytest.raises(EngineError, match="acc"):
            _run(eng, act, cls, bad.get("K", 2), bad.get("x", x), acc)
    with pytest.raises(EngineError, match="acc"):
        _run(eng, act, cls, 2, x, {**acc, "aa": acc["aa"].float()})
    with pytest.raises(EngineError, match="acc"):
        _run(eng, act, cls, 2, x, {**acc, "rows": acc["rows"].cpu()})


# ---- 4. bad arguments -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(eng):
    from imdbn.engine import native
    B, H, K, R = 64, 64, 2, 3
    act, cls, x = (_dev(t) for t in Cs.make(B, H, K, R))
    SENT = -12345.0
    acc = {"cls_sum": torch.full((1024, H), SENT, dtype=torch.float64, device=DEV), "cls_sumsq": torch.full((1024, H), SENT, dtype=torch.float64, device=DEV),
           "cls_count": torch.full((1024,), -7, dtype=torch.int64, device=DEV), "xa": torch.full((10, H), SENT, dtype=torch.float64, device=DEV),
           "aa": torch.full((H,), SENT, dtype=torch.float64, device=DEV), "xx": torch.full((10, 10), SENT, dtype=torch.float64, device=DEV),
           "rows": torch.full((2,), -7, dtype=torch.int64, device=DEV)}
    need = eng._lib.imdbn_unit_moments_ws_bytes(B, H, 1024, 8)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    x9 = torch.zeros(B, 9, device=DEV)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())

    def call(act=act, lda=H, B=B, H=H, cls=cls, K=K, x=x, ldx=R, R=R, ws_bytes=need, ws_t=ws, **null):
        a = {k: (None if null.get(k, False) else v) for k, v in acc.items()}
        rc = eng._lib.imdbn_unit_moments(p(act), lda, B, H, p(cls), K, p(x), ldx, R, p(a["cls_sum"]), p(a["cls_sumsq"]), p(a["cls_count"]),
                                         p(a["xa"]), p(a["aa"]), p(a["xx"]), p(a["rows"]), p(ws_t), ws_bytes, None)
        buf = C.create_string_buffer(512)
        eng._lib.imdbn_last_error(buf, 512)
        return rc, buf.value.decode()

    E_INVALID = -1                                                      # IMDBN_E_INVALID: the library's bad-argument code
    bad = {"R = 9": dict(x=x9, ldx=9, R=9), "K = 1025": dict(K=1025), "K = 0": dict(K=0), "K = -1": dict(K=-1), "lda 63": dict(lda=H - 1),
           "workspace": dict(ws_bytes=eng._lib.imdbn_unit_moments_ws_bytes(B, H, K, R) - 1), "workspace ": dict(ws_t=None),
           "cls_sum": dict(cls_sum=True), "cls_sumsq": dict(cls_sumsq=True), "cls_count": dict(cls_count=True), "xa": dict(xa=True),
           "aa": dict(aa=True), "xx": dict(xx=True), "rows": dict(rows=True), "B = 0": dict(B=0), "H = 0": dict(H=0), "ldx 2": dict(ldx=R - 1),
           "null x": dict(x=None), "null act": dict(act=None), "without cls": dict(cls=None)}
    for name, kw in bad.items():
        rc, msg = call(**kw)
        assert rc == E_INVALID and msg.startswith("unit_moments:") and name.strip() in msg, (name, rc, msg)
    torch.cuda.synchronize()
    for k, t in acc.items():
        assert bool((t == (-7 if t.dtype == torch.int64 else SENT)).all()), k
    rc, msg = call()                                                    # and the same call with nothing wrong goes through
    assert rc == 0, msg
    torch.cuda.synchronize()
    want = TO.unit_moments(act.cpu().numpy(), cls.cpu().numpy(), K, x.cpu().numpy())
    assert np.array_equal(acc["xa"][:R + 1].cpu().numpy(), want["xa"] + SENT) and acc["rows"].tolist() == [B - 7, -7]
    assert native.ABI_VERSION == eng._lib.imdbn_version() == 4


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------
def test_idbn_unit_tuning_end_to_end(eng, tmp_path, monkeypatch):
    from imdbn import engine as E
    from imdbn.datasets import create_dataloaders_uniform
    from imdbn.models import iDBN
    from imdbn.utils import unit_tuning as UT
    g = np.random.default_rng(2)
    n, K = 3000, 6
    lab = (np.arange(n) % K) + 1
    img = (g.random((n, 10, 10)) < (lab[:, None, None] / 10.0)).astype(np.float32)
    img[:, 0, 0] = 1.0
    np.savez(tmp_path / "stimuli.npz", D=img, N_list=lab, cumArea_list=img.reshape(n, -1).sum(1) * (1.0 + g.random(n)),
             CH_list=(1.0 + g.random(n)).astype(np.float32))
    monkeypatch.chdir(tmp_path)
    tr, va, _ = create_dataloaders_uniform(path2data=str(tmp_path), data_name="stimuli.npz", batch_size=64, device=DEV)
    params = {"LEARNING_RATE": 0.1, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95, "LEARNING_RATE_DYNAMIC": True, "CD": 1}
    torch.manual_seed(1)
    E.manual_seed(1)
    m = iDBN([100, 48, 24], params, tr, va, torch.device(DEV))
    X = torch.cat([x for x, _ in m.val_loader]).reshape(-1, 100).float()
    assert X.size(0) == 300
    emb = m.represent(X).cpu().numpy()
    f = m.features
    labv, area = f["Labels"].numpy(), f["Cumulative Area"].numpy()
    cls = (labv - labv.min()).astype(np.int32)
    x = torch.log(torch.from_numpy(np.stack([labv, area], 1).astype(np.float32)).to(DEV)).cpu().numpy()
    want = UT.tuning_from_moments({k: torch.from_numpy(v) for k, v in TO.unit_moments(emb, cls, K, x).items()},
                                  class_values=torch.log(torch.arange(1, K + 1, dtype=torch.float64)), names=["labels", "cum_area"])
    ind = TO.statistics(emb, cls, K, x, class_values=np.log(np.arange(1, K + 1, dtype=np.float64)))
    assert not ind["degenerate"].any() and ind["cond"] <= 1e3          # what the tolerance presumes
    tol = 64.0 * ind["cond"] * 300 * 2.0 ** -53
    got = m.unit_tuning()
    assert got["n"] == 300 and got["n_skipped"] == 0 and got["class_labels"].tolist() == list(range(1, K + 1))
    for k in ("mean", "var", "depth", "beta", "beta_std", "r2", "eta2", "centre", "width"):
        gk, wk = got[k].numpy(), want[k].numpy()
        err = np.abs(gk - wk) - (tol * np.abs(wk) + tol)
        print(f"{k}: largest |error| {float(np.abs(gk - wk).max()):.3g} (tolerance {tol:.3g} relative and absolute)")
        assert (err <= 0).all(), k
    for k in ("preferred", "count", "degenerate", "selective"):
        assert torch.equal(got[k], want[k]), k
    assert got["rank"] == want["rank"] == 2
    chunked = m.unit_tuning(chunk=77)
    assert torch.equal(chunked["preferred"], got["preferred"]) and torch.equal(chunked["count"], got["count"])
