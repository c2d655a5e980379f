"""CPU-only: unit tuning (imdbn/utils/unit_tuning.py) -- the ABI surface of imdbn_unit_moments, tuning_from_moments on
the double's moments against the independent statistics of tests/tuning_oracle.py, the edge cases, and the whole analysis through
the models with the engine double."""
import os
import re

import numpy as np
import pytest
import torch

import tuning_oracle as TO
from imdbn import engine as E
from imdbn.engine import native
from imdbn.utils import unit_tuning as UT
from tuning_engine_double import TuningOracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = ("mean", "var", "depth", "beta", "beta_std", "r2", "eta2", "centre", "width")
EXACT = ("preferred", "count", "degenerate", "selective")


def _moments(act, cls, K, x):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    return TuningOracleEngine().unit_moments(t(act), t(cls), K, t(x))


def _tol(want):
    """CPU check 2: relative 64 cond(C_xx) n 2^-53 plus the same absolute floor (the first-order bound of the normal equations;
    both sides are float64)."""
    return 64.0 * want["cond"] * want["n"] * 2.0 ** -53


def _compare(got, want, tol, keys=REAL):
    for k in keys:
        g, w = got[k].numpy(), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), k
        err = np.abs(g - w) - (tol * np.abs(w) + tol)
        assert not (np.nan_to_num(err, nan=-1.0) > 0).any(), (k, float(np.nanmax(err)), tol)
    for k in EXACT:
        assert np.array_equal(got[k].numpy(), np.asarray(want[k])), k
    assert got["rank"] == want["rank"] and got["n"] == want["n"] and got["n_skipped"] == want["n_skipped"]


def _draw(N, H, K, R, seed=0):
    """Regressors like log features (mean 3, unit spread, mildly correlated), classes, and sigmoid units driven by both."""
    g = np.random.default_rng([seed, N, H, K, R])
    cls = g.integers(0, K, size=N).astype(np.int32)
    x = (3.0 + g.standard_normal((N, R)) + 0.3 * g.standard_normal((N, 1))).astype(np.float32) if R else None
    drive = g.standard_normal((N, H)) + 0.7 * g.standard_normal((K, H))[cls]
    if R:
        drive = drive + (x - 3.0) @ g.standard_normal((R, H))
    return (1.0 / (1.0 + np.exp(-drive))).astype(np.float32), cls, x


# ---- 1. ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_both_symbols():
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym in ("imdbn_unit_moments", "imdbn_unit_moments_ws_bytes"):
        assert re.search(r"\b" + sym + r"\s*\(", code), sym
        assert sym in native.SIGNATURES
        assert hasattr(native.lib(), sym)
    assert re.search(r"#define IMDBN_ABI_VERSION 4\b", src) and native.ABI_VERSION == 4
    assert len(native.SIGNATURES["imdbn_unit_moments"][1]) == 19 and len(native.SIGNATURES["imdbn_unit_moments_ws_bytes"][1]) == 4


def test_workspace_size_helper():
    ws = native.lib().imdbn_unit_moments_ws_bytes
    assert ws(10000, 1500, 32, 2) > 0 and ws(10000, 1500, 32, 2) % 256 == 0
    assert ws(10000, 1500, 32, 2) <= 8 << 20                           # a few MB next to the 60 MB of activations
    for bad in ((0, 10, 1, 0), (10, 0, 1, 0), (10, 10, 1025, 0), (10, 10, -1, 0), (10, 10, 1, 9), (10, 10, 1, -1)):
        assert ws(*bad) == 0, bad
    assert ws(4099, 64, 0, 0) == ws(4099, 64, 1, 0)                    # no classes: one class of all rows


def test_the_double_follows_the_engine():
    import inspect
    from imdbn.engine.hip_engine import HipEngine
    e, d = (list(inspect.signature(getattr(c, "unit_moments")).parameters.values()) for c in (HipEngine, TuningOracleEngine))
    assert [(p.name, p.default) for p in e] == [(p.name, p.default) for p in d]
    assert [p.name for p in e] == ["self", "act", "cls", "n_classes", "x", "acc"]


# ---- 2. tuning_from_moments against the independent statistics ---------------------------------------------------------------------
@pytest.mark.parametrize("N", [40, 1000])
@pytest.mark.parametrize("H", [1, 7, 65])
@pytest.mark.parametrize("K", [1, 2, 9, 33])
@pytest.mark.parametrize("R", [0, 1, 2, 4])
def test_statistics_match_the_independent_oracle(N, H, K, R):
    act, cls, x = _draw(N, H, K, R)
    want = TO.statistics(act, cls, K, x)
    assert not want["degenerate"].any() and want["cond"] <= 1e3        # what the tolerance below presumes, on the oracle side
    got = UT.tuning_from_moments(_moments(act, cls, K, x))
    _compare(got, want, _tol(want))
    assert got["names"] == [f"x{r + 1}" for r in range(R)]
    for k in ("eta2", "r2"):
        v = got[k].numpy()
        assert ((v > -1e-9) & (v < 1 + 1e-9)).all(), k


# ---- 3. edge cases --------------------------------------------------------------------------------------------------------------------
def test_empty_class_is_nan_and_never_preferred():
    act, cls, x = _draw(200, 7, 5, 2, seed=1)
    cls[cls == 3] = 1
    act[:, 2] = np.where(cls == 4, 0.9, 0.1)                            # and a unit whose maximum is the LAST class
    got = UT.tuning_from_moments(_moments(act, cls, 5, x))
    assert got["count"][3] == 0 and torch.isnan(got["mean"][3]).all() and torch.isnan(got["var"][3]).all()
    assert not (got["preferred"] == 3).any() and got["preferred"][2] == 4
    _compare(got, TO.statistics(act, cls, 5, x), 64 * 10 * 200 * 2.0 ** -53)


def test_constant_unit_is_degenerate_and_its_neighbours_are_untouched():
    act, cls, x = _draw(300, 9, 4, 2, seed=2)
    ref = UT.tuning_from_moments(_moments(act, cls, 4, x))
    act2 = act.copy(); act2[:, 4] = 0.37
    got = UT.tuning_from_moments(_moments(act2, cls, 4, x))
    assert got["degenerate"].tolist() == [j == 4 for j in range(9)] and not got["selective"][4]
    for k in ("eta2", "r2", "centre", "width"):
        assert torch.isnan(got[k][4]), k
    assert torch.isnan(got["beta_std"][:, 4]).all()
    keep = [j for j in range(9) if j != 4]
    for k in REAL + ("preferred", "degenerate", "selective"):
        assert torch.equal(got[k][..., keep], ref[k][..., keep]), k
    assert torch.equal(got["count"], ref["count"])


def test_poisoned_unit_is_degenerate():
    act, cls, x = _draw(100, 5, 3, 1, seed=3)
    act[17, 1] = np.nan
    got = UT.tuning_from_moments(_moments(act, cls, 3, x))
    assert got["degenerate"].tolist() == [False, True, False, False, False]
    assert torch.isnan(got["r2"][1]) and torch.isfinite(got["r2"][[0, 2, 3, 4]]).all()


def test_collinear_regressors_give_a_deficient_rank_and_finite_r2():
    act, cls, x = _draw(400, 6, 4, 2, seed=4)
    x[:, 1] = 2.0 * x[:, 0]
    got = UT.tuning_from_moments(_moments(act, cls, 4, x))
    want = TO.statistics(act, cls, 4, x)
    assert got["rank"] == want["rank"] == 1 < 2
    assert torch.isfinite(got["r2"]).all() and torch.isfinite(got["beta"]).all()
    one = UT.tuning_from_moments(_moments(act, cls, 4, x[:, :1]))      # the fit is that of one regressor
    assert np.allclose(got["r2"].numpy(), one["r2"].numpy(), rtol=0, atol=1e-9)
    assert np.allclose(got["r2"].numpy(), want["r2"], rtol=0, atol=1e-9)


def test_out_of_range_classes_and_non_positive_features_are_skipped_and_counted():
    act, cls, x = _draw(120, 5, 4, 2, seed=5)
    cls[[3, 50]] = [-1, 4]
    raw = np.exp(x); raw[[7, 50, 99], [0, 1, 1]] = [0.0, -2.0, 0.0]
    with np.errstate(divide="ignore", invalid="ignore"):
        logx = np.log(raw.astype(np.float32))
    m = _moments(act, cls, 4, logx)
    assert m["rows"].tolist() == [116, 4]                               # rows 3, 7, 50, 99
    keep = np.ones(120, dtype=bool); keep[[3, 7, 50, 99]] = False
    clean = _moments(act[keep], cls[keep], 4, logx[keep])
    for k in TO.KEYS[:-1]:                                              # the same rows left the curves and the regression
        assert torch.allclose(m[k].double(), clean[k].double(), rtol=1e-13, atol=0), k
    assert int(m["cls_count"].sum()) == 116 and m["xx"][0, 0] == 116
    got = UT.tuning_from_moments(m)
    assert got["n"] == 116 and got["n_skipped"] == 4
    _compare(got, TO.statistics(act, cls, 4, logx), 64 * 10 * 120 * 2.0 ** -53)


def test_planted_structure_is_recovered():
    g = np.random.default_rng(11)
    N, K = 4000, 16
    num = g.integers(1, K + 1, size=N)
    area = np.exp(g.normal(4.0, 0.5, size=N))                          # independent of number
    ln, la = np.log(num), np.log(area)
    sig = lambda t: 1.0 / (1.0 + np.exp(-t))
    number = np.stack([sig(w * (ln - ln.mean()) + 0.3 * g.standard_normal(N)) for w in (1.5, -2.0, 3.0)], 1)
    areal = np.stack([sig(w * (la - la.mean()) + 0.3 * g.standard_normal(N)) for w in (3.0, -4.0)], 1)
    prefs = [2, 5, 9, 12]                                              # Gaussian tuning on the log axis around class p
    tuned = np.stack([np.exp(-0.5 * ((ln - np.log(p + 1)) / 0.25) ** 2) + 0.02 * g.standard_normal(N) for p in prefs], 1)
    act = np.concatenate([number, areal, tuned], 1).astype(np.float32)
    x = np.stack([ln, la], 1).astype(np.float32)
    got = UT.tuning_from_moments(_moments(act, (num - 1).astype(np.int32), K, x), names=["labels", "cum_area"])
    assert got["selective"][:3].all() and not got["selective"][3:5].any()
    assert got["preferred"][5:].tolist() == prefs
    assert np.allclose(got["centre"][5:].numpy(), np.log(np.array(prefs) + 1.0), atol=0.1)
    assert (got["beta_std"][0, :3].abs() > 0.5).all() and (got["beta_std"][1, 3:5].abs() > 0.5).all()
    assert got["preferred"][0] == K - 1 and got["preferred"][1] == 0    # monotone units peak at the ends
    pop = UT.population_curve({**got})
    assert pop.shape == (K, K) and torch.isnan(pop[1]).all() and torch.allclose(pop[K - 1], got["mean"][:, [0, 2]].mean(1))


# ---- 4. the whole analysis through the models and the double --------------------------------------------------------------------------
PARAMS = {"LEARNING_RATE": 0.1, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95, "LEARNING_RATE_DYNAMIC": True, "CD": 1,
          "CROSS_GIBBS_STEPS": 3, "JOINT_AUX_COND_STEPS": 10}


def _archive(path, n=480, side=8, K=6):
    g = np.random.default_rng(1)
    lab = (np.arange(n) % K) + 2                                       # numerosities 2 .. K + 1: class 0 is label 2
    img = (g.random((n, side, side)) < (lab[:, None, None] / 12.0)).astype(np.float32)
    img[:, 0, 0] = 1.0                                                 # no empty image: the area is positive
    np.savez(path / "stimuli.npz", D=img, N_list=lab, cumArea_list=img.reshape(n, -1).sum(1), CH_list=(1.0 + g.random(n)).astype(np.float32),
             density=g.random(n).astype(np.float32))


@pytest.fixture()
def loaders(tmp_path, monkeypatch):
    from imdbn.datasets import create_dataloaders_uniform
    _archive(tmp_path)
    monkeypatch.chdir(tmp_path)
    E.set_engine_for_testing(TuningOracleEngine())
    yield create_dataloaders_uniform(path2data=str(tmp_path), data_name="stimuli.npz", batch_size=16, device="cpu")
    E.set_engine_for_testing(None)


def _idbn(loaders, sizes=(64, 20, 11), seed=5):
    from imdbn.models import iDBN
    torch.manual_seed(seed)
    return iDBN(list(sizes), PARAMS, loaders[0], loaders[1], torch.device("cpu"))


def _val(model):
    xs, _ = zip(*list(model.val_loader))
    X = torch.cat(xs).float().reshape(len(model.val_loader.dataset), -1)
    f = model.features
    return X, f["Labels"].numpy(), f["Cumulative Area"].numpy()


@pytest.mark.parametrize("upto", [None, 1])
def test_idbn_unit_tuning_equals_the_oracle_on_represent(loaders, upto):
    m = _idbn(loaders)
    X, lab, area = _val(m)
    emb = (m.represent(X) if upto is None else m.represent(X, upto_layer=upto)).numpy()
    cls = (lab - lab.min()).astype(np.int32)
    K = int(cls.max()) + 1
    x = torch.log(torch.from_numpy(np.stack([lab, area], 1).astype(np.float32))).numpy()   # the fp32 log the analysis takes
    labels = np.arange(K) + int(lab.min())
    want = TO.statistics(emb, cls, K, x, class_values=np.log(labels.astype(np.float64)))
    assert not want["degenerate"].any() and want["cond"] <= 1e3
    got = m.unit_tuning(upto_layer=upto)
    assert got["mean"].shape == (K, emb.shape[1]) and got["class_labels"].tolist() == labels.tolist() and labels[0] == 2
    assert got["names"] == ["labels", "cum_area"] and got["n"] == len(lab) and got["n_skipped"] == 0
    _compare(got, want, _tol(want))
    # chunks of 7 rows: the same accumulators within the bound of two summation orders, so the same statistics within the tolerance
    _compare(m.unit_tuning(upto_layer=upto, chunk=7), want, _tol(want))
    three = m.unit_tuning(upto_layer=upto, regressors=("labels", "cum_area", "convex_hull"), log=False, n_classes=K - 1)
    assert three["beta"].shape[0] == 4 and three["n_skipped"] == int((cls == K - 1).sum()) and three["mean"].shape[0] == K - 1


def test_chunked_moments_stay_within_the_sum_bound(loaders):
    m = _idbn(loaders)
    X, lab, area = _val(m)
    emb = m.represent(X)
    cls = torch.from_numpy((lab - lab.min()).astype(np.int32))
    x = torch.log(torch.from_numpy(np.stack([lab, area], 1).astype(np.float32)))
    K = int(cls.max()) + 1
    eng = TuningOracleEngine()
    one, acc = eng.unit_moments(emb, cls, K, x), None
    for i in range(0, emb.size(0), 7):
        acc = eng.unit_moments(emb[i:i + 7], cls[i:i + 7], K, x[i:i + 7], acc)
    absm = TO.abs_moments(emb.numpy(), cls.numpy(), K, x.numpy())
    terms = TO.term_counts({k: v.numpy() for k, v in one.items()})
    for k in ("cls_sum", "cls_sumsq", "xa", "aa", "xx"):
        bound = 2.0 * terms[k] * 2.0 ** -53 * absm[k]
        assert (np.abs(acc[k].numpy() - one[k].numpy()) <= bound).all(), k
    assert torch.equal(acc["cls_count"], one["cls_count"]) and torch.equal(acc["rows"], one["rows"])
    with pytest.raises(ValueError):
        eng.unit_moments(emb, cls, K + 1, x, acc)


def test_imdbn_unit_tuning_joint_and_image_layers(loaders):
    from imdbn.models import iMDBN
    torch.manual_seed(3)
    m = iMDBN([64, 20], 12, params=PARAMS, dataloader=loaders[0], val_loader=loaders[1], device=torch.device("cpu"), num_labels=6)
    embeds = torch.cat([m.represent((img, lab)) for img, lab in m.val_loader]).numpy()
    X, lab, area = _val(m.image_idbn)
    cls = (lab - lab.min()).astype(np.int32)
    x = torch.log(torch.from_numpy(np.stack([lab, area], 1).astype(np.float32))).numpy()   # the fp32 log the analysis takes
    values = np.log(np.arange(6) + 2.0)
    want = TO.statistics(embeds, cls, 6, x, class_values=values)
    _compare(m.unit_tuning(), want, _tol(want))
    want = TO.statistics(m.image_idbn.represent(X, upto_layer=1).numpy(), cls, 6, x, class_values=values)
    _compare(m.unit_tuning(joint=False, upto_layer=1), want, _tol(want))


def test_logging_sends_scalars_only(loaders):
    m = _idbn(loaders)
    sent = []
    run = type("Run", (), {"log": lambda self, payload: sent.append(payload)})()
    res = UT.log_unit_tuning(m, epoch=3, wandb_run=run, r2_min=0.0, beta_min=0.0, beta_max=float("inf"))
    assert len(sent) == 1 and sent[0] is res["scalars"] and sent[0]["epoch"] == 3
    assert all(isinstance(v, (int, float)) for v in sent[0].values())
    H = res["r2"].numel()
    assert sent[0]["tuning/top/n_selective"] == H and sent[0]["tuning/top/frac_selective"] == 1.0       # thresholds wide open
    hist = [sent[0][f"tuning/top/preferred/{lab}"] for lab in range(2, 8)]
    assert hist == torch.bincount(res["preferred"], minlength=6).tolist() and sum(hist) == H
    assert abs(sent[0]["tuning/top/r2_mean"] - float(res["r2"].mean())) < 1e-15


def test_a_model_without_features_raises(loaders):
    m = _idbn(loaders)
    m.features = None
    with pytest.raises(ValueError, match="features"):
        m.unit_tuning()
    m = _idbn(loaders)
    with pytest.raises(ValueError, match="no_such"):
        m.unit_tuning(regressors=("labels", "no_such"))


def test_the_pickle_of_a_model_is_untouched_by_the_analysis(loaders):
    import pickle
    a, b = _idbn(loaders), _idbn(loaders)                               # built the same way; only b runs the analysis
    dump = lambda m: pickle.dumps({"layers": m.layers, "params": m.params})
    keys, raw = set(vars(b)), dump(b)
    b.unit_tuning()
    assert set(vars(b)) == keys and dump(b) == raw and "unit_tuning" not in str(b.params)
    assert b.params == a.params and [sorted(vars(r)) for r in b.layers] == [sorted(vars(r)) for r in a.layers]
    for ra, rb in zip(pickle.loads(dump(a))["layers"], pickle.loads(dump(b))["layers"]):
        assert all(torch.equal(p, q) for p, q in zip(ra.state_dict().values(), rb.state_dict().values()))
