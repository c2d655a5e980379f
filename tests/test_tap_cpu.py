"""CPU-only: the float64 reference and the fp32 twin of the TAP arithmetic (tests/tap_oracle.py) against first principles, and the
host logic of imdbn.utils.tap / RBM.train_epoch_tap / iDBN.train through the engine double (tests/tap_engine_double.py).  No claim
about the kernels is made here -- those are tested on the GPU in test_tap_gpu.py."""
import pickle

import numpy as np
import pytest
import torch

import tap_cases as Ck
import tap_oracle as Tt
from imdbn import engine as E
from oracle_engine import OracleEngine
from tap_engine_double import TapOracleEngine

F32, F64 = np.float32, np.float64
SIX = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")


# ---- 1. W = 0 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_without_weights_one_undamped_iteration_is_exact(order):
    _, a, c = Ck.params(12, 7, 0.3, 0)
    W = np.zeros((12, 7), F32)
    mv0 = Ck.starts(3, 12, 5)
    mv, mh, _ = Tt.iterate(W, a, c, mv0, np.full((3, 7), 0.5), 1, 0.0, order, F64)
    assert np.abs(mv - Tt.sigmoid(a.astype(F64))).max() <= 1e-15 and np.abs(mh - Tt.sigmoid(c.astype(F64))).max() <= 1e-15
    want = np.logaddexp(0, a.astype(F64)).sum() + np.logaddexp(0, c.astype(F64)).sum()
    got = -Tt.gamma(W, a, c, mv, mh, order)
    assert np.abs(got - want).max() <= 1e-12 and abs(Tt.log_z_enumerated(W, a, c) - want) <= 1e-12


# ---- 2. the gradient identity ---------------------------------------------------------------------------------------------------
def test_the_derivative_of_the_fixed_point_free_energy_is_the_negative_statistic():
    """float64 weights throughout (W2 = W W exactly): d(-Gamma*) / dW_ij = mv_i mh_j + W_ij cv_i ch_j at the fixed point."""
    W, a, c = (x.astype(F64) for x in Ck.params(12, 7, 0.3, 0))

    def fixed(Wx):
        mv, mh = np.full((1, 12), 0.5), np.full((1, 7), 0.5)
        W2 = Wx * Wx
        for _ in range(2000):
            mh = 0.5 * mh + 0.5 * Tt.sigmoid(c + mv @ Wx - (mh - 0.5) * ((mv - mv * mv) @ W2))
            mv = 0.5 * mv + 0.5 * Tt.sigmoid(a + mh @ Wx.T - (mv - 0.5) * ((mh - mh * mh) @ W2.T))
        g = (Tt.entropy(mv).sum() + Tt.entropy(mh).sum() - mv @ a - mh @ c - (mv @ Wx) @ mh.T
             - 0.5 * ((mv - mv * mv) @ W2) @ (mh - mh * mh).T)
        return -float(np.ravel(g)[0]), mv[0], mh[0]

    _, mv, mh = fixed(W)
    worst = 0.0
    for i, j in ((0, 0), (3, 5), (11, 6), (7, 2)):
        Wp, Wm = W.copy(), W.copy()
        Wp[i, j] += 1e-6
        Wm[i, j] -= 1e-6
        fd = (fixed(Wp)[0] - fixed(Wm)[0]) / 2e-6
        want = mv[i] * mh[j] + W[i, j] * (mv[i] - mv[i] ** 2) * (mh[j] - mh[j] ** 2)
        worst = max(worst, abs(fd - want))
    print(f"largest |central difference - statistic| {worst:.3g}")
    assert worst <= 1e-7


# ---- 3. calibration ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", Ck.SMALL_SEEDS)
@pytest.mark.parametrize("V,H,s", Ck.SMALL)
def test_order_two_is_ten_times_closer_to_log_z_than_naive_mean_field(V, H, s, seed):
    W, a, c = Ck.params(V, H, s, seed)
    log_z = Tt.log_z_enumerated(W, a, c)
    val = {}
    for order in (1, 2):
        f, res, _, _ = Tt.free_energy_fixed_point(W, a, c, Ck.starts(8, V, 100 + seed), 200, 0.5, order)
        assert res.max() < 1e-12, (order, res.max())
        assert f.max() - f.min() <= 1e-12
        val[order] = float(f[0])
    err1, err2 = log_z - val[1], abs(log_z - val[2])
    print(f"({V}, {H}, {s}) seed {seed}: log Z {log_z:.6f}, err1 {err1:.3g}, err2 {err2:.3g}, ratio {err2 / err1:.3g}")
    assert err1 > 0 and err2 < 0.1 * err1


# ---- the twin against the reference (what the GPU bound of tap_step is built from) ---------------------------------------
def test_the_fp32_twin_follows_the_reference_within_the_derived_bound():
    k = Ck.case(67, 33, 5)
    for order in (1, 2):
        mv, mh, res, dmv, dmh, rb = Tt.iterate_bounded(k["W"], k["a"], k["c"], k["mv"], k["mh"], 3, 0.5, order)
        tv, th, tres = Tt.iterate(k["W"], k["a"], k["c"], k["mv"], k["mh"], 3, 0.5, order, F32)
        assert tv.dtype == F32 and (np.abs(tv - mv) <= dmv).all() and (np.abs(th - mh) <= dmh).all()
        assert (np.abs(tres - res) <= rb).all() and dmv.max() < 1e-4


# ---- 4. host logic through the double ---------------------------------------------------------------------------------------------
@pytest.fixture
def double():
    eng = TapOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)


def _on_cpu(r, W=None, a=None, c=None):
    r.to("cpu")
    r.W.data = r.W.data.contiguous() if W is None else torch.from_numpy(W.copy())
    if a is not None:
        r.vis_bias.data, r.hid_bias.data = torch.from_numpy(a.copy()), torch.from_numpy(c.copy())
    r.W_m, r.hb_m, r.vb_m = torch.zeros_like(r.W.data), torch.zeros_like(r.hid_bias.data), torch.zeros_like(r.vis_bias.data)
    return r


def _rbm(k, groups=None):
    from imdbn.models import RBM
    return _on_cpu(RBM(k["V"], k["H"], Ck.LR, Ck.WEIGHT_DECAY, Ck.MOM, softmax_groups=groups), k["W"], k["a"], k["c"])


def _same(x, y):
    return all(torch.equal(getattr(x, n).data if n in SIX[:3] else getattr(x, n), getattr(y, n).data if n in SIX[:3] else getattr(y, n)) for n in SIX)


def test_train_epoch_tap_creates_keeps_and_recreates_its_magnetisations(double):
    k = Ck.case(67, 33, 5)
    r, x = _rbm(k), torch.from_numpy(k["data"])
    l0 = r.train_epoch_tap(x, 0, 10)
    assert [c[0] for c in double.calls] == ["forward", "tap_step"] and double.calls[-1] == ("tap_step", (5, 67), 3, 0.5, 2, True)
    mv, mh = r._tap_mv, r._tap_mh
    assert mv.shape == (5, 67) and mh.shape == (5, 33) and mv.data_ptr() != x.data_ptr()
    # by hand: the first magnetisations are the batch and its H+
    h, eng = _rbm(k), TapOracleEngine()
    hv = x.clone()
    hh = eng.forward(h, x).clone()
    lr, mom = h._lr_mom(0)
    want = eng.tap_step(h, x, hv, hh, lr, mom, 3)
    assert torch.equal(l0, want) and _same(r, h) and torch.equal(mv, hv) and torch.equal(mh, hh)
    # a second call keeps them; its settings reach the engine
    l1 = r.train_epoch_tap(x, 7, 10, n_iters=1, damp=0.25, order=1, monitor=False)
    assert l1 is None and r._tap_mv is mv and double.calls[-1] == ("tap_step", (5, 67), 1, 0.25, 1, False)
    lr, mom = h._lr_mom(7)
    eng.tap_step(h, x, hv, hh, lr, mom, 1, damp=0.25, order=1, monitor=False)
    assert _same(r, h) and torch.equal(mv, hv)
    # another batch size: created again
    r.train_epoch_tap(x[:2], 7, 10)
    assert r._tap_mv is not mv and r._tap_mv.shape == (2, 67) and r._tap_mh.shape == (2, 33)


def test_the_pickle_drops_the_magnetisations(double, tmp_path):
    k = Ck.case(67, 33, 5)
    r = _rbm(k)
    r.train_epoch_tap(torch.from_numpy(k["data"]), 0, 10)
    assert not {"_tap_mv", "_tap_mh", "_imdbn_desc"} & set(r.__getstate__())
    r2 = pickle.loads(pickle.dumps(r))
    assert "_tap_mv" not in r2.__dict__ and torch.equal(r2.W.data, r.W.data)


def test_refusals(double, monkeypatch):
    from imdbn.models import GaussianRBM
    from imdbn.utils import tap
    k = Ck.case(67, 33, 5)
    x = torch.from_numpy(k["data"])
    with pytest.raises(ValueError):
        _rbm(k, groups=[(60, 67)]).train_epoch_tap(x, 0, 1)
    with pytest.raises(ValueError):
        tap.tap_log_partition(_rbm(k, groups=[(60, 67)]))
    g = GaussianRBM(67, 33, 0.01, 0.0, 0.5)
    with pytest.raises(ValueError):
        tap.train_epoch_tap(g, x, 0, 1)
    with pytest.raises(ValueError):
        tap.tap_log_partition(g)
    for bad in (dict(order=3), dict(damp=1.0), dict(n_iters=-1)):
        with pytest.raises(ValueError):
            _rbm(k).train_epoch_tap(x, 0, 1, **bad)
    for bad in ({"TAP": True, "PERSISTENT": True}, {"TAP": True, "CENTERED": 0.1}, {"TAP": {"iters": 2}}):
        with pytest.raises(ValueError):
            tap.tap_params(bad)
    assert tap.tap_params({}) is None and tap.tap_params({"TAP": True}) == (3, 2, 0.5)
    assert tap.tap_params({"TAP": {"n_iters": 5, "order": 1}}) == (5, 1, 0.5)
    assert not double.calls
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        _rbm(k).train_epoch_tap(x, 0, 1)


def test_tap_log_partition_on_the_double_meets_the_enumeration(double):
    from imdbn.utils import tap
    W, a, c = Ck.params(12, 7, 0.3, 1)
    k = dict(V=12, H=7, W=W, a=a, c=c)
    r = _rbm(k)
    res = r.log_partition_tap(n_starts=4, max_iters=400, check_every=50, tol=1e-6)
    its = [c for c in double.calls if c[0] == "tap_iterate"]
    assert res["converged"] and res["iters"] == 50 * len(its) and all(c[1:] == ((4, 12), 50, 0.5, 2) for c in its)
    assert res["per_start"].dtype == torch.float64 and res["per_start"].shape == (4,) and res["log_z"] == float(res["per_start"].max())
    log_z = Tt.log_z_enumerated(W, a, c)
    nmf = tap.tap_log_partition(r, n_starts=4, max_iters=400, check_every=50, order=1)
    assert 0 < log_z - nmf["log_z"] and abs(log_z - res["log_z"]) < 0.1 * (log_z - nmf["log_z"])


# ---- iDBN.train -------------------------------------------------------------------------------------------------------------------
def _idbn(params, eng, groups=False):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import iDBN
    E.set_engine_for_testing(eng)
    torch.manual_seed(0)
    g = np.random.Generator(np.random.PCG64(3))
    X = torch.from_numpy((g.random((20, 12)) > 0.5).astype(F32))
    dl = DataLoader(TensorDataset(X, torch.zeros(20)), batch_size=8)
    net = iDBN([12, 7, 5], dict({"LEARNING_RATE": 0.1, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95,
                                 "LEARNING_RATE_DYNAMIC": True, "CD": 1}, **params), dl, dl, torch.device("cpu"))
    for r in net.layers:
        _on_cpu(r)
    if groups:
        net.layers[0].softmax_groups = [(8, 12)]
    E.manual_seed(4)
    net.train(2)
    return net


def test_idbn_train_without_the_key_is_the_parents_call_sequence():
    try:
        eng = OracleEngine()      # a double that lacks the new calls is enough
        _idbn({}, eng)
        eng2 = OracleEngine()
        _idbn({"TAP": False}, eng2)
    finally:
        E.set_engine_for_testing(None)
    per_batch = lambda rows: [("cd_step", (rows, 12), 1, True), ("forward", (rows, 12)), ("cd_step", (rows, 7), 1, False)]
    assert eng.calls == (per_batch(8) + per_batch(8) + per_batch(4)) * 2 and eng2.calls == eng.calls


def test_idbn_train_with_the_key_calls_tap_step_for_the_layers_it_may():
    try:
        e1 = TapOracleEngine()
        on = _idbn({"TAP": True}, e1)
        e2 = TapOracleEngine()
        mixed = _idbn({"TAP": {"n_iters": 2, "order": 1, "damp": 0.25}}, e2, groups=True)
        with pytest.raises(ValueError):
            _idbn({"TAP": True, "PERSISTENT": True}, TapOracleEngine())
    finally:
        E.set_engine_for_testing(None)
    s1 = [c for c in e1.calls if c[0] == "tap_step"]
    assert len(s1) == 12 and all(c[2:] == (3, 0.5, 2, True) for c in s1) and not any(c[0] == "cd_step" for c in e1.calls)
    assert all("_tap_mv" in r.__dict__ for r in on.layers) and torch.isfinite(on.loss_history[0]).all()
    # a layer with softmax groups keeps CD-k; the one above it is trained by TAP with the dict's settings
    assert sum(c[0] == "cd_step" for c in e2.calls) == 6 and all(c[1][1] == 12 for c in e2.calls if c[0] == "cd_step")
    s2 = [c for c in e2.calls if c[0] == "tap_step"]
    assert len(s2) == 6 and all(c[1][1] == 7 and c[2:] == (2, 0.25, 1, True) for c in s2)
    assert "_tap_mv" not in mixed.layers[0].__dict__ and "_tap_mv" in mixed.layers[1].__dict__


def test_the_cases_name_every_edge():
    assert len(Ck.TABLE) == 12 + len(Ck.EDGES) and {B for _, _, B in Ck.TABLE} >= {1, 5, 63, 64, 65}
    assert any(H % 4 for _, H, _ in Ck.TABLE) and any(H > 1024 for _, H, _ in Ck.TABLE)
