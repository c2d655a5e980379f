"""CPU-only: the twin of the centered update (tests/centered_oracle.py) against first principles, the pinned seeds of
tests/centered_cases.py, and the host logic of RBM.train_epoch_centered / iDBN.train through the engine double
(tests/centered_engine_double.py).  No claim about the kernels is made here -- those are tested on the GPU in test_centered_gpu.py."""
import pickle

import numpy as np
import pytest
import torch

import centered_cases as Cc
import centered_oracle as Tc
import oracle.rbm_oracle as O
import pcd_cases as Cs
import pcd_oracle as T
from centered_engine_double import CenteredOracleEngine
from imdbn import engine as E
from oracle.draws import PhiloxStream
from oracle_engine import OracleEngine
from pcd_engine_double import PcdOracleEngine

F32, F64 = np.float32, np.float64
SIX = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")


# ---- 1. the algebra -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["odd", "groups"])
def test_a_centered_parameter_step_is_the_twins_normal_parameter_step(name, mode):
    """A float64 centered RBM (W, b_c, c_c, mu, lam) with energy -(v - mu)^T W (h - lam) - b_c.(v - mu) - c_c.(h - lam) takes one
    plain gradient step with the centered gradients (gW, dv, dh) at mom = wd = 0 and fixed offsets; converted to normal parameters
    (b = b_c - W lam, c = c_c - W^T mu) it is the twin's step."""
    c = Cc.case(name)
    g = np.random.Generator(np.random.PCG64(17))
    V, H, n, lr = c["V"], c["H"], 6, 0.05
    vp, vn = (g.random((n, V)) < 0.3).astype(F64), (g.random((n, V)) < 0.5).astype(F64)
    hp, hn = g.random((n, H)), g.random((n, H))
    s = dict(pos_assoc=vp.T @ hp, neg_assoc=vn.T @ hn, pos_h_sum=hp.sum(0), neg_h_sum=hn.sum(0), data_sum=vp.sum(0), v_sum=vn.sum(0))
    W, b, cc, mu, lam = (c[k].astype(F64) for k in ("W", "b", "c", "mu", "lam"))
    # the centered model, its gradients straight from the centered variables
    b_c, c_c = b + W @ lam, cc + W.T @ mu
    gW = ((vp - mu).T @ (hp - lam) - (vn - mu).T @ (hn - lam)) / n
    W1, b_c1, c_c1 = W + lr * gW, b_c + lr * (vp.mean(0) - vn.mean(0)), c_c + lr * (hp.mean(0) - hn.mean(0))
    want = dict(W=W1, vis_bias=b_c1 - W1 @ lam, hid_bias=c_c1 - W1.T @ mu)
    st = O.RBMState(W=W.copy(), hid_bias=cc.copy(), vis_bias=b.copy(), W_m=np.zeros((V, H)), hb_m=np.zeros(H), vb_m=np.zeros(V),
                    lr=lr, weight_decay=0.0, momentum=0.0)
    mu2, lam2 = Tc.apply_centered_update(st, s, lr, 0.0, n, False, mu, lam, 0.0, mode)
    assert np.array_equal(mu2, mu) and np.array_equal(lam2, lam) and st.W.dtype == F64
    worst = max(float(np.abs(getattr(st, k) - want[k]).max()) for k in want)
    print(f"{name} mode {mode}: largest |twin - centered model| {worst:.3g}")
    assert worst <= 1e-12


def test_the_sliding_offsets_are_the_batch_means():
    c = Cc.case("odd")
    n = c["M"]
    s = O.cd_statistics(T.rbm_state(c), c["data"], 1, PhiloxStream(1))
    for mode, slide in ((0, 1.0), (1, 1.0), (0, 0.25)):
        mu2, lam2, _, dv, dh = Tc.offsets_and_gradient(s, n, c["mu"], c["lam"], slide, mode, F64)
        mv = c["data"].astype(F64).mean(0) if mode == 0 else (c["data"].astype(F64).mean(0) + s["v"].astype(F64).mean(0)) / 2
        mh = s["pos_h"].astype(F64).mean(0) if mode == 0 else (s["pos_h"].astype(F64).mean(0) + s["h_prob"].astype(F64).mean(0)) / 2
        assert np.allclose(mu2, (1 - slide) * c["mu"] + slide * mv, atol=1e-6) and np.allclose(lam2, (1 - slide) * c["lam"] + slide * mh, atol=1e-6)
        assert np.allclose(dv, c["data"].mean(0) - s["v"].mean(0), atol=1e-6)


# ---- 2. zero offsets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(Cs.CASES))
def test_zero_offsets_without_slide_are_the_plain_updates_exactly(name, mode):
    c = Cc.case(name)
    z = dict(mu=np.zeros(c["V"], F32), lam=np.zeros(c["H"], F32), slide=0.0)
    for k in Cc.PCD_KS:
        t = Cc.twin_run(c, "pcd", k, mode, **z)
        st = T.rbm_state(c, Cs.LR, Cs.WEIGHT_DECAY, Cs.MOM, sparsity=c["sparsity"], sparsity_factor=Cc.SPARSITY_TARGET)
        loss, v = T.pcd_step(st, c["data"], c["particles"], k, PhiloxStream(c["seed"]), Cs.LR, Cs.MOM)
        assert all(np.array_equal(getattr(t["st"], q), getattr(st, q)) for q in SIX), (name, k)
        assert np.array_equal(t["v"], v) and t["loss"] == loss and not t["mu"].any() and not t["lam"].any()
    t = Cc.twin_run(c, "cd", Cc.CD_K, mode, **z)
    st = T.rbm_state(c, Cs.LR, Cs.WEIGHT_DECAY, Cs.MOM, sparsity=c["sparsity"], sparsity_factor=Cc.SPARSITY_TARGET)
    stats = O.cd_statistics(st, c["data"], Cc.CD_K, PhiloxStream(c["cd_seed"]))
    O.apply_cd_update(st, stats, Cs.LR, Cs.MOM, stats["n"], st.sparsity)
    assert all(np.array_equal(getattr(t["st"], q), getattr(st, q)) for q in SIX)
    assert t["loss"] == F32(stats["sq_err"].mean(dtype=F32)) and t["v"] is None


# ---- 3. the pinned seeds and the cases --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.CASES))
def test_pinned_seeds_keep_every_decision_clear_of_a_tie(name):
    c = Cc.case(name)
    assert 0.05 < c["mu"].min() and c["mu"].max() < 0.95 and 0.05 < c["lam"].min() and c["lam"].max() < 0.95
    G = len(c["groups"])
    for kind, k in [("cd", Cc.CD_K)] + [("pcd", k) for k in Cc.PCD_KS]:
        t = Cc.twin_run(c, kind, k, 0)
        print(f"{name} {kind}-{k}: margins {t['bern']:.3g} / {t['cat']:.3g}")
        assert t["bern"] >= Cs.MARGIN and t["cat"] >= Cs.MARGIN and Cc.margins_ok(t)
        assert t["offset"] == (1 + k * (2 + G) if kind == "cd" else k * (2 + G))
        # the offsets and the update differ from the uncentered one: the case exercises the correction
        u = Cc.twin_run(c, kind, k, 0, mu=np.zeros(c["V"], F32), lam=np.zeros(c["H"], F32), slide=0.0)
        assert not np.array_equal(t["st"].W, u["st"].W)


def test_the_cases_cover_every_slide_both_paths_and_the_sparsity_term():
    cs = [Cc.case(n) for n in Cs.CASES]
    assert {c["slide"] for c in cs} == {0.0, 0.01, 1.0} and sum(c["sparsity"] for c in cs) == 1
    assert any(c["H"] % 4 for c in cs) and any(c["H"] % 4 == 0 for c in cs) and any(c["M"] > 64 for c in cs) and any(c["V"] > 1024 for c in cs)


# ---- 4. host logic through the engine double ---------------------------------------------------------------------------------
@pytest.fixture
def double():
    eng = CenteredOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)


def _on_cpu(r, W=None, b=None, c=None):
    """The double works on host tensors, whatever device the constructor chose."""
    r.to("cpu")
    r.W.data = r.W.data.contiguous() if W is None else torch.from_numpy(W.copy())
    if b is not None:
        r.vis_bias.data, r.hid_bias.data = torch.from_numpy(b.copy()), torch.from_numpy(c.copy())
    r.W_m, r.hb_m, r.vb_m = torch.zeros_like(r.W.data), torch.zeros_like(r.hid_bias.data), torch.zeros_like(r.vis_bias.data)
    return r


def _rbm(c):
    from imdbn.models import RBM
    return _on_cpu(RBM(c["V"], c["H"], Cs.LR, Cs.WEIGHT_DECAY, Cs.MOM, softmax_groups=c["groups"] or None), c["W"], c["b"], c["c"])


def _same(a, b):
    return all(torch.equal(getattr(a, k).data if k in SIX[:3] else getattr(a, k), getattr(b, k).data if k in SIX[:3] else getattr(b, k)) for k in SIX)


@pytest.mark.parametrize("route", ["cd", "pcd", "tempered"])
def test_train_epoch_centered_equals_the_hand_issued_double_calls(double, route):
    """First call: offsets from zeros with slide 1 (the first batch's means); then the caller's slide; then a short batch."""
    c = Cc.case("groups")
    x, M, V, H = torch.from_numpy(c["data"]), c["M"], c["V"], c["H"]
    betas = [0.5, 1.0] if route == "tempered" else None
    Rn = 2 if betas else 1
    kw = dict(persistent=route != "cd", betas=betas, offsets="enhanced")
    r = _rbm(c)
    assert r.centering_offsets() is None
    E.manual_seed(13)
    l0 = r.train_epoch_centered(x, 0, 10, CD=2, slide=0.25, **kw)
    mu, lam = r.centering_offsets()
    assert mu is r._ctr_mu and lam is r._ctr_lam and tuple(mu.shape) == (V,) and tuple(lam.shape) == (H,)
    assert double.calls[-1][0] == "centered_step" and double.calls[-1][3:] == (1.0, 1, True)
    first = mu.clone()
    l1 = r.train_epoch_centered(x, 7, 10, CD=2, slide=0.25, **kw)
    assert double.calls[-1][3:] == (0.25, 1, True) and r._ctr_mu is mu and not torch.equal(mu, first)
    l2 = r.train_epoch_centered(x[:2], 7, 10, CD=1, slide=0.25, monitor=False, **kw)
    assert l2 is None and double.calls[-1] == ("centered_step", None if route == "cd" else (2, V), 0 if route == "tempered" else 1, 0.25, 1, False)
    off = E.get_rng().offset
    # by hand on the same draws
    h, eng = _rbm(c), CenteredOracleEngine()
    rng = E.PhiloxRng(13)
    hm, hl = torch.zeros(V), torch.zeros(H)
    chains = None if route == "cd" else torch.cat([eng.sample_visible(h, x, rng) for _ in range(Rn)], 0)
    tries = accs = None
    want = []
    for ep, slide in ((0, 1.0), (7, 0.25)):
        lr, mom = h._lr_mom(ep)
        if route == "tempered":
            tries, accs = eng.pt_sweep(h, chains, betas, 2, rng, tries, accs)
            want.append(eng.centered_step(h, x, chains[M:], lr, mom, 0, rng, hm, hl, slide, 1))
        else:
            want.append(eng.centered_step(h, x, chains, lr, mom, 2, rng, hm, hl, slide, 1))
    lr, mom = h._lr_mom(7)
    if route == "tempered":
        part = chains.view(Rn, M, V)[:, :2].reshape(Rn * 2, V)
        tries, accs = eng.pt_sweep(h, part, betas, 1, rng, tries, accs)
        chains.view(Rn, M, V)[:, :2] = part.view(Rn, 2, V)
        eng.centered_step(h, x[:2], chains[M:M + 2], lr, mom, 0, rng, hm, hl, 0.25, 1, monitor=False)
    else:
        eng.centered_step(h, x[:2], None if chains is None else chains[:2], lr, mom, 1, rng, hm, hl, 0.25, 1, monitor=False)
    assert rng.offset == off and _same(r, h) and torch.equal(mu, hm) and torch.equal(lam, hl)
    assert torch.equal(l0, want[0]) and torch.equal(l1, want[1])
    if route == "cd":
        assert "_pcd" not in r.__dict__
    else:
        assert torch.equal(r._pcd, chains)
    # the first call made the offsets the first batch's means (enhanced: of data and model)
    assert first.min() >= 0 and first.max() <= 1


def test_the_first_offsets_are_the_first_batchs_data_means(double):
    c = Cc.case("odd")
    r, x = _rbm(c), torch.from_numpy(c["data"])
    E.manual_seed(3)
    r.train_epoch_centered(x, 0, 10)
    assert double.calls == [("centered_step", None, 1, 1.0, 0, True)]
    assert np.allclose(r._ctr_mu.numpy(), c["data"].mean(0), atol=1e-6)
    assert np.allclose(r._ctr_lam.numpy(), O.forward(T.rbm_state(c), c["data"]).mean(0), atol=1e-6)
    with pytest.raises(ValueError):
        r.train_epoch_centered(x, 0, 10, offsets="model")


def test_the_pickle_drops_the_offsets_and_a_loaded_model_reinitialises_them(double):
    c = Cc.case("odd")
    r, x = _rbm(c), torch.from_numpy(c["data"])
    r.train_epoch_centered(x, 0, 10, persistent=True)
    assert r._ctr_mu is not None and r._pcd is not None
    state = r.__getstate__()
    assert not {"_ctr_mu", "_ctr_lam", "_pcd", "_imdbn_desc"} & set(state)
    r2 = pickle.loads(pickle.dumps(r))
    assert r2.centering_offsets() is None and torch.equal(r2.W.data, r.W.data)
    r2.train_epoch_centered(x, 1, 10, slide=0.5)
    assert double.calls[-1][3] == 1.0 and r2.centering_offsets() is not None


def test_data_parallel_raises(double, monkeypatch):
    c = Cc.case("one")
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        _rbm(c).train_epoch_centered(torch.from_numpy(c["data"]), 0, 1)


# ---- 5. iDBN.train -------------------------------------------------------------------------------------------------------------
def _idbn(params, eng):
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
    E.manual_seed(4)
    net.train(2)
    return net


def test_idbn_train_without_the_key_is_todays_call_sequence():
    """Without params["CENTERED"] an engine double that lacks the new call is enough, and the engine calls iDBN.train makes are, in
    order, the parent's: per batch one cd_step per layer, the lower layer's with its forward fused in (the double's cd_step
    records the forward it runs for ``forward=True``)."""
    try:
        eng = OracleEngine()
        plain = _idbn({}, eng)
        off = _idbn({"CENTERED": False, "CENTERED_OFFSETS": "enhanced"}, PcdOracleEngine())
    finally:
        E.set_engine_for_testing(None)
    per_batch = lambda rows: [("cd_step", (rows, 12), 1, True), ("forward", (rows, 12)), ("cd_step", (rows, 7), 1, False)]
    assert eng.calls == (per_batch(8) + per_batch(8) + per_batch(4)) * 2        # 20 rows in batches of 8: three per epoch, two epochs
    for a, b in zip(plain.layers, off.layers):
        assert _same(a, b) and b.centering_offsets() is None
    assert all(torch.equal(a, b) for a, b in zip(plain.loss_history, off.loss_history))


def test_idbn_train_with_the_key_routes_every_layer_through_the_centered_update():
    try:
        plain = _idbn({}, OracleEngine())
        e1 = CenteredOracleEngine()
        on = _idbn({"CENTERED": True}, e1)
        e2 = CenteredOracleEngine()
        both = _idbn({"CENTERED": 0.2, "CENTERED_OFFSETS": "enhanced", "PERSISTENT": True}, e2)
    finally:
        E.set_engine_for_testing(None)
    # per batch: the lower layer's update, its forward (the engine's T = 1 forward call), the upper layer's update
    assert [c[0] for c in e1.calls] == ["centered_step", "forward", "centered_step"] * 6
    s1, s2 = ([c for c in e.calls if c[0] == "centered_step"] for e in (e1, e2))
    assert len(s1) == 12 and all(c[1] is None for c in s1)
    assert [c[3] for c in s1[:4]] == [1.0, 1.0, 0.01, 0.01] and {c[4] for c in s1} == {0}
    assert all(r.centering_offsets() is not None and "_pcd" not in r.__dict__ for r in on.layers)
    assert not torch.equal(on.layers[0].W.data, plain.layers[0].W.data)
    assert len(on.loss_history) == 2 and torch.isfinite(on.loss_history[0]).all()
    # persistent chains only where the input is binary: the first layer; the second keeps CD phases
    assert "_pcd" in both.layers[0].__dict__ and "_pcd" not in both.layers[1].__dict__
    assert [(c[1], c[3], c[4]) for c in s2[:4]] == [((8, 12), 1.0, 1), (None, 1.0, 1), ((8, 12), 0.2, 1), (None, 0.2, 1)]
