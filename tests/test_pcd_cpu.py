"""CPU-only: the twin of the persistent-chain calls (tests/pcd_oracle.py) against first principles, the pinned seeds of
tests/pcd_cases.py, and the host logic of RBM.train_epoch_persistent / iDBN.train through the engine double
(tests/pcd_engine_double.py).  No claim about the kernels is made here -- those are tested on the GPU in test_pcd_gpu.py."""
import itertools
import pickle

import numpy as np
import pytest
import torch

import oracle.rbm_oracle as O
import pcd_cases as Cs
import pcd_oracle as T
from imdbn import engine as E
from imdbn.engine import rng as R
from oracle.draws import PhiloxStream
from oracle_engine import OracleEngine
from pcd_engine_double import PcdOracleEngine

F32 = np.float32


# ---- 1. the exchange ratio --------------------------------------------------------------------------------------------
def test_delta_is_the_log_ratio_of_enumerated_tempered_marginals():
    """V = 5, H = 4, parameters on a 2^-10 grid (so the twin's fp32 logits are exact): for every ordered pair of the 32 states and
    two beta pairs, Delta = log [p_lo(u') p_hi(u)] - log [p_lo(u) p_hi(u')] with p_beta(v) = sum_h exp(-beta E(v, h)) enumerated."""
    g = np.random.Generator(np.random.PCG64(5))
    grid = lambda a: (np.round(a * 1024) / 1024).astype(F32)
    st = O.RBMState.create(grid(g.standard_normal((5, 4))), 0.1, 0.0, 0.5, hid_bias=grid(g.standard_normal(4) * 0.5),
                           vis_bias=grid(g.standard_normal(5) * 0.5))
    states = np.array(list(itertools.product((0.0, 1.0), repeat=5)), F32)
    u, w = np.repeat(states, 32, 0), np.tile(states, (32, 1))           # all 1024 ordered pairs
    worst = 0.0
    for b_lo, b_hi in ((0.25, 1.0), (0.5, 0.75)):
        lp = {b: T.log_tempered_marginal(st, states, b) for b in (b_lo, b_hi)}
        iu, iw = np.repeat(np.arange(32), 32), np.tile(np.arange(32), 32)
        want = lp[b_lo][iw] + lp[b_hi][iu] - lp[b_lo][iu] - lp[b_hi][iw]
        got = T.exchange_delta(st, u, w, F32(b_lo), F32(b_hi))
        worst = max(worst, float(np.abs(got - want).max()))
    print("largest |Delta - enumerated|:", worst)
    assert worst <= 1e-10


# ---- 2. the pinned seeds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.CASES))
def test_pinned_seed_keeps_every_decision_clear_of_a_tie(name):
    c = Cs.case(name)
    t = Cs.twin_run(c, c["seed"])
    print(f"{name}: margins {t['bern']:.3g} / {t['cat']:.3g} / {t['exch']:.3g}, accepted {t['accs'].tolist()} of {t['tries'].tolist()}")
    assert t["bern"] > Cs.MARGIN and t["cat"] > Cs.MARGIN
    assert t["exch"] > Cs.exchange_margin(c["H"])
    if c["R"] >= 2:
        assert t["accs"].sum() > 0 and (t["tries"] - t["accs"]).sum() > 0          # both outcomes are exercised
        per_pair = [c["M"] * len([s for s in range(Cs.SWEEPS) if s % 2 == r % 2]) for r in range(c["R"] - 1)]
        assert t["tries"].tolist() == per_pair
    else:
        assert t["tries"].tolist() == [0] and t["accs"].tolist() == [0]
    assert Cs.seed_ok(c, t)
    v = t["state"]
    assert set(np.unique(v)) <= {0.0, 1.0} and all((v[:, s:e].sum(1) == 1).all() for s, e in c["groups"])


# ---- 3. the twin against the oracle's own steps -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "groups"])
def test_one_replica_is_plain_gibbs(name):
    c = Cs.case(name)
    st = T.rbm_state(c)
    v0 = c["state"][:c["M"]]
    got, tries, accs, _ = T.pt_sweep(st, v0, [1.0], 3, PhiloxStream(7))
    ps, want = PhiloxStream(7), v0
    for _ in range(3):
        want = O.gibbs_step(st, want, ps)[0]
    assert np.array_equal(got, want) and tries.tolist() == [0]


@pytest.mark.parametrize("name", ["odd", "groups"])
def test_pcd_then_pcd0_leaves_the_particles_where_the_gibbs_steps_put_them(name):
    c = Cs.case(name)
    st = T.rbm_state(c, Cs.LR, Cs.WEIGHT_DECAY, Cs.MOM)
    frozen = st.copy()
    ps = PhiloxStream(3)
    _, v2 = T.pcd_step(st, c["data"], c["particles"], 2, ps, Cs.LR, Cs.MOM)
    off = ps.offset
    _, v0 = T.pcd_step(st, c["data"], v2, 0, ps, Cs.LR, Cs.MOM)
    assert ps.offset == off and np.array_equal(v0, v2)                    # cd_k = 0 draws nothing and moves nothing
    ps, want = PhiloxStream(3), c["particles"]
    for _ in range(2):
        want = O.gibbs_step(frozen, want, ps)[0]                          # under the parameters on entry
    assert np.array_equal(v2, want)
    assert not np.array_equal(st.W, frozen.W)


@pytest.mark.parametrize("name", list(Cs.CASES))
def test_draw_counts(name):
    c = Cs.case(name)
    G, R_ = len(c["groups"]), c["R"]
    for k in (0, 1, 2):
        ps = PhiloxStream(1)
        T.pcd_step(T.rbm_state(c), c["data"], c["particles"], k, ps, Cs.LR, Cs.MOM)
        assert len(ps.log) == k * (2 + G) == len(R.sched_pcd(c["V"], c["H"], c["groups"], k))
        assert [(t, s[1] if t == "u" else None) for t, s in ps.log] == \
               [(t, n if t == "u" else None) for t, n in R.sched_pcd(c["V"], c["H"], c["groups"], k)]
    ps = PhiloxStream(1)
    T.pt_sweep(T.rbm_state(c), c["state"], c["betas"], Cs.SWEEPS, ps)
    sched = R.sched_pt(c["V"], c["H"], c["groups"], R_, Cs.SWEEPS)
    assert len(ps.log) == Cs.SWEEPS * (2 + G + (1 if R_ >= 2 else 0)) == len(sched)
    assert all(s[0] == R_ * c["M"] for _, s in ps.log)                     # every tensor spans all R M rows
    assert [(t, s[1] if t == "u" else None) for t, s in ps.log] == [(t, n if t == "u" else None) for t, n in sched]


# ---- 4. host logic through the engine double ---------------------------------------------------------------------------
@pytest.fixture
def double():
    eng = PcdOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)


def _rbm(c, **kw):
    from imdbn.models import RBM
    r = RBM(c["V"], c["H"], Cs.LR, Cs.WEIGHT_DECAY, Cs.MOM, softmax_groups=c["groups"] or None, **kw)
    return _on_cpu(r, c["W"], c["b"], c["c"])


def _on_cpu(r, W=None, b=None, c=None):
    """The double works on host tensors, whatever device the constructor chose."""
    r.to("cpu")
    r.W.data = r.W.data.contiguous() if W is None else torch.from_numpy(W.copy())
    if b is not None:
        r.vis_bias.data, r.hid_bias.data = torch.from_numpy(b.copy()), torch.from_numpy(c.copy())
    r.W_m, r.hb_m, r.vb_m = torch.zeros_like(r.W.data), torch.zeros_like(r.hid_bias.data), torch.zeros_like(r.vis_bias.data)
    return r


def test_first_use_creates_the_chains_from_the_data_and_pcd_advances_them(double):
    c = Cs.case("groups")
    r, x = _rbm(c), torch.from_numpy(c["data"])
    E.manual_seed(11)
    loss = r.train_epoch_persistent(x, 0, 10, CD=2)
    assert loss.dim() == 0 and tuple(r._pcd.shape) == (c["M"], c["V"]) and double.calls == [("pcd_step", (c["M"], c["V"]), 2, True)]
    # the twin: chains = sample_visible(data), then pcd(2) on the same stream
    st, ps = T.rbm_state(dict(c, W_m=np.zeros_like(c["W"]), hb_m=np.zeros_like(c["c"]), vb_m=np.zeros_like(c["b"])), Cs.LR, Cs.WEIGHT_DECAY, Cs.MOM), PhiloxStream(11)
    v0 = O.sample_visible(st, c["data"], ps)
    want_loss, v = T.pcd_step(st, c["data"], v0, 2, ps, Cs.LR, Cs.MOM)
    assert np.array_equal(r._pcd.numpy(), v) and np.array_equal(r.W.data.numpy(), st.W) and float(loss) == float(want_loss)
    assert E.get_rng().offset == ps.offset
    chains = r._pcd
    assert r.train_epoch_persistent(x, 1, 10, CD=1, monitor=False) is None and r._pcd is chains          # kept, advanced in place
    assert double.calls[-1] == ("pcd_step", (c["M"], c["V"]), 1, False)
    assert r.pt_swap_rates() is None


def test_short_last_batch_uses_and_advances_the_first_rows_only(double):
    c = Cs.case("odd")
    r, x = _rbm(c), torch.from_numpy(c["data"])
    E.manual_seed(2)
    r.train_epoch_persistent(x, 0, 10, CD=1)
    before = r._pcd.clone()
    r.train_epoch_persistent(x[:2], 0, 10, CD=1)
    assert double.calls[-1] == ("pcd_step", (2, c["V"]), 1, True)
    assert torch.equal(r._pcd[2:], before[2:]) and not torch.equal(r._pcd[:2], before[:2])
    # tempered: R replicas of the batch, the first rows of EVERY replica on a short batch, the update from the beta = 1 replica
    r2, betas = _rbm(c), [0.4, 0.7, 1.0]
    r2.train_epoch_persistent(x, 0, 10, CD=2, betas=betas)
    M, V = c["M"], c["V"]
    assert tuple(r2._pcd.shape) == (3 * M, V)
    assert double.calls[-2:] == [("pt_sweep", (3 * M, V), 3, 2), ("pcd_step", (M, V), 0, True)]
    before = r2._pcd.clone()
    r2.train_epoch_persistent(x[:2], 0, 10, CD=1, betas=betas, monitor=False)
    assert double.calls[-2:] == [("pt_sweep", (6, V), 3, 1), ("pcd_step", (2, V), 0, False)]
    now, was = r2._pcd.view(3, M, V), before.view(3, M, V)
    assert torch.equal(now[:, 2:], was[:, 2:]) and not torch.equal(now[:, :2], was[:, :2])
    rates = r2.pt_swap_rates()
    assert tuple(rates.shape) == (2,) and rates.dtype == torch.float64
    tries = r2._pt_try.tolist()
    assert tries == [M + 2, M]                                           # sweeps 0, 1 of the first call, sweep 0 of the second
    with pytest.raises(ValueError):
        r2.train_epoch_persistent(x, 0, 10, betas=[1.0])


def test_the_pickle_drops_the_chains_and_a_loaded_model_restarts_them(double):
    c = Cs.case("odd")
    r, x = _rbm(c), torch.from_numpy(c["data"])
    r.train_epoch_persistent(x, 0, 10, CD=1, betas=[0.5, 1.0])
    assert r._pcd is not None and r._pt_try is not None
    state = r.__getstate__()
    assert not {"_pcd", "_pcd_replicas", "_pt_try", "_pt_acc", "_imdbn_desc"} & set(state)
    r2 = pickle.loads(pickle.dumps(r))
    assert "_pcd" not in r2.__dict__ and torch.equal(r2.W.data, r.W.data) and r2.pt_swap_rates() is None
    r2.train_epoch_persistent(x, 1, 10, CD=1)
    assert tuple(r2._pcd.shape) == (c["M"], c["V"])


def test_data_parallel_raises(double, monkeypatch):
    c = Cs.case("one")
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        _rbm(c).train_epoch_persistent(torch.from_numpy(c["data"]), 0, 1)


# ---- 5. iDBN.train -----------------------------------------------------------------------------------------------------
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


def test_idbn_train_without_the_switch_is_todays_run_bit_for_bit():
    try:
        plain = _idbn({}, OracleEngine())                   # an engine double WITHOUT the new calls: they are never reached
        off = _idbn({"PERSISTENT": False, "PT_BETAS": [0.5, 1.0]}, PcdOracleEngine())
        on = _idbn({"PERSISTENT": True}, PcdOracleEngine())
        eng = PcdOracleEngine()
        pt = _idbn({"PERSISTENT": True, "PT_BETAS": [0.5, 1.0]}, eng)
    finally:
        E.set_engine_for_testing(None)
    for a, b in zip(plain.layers, off.layers):
        for k in ("W", "hid_bias", "vis_bias"):
            assert torch.equal(getattr(a, k).data, getattr(b, k).data)
        assert "_pcd" not in b.__dict__
    assert all(torch.equal(a, b) for a, b in zip(plain.loss_history, off.loss_history))
    # switched on: the first layer (binary input) trains on persistent chains, the second (probabilities) keeps CD
    assert "_pcd" in on.layers[0].__dict__ and "_pcd" not in on.layers[1].__dict__
    assert not torch.equal(on.layers[0].W.data, plain.layers[0].W.data)
    assert tuple(on.layers[0]._pcd.shape) == (8, 12) and tuple(pt.layers[0]._pcd.shape) == (16, 12)
    assert [c[0] for c in eng.calls[:2]] == ["pt_sweep", "pcd_step"] and pt.layers[0].pt_swap_rates() is not None
    assert len(on.loss_history) == 2 and torch.isfinite(on.loss_history[0]).all()
