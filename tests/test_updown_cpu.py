"""CPU-only: the pinned seeds of tests/updown_cases.py, the twin of the up-down calls (tests/updown_oracle.py) against autograd, and
the host logic of iDBN.untie / updown_step / finetune_updown and of the untied likelihood functions through the engine double
(tests/updown_engine_double.py).  No claim about the kernels is made here -- those are tested on the GPU in test_updown_gpu.py."""
import io
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import updown_cases as Cs
import updown_oracle as U
from imdbn import engine as E
from pcd_cases import MARGIN
from updown_engine_double import UpDownOracleEngine

F32, F64 = np.float32, np.float64
PARAMS = {"LEARNING_RATE": 0.1, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95, "LEARNING_RATE_DYNAMIC": True, "CD": 1}


# ---- 1. the pinned seeds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.CASES))
def test_the_pinned_seed_is_the_first_admissible_one(name):
    c = Cs.case(name)
    seed, margin = Cs.first_seed(c, c["seed"] + 1)
    print(f"{name}: first seed {seed}, smallest margin {margin:.3g}")
    assert seed == c["seed"] and margin > MARGIN


# ---- 2. the twin's steps are gradient steps -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["down", "up"])
def test_the_twins_delta_step_is_the_gradient_of_the_mean_log_probability(direction):
    g = np.random.Generator(np.random.PCG64(5))
    V, H, B, lr = 7, 5, 6, 0.3
    W, b, c = g.standard_normal((V, H)) * 0.7, g.standard_normal(V) * 0.5, g.standard_normal(H) * 0.5
    lo, hi = (g.random((B, V)) < 0.4).astype(F64), (g.random((B, H)) < 0.5).astype(F64)
    x, t = (lo, hi) if direction == "up" else (hi, lo)
    st = SimpleNamespace(W=W.copy(), vis_bias=b.copy(), hid_bias=c.copy(), W_m=np.zeros((V, H)), hb_m=np.zeros(H), vb_m=np.zeros(V),
                         weight_decay=0.0)
    lp = U.delta_step(st, direction, x, t, lr, 0.0, dt=F64)
    Wt, bt, ct = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (W, b, c))
    xt, tt = torch.from_numpy(x), torch.from_numpy(t)
    a = xt @ Wt + ct if direction == "up" else xt @ Wt.T + bt
    rows = (tt * a - torch.nn.functional.softplus(a)).sum(1)
    rows.mean().backward()
    rel = lambda got, want: np.linalg.norm(got - want) / np.linalg.norm(want)
    assert rel(lp, rows.detach().numpy()) < 1e-10
    assert rel(st.W - W, lr * Wt.grad.numpy()) < 1e-10
    if direction == "up":
        assert rel(st.hid_bias - c, lr * ct.grad.numpy()) < 1e-10 and np.array_equal(st.vis_bias, b) and not st.vb_m.any()
    else:
        assert rel(st.vis_bias - b, lr * bt.grad.numpy()) < 1e-10 and np.array_equal(st.hid_bias, c) and not st.hb_m.any()


# ---- 3. host logic on the engine double ----------------------------------------------------------------------------------------------
@pytest.fixture
def double():
    eng = UpDownOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)


def _net(sizes=(12, 7, 5)):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import iDBN
    torch.manual_seed(0)
    g = np.random.Generator(np.random.PCG64(3))
    X = torch.from_numpy((g.random((20, sizes[0])) > 0.5).astype(F32))
    dl = DataLoader(TensorDataset(X, torch.zeros(20)), batch_size=8)
    net = iDBN(list(sizes), dict(PARAMS), dl, dl, torch.device("cpu"))
    for r in net.layers:
        r.to("cpu")
        r.W.data = r.W.data.contiguous()
        r.hid_bias.data.normal_(0, 0.3); r.vis_bias.data.normal_(0, 0.3)
        r.W_m, r.hb_m, r.vb_m = torch.zeros_like(r.W.data), torch.zeros_like(r.hid_bias.data), torch.zeros_like(r.vis_bias.data)
    return net, X


def _dump(net):
    f = io.BytesIO()
    pickle.dump({"layers": net.layers, "params": net.params}, f)
    return f.getvalue()


def test_a_model_that_is_never_untied_keeps_its_attributes_and_its_pickle(double, tmp_path):
    net, X = _net()
    keys, raw = sorted(net.__dict__), _dump(net)
    assert not net.is_untied() and "gen_layers" not in net.__dict__
    net.represent(X[:4]); net.decode(net.represent(X[:4])); net.reconstruct(X[:4])
    assert sorted(net.__dict__) == keys and _dump(net) == raw
    path = str(tmp_path / "tied.pkl")
    net.save_model(path)
    assert open(path, "rb").read() == raw


def test_untie_copies_is_idempotent_and_decode_uses_the_twins(double):
    net, X = _net()
    top = net.represent(X[:4])
    tied = net.decode(top)
    gen = net.untie()
    assert net.is_untied() and net.untie() is gen and len(gen) == len(net.layers) - 1
    for g, r in zip(gen, net.layers):
        assert torch.equal(g.W.data, r.W.data) and torch.equal(g.vis_bias.data, r.vis_bias.data) and g.W.data_ptr() != r.W.data_ptr()
        assert not g.W_m.any() and not g.hb_m.any() and not g.vb_m.any()
        assert (g.lr, g.weight_decay, g.momentum, g.final_momentum, g.dynamic_lr) == (r.lr, r.weight_decay, r.momentum, r.final_momentum, r.dynamic_lr)
    assert torch.equal(net.decode(top), tied)
    gen[0].vis_bias.data += 1.0                                  # only the twin moves: decode and reconstruct follow it, represent does not
    assert not torch.equal(net.decode(top), tied) and torch.equal(net.represent(X[:4]), top)
    assert torch.equal(net.reconstruct(X[:4]), net.decode(top))


def test_an_untied_model_round_trips_through_save_and_load(double, tmp_path):
    net, X = _net()
    E.manual_seed(3)
    net.updown_step(X[:8], 0, 1)
    path = str(tmp_path / "untied.pkl")
    net.save_model(path)
    other, _ = _net()
    other.load_model(path)
    assert other.is_untied()
    for a, b in zip(net.layers + net.gen_layers, other.layers + other.gen_layers):
        assert "_imdbn_desc" not in b.__dict__ and b.W.is_contiguous()
        for k in ("W", "hid_bias", "vis_bias"):
            assert torch.equal(getattr(a, k).data, getattr(b, k).data)
        for k in ("W_m", "hb_m", "vb_m"):
            assert torch.equal(getattr(a, k), getattr(b, k))
    tied, _ = _net()
    tied.save_model(path)
    other.load_model(path)
    assert not other.is_untied()


def test_updown_step_issues_the_sequence_and_matches_the_twin(double):
    import pcd_oracle as P
    from oracle.draws import PhiloxStream
    net, X = _net((12, 7, 6, 5))
    x = X[:8]
    as_case = lambda r: dict(W=r.W.data.numpy().copy(), b=r.vis_bias.data.numpy().copy(), c=r.hid_bias.data.numpy().copy(), groups=[])
    mk = lambda r: P.rbm_state(as_case(r), r.lr, r.weight_decay, r.momentum)
    rec = [mk(r) for r in net.layers]
    gen = [mk(r) for r in net.layers[:-1]]
    for s in rec + gen:
        s.W_m[...] = 0; s.hb_m[...] = 0; s.vb_m[...] = 0
    E.manual_seed(9)
    m = net.updown_step(x, 2, 10, CD=2, lr_scale=0.5)
    lr, mom = net.layers[0]._lr_mom(2)
    rng = PhiloxStream(9)
    want = U.updown_step(rec, gen, x.numpy(), [(lr * 0.5, mom)] * 3, 2, rng)
    assert E.get_rng().offset == rng.offset
    kinds = [c[0] if c[0] != "delta_step" else c[:2] for c in double.calls]
    assert kinds == ["updown_step", "pcd_step", ("delta_step", "down"), ("delta_step", "down"), ("delta_step", "up"), ("delta_step", "up")]
    for a, s in zip(net.layers + net.gen_layers, rec + gen):
        np.testing.assert_array_equal(a.W.data.numpy(), s.W)
        np.testing.assert_array_equal(a.vis_bias.data.numpy(), s.vis_bias)
        np.testing.assert_array_equal(a.hid_bias.data.numpy(), s.hid_bias)
    assert set(m) == {"wake_nll", "sleep_nll", "top_loss"} and all(v.dim() == 0 for v in m.values())
    assert abs(float(m["wake_nll"]) - want["wake_nll"]) < 1e-12 and abs(float(m["sleep_nll"]) - want["sleep_nll"]) < 1e-12
    assert float(m["top_loss"]) == float(want["top_loss"])


def test_monitor_off_returns_none_and_evaluates_nothing(double):
    net, X = _net()
    E.manual_seed(3)
    assert net.updown_step(X[:8], 0, 1, monitor=False) is None
    assert [c for c in double.calls if c[0] == "pcd_step"][0][3] is False
    assert all(c[4] is False for c in double.calls if c[0] == "delta_step")


def test_persistent_uses_the_top_rbms_own_chains(double):
    net, X = _net()
    E.manual_seed(3)
    net.updown_step(X[:8], 0, 1, persistent=True)
    chains = net.layers[-1]._pcd
    assert tuple(chains.shape) == (8, net.layers[-1].num_visible)
    before = chains.clone()
    net.updown_step(X[:8], 0, 1, persistent=True)
    assert net.layers[-1]._pcd is chains and not torch.equal(chains, before)
    assert "_pcd" not in net.layers[0].__dict__


def test_data_parallel_raises(double, monkeypatch):
    net, X = _net()
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        net.updown_step(X[:8], 0, 1)
    with pytest.raises(NotImplementedError):
        double.updown_step(net.layers, net.untie(), X[:8], [(0.1, 0.5)] * 2, 1, None, E.get_rng())


def test_finetune_updown_is_explicit_and_reads_the_host_once_per_logged_epoch(double):
    net, X = _net()
    E.manual_seed(4)
    net.train(1)
    assert not net.is_untied() and not any(c[0] == "updown_step" for c in double.calls)
    net.finetune_updown(3, log_every=2)
    assert net.is_untied() and sum(c[0] == "updown_step" for c in double.calls) == 9
    assert [h[0] for h in net.updown_history] == [0, 2] and all(len(h) == 4 and np.isfinite(h[1:]).all() for h in net.updown_history)


# ---- 4. the untied likelihood right after untie() -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["entropy", "logq"])
def test_untied_sample_values_equal_the_tied_ones_right_after_untie(double, mode):
    from imdbn.utils import likelihood as LK
    net, X = _net((12, 7, 6, 5))
    tied = LK.dbn_sample_values(net, X[:6], 1.5, n_samples=3, mode=mode, seed=8)
    assert not any(c[0] == "delta_step" for c in double.calls)
    net.untie()
    untied = LK.dbn_sample_values(net, X[:6], 1.5, n_samples=3, mode=mode, seed=8)
    assert sum(c[0] == "delta_step" for c in double.calls) == 4 and untied.dtype == torch.float64 and tuple(untied.shape) == (6, 3)
    # the same fp32 logits summed in float64 twice; in mode entropy the tied twin takes sigmoid in float64 and the untied path's
    # target is the fp32 probability: |x_j| 2^-24 per hidden unit.  1e-4 is below the 1e-5 per-unit budget of the 32 units here
    np.testing.assert_allclose(untied.numpy(), tied.numpy(), rtol=0, atol=1e-4)
    lb = LK.dbn_lower_bound(net, X[:6], 1.5, n_samples=3, seed=8) if mode == "entropy" else LK.dbn_log_likelihood_is(net, X[:6], 1.5, n_samples=3, seed=8)
    assert tuple(lb.shape) == (6,)
