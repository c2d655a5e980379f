"""CPU-only: the twin of the backprop calls (tests/backprop_oracle.py) against finite differences of its own loss, and the host logic
of iDBN.autoencoder_step / finetune_autoencoder through the engine double (tests/backprop_engine_double.py).  No claim about the
kernels is made here -- those are tested on the GPU in test_backprop_gpu.py."""
import io
import pickle

import numpy as np
import pytest
import torch

import backprop_cases as Cs
import backprop_oracle as Bp
from backprop_engine_double import BackpropOracleEngine
from imdbn import engine as E

F32, F64 = np.float32, np.float64
PARAMS = {"LEARNING_RATE": 0.1, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95, "LEARNING_RATE_DYNAMIC": True, "CD": 1}


# ---- 1. the twin's step is a gradient step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "h130"])
def test_the_twins_autoencoder_step_is_the_gradient_of_the_loss(name):
    """lr = 1, no momentum, no weight decay: the parameter deltas of one step are minus the gradient of the loss, checked against
    central differences (step 1e-5, float64) at 40 random entries of every tensor -- the tied top W, whose gradient is the sum of
    the two pairs of one weight pass, included; a tensor the loss does not depend on must not move."""
    c = Cs.case(name)
    rec, gen = ([Bp.f64_state(s) for s in ss] for ss in Cs.states(c))
    for s in rec + gen:
        s.weight_decay = 0.0
    x = c["data"].astype(F64)
    before = [{k: getattr(s, k).copy() for k in ("W", "hid_bias", "vis_bias")} for s in rec + gen]
    moved = [Bp.f64_state(s) for s in rec + gen]
    L = len(rec)
    Bp.autoencoder_step(moved[:L], moved[L:], x, [(1.0, 0.0)] * L)
    g = np.random.Generator(np.random.PCG64(17))
    h = 1e-5
    worst = 0.0
    for i, (s, b, m) in enumerate(zip(rec + gen, before, moved)):
        for k in ("W", "hid_bias", "vis_bias"):
            p = getattr(s, k)
            for flat in g.choice(p.size, size=min(40, p.size), replace=False):
                idx = np.unravel_index(flat, p.shape)
                p[idx] = b[k][idx] + h
                up = Bp.xent(rec, gen, x)
                p[idx] = b[k][idx] - h
                dn = Bp.xent(rec, gen, x)
                p[idx] = b[k][idx]
                fd = -(up - dn) / (2 * h)
                delta = getattr(m, k)[idx] - b[k][idx]
                worst = max(worst, abs(delta - fd) / (1e-6 * abs(fd) + 1e-9))
                assert abs(delta - fd) <= 1e-6 * abs(fd) + 1e-9, f"{name}: {'rec' if i < L else 'gen'} {i % L if i < L else i - L} {k}{idx}: {delta} vs {fd}"
    print(f"{name}: largest |delta - fd| / tolerance {worst:.3g}")
    # what the loss does not depend on stays where it was: the visible biases below the top RBM, the twins' hidden biases
    for s, b in zip(moved[:L - 1], before[:L - 1]):
        assert np.array_equal(s.vis_bias, b["vis_bias"])
    for s, b in zip(moved[L:], before[L:]):
        assert np.array_equal(s.hid_bias, b["hid_bias"])


def test_thirty_twin_steps_lower_the_cross_entropy():
    c = Cs.case("odd")
    rec, gen = Cs.states(c)
    xs = [Bp.autoencoder_step(rec, gen, c["data"], [(Cs.LR, Cs.MOM)] * len(rec))["xent"] for _ in range(30)]
    print(f"xent: first {xs[0]:.4f}, last {xs[-1]:.4f}")
    assert xs[-1] < xs[0]


# ---- 2. host logic on the engine double ----------------------------------------------------------------------------------------------
@pytest.fixture
def double():
    eng = BackpropOracleEngine()
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


def _params(r):
    return [getattr(r, k).data.clone() for k in ("W", "hid_bias", "vis_bias")] + [getattr(r, k).clone() for k in ("W_m", "hb_m", "vb_m")]


def test_idbn_autoencoder_step_is_the_hand_issued_engine_calls_and_unties_once(double):
    net, X = _net((12, 7, 6, 5))
    ref, _ = _net((12, 7, 6, 5))
    x = X[:8]
    assert not net.is_untied()
    m0 = net.autoencoder_step(x, 2, 10, lr_scale=0.5)
    gen = net.gen_layers
    m1 = net.autoencoder_step(x, 7, 10, lr_scale=0.5)
    assert net.is_untied() and net.gen_layers is gen and len(gen) == 2
    twins = ref.untie()
    outs = []
    for epoch in (2, 7):
        scalars = [(r._lr_mom(epoch)[0] * 0.5, r._lr_mom(epoch)[1]) for r in ref.layers]
        outs.append(double.autoencoder_step(ref.layers, twins, x, scalars))
    for a, b in zip(net.layers + net.gen_layers, ref.layers + twins):
        assert all(torch.equal(p, q) for p, q in zip(_params(a), _params(b)))
    for m, o in zip((m0, m1), outs):
        assert set(m) == {"xent", "mse"} and all(v.dim() == 0 for v in m.values())
        assert torch.equal(m["xent"], o["xent"]) and torch.equal(m["mse"], o["mse"]) and m["xent"].dtype == torch.float64
        assert tuple(o["recon"].shape) == (8, 12) and tuple(o["code"].shape) == (8, 5)
    assert float(m0["xent"]) > 0 and float(m0["mse"]) > 0


def test_the_step_issues_the_sequence_and_matches_the_twin(double):
    import pcd_oracle as P
    net, X = _net((12, 7, 6, 5))
    x = X[:8]
    as_case = lambda r: dict(W=r.W.data.numpy().copy(), b=r.vis_bias.data.numpy().copy(), c=r.hid_bias.data.numpy().copy(), groups=[])
    mk = lambda r: P.rbm_state(as_case(r), r.lr, r.weight_decay, r.momentum)
    rec = [mk(r) for r in net.layers]
    gen = [mk(r) for r in net.layers[:-1]]
    for s in rec + gen:
        s.W_m[...] = 0; s.hb_m[...] = 0; s.vb_m[...] = 0
    m = net.autoencoder_step(x, 2, 10, lr_scale=0.5)
    lr, mom = net.layers[0]._lr_mom(2)
    want = Bp.autoencoder_step(rec, gen, x.numpy(), [(lr * 0.5, mom)] * 3)
    steps = [c for c in double.calls if c[0] == "backprop_step"]
    # (call, up rows, down rows, apply, want_v, want_h): down the twins, the top RBM evaluate-only and with both pairs, up the encoder
    assert steps == [("backprop_step", None, (8, 7), True, False, True), ("backprop_step", None, (8, 6), True, False, True),
                     ("backprop_step", None, (8, 5), False, False, True), ("backprop_step", (8, 6), (8, 5), True, True, False),
                     ("backprop_step", (8, 7), None, True, True, False), ("backprop_step", (8, 12), None, True, False, False)]
    # the double's forward pass is the fp32 oracle's, the twin's float64: the parameters agree to fp32 rounding of the activations
    for a, s in zip(net.layers + net.gen_layers, rec + gen):
        np.testing.assert_allclose(a.W.data.numpy(), s.W, rtol=0, atol=2e-6)
        np.testing.assert_allclose(a.vis_bias.data.numpy(), s.vis_bias, rtol=0, atol=2e-6)
        np.testing.assert_allclose(a.hid_bias.data.numpy(), s.hid_bias, rtol=0, atol=2e-6)
    assert abs(float(m["xent"]) - want["xent"]) < 1e-4 and abs(float(m["mse"]) - want["mse"]) < 1e-6


def test_monitor_off_returns_none_and_evaluates_nothing(double):
    net, X = _net()
    assert net.autoencoder_step(X[:8], 0, 1, monitor=False) is None
    assert not any(c[0] == "delta_step" for c in double.calls)
    out = double.autoencoder_step(net.layers, net.gen_layers, X[:8], [(0.1, 0.5)] * 2, monitor=False)
    assert out["xent"] is None and out["mse"] is None and out["recon"] is not None and out["code"] is not None


def test_a_model_that_is_never_fine_tuned_keeps_its_attributes_and_its_pickle(double, tmp_path):
    net, X = _net()
    keys, raw = sorted(net.__dict__), _dump(net)
    net.represent(X[:4]); net.decode(net.represent(X[:4])); net.reconstruct(X[:4])
    assert "autoencoder_history" not in net.__dict__ and not net.is_untied()
    assert not any(c[0] in ("autoencoder_step", "backprop_step") for c in double.calls)
    assert sorted(net.__dict__) == keys and _dump(net) == raw
    path = str(tmp_path / "tied.pkl")
    net.save_model(path)
    assert open(path, "rb").read() == raw


def test_data_parallel_raises(double, monkeypatch):
    net, X = _net()
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        net.autoencoder_step(X[:8], 0, 1)
    with pytest.raises(NotImplementedError):
        double.autoencoder_step(net.layers, net.untie(), X[:8], [(0.1, 0.5)] * 2)


def test_finetune_autoencoder_is_explicit_and_fills_the_history_on_watched_epochs_only(double):
    net, X = _net()
    E.manual_seed(4)
    net.train(1)
    assert not net.is_untied() and not any(c[0] == "autoencoder_step" for c in double.calls)
    net.finetune_autoencoder(3, log_every=2)
    assert net.is_untied() and sum(c[0] == "autoencoder_step" for c in double.calls) == 9
    assert [h[0] for h in net.autoencoder_history] == [0, 2] and all(len(h) == 3 and np.isfinite(h[1:]).all() for h in net.autoencoder_history)
    # the monitors are evaluated on watched epochs only: one evaluate-only delta_step per watched step
    assert sum(c[0] == "delta_step" for c in double.calls) == 6
    net.finetune_autoencoder(1)
    assert len(net.autoencoder_history) == 2
