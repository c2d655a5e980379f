"""CPU-only: the twin of the Gaussian backprop calls (tests/gauss_backprop_oracle.py) against finite differences of its own loss, and
the host logic of iDBN.gaussian_untie / gaussian_autoencoder_step / finetune_gaussian_autoencoder through the engine double
(tests/gauss_backprop_engine_double.py).  No claim about the kernels is made here -- those are tested on the GPU in
test_gauss_backprop_gpu.py."""
import io
import pickle

import numpy as np
import pytest
import torch

import gauss_backprop_cases as Cs
import gauss_backprop_oracle as Go
import gauss_oracle as G
from gauss_backprop_engine_double import GaussBackpropOracleEngine
from imdbn import engine as E

F32, F64 = np.float32, np.float64
PARAMS = {"LEARNING_RATE": 0.02, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.9, "LEARNING_RATE_DYNAMIC": True, "CD": 1,
          "GAUSSIAN_VISIBLE": True, "GAUSSIAN_LR_SIGMA_MULT": 0.5}


# ---- 1. the twin's step is a gradient step ------------------------------------------------------------------------------------------
def _fd_stack(sizes, L):
    """Float64 states of a random stack of `sizes` cut to `L` layers, and a real batch."""
    g = np.random.Generator(np.random.PCG64(23 + len(sizes) + sizes[0]))
    n = lambda *s: g.standard_normal(s)
    V, H = sizes[0], sizes[1]
    rec = [G.GState(n(V, H) * 0.4, n(V) * 0.3, n(H) * 0.3, -0.5 + g.random(V))]
    for a, b in zip(sizes[1:L], sizes[2:L + 1]):
        rec.append(Go.bern_state(n(a, b) * 0.4, n(b) * 0.3, n(a) * 0.3))
    gen = []
    for i, r in enumerate(rec[:-1]):               # twins that differ from the layers: an untied model some steps in
        if i == 0:
            gen.append(G.GState(r.W + n(V, H) * 0.05, r.b + n(V) * 0.05, r.c, r.z + n(V) * 0.1))
        else:
            gen.append(Go.bern_state(r.W + n(*r.W.shape) * 0.05, r.hid_bias, r.vis_bias + n(*r.vis_bias.shape) * 0.05))
    x = 0.3 + 1.5 * n(6, V)
    return rec, gen, x


def _copy(s):
    if isinstance(s, G.GState):
        return s.copy()
    return Go.bern_state(s.W, s.hid_bias, s.vis_bias, s.weight_decay, F64, s.W_m, s.hb_m, s.vb_m)


def _tensors(s):
    return ("W", "b", "c", "z") if isinstance(s, G.GState) else ("W", "hid_bias", "vis_bias")


@pytest.mark.parametrize("sizes,L", [((6, 5, 4), 2), ((7, 4), 1), ((5, 3), 1), ((6, 5, 4, 3), 3)], ids=["6-5-4", "7-4", "5-3-tied", "6-5-4-3"])
def test_the_twins_step_is_the_gradient_of_the_gaussian_loss(sizes, L):
    """lr = 1, lr_sigma_mult = 1, no momentum, no weight decay: the parameter deltas of one step are minus the gradient of J, checked
    against central differences (step 1e-5, float64) of the twin's own J at 40 random entries of every tensor -- every W, both biases,
    the encoder's z and the decoder's zeta; with one layer z is tied and receives gzeta + gz.  A tensor J does not depend on must
    not move."""
    rec, gen, x = _fd_stack(sizes, L)
    before = [{k: getattr(s, k).copy() for k in _tensors(s)} for s in rec + gen]
    moved = [_copy(s) for s in rec + gen]
    Go.autoencoder_step(moved[:L], moved[L:], x, [(1.0, 0.0)] * L, (1.0, -np.inf, np.inf))
    g = np.random.Generator(np.random.PCG64(17))
    h = 1e-5
    worst = 0.0
    for i, (s, b, m) in enumerate(zip(rec + gen, before, moved)):
        for k in _tensors(s):
            p = getattr(s, k)
            for flat in g.choice(p.size, size=min(40, p.size), replace=False):
                idx = np.unravel_index(flat, p.shape)
                p[idx] = b[k][idx] + h
                up = Go.nll(rec, gen, x)
                p[idx] = b[k][idx] - h
                dn = Go.nll(rec, gen, x)
                p[idx] = b[k][idx]
                fd = -(up - dn) / (2 * h)
                delta = getattr(m, k)[idx] - b[k][idx]
                worst = max(worst, abs(delta - fd) / (1e-6 * abs(fd) + 1e-9))
                assert abs(delta - fd) <= 1e-6 * abs(fd) + 1e-9, f"{sizes}: {'rec' if i < L else 'gen'} {i % L if i < L else i - L} {k}{idx}: {delta} vs {fd}"
    print(f"{sizes}: largest |delta - fd| / tolerance {worst:.3g}")
    if L > 1:      # J does not depend on: the encoder's visible bias, the visible biases below the top RBM, the twins' hidden biases
        assert np.array_equal(moved[0].b, before[0]["b"])
        for s, b in zip(moved[1:L - 1], before[1:L - 1]):
            assert np.array_equal(s.vis_bias, b["vis_bias"])
        assert np.array_equal(moved[L].c, before[L]["c"])
        assert not np.array_equal(moved[L].z, before[L]["z"]) and not np.array_equal(moved[0].z, before[0]["z"])


def test_the_fp32_restatement_stays_near_the_twin():
    e = Cs.fp32_errors()
    print("fp32 restatement vs float64 twin:", e)
    assert all(0 < v < 1e-4 for v in e.values())


# ---- 2. host logic on the engine double ----------------------------------------------------------------------------------------------
@pytest.fixture
def double():
    eng = GaussBackpropOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)


def _net(sizes=(12, 7, 5), **extra):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import iDBN
    torch.manual_seed(0)
    g = np.random.Generator(np.random.PCG64(3))
    X = (0.5 + 2.0 * g.standard_normal((20, sizes[0])))
    X = torch.from_numpy(((X - X.mean(0)) / X.std(0)).astype(F32))       # a fixed standardised 20 x 12 batch
    dl = DataLoader(TensorDataset(X, torch.zeros(20)), batch_size=20)
    net = iDBN(list(sizes), dict(PARAMS, **extra), dl, dl, torch.device("cpu"))
    for r in net.layers:
        r.to("cpu")
        r.W.data = r.W.data.contiguous()
        r.hid_bias.data.normal_(0, 0.3); r.vis_bias.data.normal_(0, 0.3)
        r.W_m, r.hb_m, r.vb_m = torch.zeros_like(r.W.data), torch.zeros_like(r.hid_bias.data), torch.zeros_like(r.vis_bias.data)
    net.layers[0].logvar.data.uniform_(-0.3, 0.3)
    return net, X


def _params(r):
    out = [getattr(r, k).data.clone() for k in ("W", "hid_bias", "vis_bias")] + [getattr(r, k).clone() for k in ("W_m", "hb_m", "vb_m")]
    if hasattr(r, "logvar"):
        out += [r.logvar.data.clone(), r.logvar_m.clone()]
    return out


def test_gaussian_untie_builds_the_twins_once_and_without_draws(double):
    from imdbn.models import RBM, GaussianRBM
    net, X = _net((12, 7, 6, 5), GAUSSIAN_LOGVAR_MIN=-2.0, GAUSSIAN_LOGVAR_MAX=1.5)
    state = torch.get_rng_state()
    gen = net.gaussian_untie()
    assert torch.equal(torch.get_rng_state(), state)
    assert net.is_untied() and net.gaussian_untie() is gen and len(gen) == 2
    g0, r0 = gen[0], net.layers[0]
    assert type(g0) is GaussianRBM and type(gen[1]) is RBM
    for g, r in zip(gen, net.layers):
        assert g.W.shape == r.W.shape and g.W.stride() == r.W.stride() and g.W_m.stride() == r.W.stride()
        assert torch.equal(g.W.data, r.W.data) and g.W.data_ptr() != r.W.data_ptr() and torch.equal(g.vis_bias.data, r.vis_bias.data)
        assert not g.W_m.any() and not g.hb_m.any() and not g.vb_m.any()
        assert (g.lr, g.weight_decay, g.momentum, g.final_momentum, g.dynamic_lr) == (r.lr, r.weight_decay, r.momentum, r.final_momentum, r.dynamic_lr)
    assert torch.equal(g0.logvar.data, r0.logvar.data) and g0.logvar.data_ptr() != r0.logvar.data_ptr() and not g0.logvar_m.any()
    assert (g0.lr_sigma_mult, g0.logvar_min, g0.logvar_max) == (0.5, -2.0, 1.5) == (r0.lr_sigma_mult, r0.logvar_min, r0.logvar_max)


def test_the_bernoulli_passes_still_refuse_a_gaussian_stack_and_a_default_stack_refuses_gaussian_untie(double):
    net, X = _net()
    for untied in (False, True):
        if untied:
            net.gaussian_untie()
        for call in (net.untie, lambda: net.updown_step(X[:8], 0, 1), lambda: net.autoencoder_step(X[:8], 0, 1)):
            with pytest.raises(ValueError, match="GaussianRBM"):
                call()
        for call in (lambda: net.gaussian_log_likelihood_bound(X[:4], 0.0), lambda: net.gaussian_log_likelihood_bound_conservative(X[:4])):
            if untied:
                with pytest.raises(NotImplementedError):
                    call()
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import iDBN
    dl = DataLoader(TensorDataset(X, torch.zeros(20)), batch_size=8)
    plain = iDBN([12, 7, 5], {k: v for k, v in PARAMS.items() if not k.startswith("GAUSSIAN")}, dl, dl, torch.device("cpu"))
    with pytest.raises(ValueError, match="gaussian_untie"):
        plain.gaussian_untie()
    with pytest.raises(ValueError, match="gaussian_untie"):
        plain.gaussian_autoencoder_step(X[:8], 0, 1)
    assert not plain.is_untied()


@pytest.mark.parametrize("sizes", [(12, 7, 6, 5), (12, 7, 5), (12, 7)], ids=["L3", "L2", "L1"])
def test_the_step_issues_the_sequence_and_matches_the_twin(double, sizes):
    net, X = _net(sizes)
    L = len(sizes) - 1
    x = X[:8]
    r0 = net.layers[0]
    rec = [G.GState(r0.W.data.numpy(), r0.vis_bias.data.numpy(), r0.hid_bias.data.numpy(), r0.logvar.data.numpy(), weight_decay=r0.weight_decay)]
    rec += [Go.bern_state(r.W.data.numpy(), r.hid_bias.data.numpy(), r.vis_bias.data.numpy(), r.weight_decay) for r in net.layers[1:]]
    gen = [_copy(s) for s in rec[:-1]]
    want_recon = None
    m = net.gaussian_autoencoder_step(x, 2, 10, lr_scale=0.5)
    assert set(m) == {"nll", "mse"} and all(v.dim() == 0 for v in m.values())
    lr, mom = net.layers[0]._lr_mom(2)
    want = Go.autoencoder_step(rec, gen, x.numpy(), [(lr * 0.5, mom)] * L, (0.5, -np.inf, np.inf))
    steps = [c[:6] for c in double.calls if c[0] in ("backprop_step", "gauss_backprop_step")]
    B = 8
    if L == 1:       # (call, up rows, down rows, apply, want_h, monitor)
        assert steps == [("gauss_backprop_step", None, (B, 7), False, True, True), ("gauss_backprop_step", (B, 7), (B, 7), True, False, False)]
    elif L == 2:
        assert steps == [("gauss_backprop_step", None, (B, 7), True, True, True), ("backprop_step", None, (B, 5), False, False, True),
                         ("backprop_step", (B, 7), (B, 5), True, True, False), ("gauss_backprop_step", (B, 7), None, True, False, False)]
    else:
        assert steps == [("gauss_backprop_step", None, (B, 7), True, True, True), ("backprop_step", None, (B, 6), True, False, True),
                         ("backprop_step", None, (B, 5), False, False, True), ("backprop_step", (B, 6), (B, 5), True, True, False),
                         ("backprop_step", (B, 7), None, True, True, False), ("gauss_backprop_step", (B, 7), None, True, False, False)]
    lr_zs = [c[6] for c in double.calls if c[0] == "gauss_backprop_step" and c[3]]
    assert all(abs(v - 0.5 * lr * 0.5) < 1e-12 for v in lr_zs)
    models = net.layers + net.gen_layers
    for a, s in zip(models, rec + gen):
        gauss = isinstance(s, G.GState)
        np.testing.assert_allclose(a.W.data.numpy(), s.W, rtol=0, atol=2e-6)
        np.testing.assert_allclose(a.vis_bias.data.numpy(), s.b if gauss else s.vis_bias, rtol=0, atol=2e-6)
        np.testing.assert_allclose(a.hid_bias.data.numpy(), s.c if gauss else s.hid_bias, rtol=0, atol=2e-6)
        if gauss:
            np.testing.assert_allclose(a.logvar.data.numpy(), s.z, rtol=0, atol=2e-6)
            np.testing.assert_allclose(a.logvar_m.numpy(), s.z_m, rtol=0, atol=2e-6)
    assert abs(float(m["nll"]) - want["nll"]) < 1e-4 and abs(float(m["mse"]) - want["mse"]) < 1e-5


def test_reconstruct_after_untying_is_d0_of_the_step_and_a_pickle_keeps_the_twins(double, tmp_path):
    net, X = _net((12, 7, 5))
    x = X[:8]
    net.gaussian_autoencoder_step(x, 0, 5)              # twins now differ from the layers
    net.gaussian_autoencoder_step(x, 1, 5)
    assert not torch.equal(net.gen_layers[0].W.data, net.layers[0].W.data)
    assert not torch.equal(net.gen_layers[0].logvar.data, net.layers[0].logvar.data)
    want = net.reconstruct(x)
    scalars = [r._lr_mom(2) for r in net.layers]
    out = double.gauss_autoencoder_step(net.layers, net.gen_layers, x, scalars)
    assert torch.equal(out["recon"], want) and tuple(out["code"].shape) == (8, 5)
    assert torch.equal(net.decode(net.represent(x)), net.reconstruct(x))
    path = str(tmp_path / "untied.pkl")
    net.save_model(path)
    other, _ = _net((12, 7, 5))
    other.load_model(path)
    assert other.is_untied() and hasattr(other.gen_layers[0], "logvar")
    for a, b in zip(other.layers + other.gen_layers, net.layers + net.gen_layers):
        assert all(torch.equal(p, q) for p, q in zip(_params(a), _params(b)))
    assert torch.equal(other.reconstruct(x), net.reconstruct(x))
    g0 = pickle.load(io.BytesIO(pickle.dumps(net.gen_layers[0])))
    assert torch.equal(g0.logvar.data, net.gen_layers[0].logvar.data) and g0.lr_sigma_mult == 0.5


@pytest.mark.parametrize("sizes", [(12, 7, 5), (12, 7)], ids=["L2", "L1"])
def test_thirty_steps_lower_the_loss(double, sizes):
    net, X = _net(sizes)
    js = [float(net.gaussian_autoencoder_step(X, e, 30)["nll"]) for e in range(30)]
    print(f"J: first {js[0]:.4f}, last {js[-1]:.4f}")
    assert js[-1] < js[0]


def test_lr_sigma_mult_zero_leaves_every_logvar_bit_equal(double):
    net, X = _net((12, 7, 5), GAUSSIAN_LR_SIGMA_MULT=0.0)
    gen = net.gaussian_untie()
    z0, zeta0 = net.layers[0].logvar.data.clone(), gen[0].logvar.data.clone()
    W0 = net.layers[0].W.data.clone()
    for e in range(3):
        net.gaussian_autoencoder_step(X, e, 3)
    assert torch.equal(net.layers[0].logvar.data, z0) and torch.equal(gen[0].logvar.data, zeta0)
    assert not net.layers[0].logvar_m.any() and not gen[0].logvar_m.any() and not torch.equal(net.layers[0].W.data, W0)


def test_the_logvar_clamps_hold(double):
    net, X = _net((12, 7, 5), GAUSSIAN_LR_SIGMA_MULT=200.0, GAUSSIAN_LOGVAR_MIN=-0.375, GAUSSIAN_LOGVAR_MAX=0.5)
    for e in range(3):
        net.gaussian_autoencoder_step(X, e, 3)
    hit = False
    for r in (net.layers[0], net.gen_layers[0]):
        z = r.logvar.data
        assert float(z.min()) >= -0.375 and float(z.max()) <= 0.5
        hit = hit or bool((z == -0.375).any()) or bool((z == 0.5).any())
    assert hit


# ---- 3. monitor off, 4. the history ------------------------------------------------------------------------------------------------------
def test_monitor_off_returns_none(double):
    net, X = _net()
    assert net.gaussian_autoencoder_step(X[:8], 0, 1, monitor=False) is None
    assert not any(c[0] == "gauss_backprop_step" and c[5] for c in double.calls)
    out = double.gauss_autoencoder_step(net.layers, net.gen_layers, X[:8], [(0.01, 0.5)] * 2, monitor=False)
    assert out["nll"] is None and out["mse"] is None and out["recon"] is not None and out["code"] is not None


def test_data_parallel_raises(double, monkeypatch):
    net, X = _net()
    gen = net.gaussian_untie()
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        net.gaussian_autoencoder_step(X[:8], 0, 1)
    with pytest.raises(NotImplementedError):
        double.gauss_autoencoder_step(net.layers, gen, X[:8], [(0.1, 0.5)] * 2)


def test_finetune_fills_the_history_on_watched_epochs_only(double):
    net, X = _net()
    assert "gaussian_autoencoder_history" not in net.__dict__
    net.finetune_gaussian_autoencoder(3, log_every=2)
    assert net.is_untied() and sum(c[0] == "gauss_autoencoder_step" for c in double.calls) == 3
    hist = net.gaussian_autoencoder_history
    assert [h[0] for h in hist] == [0, 2] and all(len(h) == 3 and np.isfinite(h[1:]).all() for h in hist)
    assert sum(c[0] == "gauss_backprop_step" and c[5] for c in double.calls) == 2      # monitors on watched epochs only
    net.finetune_gaussian_autoencoder(1)
    assert len(net.gaussian_autoencoder_history) == 2
