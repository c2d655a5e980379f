"""CPU-only: the twin of the Gaussian-visible update (tests/gauss_oracle.py) against the exact model, the pinned seeds of
tests/gauss_cases.py, and the host logic of GaussianRBM / iDBN(GAUSSIAN_VISIBLE) through the engine double
(tests/gauss_engine_double.py).  No claim about the kernels is made here -- those are tested on the GPU in test_gauss_gpu.py."""
import pickle

import numpy as np
import pytest
import torch

import gauss_cases as Gc
import gauss_oracle as G
import pcd_cases as Cs
from gauss_engine_double import GaussOracleEngine
from imdbn import engine as E
from oracle.draws import PhiloxStream

F32, F64 = np.float32, np.float64
SIX = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")


# ---- 1. the gradient against the exact model ---------------------------------------------------------------------------------------
def _tiny(seed=5, V=4, H=3, n=7):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.standard_normal((V, H)) * 0.6, g.standard_normal(V) * 0.5, g.standard_normal(H) * 0.5, -0.7 + 1.4 * g.random(V),
            g.standard_normal((n, V)) * 1.3 + 0.4)


def test_the_twins_gradient_with_exact_model_expectations_is_the_gradient_of_the_exact_log_likelihood():
    """V = 4, H = 3: h enumerated, v integrated in closed form.  Central differences of the exact mean log-likelihood in float64
    against (gW, gb, gc, gz) of the twin's formulas fed with exact model expectations: 1e-6 relative.  Pins gz, the r_i identity
    included."""
    W, b, c, z, data = _tiny()
    st = G.GState(W, b, c, z)
    got = dict(zip("Wbcz", G.exact_gradients(st, data)))
    eps = 1e-5
    worst = 0.0
    for k in "Wbcz":
        p = dict(W=W, b=b, c=c, z=z)
        num = np.zeros_like(p[k])
        for idx in np.ndindex(p[k].shape):
            hi, lo = {q: v.copy() for q, v in p.items()}, {q: v.copy() for q, v in p.items()}
            hi[k][idx] += eps
            lo[k][idx] -= eps
            num[idx] = (G.mean_log_likelihood(hi["W"], hi["b"], hi["c"], hi["z"], data)
                        - G.mean_log_likelihood(lo["W"], lo["b"], lo["c"], lo["z"], data)) / (2 * eps)
        rel = float(np.abs(num - got[k]).max() / np.abs(num).max())
        print(f"d/d{k}: largest |finite difference - twin| / largest |gradient| {rel:.3g}")
        worst = max(worst, rel)
    assert worst <= 1e-6


def test_the_twins_sampled_gradient_uses_the_same_formulas_as_the_exact_one():
    """With the model expectation replaced by ONE hidden state of probability 1 (c pushed far out) the CD statistics of the mean
    (sample_v off, so v = m) miss only sigma^2 in q1: gz differs from the exact one by exactly 1/2, everything else agrees."""
    W, b, c, z, data = _tiny()
    c = np.array([40.0, -40.0, 40.0])
    st = G.GState(W, b, c, z)
    exact = G.exact_gradients(st, data)
    rec = {}
    G.cd_step(st.copy(), data, 1, PhiloxStream(3), 0.0, 0.0, 0.0, sample_v=False, record=rec)
    gW, gb, gc, gz = rec["g"]
    assert np.allclose(gW, exact[0], atol=1e-12) and np.allclose(gb, exact[1], atol=1e-12) and np.allclose(gc, exact[2], atol=1e-12)
    assert np.allclose(gz, exact[3] + 0.5, atol=1e-12)


# ---- 2. seeds and tolerances ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Gc.CASES)
def test_the_pinned_seed_is_the_first_with_clear_margins(name):
    c = Gc.case(name)
    first = next(s for s in range(1, 65) if Gc.seed_ok(c, s))
    assert first == c["seed"]
    for k in c["cd_ks"]:
        for sv in (True, False):
            t = Gc.twin_run(c, k, sv)
            assert t["offset"] == k * (1 + sv) and len(t["rec"]["h"]) == k and len(t["rec"]["m"]) == k


def test_the_fp32_restatement_stays_inside_an_eighth_of_the_gpu_tolerances():
    err = Gc.fp32_errors()
    print("fp32 restatement vs float64 twin:", err)
    assert 0 < err["z"] < 1e-5 and 0 < err["z_m"] < 1e-5 and 0 < err["F"] < 1e-3


def test_fixed_variances_and_clamps_in_the_twin():
    c = Gc.case("odd")
    t = Gc.twin_run(c, 1, True, lr_z=0.0)
    assert np.array_equal(t["st"].z, c["z"].astype(F64)) and np.array_equal(t["st"].z_m, c["z_m"].astype(F64))
    st = Gc.state(c)
    G.cd_step(st, c["data"], 1, PhiloxStream(1), Gc.LR, Gc.MOM, 5.0, z_lo=-0.25, z_hi=0.5)
    assert st.z.min() >= -0.25 and st.z.max() <= 0.5 and (st.z == -0.25).any() and (st.z == 0.5).any()


# ---- 3. host logic through the engine double ---------------------------------------------------------------------------------
@pytest.fixture
def double():
    eng = GaussOracleEngine()
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
    if hasattr(r, "logvar"):
        r.logvar_m = torch.zeros_like(r.logvar.data)
    return r


def _grbm(c, **kw):
    from imdbn.models import GaussianRBM
    r = _on_cpu(GaussianRBM(c["V"], c["H"], Gc.LR, Gc.WEIGHT_DECAY, Gc.MOM, **kw), c["W"], c["b"], c["c"])
    r.logvar.data.copy_(torch.from_numpy(c["z"]))
    return r


def test_shapes_and_draws_of_the_model_class(double):
    c = Gc.case("odd")
    r = _grbm(c)
    x = torch.from_numpy(c["data"])
    B, V, H = x.shape[0], c["V"], c["H"]
    E.manual_seed(11)
    try:
        rng = E.get_rng()
        h = r.forward(x)
        assert h.shape == (B, H) and h._imdbn_binary is False and rng.offset == 0
        m = r.backward(h)
        assert m.shape == (B, V) and torch.equal(m, r.visible_probs(h)) and torch.equal(m, r.backward(h, return_logits=True))
        assert r.free_energy(x).shape == (B,) and rng.offset == 0
        v = r.sample_visible(m)
        assert v.shape == (B, V) and rng.offset == 1 and not torch.equal(v, m)
        assert r.backward_sample(h).shape == (B, V) and rng.offset == 2
        out = r.gibbs_step(x)
        assert [t.shape for t in out] == [(B, V), (B, V), (B, H), (B, H)] and rng.offset == 4
        out = r.gibbs_step(x, sample_h=False, sample_v=False)
        assert torch.equal(out[0], out[1]) and torch.equal(out[2], out[3]) and rng.offset == 4
        for cd, sv, used in ((1, True, 2), (2, True, 4), (2, False, 2), (1, False, 1)):
            before = rng.offset
            loss = r.train_epoch(x, 0, 5, CD=cd, sample_v=sv)
            assert loss.shape == () and rng.offset - before == used
        assert r.train_epoch(x, 0, 5, monitor=False) is None
        with pytest.raises(ValueError, match="visible_probs"):
            r.visible_probs(h, T=2.0)
    finally:
        E.set_rng(None)
    assert double.calls[-1] == ("gauss_cd_step", (B, V), 1, True, Gc.LR, False)


def test_train_epoch_is_the_twin_and_follows_the_schedule(double):
    c = Gc.case("h130")
    r = _grbm(c, lr_sigma_mult=0.5, dynamic_lr=True, final_momentum=0.8, sparsity=True, sparsity_factor=Gc.SPARSITY_TARGET)
    r.W_m, r.hb_m, r.vb_m = (torch.from_numpy(c[k].copy()) for k in ("W_m", "hb_m", "vb_m"))
    r.logvar_m = torch.from_numpy(c["z_m"].copy())
    E.manual_seed(c["seed"])
    try:
        loss = r.train_epoch(torch.from_numpy(c["data"]), 7, 10)
    finally:
        E.set_rng(None)
    lr, mom = Gc.LR / 1.07, 0.8
    assert double.calls[-1][4] == pytest.approx(0.5 * lr)
    st = Gc.state(c, F32)
    want = G.cd_step(st, c["data"], 1, PhiloxStream(c["seed"]), lr, mom, 0.5 * lr)
    assert float(loss) == float(want) and np.array_equal(r.logvar.data.numpy(), st.z) and np.array_equal(r.logvar_m.numpy(), st.z_m)
    assert np.array_equal(r.W.data.numpy(), st.W) and np.array_equal(r.hid_bias.data.numpy(), st.c) and np.array_equal(r.vis_bias.data.numpy(), st.b)


def test_lr_sigma_mult_zero_leaves_logvar_bit_identical_and_the_clamps_hold(double):
    c = Gc.case("odd")
    x = torch.from_numpy(c["data"])
    r = _grbm(c, lr_sigma_mult=0.0)
    r.logvar_m = torch.from_numpy(c["z_m"].copy())
    E.manual_seed(1)
    try:
        for ep in range(3):
            r.train_epoch(x, ep, 3)
        assert np.array_equal(r.logvar.data.numpy(), c["z"]) and np.array_equal(r.logvar_m.numpy(), c["z_m"])
        r2 = _grbm(c, lr_sigma_mult=100.0, logvar_min=-0.25, logvar_max=0.5)
        for ep in range(3):
            r2.train_epoch(x, ep, 3)
    finally:
        E.set_rng(None)
    z = r2.logvar.data
    assert float(z.min()) >= -0.25 and float(z.max()) <= 0.5 and bool((z == -0.25).any()) and bool((z == 0.5).any())
    from imdbn.models import GaussianRBM
    with pytest.raises(ValueError, match="logvar_min"):
        GaussianRBM(4, 3, 0.1, 0.0, 0.5, logvar_min=1.0, logvar_max=0.0)


def test_init_from_data(double):
    c = Gc.case("odd")
    data = c["data"].copy()
    data[:, 3] = 0.75                                     # a constant column: its variance is floored
    r = _grbm(c).init_from_data(torch.from_numpy(data))
    var = data.astype(F64).var(0)
    floor = var[var > 0].min()
    assert np.allclose(r.vis_bias.data.numpy(), data.astype(F64).mean(0), atol=1e-6)
    assert np.allclose(r.logvar.data.numpy(), np.log(np.where(var > 0, var, floor)), atol=1e-5)
    assert r.logvar.data[3] == r.logvar.data.min() and torch.allclose(r.variances(), torch.exp(r.logvar.data))


def test_pickle_round_trip(double):
    from imdbn.models import GaussianRBM
    c = Gc.case("odd")
    r = _grbm(c, lr_sigma_mult=0.3, logvar_min=-2.0, logvar_max=3.0)
    E.manual_seed(2)
    try:
        r.train_epoch(torch.from_numpy(c["data"]), 0, 1)
    finally:
        E.set_rng(None)
    q = pickle.loads(pickle.dumps(r))
    assert isinstance(q, GaussianRBM) and "_imdbn_desc" not in q.__dict__
    assert (q.lr_sigma_mult, q.logvar_min, q.logvar_max) == (0.3, -2.0, 3.0)
    assert torch.equal(q.logvar.data, r.logvar.data) and torch.equal(q.logvar_m, r.logvar_m) and q.logvar_m.abs().sum() > 0
    for k in SIX:
        assert torch.equal(getattr(q, k), getattr(r, k)), k
    x = torch.from_numpy(c["data"])
    assert torch.equal(q.free_energy(x), r.free_energy(x))


def test_every_method_that_assumes_bernoulli_visibles_raises(double, monkeypatch):
    from imdbn.models import grbm
    from imdbn.utils import likelihood as LK
    c = Gc.case("odd")
    r = _grbm(c)
    x = torch.from_numpy(c["data"])
    n = len(double.calls)
    for name in grbm.REFUSED:
        with pytest.raises(ValueError, match=name):
            getattr(r, name)(x, x, 0, 1)
    for fn in (LK.estimate_log_partition, lambda m: LK.log_likelihood(m, x, 0.0), lambda m: LK.pseudo_log_likelihood(m, x),
               lambda m: LK.reverse_ais_log_likelihood(m, x), lambda m: LK.dbn_lower_bound(m, x, 0.0)):
        with pytest.raises(ValueError, match="Gaussian"):
            fn(r)
    assert len(double.calls) == n                         # nothing reached the engine
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        r.train_epoch(x, 0, 1)


# ---- 4. iDBN -------------------------------------------------------------------------------------------------------------------------
def _idbn(params, eng, epochs=2):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import iDBN
    E.set_engine_for_testing(eng)
    torch.manual_seed(0)
    g = np.random.Generator(np.random.PCG64(3))
    X = torch.from_numpy((0.5 + 2.0 * g.standard_normal((20, 12))).astype(F32))
    dl = DataLoader(TensorDataset(X, torch.zeros(20)), batch_size=8)
    net = iDBN([12, 7, 5], dict({"LEARNING_RATE": 0.05, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95,
                                 "LEARNING_RATE_DYNAMIC": True, "CD": 1}, **params), dl, dl, torch.device("cpu"))
    for r in net.layers:
        _on_cpu(r)
    E.manual_seed(4)
    try:
        net.train(epochs)
    finally:
        E.set_rng(None)
    return net, X


def test_a_default_idbn_builds_no_gaussian_rbm_and_the_flag_makes_layer_zero_one():
    from imdbn.models import RBM, GaussianRBM
    try:
        eng = GaussOracleEngine()
        plain, _ = _idbn({}, eng)
        assert all(type(r) is RBM for r in plain.layers) and not any(c[0].startswith("gauss") for c in eng.calls)
        off, _ = _idbn({"GAUSSIAN_VISIBLE": False}, GaussOracleEngine())
        assert all(type(r) is RBM for r in off.layers)
        eng = GaussOracleEngine()
        net, X = _idbn({"GAUSSIAN_VISIBLE": True, "GAUSSIAN_LR_SIGMA_MULT": 0.25, "GAUSSIAN_LOGVAR_MIN": -3.0}, eng)
        assert type(net.layers[0]) is GaussianRBM and type(net.layers[1]) is RBM
        assert (net.layers[0].lr_sigma_mult, net.layers[0].logvar_min, net.layers[0].logvar_max) == (0.25, -3.0, float("inf"))
        per_batch = lambda rows: ["gauss_cd_step", "gauss_forward", "cd_step"]
        assert [c[0] for c in eng.calls] == per_batch(8) * 6
        assert net.layers[0].logvar.data.abs().sum() > 0 and len(net.loss_history) == 2 and net.loss_history[0].shape == (6,)
        z = net.represent(X)
        assert z.shape == (20, 5) and float(z.min()) >= 0 and float(z.max()) <= 1
        assert net.represent(X, upto_layer=1).shape == (20, 7) and net.reconstruct(X).shape == (20, 12)
        for who, call in (("untie", lambda: net.untie()), ("updown_step", lambda: net.updown_step(X, 0, 1)),
                          ("autoencoder_step", lambda: net.autoencoder_step(X, 0, 1)),
                          ("log_likelihood_bound", lambda: net.log_likelihood_bound(X, 0.0)),
                          ("log_likelihood_bound_conservative", lambda: net.log_likelihood_bound_conservative(X))):
            with pytest.raises(ValueError, match=who):
                call()
        assert not net.is_untied()
    finally:
        E.set_engine_for_testing(None)


# ---- 5. learning ---------------------------------------------------------------------------------------------------------------------
def test_cd1_on_a_gaussian_mixture_raises_the_exact_log_likelihood_and_moves_the_variances(double):
    """20 CD-1 epochs on a 2-component mixture in 6 dimensions, H = 4, through the double: the exact mean log-likelihood (the
    enumerator of test 1) rises from the first epoch to the last, and the learned sigma^2 move from 1 towards the
    within-component variance.  Direction only."""
    from imdbn.models import GaussianRBM
    g = np.random.Generator(np.random.PCG64(21))
    V, H, n, within = 6, 4, 200, 0.25
    centres = np.stack([np.full(V, 1.0), np.full(V, -1.0)])
    X = (centres[g.integers(0, 2, n)] + np.sqrt(within) * g.standard_normal((n, V))).astype(F32)
    torch.manual_seed(0)
    r = _on_cpu(GaussianRBM(V, H, 0.02, 0.0, 0.5, lr_sigma_mult=1.0))
    ll = lambda: G.mean_log_likelihood(*(t.detach().numpy().astype(F64) for t in (r.W.data, r.vis_bias.data, r.hid_bias.data, r.logvar.data)), X)
    E.manual_seed(9)
    lls = []
    try:
        for ep in range(20):
            for i in range(0, n, 50):
                r.train_epoch(torch.from_numpy(X[i:i + 50]), ep, 20)
            lls.append(ll())
    finally:
        E.set_rng(None)
    var = r.variances().numpy()
    print(f"exact mean log-likelihood: epoch 1 {lls[0]:.4f}, epoch 20 {lls[-1]:.4f}; sigma^2 {np.round(var, 3)}")
    assert lls[-1] > lls[0]
    assert (var < 1.0).all() and (np.abs(var - within) < np.abs(1.0 - within)).all()
