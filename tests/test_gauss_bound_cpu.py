"""CPU-only: the numpy twin of imdbn_rbm_gauss_bound_step (tests/gauss_bound_oracle.py) against the enumerated log-density and
variational bound of a small stack with a Gaussian bottom layer, the host logic of the Gaussian stack bounds of
imdbn/utils/likelihood.py on a test double of the engine, the draw schedule and the export's declaration and binding.

Truth: stacks 6-5-4 and 6-5-4-3 from numpy.random.Generator(PCG64(7)) (W ~ 0.5 N, b_1 ~ 0.5 N, c ~ 0.3 N, z ~ 0.4 N, b_2.. ~ 0.3 N), 8
rows v = b_1 + e^{z/2} n + h W_1^T, under the project's Philox draws.  Statistic: sum over the rows of (estimate - exact) against
sqrt(sum of the rows' se^2); mode entropy with S = 256 against the exact bound, mode logq with S = 2048 against the exact log p (se by
the delta method on the weights); within 3 se.  Seeds 1..8 were run once (`python tests/gauss_bound_cases.py`), 6-5-4, in se:
entropy +0.16 +0.87 +0.07 -0.32 -1.45 +0.56 +0.27 +1.85, logq +1.19 +0.91 +0.66 +0.06 -0.61 -0.08 +1.11 +0.37 -- all sixteen inside
3 se; seed 1 is pinned (gauss_bound_cases.TRUTH_SEED).  The gaps between log p and the bound are 0.73 .. 1.31 nats per row."""
import os
import re

import numpy as np
import pytest
import torch

import anneal_oracle as A
import bound_oracle as B
import gauss_bound_cases as Cs
import gauss_bound_oracle as GB
import gauss_oracle as G
from gauss_engine_double import GaussOracleEngine
from imdbn import engine as E
from imdbn.engine import native, rng as R
from imdbn.utils import likelihood as LK
from oracle.draws import PhiloxStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
PARAMS = {"LEARNING_RATE": 0.05, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95, "LEARNING_RATE_DYNAMIC": True, "CD": 1}


@pytest.fixture()
def double():
    eng = GaussOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)
    E.set_rng(None)


def _grbm(W, b, c, z):
    from imdbn.models import GaussianRBM
    r = GaussianRBM(W.shape[0], W.shape[1], 0.01, 0.0, 0.5).to("cpu")
    r.W.data = torch.from_numpy(np.array(W, F32))
    r.vis_bias.data, r.hid_bias.data = torch.from_numpy(np.array(b, F32)), torch.from_numpy(np.array(c, F32))
    r.logvar.data = torch.from_numpy(np.array(z, F32))
    return r


class _Stack:
    """What the likelihood functions read off a model: its layers (and a loader, a run)."""

    def __init__(self, z, layers):
        self.layers = [_grbm(*layers[0], z)] + [B.host_rbm(l) for l in layers[1:]]


def _net(sizes, seed=0):
    """An ``iDBN`` built with GAUSSIAN_VISIBLE on 16 real-valued rows -> (net, X, z, layers as the twin takes them)."""
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import GaussianRBM, iDBN
    g = np.random.Generator(np.random.PCG64(3))
    X = torch.from_numpy((0.5 + 2.0 * g.standard_normal((16, sizes[0]))).astype(F32))
    dl = DataLoader(TensorDataset(X, torch.zeros(16)), batch_size=8)
    torch.manual_seed(seed)
    net = iDBN(list(sizes), dict(PARAMS, GAUSSIAN_VISIBLE=True), dl, dl, torch.device("cpu"))
    assert isinstance(net.layers[0], GaussianRBM)
    for r in net.layers:
        r.W.data = (r.W.data * 20).contiguous()              # weights large enough for the layers to matter
        r.hid_bias.data = torch.from_numpy((0.3 * g.standard_normal(r.hid_bias.numel())).astype(F32))
    net.layers[0].init_from_data(X)
    layers = [(r.W.data.numpy(), r.vis_bias.data.numpy(), r.hid_bias.data.numpy()) for r in net.layers]
    return net, X, net.layers[0].logvar.data.numpy(), layers


# ---- 1. the twin against enumeration ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(6, 5, 4), (6, 5, 4, 3)], ids=["6-5-4", "6-5-4-3"])
def test_the_exact_bound_is_below_the_exact_log_density_on_every_row(sizes):
    z, layers, v = Cs.truth_stack(sizes)
    lp, lb = GB.exact_log_p(z, layers, v), GB.exact_bound(z, layers, v)
    print("log p - bound:", (lp - lb).round(3))
    assert lp.shape == lb.shape == (8,) and np.isfinite(lp).all() and (lb <= lp).all() and (lp - lb > 0.1).all()


def test_the_enumerated_density_integrates_to_what_the_gaussian_rbm_alone_gives_for_two_layers():
    """Two layers tie the top RBM to nothing below: with W_2 = 0 the marginal p(h_1) is a product of sigmoid(b_2) and the density is a
    mixture the Gaussian twin's enumeration can state too: log sum_h prod_j sigmoid(b_2,j)^h_j ... N(v; b_1 + h W_1^T)."""
    z, layers, v = Cs.truth_stack()
    (W1, b1, c1), (W2, b2, c2) = layers
    flat = [(W1, b1, c1), (np.zeros_like(W2), b2, c2)]
    hs = A._states(5)
    lp_h = hs @ b2.astype(F64) - A.softplus(b2.astype(F64)).sum()
    m = hs @ W1.astype(F64).T + b1.astype(F64)
    d = v.astype(F64)[:, None, :] - m[None, :, :]
    ln = -(d * d * np.exp(-z.astype(F64)) / 2 + z.astype(F64) / 2).sum(2) - 3 * np.log(2 * np.pi)
    assert np.allclose(GB.exact_log_p(z, flat, v), A._lse(ln + lp_h[None, :], 1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("mode", Cs.MODES)
@pytest.mark.parametrize("sizes", [(6, 5, 4), (6, 5, 4, 3)], ids=["6-5-4", "6-5-4-3"])
def test_twin_estimates_are_within_three_standard_errors_of_the_enumeration(sizes, mode):
    d, se, exact, est = Cs.truth_statistic(mode, Cs.TRUTH_SEED, sizes)
    print(f"{sizes} {mode}: sum(estimate - exact) {d:+.4f} = {d / se:+.2f} se (se {se:.4f}); per row {(est - exact).round(3)}")
    assert 0 < se < 0.5
    assert abs(d) <= 3 * se


# ---- 2. the closed form -------------------------------------------------------------------------------------------------------------
def test_without_bottom_weights_the_entropy_value_is_the_closed_form():
    """W_1 = 0, L = 2: m = b_1 whatever h, so log N is the same for every sample, q(h_1) = sigmoid(c_1) whatever v, and the bound is
    log N(v; b_1, sigma^2) + H(q) + E_q[-F_top] - log Z_top."""
    z, layers, v = Cs.truth_stack()
    (W1, b1, c1), top = layers
    layers = [(np.zeros_like(W1), b1, c1), top]
    lz = A.exact_log_z(*top)
    c64 = c1.astype(F64)
    hs = A._states(5)
    q = np.exp(hs @ c64 - A.softplus(c64).sum())
    ent = (A.softplus(c64) - c64 * A.sigmoid(c64)).sum()
    want = GB.log_normal(v, np.broadcast_to(b1, v.shape), z) + ent + q @ A.neg_free_energy(*top, hs) - lz
    assert np.allclose(GB.exact_bound(z, layers, v), want, rtol=0, atol=1e-12)
    S = 16
    acc, h, margin, e, ln = GB.gauss_bound_step(*layers[0], z, np.repeat(v, S, axis=0), "entropy", PhiloxStream(2))
    ln, e = ln.reshape(8, S), e.reshape(8, S)
    assert (ln == ln[:, :1]).all() and (e == e[0, 0]).all() and h.min() == 0 and h.max() == 1
    assert np.allclose(ln[:, 0], GB.log_normal(v, np.broadcast_to(b1, v.shape), z), rtol=0, atol=1e-12) and abs(e[0, 0] - ent) <= 1e-12
    # the mean over samples of the twin's values: only the top term varies, and its expectation is the closed form's
    w, _, _, _ = GB.gauss_dbn_values(z, layers, v, 4096, "entropy", PhiloxStream(2), lz)
    se = w.std(1, ddof=1) / 64.0
    assert (np.abs(w.mean(1) - want) <= 4 * se).all()


# ---- 3. a stack of one ----------------------------------------------------------------------------------------------------------------
def test_a_stack_of_one_is_gaussian_log_likelihood_bit_for_bit_and_draws_nothing(double):
    c = Cs.case("tiny")
    r = _grbm(c["W"], c["b"], c["c"], c["z"])
    v = torch.from_numpy(c["v"])
    E.manual_seed(3)
    for mode in Cs.MODES:
        w = LK.gaussian_dbn_sample_values(r, v, 12.5, mode=mode)
        assert w.dtype == torch.float64 and tuple(w.shape) == (c["M"], 1)
        assert torch.equal(w[:, 0], LK.gaussian_log_likelihood(r, v, 12.5))
    assert torch.equal(LK.gaussian_dbn_lower_bound(r, v, 12.5, n_samples=3), LK.gaussian_log_likelihood(r, v, 12.5))
    assert E.get_rng().offset == 0 and not [x for x in double.calls if x[0] in ("gauss_bound_step", "bound_step")]
    want = -G.free_energy(double._gstate(r, r.logvar.data), c["v"]).astype(F64) - 12.5
    assert np.array_equal(w[:, 0].numpy(), want)


# ---- 4. host logic through the double -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", Cs.MODES)
@pytest.mark.parametrize("sizes", [(12, 7, 5), (12, 7, 5, 4)], ids=["12-7-5", "12-7-5-4"])
def test_call_order_rows_and_values_of_a_stack(double, sizes, mode):
    net, X, z, layers = _net(sizes)
    S, L = 3, len(sizes) - 1
    E.manual_seed(21)
    w = LK.gaussian_dbn_sample_values(net, X[:5], 1.25, n_samples=S, mode=mode, seed=4)
    assert E.get_rng().offset == 0 and E.get_rng().seed == 21              # seed=int: a private source
    calls = [x for x in double.calls if x[0] in ("gauss_bound_step", "bound_step", "free_energy")]
    assert calls == [("gauss_bound_step", (5 * S, 12), mode)] + [("bound_step", (5 * S, sizes[l]), mode) for l in range(1, L - 1)] + \
        [("free_energy", (5 * S, sizes[L - 1]))]
    assert w.dtype == torch.float64 and tuple(w.shape) == (5, S)
    want, _, _, _ = GB.gauss_dbn_values(z, layers, X[:5].numpy(), S, mode, PhiloxStream(4), 1.25, dt=F32)
    assert np.allclose(w.numpy(), want, rtol=1e-6, atol=1e-5)
    # the rows of a sample are the S consecutive engine rows: row 1 alone, under a source that starts at its first engine row
    one, _, _, _ = GB.gauss_dbn_values(z, layers, X[1:2].numpy(), S, mode, PhiloxStream(4, 0, S), 1.25, dt=F32)
    assert np.allclose(w.numpy()[1], one[0], rtol=1e-6, atol=1e-5)
    # seed=None: the ambient source, one draw per directed layer
    LK.gaussian_dbn_sample_values(net, X[:5], 1.25, n_samples=S, mode=mode)
    assert E.get_rng().offset == L - 1
    # the thin method and the two reductions
    lb = net.gaussian_log_likelihood_bound(X[:5], 1.25, n_samples=S, seed=4)
    assert torch.equal(lb, LK.gaussian_dbn_lower_bound(net, X[:5], 1.25, n_samples=S, seed=4))
    assert torch.equal(lb, LK.gaussian_dbn_sample_values(net, X[:5], 1.25, S, "entropy", 4).mean(1))
    li = net.gaussian_log_likelihood_bound(X[:5], 1.25, n_samples=S, importance=True, seed=4)
    wq = LK.gaussian_dbn_sample_values(net, X[:5], 1.25, S, "logq", 4).numpy()
    assert np.allclose(li.numpy(), [A.logmeanexp(r) for r in wq], rtol=1e-12)


class _Run:
    def __init__(self): self.logged = []
    def log(self, d): self.logged.append(dict(d))


def test_evaluate_over_a_ragged_loader_makes_one_estimate_and_one_host_copy(double, monkeypatch):
    net, X, z, layers = _net((12, 7, 5))
    loader = [X[:6], X[6:12], X[12:15]]                                          # 6 + 6 + 3 rows
    n_est = []
    real_est = LK.estimate_log_partition
    monkeypatch.setattr(LK, "estimate_log_partition", lambda *a, **k: (n_est.append(a[0]), real_est(*a, **k))[1])
    E.manual_seed(5)
    res = LK.evaluate_gaussian_dbn_bound(net, loader=loader, n_samples=4, n_chains=8, n_betas=5, seed=3)
    assert n_est == [net.layers[-1]] and E.get_rng().offset == 0                 # one estimate, of the top RBM; a private source
    est = real_est(net.layers[-1], n_chains=8, n_betas=5, seed=3)
    assert set(res) == {"mean_bound", "sum_bound", "n", "log_z_top", "se", "ess", "n_samples"}
    assert res["n"] == 15 and res["n_samples"] == 4 and res["log_z_top"] == est["log_z"] and res["se"] == est["se"] and res["ess"] == est["ess"]
    # the batches share ONE private source: batch k starts where batch k - 1 stopped
    ps, tot = PhiloxStream(3), 0.0
    for xb in loader:
        w, _, _, _ = GB.gauss_dbn_values(z, layers, xb.numpy(), 4, "entropy", ps, est["log_z"], dt=F32)
        tot += w.mean(1).sum()
    assert res["sum_bound"] == pytest.approx(tot, rel=1e-6) and res["mean_bound"] == pytest.approx(tot / 15, rel=1e-6)
    # a given log Z: no estimate, se and ess None; max_batches; importance; the model's own loader and run
    copies = []
    real = torch.Tensor.cpu

    def counted(self, *a, **k):                                                  # (the double reads its fp32 inputs with .cpu() too)
        if self.dtype == torch.float64:
            copies.append(tuple(self.shape))
        return real(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", counted)
    res = LK.evaluate_gaussian_dbn_bound(net, loader=loader, log_z_top=2.5, n_samples=2, max_batches=2)
    assert [s for s in copies if s == (1,)] == [(1,)] and len(n_est) == 1
    assert res["n"] == 12 and res["se"] is None and res["ess"] is None and res["log_z_top"] == 2.5
    net.wandb_run = _Run()
    res = LK.evaluate_gaussian_dbn_bound(net, log_z_top=2.5, n_samples=2, importance=True, seed=1)
    assert res["n"] == 16
    assert net.wandb_run.logged == [{"ll/gdbn_mean_bound": res["mean_bound"], "ll/gdbn_log_z_top": 2.5, "ll/gdbn_n_samples": 2}]
    net.val_loader = None
    assert LK.evaluate_gaussian_dbn_bound(net, log_z_top=2.5) is None


def test_evaluate_on_a_stack_of_one_estimates_the_gaussian_log_partition(double):
    c = Cs.case("tiny")
    r = _grbm(c["W"], c["b"], c["c"], c["z"])
    X = torch.from_numpy(c["v"])
    res = LK.evaluate_gaussian_dbn_bound(r, loader=[X[:3], X[3:]], n_chains=8, n_betas=5, seed=2)
    assert [x for x in double.calls if x[0] == "gauss_ais"] == [("gauss_ais", 8, 5, False)]
    est = LK.estimate_gaussian_log_partition(r, n_chains=8, n_betas=5, seed=2)
    assert res["n"] == 5 and res["log_z_top"] == est["log_z"]
    assert res["mean_bound"] == pytest.approx(float(LK.gaussian_log_likelihood(r, X, est["log_z"]).mean()), rel=1e-12)


def test_the_new_functions_refuse_a_bernoulli_stack_and_the_generic_ones_a_gaussian_one(double):
    from imdbn.models import RBM, grbm, iDBN
    net, X, z, layers = _net((12, 7, 5))
    plain = iDBN.__new__(iDBN)
    plain.layers = [RBM(12, 7, 0.1, 0.0, 0.5).to("cpu"), RBM(7, 5, 0.1, 0.0, 0.5).to("cpu")]
    plain.val_loader, plain.wandb_run = [X], None
    for model in (plain, plain.layers[0]):
        for call in (lambda: LK.gaussian_dbn_sample_values(model, X, 0.0), lambda: LK.gaussian_dbn_lower_bound(model, X, 0.0),
                     lambda: LK.gaussian_dbn_log_likelihood_is(model, X, 0.0), lambda: LK.evaluate_gaussian_dbn_bound(model, loader=[X], log_z_top=0.0)):
            with pytest.raises(ValueError, match="GaussianRBM"):
                call()
    with pytest.raises(ValueError, match="GaussianRBM"):
        plain.gaussian_log_likelihood_bound(X, 0.0)
    for call in (lambda: LK.dbn_sample_values(net, X, 0.0), lambda: LK.dbn_lower_bound(net, X, 0.0), lambda: LK.dbn_log_likelihood_is(net, X, 0.0),
                 lambda: LK.evaluate_dbn_bound(net, loader=[X], log_z_top=0.0), lambda: LK.dbn_lower_bound(net.layers[0], X, 0.0)):
        with pytest.raises(ValueError, match="Gaussian"):
            call()
    with pytest.raises(ValueError, match="log_likelihood_bound"):
        net.log_likelihood_bound(X, 0.0)
    assert len(grbm.REFUSED) == 13
    # an untied model has no Gaussian form (untie itself refuses such a stack: the attribute is put there by hand)
    net.gen_layers = []
    with pytest.raises(NotImplementedError):
        LK.gaussian_dbn_sample_values(net, X, 0.0)
    del net.gen_layers
    for bad in (dict(mode="mean"), dict(n_samples=0)):
        with pytest.raises(ValueError):
            LK.gaussian_dbn_sample_values(net, X, 0.0, **bad)
    assert not [x for x in double.calls if x[0] in ("gauss_bound_step", "bound_step")]
    assert {"gaussian_dbn_sample_values", "gaussian_dbn_lower_bound", "gaussian_dbn_log_likelihood_is", "evaluate_gaussian_dbn_bound"} <= set(LK.__all__)


# ---- 5. the draw schedule and the parity seeds ------------------------------------------------------------------------------------------
def test_the_schedule_is_what_the_twin_draws():
    c = Cs.case("tiny")
    for mode in Cs.MODES:
        ps = PhiloxStream(5)
        GB.gauss_bound_step(c["W"], c["b"], c["c"], c["z"], c["v"], mode, ps)
        assert [(k, shape[1]) for k, shape in ps.log] == R.sched_bound(c["H"]) == [("u", c["H"])] and ps.offset == 1
        assert ps.log[0][1][0] == c["M"]


def test_every_parity_seed_is_clear_of_a_tie_and_the_restatement_draws_the_same_h():
    for c, kind in Cs.all_runs():
        a, b = Cs.twin_run(c, kind), Cs.twin_run(c, kind, dt=F32)
        assert a["margin"] >= Cs.MARGIN and np.array_equal(a["h"], b["h"]), (c["name"], c["mode"], kind, a["margin"])
        assert 0 < a["h"].mean() < 1
    e = Cs.fp32_error()
    print("fp32 restatement vs float64 twin:", e)
    assert 0 < e < 1e-5


# ---- 6. ABI -------------------------------------------------------------------------------------------------------------------------------
def test_export_is_declared_bound_and_present():
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    assert re.search(r"\bint\s+imdbn_rbm_gauss_bound_step\s*\(", src) and "#define IMDBN_ABI_VERSION 4" in src
    res, args = native.SIGNATURES["imdbn_rbm_gauss_bound_step"]
    assert len(args) == 13
    from imdbn.engine.hip_engine import HipEngine
    import inspect
    assert list(inspect.signature(HipEngine.gauss_bound_step).parameters) == ["self", "rbm", "logvar", "v", "rng", "acc", "mode"]
    assert hasattr(native.lib(), "imdbn_rbm_gauss_bound_step")
