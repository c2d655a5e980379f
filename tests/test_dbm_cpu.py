"""CPU-only: the float64 reference of the DBM arithmetic (tests/dbm_oracle.py) against exact enumeration, and the host logic of
imdbn.models.dbm / HipEngine.dbm_* through the engine double (tests/dbm_engine_double.py).  No claim about the kernel is made here
-- that is tested on the GPU in test_dbm_gpu.py."""
import numpy as np
import pytest
import torch

import dbm_cases as Ck
import dbm_oracle as Dt
import oracle.rbm_oracle as O
from dbm_engine_double import DbmOracleEngine
from imdbn import engine as E
from imdbn.engine import rng as R

F32, F64 = np.float32, np.float64
PARAMS = {"LEARNING_RATE": 0.1, "WEIGHT_PENALTY": 0.0, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.9, "LEARNING_RATE_DYNAMIC": False, "CD": 1}


def _data(n0, B, seed):
    return (np.random.default_rng(seed).random((B, n0)) < 0.4).astype(F64)


# ---- 1. the variational bound -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", Ck.SMALL_SEEDS)
@pytest.mark.parametrize("sizes,scale", Ck.SMALL)
def test_the_bound_rises_under_gauss_seidel_sweeps_and_stays_under_log_p(sizes, scale, seed):
    Ws, bs = Ck.model(sizes, scale, seed)
    v = _data(sizes[0], 6, 50 + seed)
    lz = Dt.log_z(Ws, bs)
    lp = Dt.log_p(Ws, bs, v, lz)
    trace = []
    _, res = Dt.infer(Ws, bs, v, 300, 0.0, F64, trace=trace)
    bound = np.array([Dt.variational_bound(Ws, bs, v, mu, lz) for mu in trace])
    print(f"{sizes} scale {scale} seed {seed}: log Z {lz:.6f}, bound {bound[0].mean():.4f} -> {bound[-1].mean():.4f}, log p {lp.mean():.4f}, res {res.max():.3g}")
    assert (np.diff(bound, axis=0) >= -1e-12).all()
    assert (bound <= lp[None, :] + 1e-12).all()
    assert res.max() < 1e-10


def test_log_p_sums_to_one():
    Ws, bs = Ck.model((6, 5, 4, 3), 0.8, 4)
    allv = Dt._bits(6)
    assert abs(np.exp(Dt.log_p(Ws, bs, allv)).sum() - 1.0) < 1e-12


# ---- 2. the sampler ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,scale", Ck.SMALL)
def test_block_gibbs_leaves_the_exact_marginals_stationary(sizes, scale):
    Ws, bs = Ck.model(sizes, scale, 0)
    M, burn = 4000, 300
    src = Ck.Tape(77)
    start = [(src.g.random((M, n)) < 0.5).astype(F64) for n in sizes]
    s = Dt.gibbs(Ws, bs, start, burn, src, F64)
    want = Dt.marginals(Ws, bs)
    worst = 0.0
    for l, (got, p) in enumerate(zip(s, want)):
        se = np.sqrt(p * (1 - p) / M)
        worst = max(worst, float((np.abs(got.mean(0) - p) / se).max()))
    print(f"{sizes} scale {scale}: largest |marginal error| {worst:.2f} standard errors over {sum(sizes)} units")
    assert worst <= 5.0


# ---- the twin against the reference (what the GPU bounds are built from) ---------------------------------------------------------------
def test_the_fp32_twin_follows_the_reference_within_the_derived_bound():
    k = Ck.stack_case((67, 64, 33, 5), 5)
    mu, res, dmu, rb = Dt.infer_bounded(k["Ws"], k["bs"], k["data"], 3, 0.5)
    tmu, tres = Dt.infer(k["Ws"], k["bs"], k["data"], 3, 0.5, F32)
    assert all(t.dtype == F32 and (np.abs(t - m) <= d).all() for t, m, d in zip(tmu, mu, dmu))
    assert (np.abs(tres - res) <= rb).all() and max(d.max() for d in dmu) < 1e-4


# ---- 6 / 8 (CPU side): no comparison of the GPU tests is a near tie ----------------------------------------------------------------
@pytest.mark.parametrize("case", Ck.LAYER_CASES, ids=str)
def test_no_uniform_of_a_layer_case_lies_within_the_bound_of_its_probability(case):
    k = Ck.layer_case(*case, binary=True, seed=Ck.SAMPLE_SEEDS[case])
    p = Dt.sigmoid(Dt.pre(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"], F64))
    b = Dt.pre_bound(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"]) / 4 + Dt.EPS_P
    assert (np.abs(p - k["u"].astype(F64)) > b).all()


@pytest.mark.parametrize("sizes,B", Ck.STACKS, ids=str)
def test_no_uniform_of_a_stack_case_lies_within_the_bound_of_its_probability(sizes, B):
    k = Ck.stack_case(sizes, B)
    for clamp in (None, k["data"]):
        margins = []
        Dt.gibbs(k["Ws"], k["bs"], k["particles"], Ck.GIBBS_SWEEPS, Ck.Tape(Ck.GIBBS_SEEDS[(sizes, B)]), F64, clamp_bottom=clamp, margins=margins)
        assert min(margins) > 0.0
    # two consecutive steps as the GPU test runs them, in float64.  The device's parameters after the first step are the reference's
    # only up to the twin's distance (about 1e-6 relative), which moves a probability by that much: STEP_MARGIN of room is asked for
    sts = Dt.states_as(_states(k), F64)
    parts = k["particles"]
    for step_seed in Ck.STEP_SEEDS[(sizes, B)]:
        margins = []
        parts = Dt.step(sts, k["data"], parts, Ck.STEP_SCALARS[:len(sts)], Ck.STEP_N_MF, Ck.STEP_DAMP, Ck.STEP_GIBBS_K, Ck.Tape(step_seed),
                        margins=margins)["particles"]
        assert min(margins) > Ck.STEP_MARGIN


def _states(k):
    sts = []
    for l, W in enumerate(k["Ws"]):
        sts.append(O.RBMState.create(W, Ck.LR, Ck.WEIGHT_DECAY, Ck.MOM, hid_bias=k["bs"][l + 1],
                                     vis_bias=k["bs"][l] if l == 0 else np.zeros_like(k["bs"][l])))
    return sts


# ---- host logic through the double -------------------------------------------------------------------------------------------------
@pytest.fixture
def double():
    eng = DbmOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)
    E.set_rng(None)


def _on_cpu(r):
    r.to("cpu")
    r.W.data = r.W.data.contiguous()
    r.W_m, r.hb_m, r.vb_m = torch.zeros_like(r.W.data), torch.zeros_like(r.hid_bias.data), torch.zeros_like(r.vis_bias.data)
    return r


def _dbm(sizes, Ws=None, bs=None, params=PARAMS, dataloader=None):
    from imdbn.models import DBM
    torch.manual_seed(0)
    net = DBM(list(sizes), dict(params), dataloader=dataloader, device="cpu")
    for l, r in enumerate(net.layers):
        _on_cpu(r)
        if Ws is not None:
            r.W.data = torch.from_numpy(Ws[l].copy())
            r.hid_bias.data = torch.from_numpy(bs[l + 1].copy())
    if bs is not None:
        net.layers[0].vis_bias.data = torch.from_numpy(bs[0].copy())
    return net


def _idbn(sizes=(12, 7, 5), groups=None, gaussian=False):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import iDBN
    torch.manual_seed(0)
    g = np.random.Generator(np.random.PCG64(3))
    X = torch.from_numpy((g.random((20, sizes[0])) > 0.5).astype(F32))
    dl = DataLoader(TensorDataset(X, torch.zeros(20)), batch_size=8)
    p = dict(PARAMS, WEIGHT_PENALTY=1e-4)
    if gaussian:
        p["GAUSSIAN_VISIBLE"] = True
    net = iDBN(list(sizes), p, dl, dl, torch.device("cpu"))
    for r in net.layers:
        _on_cpu(r)
        r.hid_bias.data.normal_(0, 0.3); r.vis_bias.data.normal_(0, 0.3)
    if groups:
        net.layers[-1].softmax_groups = groups
    return net, X


# ---- 3. learning ---------------------------------------------------------------------------------------------------------------------
def _toy(seed=5, n=32):
    g = np.random.default_rng(seed)
    protos = np.array([[1, 1, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 1, 1, 1, 1], [1, 1, 0, 0, 1, 1, 0, 0], [0, 0, 1, 1, 0, 0, 1, 1]], F32)
    x = protos[g.integers(0, 4, n)]
    flip = g.random(x.shape) < 0.05
    return np.where(flip, 1 - x, x).astype(F32)


def test_training_on_the_double_raises_the_exact_log_likelihood(double):
    Ws, bs = Ck.model((8, 6, 4), 0.1, 11)
    # persistent chains follow the model only while it moves slowly: lr 0.05 with momentum 0.5 throughout (an effective 0.1)
    net = _dbm((8, 6, 4), Ws, bs, params=dict(PARAMS, LEARNING_RATE=0.05, FINAL_MOMENTUM=0.5))
    X = _toy()
    model = lambda: ([r.W.data.numpy().astype(F64) for r in net.layers], [b.numpy().astype(F64) for b in net.biases()])
    before = Dt.log_p(*model(), X).mean()
    E.set_rng(R.ReplayRng(Ck.Tape(123)))
    x = torch.from_numpy(X)
    for epoch in range(300):
        net.train_step(x, epoch, 300, n_mf=10, damp=0.0, gibbs_k=5, monitor=False)
    after = Dt.log_p(*model(), X).mean()
    print(f"mean exact log-likelihood of the toy set: {before:.4f} -> {after:.4f}")
    assert after > before


def test_the_double_is_the_twin_and_the_step_applies_pos_minus_neg_over_B(double):
    k = Ck.stack_case((8, 6, 4), 7, seed=31)
    net = _dbm((8, 6, 4), k["Ws"], k["bs"], params=dict(PARAMS, INIT_MOMENTUM=0.0))
    sts = _states(k)
    for s in sts:
        s.weight_decay, s.momentum = 0.0, 0.0
    W0 = [s.W.copy() for s in sts]
    b0 = [b.copy() for b in Dt.model_of(sts)[1]]
    parts = [torch.from_numpy(p.copy()) for p in k["particles"]]
    scalars = [(0.1, 0.0), (0.05, 0.0)]
    out = double.dbm_step(net.layers, torch.from_numpy(k["data"]), parts, scalars, 4, 0.25, 3, R.ReplayRng(Ck.Tape(9)))
    ref = Dt.step(sts, k["data"], k["particles"], scalars, 4, 0.25, 3, Ck.Tape(9))
    # bit for bit the twin: parameters, momenta, magnetisations, particles
    for r, s in zip(net.layers, sts):
        assert np.array_equal(r.W.data.numpy(), s.W) and np.array_equal(r.hid_bias.data.numpy(), s.hid_bias) and np.array_equal(r.W_m.numpy(), s.W_m)
    assert np.array_equal(net.layers[0].vis_bias.data.numpy(), sts[0].vis_bias)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(out["mu"], ref["mu"]))
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(parts, ref["particles"])) and out["particles"] is parts
    assert np.array_equal(out["res"].numpy(), ref["res"]) and abs(float(out["recon_loss"]) - float(ref["recon_loss"])) < 1e-6
    # the gradient is (pos - neg) / B of the oracle's phase tensors, for every RBM and every model bias
    pos = [k["data"]] + ref["mu"]
    neg = ref["particles"]
    B = k["data"].shape[0]
    _, b1 = Dt.model_of(sts)
    for l, (lr, _) in enumerate(scalars):
        gW = (pos[l].astype(F64).T @ pos[l + 1] - neg[l].astype(F64).T @ neg[l + 1]) / B
        assert np.abs((sts[l].W.astype(F64) - W0[l]) - lr * gW).max() < 1e-6
    lrs = [scalars[0][0]] + [lr for lr, _ in scalars]
    for l in range(3):
        gb = (pos[l].astype(F64).sum(0) - neg[l].astype(F64).sum(0)) / B
        assert np.abs((b1[l].astype(F64) - b0[l]) - lrs[l] * gb).max() < 1e-6


# ---- 4. host logic ---------------------------------------------------------------------------------------------------------------------
def test_from_idbn_copies_scales_and_keeps_the_bias_convention(double):
    net, _ = _idbn()
    before = [{n: getattr(r, n).data.clone() if n in ("W", "hid_bias", "vis_bias") else getattr(r, n).clone()
               for n in ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")} for r in net.layers]
    dbm = net.to_dbm(weight_scale=[1.0, 0.5])
    for r, b in zip(net.layers, before):                    # the iDBN is bit-identical, and shares no storage
        for n, t in b.items():
            cur = getattr(r, n)
            assert torch.equal(cur.data if isinstance(cur, torch.nn.Parameter) else cur, t)
    assert dbm.layers[0].W.data_ptr() != net.layers[0].W.data_ptr()
    assert torch.equal(dbm.layers[0].W.data, net.layers[0].W.data) and torch.equal(dbm.layers[1].W.data, net.layers[1].W.data * 0.5)
    bs = dbm.biases()
    assert len(bs) == 3 and torch.equal(bs[0], net.layers[0].vis_bias.data) and torch.equal(bs[1], net.layers[0].hid_bias.data)
    assert torch.equal(bs[2], net.layers[1].hid_bias.data) and bs[1].data_ptr() == dbm.layers[0].hid_bias.data_ptr()
    assert float(dbm.layers[1].vis_bias.data.abs().max()) == 0.0 and float(net.layers[1].vis_bias.data.abs().max()) > 0.0
    assert dbm.sizes == [12, 7, 5] and all(not r.sparsity for r in dbm.layers)
    with pytest.raises(ValueError):
        net.to_dbm(weight_scale=[1.0])


def test_softmax_groups_and_gaussian_layers_are_refused(double):
    from imdbn.models import DBM
    with pytest.raises(ValueError, match="softmax"):
        _idbn(groups=[(5, 7)])[0].to_dbm()
    with pytest.raises(ValueError, match="Gaussian"):
        DBM.from_idbn(_idbn(gaussian=True)[0])


def test_save_and_load_reproduce_infer_and_resume_the_particles(double, tmp_path):
    net, X = _idbn()
    dbm = net.to_dbm()
    E.set_rng(R.ReplayRng(Ck.Tape(5)))
    dbm.train_step(X[:8], 0, 1, n_mf=3, gibbs_k=2)
    path = str(tmp_path / "dbm.pkl")
    dbm.save_model(path)
    other = _idbn()[0].to_dbm()
    other.layers[1].vis_bias.data.fill_(3.0)
    other.load_model(path)
    a, b = dbm.infer(X, 5, 0.25), other.infer(X, 5, 0.25)
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) and x.data_ptr() != y.data_ptr() for x, y in zip(dbm.particles, other.particles))
    assert all(torch.equal(x, y) for x, y in zip(dbm.bias_momenta(), other.bias_momenta()))
    assert all(torch.equal(r.W_m, s.W_m) for r, s in zip(dbm.layers, other.layers)) and float(other.layers[1].vis_bias.data.abs().max()) == 0.0
    import pickle
    state = pickle.load(open(path, "rb"))
    assert sorted(state) == ["W", "W_m", "bias_momenta", "biases", "particles", "sizes"] and len(state["biases"]) == 3
    # resumed: the same draws advance both sets of particles alike
    E.set_rng(R.ReplayRng(Ck.Tape(6))); dbm.gibbs(2)
    E.set_rng(R.ReplayRng(Ck.Tape(6))); other.gibbs(2)
    assert all(torch.equal(x, y) for x, y in zip(dbm.particles, other.particles))


@pytest.mark.parametrize("sizes", [(9, 6), (12, 7, 5), (10, 8, 6, 4), (7, 6, 5, 4, 3)])
@pytest.mark.parametrize("clamp", [False, True])
def test_the_schedule_is_what_the_double_draws(double, sizes, clamp):
    Ws, bs = Ck.model(sizes, 0.3, 1)
    net = _dbm(sizes, Ws, bs)
    tape = Ck.Tape(2)
    M = 3
    parts = [torch.from_numpy((tape.g.random((M, n)) < 0.5).astype(F32)) for n in sizes]
    bottom = parts[0].clone()
    double.dbm_gibbs(net.layers, net.biases(), parts, 2, R.ReplayRng(tape), clamp_bottom=bottom if clamp else None)
    assert tape.shapes == [(M, n) for _, n in R.sched_dbm_gibbs(sizes, 2, clamp_bottom=clamp)]
    assert len(tape.shapes) == 2 * (len(sizes) - (1 if clamp else 0))
    if clamp:
        assert torch.equal(parts[0], bottom)
    # ... and the states are the oracle's
    tape2 = Ck.Tape(2)
    start = [(tape2.g.random((M, n)) < 0.5).astype(F32) for n in sizes]
    want = Dt.gibbs(Ws, bs, start, 2, tape2, F32, clamp_bottom=start[0] if clamp else None)
    assert all(np.array_equal(p.numpy(), w) for p, w in zip(parts, want))


def test_infer_through_the_double_is_the_oracle(double):
    k = Ck.stack_case((12, 7, 5), 4)
    net = _dbm((12, 7, 5), k["Ws"], k["bs"])
    mu, res = net.infer(torch.from_numpy(k["data"]), 3, 0.5)
    want, wres = Dt.infer(k["Ws"], k["bs"], k["data"], 3, 0.5, F32)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(mu, want)) and np.array_equal(res.numpy(), wres)
    assert torch.equal(net.represent(torch.from_numpy(k["data"]), n_mf=3, damp=0.5), mu[-1])
    assert torch.equal(net.represent(torch.from_numpy(k["data"]), upto_layer=1, n_mf=3, damp=0.5), mu[0])
    mu0, res0 = double.dbm_infer(net.layers, net.biases(), torch.from_numpy(k["data"]), 0)
    assert float(res0.abs().max()) == 0.0 and np.array_equal(mu0[0].numpy(), Dt.infer(k["Ws"], k["bs"], k["data"], 0, 0.0, F32)[0][0])


def test_without_monitor_no_reconstruction_is_launched(double):
    net, X = _idbn()
    dbm = net.to_dbm()
    E.set_rng(R.ReplayRng(Ck.Tape(5)))
    dbm.init_particles(X[:8])
    downs = lambda: sum(1 for c in double.calls if c[0] == "prop_down")
    double.calls.clear()
    assert dbm.train_step(X[:8], 0, 1, n_mf=2, gibbs_k=3, monitor=False) is None
    quiet = downs()
    assert double.calls[0] == ("dbm_step", (8, 12), 2, 0.0, 3, False) and sum(1 for c in double.calls if c[0] == "assoc_update") == 2
    double.calls.clear()
    out = dbm.train_step(X[:8], 0, 1, n_mf=2, gibbs_k=3, monitor=True)
    assert downs() == quiet + 1 and out["recon_loss"].dim() == 0 and out["res"].shape == (8,)
    # a shorter batch advances the first rows of the same particles
    p0 = dbm.particles[0]
    dbm.train_step(X[:5], 0, 1, n_mf=1, gibbs_k=1, monitor=False)
    assert dbm.particles[0] is p0 and p0.shape == (8, 12)


def test_finetune_runs_over_the_loader_and_logs(double):
    net, X = _idbn()
    dbm = net.to_dbm()
    E.set_rng(R.ReplayRng(Ck.Tape(8)))
    dbm.finetune(2, n_mf=2, gibbs_k=1, lr_scale=0.5, log_every=1)
    assert [h[0] for h in dbm.history] == [0, 1] and all(np.isfinite(h[1]) and h[2] >= 0 for h in dbm.history)
    assert sum(1 for c in double.calls if c[0] == "dbm_step") == 6


def test_data_parallel_runs_are_refused(double, monkeypatch):
    net, X = _idbn()
    dbm = net.to_dbm()
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        dbm.train_step(X[:8], 0, 1)
    parts = [torch.zeros(8, n) for n in dbm.sizes]
    with pytest.raises(NotImplementedError):
        double.dbm_step(dbm.layers, X[:8], parts, [(0.1, 0.5)] * 2, 1, 0.0, 1, R.ReplayRng(Ck.Tape(1)))
