"""CPU-only: the float64 reference of the multimodal DBM arithmetic (tests/mdbm_oracle.py) against exact enumeration, and the host logic
of imdbn.models.mdbm / HipEngine.mdbm_* through the engine double (mdbm_oracle.MdbmOracleEngine).  No claim about the kernel is made
here -- that is tested on the GPU in test_mdbm_gpu.py."""
import pickle

import numpy as np
import pytest
import torch

import dbm_oracle as Dt
import mdbm_cases as Ck
import mdbm_oracle as Mt
import oracle.rbm_oracle as O
from imdbn import engine as E
from imdbn.engine import rng as R

F32, F64 = np.float32, np.float64
PARAMS = {"LEARNING_RATE": 0.1, "WEIGHT_PENALTY": 0.0, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.9, "LEARNING_RATE_DYNAMIC": False, "CD": 1,
          "JOINT_CD": 1}


def _data(n0, B, seed):
    return (np.random.default_rng(seed).random((B, n0)) < 0.4).astype(F64)


def _small(case, seed):
    sizes, K, J, scale = case
    return Mt.Model(*Ck.model(sizes, K, J, scale, seed))


# ---- 1. the variational bound -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("free", [False, True], ids=["clamped", "free"])
@pytest.mark.parametrize("seed", Ck.SMALL_SEEDS)
@pytest.mark.parametrize("case", Ck.SMALL, ids=str)
def test_the_bound_does_not_fall_under_undamped_sweeps_and_stays_under_the_exact_value(case, seed, free):
    M = _small(case, seed)
    g = np.random.default_rng(60 + seed)
    v = _data(case[0][0], 6, 50 + seed)
    labels = g.integers(0, M.K, 6)
    lz = Mt.log_z(M)
    if free:
        exact = np.array([Mt._lse(Mt.configs(M, v=row)[2]) - lz for row in v])           # log p(v)
    else:
        exact = Mt.log_p_joint(M, v, labels, lz)                                          # log p(v, y)
    trace = []
    Mt.infer(M, v, None if free else np.eye(M.K)[labels], 60, 0.0, F64, trace=trace)
    bound = np.array([Mt.variational_bound(M, v, mu, lz) for mu in trace])
    print(f"{case} seed {seed} {'free' if free else 'clamped'}: log Z {lz:.6f}, bound {bound[0].mean():.4f} -> {bound[-1].mean():.4f}, "
          f"exact {exact.mean():.4f}")
    assert (np.diff(bound, axis=0) >= -1e-12).all()
    assert (bound <= exact[None, :] + 1e-12).all()


def test_the_enumeration_sums_to_one():
    M = _small(((6, 5, 4), 4, 3, 0.8), 4)
    lz = Mt.log_z(M)
    allv = Dt._bits(6)
    total = sum(np.exp(Mt.log_p_joint(M, allv, np.full(len(allv), c), lz)).sum() for c in range(M.K))
    assert abs(total - 1.0) < 1e-12
    post = Mt.label_posterior(M, allv[:5])
    assert np.allclose(post.sum(1), 1.0, atol=1e-12)
    assert abs(sum(Mt.marginals(M)[-1]) - 1.0) < 1e-12


# ---- 2. the sampler ------------------------------------------------------------------------------------------------------------------
# Tape seed 77 was the first tried for both tests (1 seed tried each).
@pytest.mark.parametrize("case", Ck.SMALL, ids=str)
def test_block_gibbs_leaves_the_exact_marginals_stationary(case):
    M = _small(case, 0)
    n, burn = 4000, 300
    src = Ck.Tape(77)
    sizes = M.sizes
    start = [(src.g.random((n, k)) < 0.5).astype(F64) for k in sizes[:M.L]]
    start.append(np.concatenate([(src.g.random((n, M.Dz)) < 0.5).astype(F64), np.eye(M.K)[src.g.integers(0, M.K, n)]], 1))
    start.append((src.g.random((n, M.J)) < 0.5).astype(F64))

    class Exact(Ck.Tape):                         # the categorical of the model, by inverse CDF on this tape's uniforms
        def categorical(self, probs):
            u = self.g.random(probs.shape[0])
            return np.minimum((np.cumsum(probs, 1) <= u[:, None]).sum(1), probs.shape[1] - 1)
    ex = Exact(78)
    ex.g = src.g
    s = Mt.gibbs(M, start, burn, ex, F64)
    got = s[:M.L] + [s[M.L][:, :M.Dz], s[M.L + 1], s[M.L][:, M.Dz:]]
    want = Mt.marginals(M)
    worst = 0.0
    for g_, p in zip(got, want):
        se = np.sqrt(p * (1 - p) / n)
        worst = max(worst, float((np.abs(g_.mean(0) - p) / se).max()))
    print(f"{case}: largest |marginal error| {worst:.2f} standard errors over {sum(len(p) for p in want)} units and categories")
    assert worst <= 5.0


@pytest.mark.parametrize("case", Ck.SMALL, ids=str)
def test_gibbs_with_the_image_clamped_reproduces_the_label_posterior(case):
    M = _small(case, 1)
    n, burn = 4000, 200
    v = _data(case[0][0], 1, 9)
    src = Ck.Tape(77)

    class Exact(Ck.Tape):
        def categorical(self, probs):
            u = self.g.random(probs.shape[0])
            return np.minimum((np.cumsum(probs, 1) <= u[:, None]).sum(1), probs.shape[1] - 1)
    ex = Exact(77)
    start = [(ex.g.random((n, k)) < 0.5).astype(F64) for k in M.sizes[:M.L]]
    start.append(np.concatenate([(ex.g.random((n, M.Dz)) < 0.5).astype(F64), np.eye(M.K)[ex.g.integers(0, M.K, n)]], 1))
    start.append((ex.g.random((n, M.J)) < 0.5).astype(F64))
    s = Mt.gibbs(M, start, burn, ex, F64, clamp_bottom=np.tile(v, (n, 1)))
    p = Mt.label_posterior(M, v)[0]
    freq = s[M.L][:, M.Dz:].mean(0)
    worst = float((np.abs(freq - p) / np.sqrt(p * (1 - p) / n)).max())
    print(f"{case}: p(y | v) {np.round(p, 4)}, sampled {np.round(freq, 4)}: {worst:.2f} standard errors")
    assert np.array_equal(s[0], np.tile(v, (n, 1))) and worst <= 5.0


# ---- the twin against the reference (what the GPU bounds are built from) ---------------------------------------------------------------
@pytest.mark.parametrize("free", [False, True])
def test_the_fp32_twin_follows_the_reference_within_the_derived_bound(free):
    k = Ck.stack_case((67, 64, 33), 32, 5, 5)
    M = Mt.Model(k["Ws"], k["WJ"], k["bs"])
    y = None if free else k["y"]
    mu, res, dmu, rb = Mt.infer_bounded(M, k["data"], y, 3, 0.5)
    tmu, tres = Mt.infer(M, k["data"], y, 3, 0.5, F32)
    assert all(t.dtype == F32 and (np.abs(t - m) <= d).all() for t, m, d in zip(tmu, mu, dmu))
    assert (np.abs(tres - res) <= rb).all() and max(d.max() for d in dmu) < 1e-4


@pytest.mark.parametrize("case", Ck.GROUP_CASES, ids=str)
def test_the_softmax_twin_stays_inside_its_bound(case):
    k = Ck.group_case(*case)
    G = Mt.ends_to_groups(k["ends"])
    x = Dt.pre(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"], F64)
    p = Mt.softmax(x, G, F64)
    dp = Mt.softmax_bound(x, p, G, Dt.pre_bound(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"]))
    t = Mt.softmax(Dt.pre(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"], F32), G, F32)
    assert (np.abs(t - p) <= dp).all() and np.allclose(p.sum(1), len(G))


# ---- (CPU side of the GPU tests): no comparison of the GPU tests is a near tie ------------------------------------------------------
@pytest.mark.parametrize("case", Ck.GROUP_CASES, ids=str)
def test_no_pick_of_a_group_case_lies_within_the_bound_of_its_cumulative_sums(case):
    k = Ck.group_case(*case, binary=True)
    G = Mt.ends_to_groups(k["ends"])
    x = Dt.pre(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"], F64)
    p = Mt.softmax(x, G, F64)
    dp = Mt.softmax_bound(x, p, G, Dt.pre_bound(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"]))
    for g, (s, e) in enumerate(G):
        _, margin, tot = Mt.pick(p[:, s:e], Mt.philox_uniform(Ck.PICK_SEEDS[case], g, 0, k["B"]))
        assert (margin > Mt.pick_bound(dp[:, s:e], tot)).all()


def _states(k):
    sts = []
    for l, W in enumerate(k["Ws"]):
        sts.append(O.RBMState.create(W, Ck.LR, Ck.WEIGHT_DECAY, Ck.MOM, hid_bias=k["bs"][l + 1],
                                     vis_bias=k["bs"][l] if l == 0 else np.zeros_like(k["bs"][l])))
    L, Dz = len(k["Ws"]), k["sizes"][-1]
    sts.append(O.RBMState.create(k["WJ"], Ck.LR, Ck.WEIGHT_DECAY, Ck.MOM, hid_bias=k["bs"][L + 1],
                                 vis_bias=np.concatenate([np.zeros(Dz, F32), k["bs"][L + 2]]), softmax_groups=[(Dz, Dz + k["K"])]))
    return sts


@pytest.mark.parametrize("case", Ck.STACKS, ids=str)
def test_no_uniform_of_a_stack_case_lies_within_the_bound_of_its_probability(case):
    k = Ck.stack_case(*case)
    M = Mt.Model(k["Ws"], k["WJ"], k["bs"])
    for cb, cl in ((None, None), (k["data"], k["y"])):
        margins = []
        Mt.gibbs(M, k["particles"], Ck.GIBBS_SWEEPS, Ck.Tape(Ck.GIBBS_SEEDS[case]), F64, clamp_bottom=cb, clamp_labels=cl, margins=margins)
        assert min(margins) > 0.0
    # two consecutive steps as the GPU test runs them, in float64; STEP_MARGIN of room as in tests/test_dbm_cpu.py
    sts = Dt.states_as(_states(k), F64)
    parts = k["particles"]
    for step_seed in Ck.STEP_SEEDS[case]:
        margins = []
        parts = Mt.step(sts, k["data"], k["y"], parts, Ck.STEP_SCALARS[:len(sts)], Ck.STEP_N_MF, Ck.STEP_DAMP, Ck.STEP_GIBBS_K,
                        Ck.Tape(step_seed), margins=margins)["particles"]
        assert min(margins) > Ck.STEP_MARGIN


# ---- host logic through the double -------------------------------------------------------------------------------------------------
@pytest.fixture
def double():
    eng = Mt.MdbmOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)
    E.set_rng(None)


def _on_cpu(r):
    r.to("cpu")
    r.W.data = r.W.data.contiguous()
    r.W_m, r.hb_m, r.vb_m = torch.zeros_like(r.W.data), torch.zeros_like(r.hid_bias.data), torch.zeros_like(r.vis_bias.data)
    return r


def _imdbn(sizes=(12, 7), K=3, J=5, X=None, labels=None, params=PARAMS, batch=8, randomise=True):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import iMDBN
    torch.manual_seed(0)
    g = np.random.Generator(np.random.PCG64(3))
    if X is None:
        X = (g.random((20, sizes[0])) > 0.5).astype(F32)
        labels = np.arange(20) % K
    Xt, Yt = torch.from_numpy(X), torch.from_numpy(np.eye(K, dtype=F32)[labels])
    dl = DataLoader(TensorDataset(Xt, Yt), batch_size=batch)
    net = iMDBN(list(sizes), J, params=dict(params, WEIGHT_PENALTY=params["WEIGHT_PENALTY"]), dataloader=dl, val_loader=dl,
                device=torch.device("cpu"), num_labels=K)
    for r in net.image_idbn.layers + [net.joint_rbm]:
        _on_cpu(r)
        if randomise:
            r.hid_bias.data.normal_(0, 0.3); r.vis_bias.data.normal_(0, 0.3)
    return net, Xt, Yt


def _load(dbm, Ws, WJ, bs):
    """Put a model of mdbm_cases into a MultimodalDBM."""
    L = len(Ws)
    for l, r in enumerate(dbm.layers):
        r.W.data = torch.from_numpy(Ws[l].copy())
        r.hid_bias.data = torch.from_numpy(bs[l + 1].copy())
        r.vis_bias.data = torch.from_numpy(bs[0].copy() if l == 0 else np.zeros_like(bs[l]))
    dbm.joint.W.data = torch.from_numpy(WJ.copy())
    dbm.joint.hid_bias.data = torch.from_numpy(bs[L + 1].copy())
    dbm.joint.vis_bias.data = torch.from_numpy(np.concatenate([np.zeros(dbm.Dz, F32), bs[L + 2]]))
    for r in dbm.layers + [dbm.joint]:
        r.W_m, r.hb_m, r.vb_m = torch.zeros_like(r.W.data), torch.zeros_like(r.hid_bias.data), torch.zeros_like(r.vis_bias.data)
    return dbm


def _model_of(dbm):
    return Mt.Model([r.W.data.numpy().astype(F64) for r in dbm.layers], dbm.joint.W.data.numpy().astype(F64),
                    [b.numpy().astype(F64) for b in dbm.biases()])


# ---- 3. learning ---------------------------------------------------------------------------------------------------------------------
def _toy(seed=5, n=32):
    g = np.random.default_rng(seed)
    protos = np.array([[1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1], [1, 0, 1, 0, 1, 0]], F32)
    labels = g.integers(0, 3, n)
    x = protos[labels]
    return np.where(g.random(x.shape) < 0.05, 1 - x, x).astype(F32), labels


def test_training_on_the_double_raises_the_exact_joint_log_likelihood(double):
    X, labels = _toy()
    # lr 0.05 with momentum 0.5 throughout, as tests/test_dbm_cpu.py
    net, Xt, Yt = _imdbn((6, 4), 3, 4, X, labels, params=dict(PARAMS, LEARNING_RATE=0.05, FINAL_MOMENTUM=0.5), batch=32, randomise=False)
    dbm = _load(net.to_dbm(), *Ck.model((6, 4), 3, 4, 0.1, 11))
    before = Mt.log_p_joint(_model_of(dbm), X, labels).mean()
    E.set_rng(R.ReplayRng(_ExactTape(123)))
    dbm.finetune(300, n_mf=10, damp=0.0, gibbs_k=5)
    after = Mt.log_p_joint(_model_of(dbm), X, labels).mean()
    print(f"mean exact log p(v, y) of the toy set: {before:.4f} -> {after:.4f}")
    assert after > before and dbm.history == []
    mu_y, pred = dbm.predict_labels(Xt)
    print(f"free-label mean field names {float((pred.numpy() == labels).mean()):.2f} of the toy labels")
    assert mu_y.shape == (32, 3) and np.allclose(mu_y.sum(1).numpy(), 1.0, atol=1e-5)


class _ExactTape(Ck.Tape):
    """A replay provider for TRAINING on the double: the double hands ``categorical`` the model's probabilities, so the labels of the
    particles follow the model (``ReplayRng.build`` is never called on the double's path)."""

    def categorical(self, probs):
        u = self.g.random(probs.shape[0])
        c = np.cumsum(probs.astype(F64), 1)
        return np.minimum((c <= (u * c[:, -1])[:, None]).sum(1), probs.shape[1] - 1)


def test_the_double_is_the_twin_bit_for_bit(double):
    k = Ck.stack_case((8, 6, 4), 3, 5, 7, seed=31)
    net, _, _ = _imdbn((8, 6, 4), 3, 5)
    dbm = _load(net.to_dbm(), k["Ws"], k["WJ"], k["bs"])
    sts = _states(k)
    for s, r in zip(sts, dbm.layers + [dbm.joint]):
        s.weight_decay = r.weight_decay = 1e-4
    parts = [torch.from_numpy(p.copy()) for p in k["particles"]]
    scalars = [(0.1, 0.5), (0.05, 0.5), (0.02, 0.5)]
    for seed in (9, 10):
        out = double.mdbm_step(dbm.layers, dbm.joint, torch.from_numpy(k["data"]), torch.from_numpy(k["y"]), parts, scalars, 4, 0.25, 3,
                               R.ReplayRng(Ck.Tape(seed)))
        ref = Mt.step(sts, k["data"], k["y"], [p.numpy().copy() for p in parts] if seed == 10 else k["particles"], scalars, 4, 0.25, 3,
                      Ck.Tape(seed))
        for r, s in zip(dbm.layers + [dbm.joint], sts):
            assert np.array_equal(r.W.data.numpy(), s.W) and np.array_equal(r.hid_bias.data.numpy(), s.hid_bias)
            assert np.array_equal(r.W_m.numpy(), s.W_m) and np.array_equal(r.vis_bias.data.numpy(), s.vis_bias)
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(out["mu"], ref["mu"]))
        if seed == 9:
            assert all(np.array_equal(a.numpy(), b) for a, b in zip(parts, ref["particles"])) and out["particles"] is parts
        assert np.array_equal(out["res"].numpy(), ref["res"]) and abs(float(out["recon_loss"]) - float(ref["recon_loss"])) < 1e-6
    # the label stayed clamped in the positive phase and the particles' labels are one-hot
    assert np.array_equal(out["mu"][-1].numpy(), k["y"]) and np.array_equal(parts[2][:, 4:].sum(1).numpy(), np.ones(7, F32))


def test_infer_through_the_double_is_the_oracle_clamped_and_free(double):
    k = Ck.stack_case((12, 7), 3, 5, 4)
    net, _, _ = _imdbn()
    dbm = _load(net.to_dbm(), k["Ws"], k["WJ"], k["bs"])
    M = Mt.Model(k["Ws"], k["WJ"], k["bs"])
    for y in (k["y"], None):
        mu, res = dbm.infer(torch.from_numpy(k["data"]), None if y is None else torch.from_numpy(k["labels"]), 3, 0.5)
        want, wres = Mt.infer(M, k["data"], y, 3, 0.5, F32)
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(mu, want)) and np.array_equal(res.numpy(), wres)
        assert mu[0]._base is mu[-1]._base and tuple(mu[0]._base.shape) == (4, 10)
    mu0, res0 = double.mdbm_infer(dbm.layers, dbm.joint, dbm.biases(), torch.from_numpy(k["data"]), None, 0)
    assert float(res0.abs().max()) == 0.0 and np.array_equal(mu0[-1].numpy(), Mt.infer(M, k["data"], None, 0, 0.0, F32)[0][-1])
    muy, pred = dbm.predict_labels(torch.from_numpy(k["data"]), n_mf=3, damp=0.5)
    assert torch.equal(muy, mu[-1]) and torch.equal(pred, mu[-1].argmax(1))


# ---- 4. host logic ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(9, 6), (12, 7, 5), (10, 8, 6, 4)])
@pytest.mark.parametrize("cb,cl", [(False, False), (True, False), (False, True), (True, True)])
def test_the_schedule_is_what_the_double_draws(double, sizes, cb, cl):
    K, J, n = 4, 5, 3
    Ws, WJ, bs = Ck.model(sizes, K, J, 0.3, 1)
    net, _, _ = _imdbn(sizes, K, J)
    dbm = _load(net.to_dbm(), Ws, WJ, bs)
    k = Ck.stack_case(sizes, K, J, n, seed=5)
    parts = [torch.from_numpy(p.copy()) for p in k["particles"]]
    bottom, lab = parts[0].clone(), torch.from_numpy(k["y"])
    tape = Ck.Tape(2)
    rng = R.ReplayRng(tape)
    double.mdbm_gibbs(dbm.layers, dbm.joint, dbm.biases(), parts, 2, rng, clamp_bottom=bottom if cb else None, clamp_labels=lab if cl else None)
    sched = R.sched_mdbm_gibbs(list(sizes) + [J], K, 2, clamp_bottom=cb, clamp_labels=cl)
    assert Ck.draws_of(tape.shapes) == sched and all(s[-2] == n for s in tape.shapes)
    assert len(sched) == 2 * (len(sizes) + 2 - int(cb) - int(cl))
    L = len(sizes) - 1
    # J's class first: the sweep opens with the lowest layer of parity L + 1 and Y follows layer L directly
    first = (L + 1) & 1 if not (cb and (L + 1) & 1 == 0) else 2      # a clamped layer 0 draws nothing
    assert sched[0] == ("u", (list(sizes) + [J])[first]) and (cl or sched[sched.index(("c", K)) - 1] == ("u", sizes[L]))
    if cb:
        assert torch.equal(parts[0], bottom)
    if cl:
        assert torch.equal(parts[L][:, sizes[-1]:], lab)
    want = Mt.gibbs(Mt.Model(Ws, WJ, bs), k["particles"], 2, Ck.Tape(2), F32, clamp_bottom=k["particles"][0] if cb else None,
                    clamp_labels=k["y"] if cl else None)
    assert all(np.array_equal(p.numpy(), w) for p, w in zip(parts, want))
    # Philox: draws_used is the schedule's length
    prng = R.PhiloxRng(11)
    double.mdbm_gibbs(dbm.layers, dbm.joint, dbm.biases(), parts, 2, prng, clamp_bottom=bottom if cb else None, clamp_labels=lab if cl else None)
    assert prng.offset == len(sched)


def test_to_dbm_copies_scales_and_keeps_the_bias_convention(double):
    from imdbn.models import MultimodalDBM
    net, _, _ = _imdbn((12, 7, 5), 3, 6)
    rbms = net.image_idbn.layers + [net.joint_rbm]
    names = ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")
    before = [{n: (getattr(r, n).data if n in names[:3] else getattr(r, n)).clone() for n in names} for r in rbms]
    dbm = net.to_dbm(weight_scale=[1.0, 0.5, 2.0])
    assert isinstance(dbm, MultimodalDBM)
    for r, b in zip(rbms, before):                          # the iMDBN is bit-identical, and shares no storage
        for n, t in b.items():
            cur = getattr(r, n)
            assert torch.equal(cur.data if isinstance(cur, torch.nn.Parameter) else cur, t)
    assert net.joint_rbm.softmax_groups == [(5, 8)] and dbm.joint.softmax_groups == [(5, 8)]
    assert dbm.layers[0].W.data_ptr() != rbms[0].W.data_ptr() and dbm.joint.W.data_ptr() != rbms[2].W.data_ptr()
    assert torch.equal(dbm.layers[0].W.data, rbms[0].W.data) and torch.equal(dbm.layers[1].W.data, rbms[1].W.data * 0.5)
    assert torch.equal(dbm.joint.W.data, rbms[2].W.data * 2.0)
    bs = dbm.biases()
    assert len(bs) == 5 and torch.equal(bs[0], rbms[0].vis_bias.data) and torch.equal(bs[1], rbms[0].hid_bias.data)
    assert torch.equal(bs[2], rbms[1].hid_bias.data) and torch.equal(bs[3], rbms[2].hid_bias.data)
    assert torch.equal(bs[4], rbms[2].vis_bias.data[5:]) and bs[4].data_ptr() == dbm.joint.vis_bias.data[5:].data_ptr()
    assert float(dbm.layers[1].vis_bias.data.abs().max()) == 0.0 and float(dbm.joint.vis_bias.data[:5].abs().max()) == 0.0
    assert float(rbms[2].vis_bias.data[:5].abs().max()) > 0.0
    assert dbm.sizes == [12, 7, 5, 6, 3] and all(not r.sparsity for r in dbm.layers + [dbm.joint])
    with pytest.raises(ValueError):
        net.to_dbm(weight_scale=[1.0, 1.0])


def test_softmax_groups_in_the_image_stack_and_gaussian_layers_are_refused(double):
    from imdbn.models import GaussianRBM
    net, _, _ = _imdbn()
    net.image_idbn.layers[0].softmax_groups = [(2, 5)]
    with pytest.raises(ValueError, match="softmax"):
        net.to_dbm()
    net, _, _ = _imdbn()
    net.image_idbn.layers[0] = GaussianRBM(12, 7, 0.1, 0.0, 0.5)
    with pytest.raises(ValueError, match="Gaussian"):
        net.to_dbm()
    net, _, _ = _imdbn()
    net.joint_rbm.softmax_groups = []
    with pytest.raises(ValueError, match="softmax group"):
        net.to_dbm()


def test_the_group_layer_double_refuses_what_the_engine_refuses(double):
    from imdbn.engine.hip_engine import HipEngine
    from imdbn.engine import native as N
    net, _, _ = _imdbn()
    dbm = net.to_dbm()
    with pytest.raises(N.EngineError, match="softmax group"):
        HipEngine._mdbm_check("t", dbm.layers, dbm.layers[0], dbm.biases())
    with pytest.raises(N.EngineError, match="layer biases"):
        HipEngine._mdbm_check("t", dbm.layers, dbm.joint, dbm.biases()[:-1])
    with pytest.raises(N.EngineError, match="state tensors"):
        double.mdbm_gibbs(dbm.layers, dbm.joint, dbm.biases(), [torch.zeros(2, 12)], 1, R.ReplayRng(Ck.Tape(1)))
    with pytest.raises(N.EngineError, match="side by side"):
        double.mdbm_gibbs(dbm.layers, dbm.joint, dbm.biases(), [torch.zeros(2, 12), torch.zeros(2, 7), torch.zeros(2, 5)], 1,
                          R.ReplayRng(Ck.Tape(1)))
    with pytest.raises(ValueError, match="no particles"):
        dbm.gibbs(1)


def test_save_and_load_reproduce_infer_and_resume_the_particles(double, tmp_path):
    net, X, Y = _imdbn()
    dbm = net.to_dbm()
    E.set_rng(R.ReplayRng(Ck.Tape(5)))
    dbm.train_step(X[:8], Y[:8], 0, 1, n_mf=3, gibbs_k=2)
    path = str(tmp_path / "mdbm.pkl")
    dbm.save_model(path)
    other = _imdbn()[0].to_dbm()
    other.joint.vis_bias.data[:7].fill_(3.0)
    other.load_model(path)
    for y in (Y, None):
        a, b = dbm.infer(X, y, 5, 0.25), other.infer(X, y, 5, 0.25)
        assert all(torch.equal(p, q) for p, q in zip(a[0], b[0])) and torch.equal(a[1], b[1])
    assert all(torch.equal(p, q) and p.data_ptr() != q.data_ptr() for p, q in zip(dbm.particles, other.particles))
    assert all(torch.equal(p, q) for p, q in zip(dbm.bias_momenta(), other.bias_momenta()))
    assert all(torch.equal(r.W_m, s.W_m) for r, s in zip(dbm._rbms(), other._rbms())) and float(other.joint.vis_bias.data[:7].abs().max()) == 0.0
    state = pickle.load(open(path, "rb"))
    assert sorted(state) == ["W", "W_m", "bias_momenta", "biases", "particles", "sizes"] and len(state["biases"]) == 4
    assert tuple(state["biases"][-1].shape) == (3,) and len(state["W"]) == 2
    E.set_rng(R.ReplayRng(Ck.Tape(6))); dbm.gibbs(2)
    E.set_rng(R.ReplayRng(Ck.Tape(6))); other.gibbs(2)
    assert all(torch.equal(p, q) for p, q in zip(dbm.particles, other.particles))


def test_without_monitor_no_reconstruction_is_launched_and_finetune_logs(double):
    net, X, Y = _imdbn()
    dbm = net.to_dbm()
    E.set_rng(R.ReplayRng(Ck.Tape(5)))
    dbm.init_particles(X[:8], Y[:8])
    assert [tuple(p.shape) for p in dbm.particles] == [(8, 12), (8, 10), (8, 5)] and torch.equal(dbm.particles[1][:, 7:], Y[:8])
    downs = lambda: sum(1 for c in double.calls if c[0] == "prop_down")
    double.calls.clear()
    assert dbm.train_step(X[:8], Y[:8], 0, 1, n_mf=2, gibbs_k=3, monitor=False) is None
    quiet = downs()
    assert double.calls[0] == ("mdbm_step", (8, 12), 2, 0.0, 3, False) and sum(1 for c in double.calls if c[0] == "assoc_update") == 2
    double.calls.clear()
    out = dbm.train_step(X[:8], Y[:8].argmax(1), 0, 1, n_mf=2, gibbs_k=3, monitor=True)          # class indices are accepted too
    assert downs() == quiet + 1 and out["recon_loss"].dim() == 0 and out["res"].shape == (8,)
    p0 = dbm.particles[0]
    dbm.train_step(X[:5], Y[:5], 0, 1, n_mf=1, gibbs_k=1, monitor=False)
    assert dbm.particles[0] is p0 and p0.shape == (8, 12)
    double.calls.clear()
    dbm.finetune(2, n_mf=2, gibbs_k=1, lr_scale=0.5, log_every=1)
    assert [h[0] for h in dbm.history] == [0, 1] and all(np.isfinite(h[1]) and h[2] >= 0 for h in dbm.history)
    assert sum(1 for c in double.calls if c[0] == "mdbm_step") == 6
    img = dbm.generate(torch.tensor([0, 1, 2]), n_sweeps=3)
    assert tuple(img.shape) == (3, 12) and float(img.min()) >= 0.0 and float(img.max()) <= 1.0 and dbm.particles[0] is p0


def test_data_parallel_runs_are_refused(double, monkeypatch):
    net, X, Y = _imdbn()
    dbm = net.to_dbm()
    parts = dbm.init_particles(X[:8], Y[:8])
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        dbm.train_step(X[:8], Y[:8], 0, 1)
    with pytest.raises(NotImplementedError):
        double.mdbm_step(dbm.layers, dbm.joint, X[:8], Y[:8], parts, [(0.1, 0.5)] * 2, 1, 0.0, 1, R.ReplayRng(Ck.Tape(1)))
    with pytest.raises(NotImplementedError):
        double.mdbm_infer(dbm.layers, dbm.joint, dbm.biases(), X[:8], None, 1)
    with pytest.raises(NotImplementedError):
        double.mdbm_gibbs(dbm.layers, dbm.joint, dbm.biases(), parts, 1, R.ReplayRng(Ck.Tape(1)))
