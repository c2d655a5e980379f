"""CPU-only: the float64 reference and the fp32 twin of the DBM density arithmetic (tests/dbm_ais_oracle.py) against exact
enumeration (tests/dbm_oracle.py), the margins that let the GPU tests compare states bit for bit, and the host logic of
imdbn.utils.likelihood's DBM functions through the engine double (tests/dbm_ais_engine_double.py).  No claim about the kernel is
made here -- that is tested on the GPU in test_dbm_ais_gpu.py."""
import numpy as np
import pytest
import torch

import dbm_ais_cases as Ca
import dbm_ais_oracle as At
import dbm_cases as Ck
import dbm_oracle as Dt
from dbm_ais_engine_double import DbmAisOracleEngine
from imdbn import engine as E
from imdbn.engine import rng as R
from test_dbm_cpu import _dbm

F32, F64 = np.float32, np.float64


# ---- 1. AIS against enumeration ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,scale,with_base", Ca.SMALL, ids=str)
def test_the_twins_log_z_is_within_three_standard_errors_of_the_enumeration(sizes, scale, with_base):
    Ws, bs, base = Ca.small_model(sizes, scale)
    base = base if with_base else None
    want = Dt.log_z(Ws, bs)
    betas = np.linspace(0.0, 1.0, Ca.SMALL_K + 1).astype(F32)
    seed = Ca.SMALL_SEEDS[tuple(sizes)]
    logw, _ = At.ais(Ws, bs, betas, Ca.SMALL_M, Ck.Tape(seed), base, F32)
    got, se = At.weight_stats(logw, At.log_z_base(sizes, base))
    print(f"{sizes} seed {seed}: log Z {got:.5f} vs exact {want:.5f}: {abs(got - want) / se:.2f} se (se {se:.4f})")
    assert np.isfinite(got) and se > 0 and abs(got - want) <= 3 * se


def test_the_twin_follows_the_reference_on_equal_states():
    Ws, bs, base = Ca.ais_case((67, 64, 33, 5), 5)
    bound, margins = [], []
    ref, rs = At.ais(Ws, bs, Ca.AIS_BETAS, 5, Ck.Tape(Ca.AIS_SEEDS[((67, 64, 33, 5), 1)]), base, F64, margins=margins, bound=bound)
    tw, ts = At.ais(Ws, bs, Ca.AIS_BETAS, 5, Ck.Tape(Ca.AIS_SEEDS[((67, 64, 33, 5), 1)]), base, F32)
    assert min(margins) > 0 and all(np.array_equal(a, b) for a, b in zip(rs, ts))
    assert (np.abs(tw - ref) <= bound[0]).all()


# ---- 2. the bound against enumeration -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,scale,with_base", Ca.SMALL, ids=str)
def test_the_bound_is_the_enumerated_one_stays_under_log_p_and_does_not_fall(sizes, scale, with_base):
    Ws, bs, _ = Ca.small_model(sizes, scale)
    v = (np.random.default_rng(60).random((6, sizes[0])) < 0.4).astype(F64)
    lz = Dt.log_z(Ws, bs)
    lp = Dt.log_p(Ws, bs, v, lz)
    trace = []
    Dt.infer(Ws, bs, v, 30, 0.0, F64, trace=trace)
    got = np.array([At.bound_rows(Ws, bs, v, mu) - lz for mu in trace])
    want = np.array([Dt.variational_bound(Ws, bs, v, mu, lz) for mu in trace])
    assert np.abs(got - want).max() < 1e-11
    assert (got <= lp[None, :] + 1e-12).all()
    assert (np.diff(got, axis=0) >= -1e-12).all()


# ---- 3. replay margins: no comparison of the GPU tests is a near tie -------------------------------------------------------------------------
def layer_margin(k):
    """The smallest |p - U| minus the bound of p over the draws test_dbm_ais_gpu.py makes from a layer case: at beta = 1 without a base
    and at BETA with one."""
    ops = (k["W_lo"], k["x_lo"], k["W_hi"], k["x_hi"], k["bias"])
    u = k["u"].astype(F64)
    out = []
    for beta, base in ((1.0, None), (Ca.BETA, k["base"])):
        out.append(float((np.abs(At.sample_p(*ops, beta, base, F64) - u) - At.sample_p_bound(*ops, beta, base)).min()))
    return min(out)


def ais_margin(sizes, M, seed):
    Ws, bs, base = Ca.ais_case(sizes, M)
    margins = []
    At.ais(Ws, bs, Ca.AIS_BETAS, M, Ck.Tape(seed), base, F64, margins=margins)
    return min(margins)


@pytest.mark.parametrize("case", Ca.LAYER_CASES, ids=str)
def test_no_uniform_of_a_layer_case_lies_within_the_bound_of_its_probability(case):
    assert layer_margin(Ca.layer_case(case)) > 0.0


@pytest.mark.parametrize("sizes,M", Ca.STACKS, ids=str)
def test_no_uniform_of_a_whole_run_lies_within_the_bound_of_its_probability(sizes, M):
    assert ais_margin(sizes, M, Ca.AIS_SEEDS[(sizes, M)]) > 0.0


# ---- 4. host logic through the double ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def double():
    eng = DbmAisOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)
    E.set_rng(None)


def test_the_draw_schedule():
    assert R.sched_dbm_ais((8, 6, 4), 3) == [("u", 6)] + 2 * [("u", 8), ("u", 4), ("u", 6)]
    assert R.sched_dbm_ais((6, 5, 4, 3), 2) == [("u", 5), ("u", 3), ("u", 6), ("u", 4), ("u", 5), ("u", 3)]
    assert R.sched_dbm_ais((8, 5), 1) == [("u", 5)]


@pytest.mark.parametrize("sizes", [(8, 6, 4), (6, 5, 4, 3), (8, 5)], ids=str)
def test_the_run_draws_its_schedule_and_is_the_twin(double, sizes):
    from imdbn.utils import likelihood as LL
    Ws, bs, base = Ca.small_model(sizes, 0.5)
    net = _dbm(sizes, Ws, bs)
    betas = LL.linear_betas(4)
    tape = Ck.Tape(3)
    logw, states = double.dbm_ais(net.layers, net.biases(), betas, 7, R.ReplayRng(tape), base_bias=torch.from_numpy(base), return_state=True)
    assert tape.shapes == [(7, n) for _, n in R.sched_dbm_ais(sizes, 4)]
    want, s = At.ais(Ws, bs, betas.numpy(), 7, Ck.Tape(3), base, F32)
    assert np.array_equal(logw.numpy(), want) and all(np.array_equal(a.numpy(), b) for a, b in zip(states, s[1::2]))
    # a Philox source advances by the schedule's length
    prng = E.PhiloxRng(5)
    double.dbm_ais(net.layers, net.biases(), betas, 7, prng)
    assert prng.offset == len(R.sched_dbm_ais(sizes, 4))


def test_estimate_and_bound_on_the_double(double):
    from imdbn.utils import likelihood as LL
    sizes = (8, 6, 4)
    Ws, bs, base = Ca.small_model(sizes, 0.5)
    net = _dbm(sizes, Ws, bs)
    E.set_rng(E.PhiloxRng(11))
    est = net.log_partition(n_chains=32, n_betas=50, base_bias=torch.from_numpy(base), seed=4)
    assert E.get_rng().offset == 0, "a seeded estimate moved the ambient draw counter"
    again = LL.estimate_dbm_log_partition(net, n_chains=32, n_betas=50, base_bias=torch.from_numpy(base), seed=4)
    assert set(est) == {"log_z", "log_z_base", "logw", "ess", "se"} and est["log_z"] == again["log_z"]
    assert abs(est["log_z_base"] - At.log_z_base(sizes, base)) < 1e-9 and abs(est["log_z"] - Dt.log_z(Ws, bs)) < 1.0
    # the bound: the float64 figure of the twin's magnetisations, under log p
    v = (np.random.default_rng(61).random((5, 8)) < 0.4).astype(F32)
    lz = Dt.log_z(Ws, bs)
    got = net.log_likelihood_bound(torch.from_numpy(v), lz, n_mf=12).numpy()
    mu, _ = Dt.infer(Ws, bs, v, 12, 0.0, F32)
    assert got.dtype == F64 and np.abs(got - (At.bound_rows(Ws, bs, v, mu, F32) - lz)).max() < 1e-9
    assert np.abs(got - Dt.variational_bound(Ws, bs, v, mu, lz)).max() < 1e-4 and (got <= Dt.log_p(Ws, bs, v, lz) + 1e-6).all()


def test_evaluate_sums_over_the_loader_and_logs(double):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.utils import likelihood as LL
    sizes = (8, 6, 4)
    Ws, bs, _ = Ca.small_model(sizes, 0.5)
    X = torch.from_numpy((np.random.default_rng(62).random((11, 8)) < 0.4).astype(F32))
    net = _dbm(sizes, Ws, bs, dataloader=DataLoader(TensorDataset(X, torch.zeros(11)), batch_size=4))
    logged = []
    net.wandb_run = type("Run", (), {"log": lambda self, d: logged.append(d)})()
    lz = Dt.log_z(Ws, bs)
    res = LL.evaluate_dbm_log_likelihood(net, log_z=lz, n_mf=5)
    want = net.log_likelihood_bound(X, lz, n_mf=5).sum().item()
    assert res["n"] == 11 and abs(res["sum_bound"] - want) < 1e-9 and abs(res["mean_bound"] - want / 11) < 1e-9
    assert res["se"] is None and res["ess"] is None and res["log_z"] == lz
    assert logged == [{"ll/dbm_mean_bound": res["mean_bound"], "ll/dbm_log_z": lz}]
    two = LL.evaluate_dbm_log_likelihood(net, log_z=lz, n_mf=5, max_batches=2)
    assert two["n"] == 8
    est = LL.evaluate_dbm_log_likelihood(net, n_mf=5, n_chains=16, n_betas=20, seed=1)
    assert est["se"] is not None and est["ess"] > 1 and np.isfinite(est["mean_bound"])
    net.dataloader = None
    assert LL.evaluate_dbm_log_likelihood(net, log_z=lz) is None


def test_refusals(double, monkeypatch):
    from imdbn.models.grbm import GaussianRBM
    from imdbn.utils import likelihood as LL
    sizes = (8, 6, 4)
    Ws, bs, _ = Ca.small_model(sizes, 0.5)
    net = _dbm(sizes, Ws, bs)
    v = torch.zeros(2, 8)
    with pytest.raises(ValueError, match="base_bias must have 8"):
        net.log_partition(n_chains=4, n_betas=3, base_bias=torch.zeros(7))
    net.layers[1].softmax_groups = [(0, 3)]
    for call in (lambda: net.log_partition(n_chains=4, n_betas=3), lambda: net.log_likelihood_bound(v, 0.0),
                 lambda: LL.evaluate_dbm_log_likelihood(net, log_z=0.0)):
        with pytest.raises(ValueError, match="softmax groups"):
            call()
    net.layers[1].softmax_groups = []
    keep = net.layers[0]
    net.layers[0] = GaussianRBM(8, 6, 0.1, 0.0, 0.5)
    with pytest.raises(ValueError, match="GaussianRBM"):
        net.log_partition(n_chains=4, n_betas=3)
    with pytest.raises(ValueError, match="GaussianRBM"):
        net.log_likelihood_bound(v, 0.0)
    net.layers[0] = keep
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        net.log_partition(n_chains=4, n_betas=3)
    with pytest.raises(NotImplementedError):
        net.log_likelihood_bound(v, 0.0)
    monkeypatch.undo()
    with pytest.raises(Exception):
        double.dbm_ais(net.layers, net.biases()[:-1], [0.0, 1.0], 4, E.PhiloxRng(1))
    assert not [c for c in double.calls if c[0] in ("dbm_ais", "dbm_bound", "dbm_infer")], "a refused call reached the engine"
