"""GPU: imdbn_rbm_bound_step / HipEngine.bound_step and the dbn_* functions of imdbn/utils/likelihood.py against the numpy twin
(tests/bound_oracle.py) and the enumerated bound and likelihood of small stacks.

Parity: every case's seed was chosen on the CPU so that the twin's smallest Bernoulli margin |p - u| is >= 1e-5 (asserted first), so
every decision of the device must be the twin's: h is compared exactly.  acc is held to (V + H) * 1e-5 + 1e-9 |acc|: an error delta
in a logit a_i moves v_i a_i - softplus(a_i) by |v_i - sigmoid(a_i)| delta <= delta per visible unit, an error in x_j moves the
entropy by |x_j| sigmoid'(x_j) delta < delta and log q by |h_j - sigmoid(x_j)| delta <= delta per hidden unit, and 1e-5 is the
logit agreement the parity tests of the propagations hold (test_parity_gpu.py) -- the rule of test_ais_gpu.py.  The whole path adds
the top layer's free energy, which the engine sums in fp32: n = V + H terms, at most n 2^-24 of the sum of their magnitudes.
Truth: the device estimates within 5 of the TWIN's standard errors of the enumerated values."""
import ctypes as C

import numpy as np
import pytest
import torch

import anneal_oracle as A
import bound_cases as Cs
import bound_oracle as B
from likelihood_gpu import DEV, _native, close, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)
from oracle.draws import DrawStream, PhiloxStream

pytestmark = pytest.mark.gpu
REPLAY_SEED = 11
MODES = ["entropy", "logq"]


class _Stack:
    def __init__(self, layers):
        self.layers = [device_rbm(l) for l in layers]


def _twin(name, mode):
    """(case, acc, h, margin) of a parity case under its pinned Philox seed."""
    def run():
        c = Cs.parity_case(name)
        return (c,) + B.bound_step(c["W"], c["b"], c["c"], c["v"], mode, PhiloxStream(c["seed"]))
    return twin(("bound_step", name, mode), run)


def _close(got, want, n_units, what, extra=0.0):
    close(got, want, n_units * 1e-5 + 1e-9 * np.abs(want) + extra, what)


# ---- 1. parity with the twin ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(Cs.PARITY))
def test_parity_with_the_twin(eng, name, mode):
    from imdbn import engine as E
    c, acc, h, margin = _twin(name, mode)
    print(f"{name}: twin margin {margin:.3g}")
    assert margin >= Cs.MARGIN
    r = device_rbm(c)
    rng = E.PhiloxRng(c["seed"])
    a, hd = eng.bound_step(r, dev(c["v"]), rng, mode=mode)
    torch.cuda.synchronize()
    assert a.dtype == torch.float64 and tuple(a.shape) == (c["M"],) and tuple(hd.shape) == (c["M"], c["H"]) and rng.offset == 1
    bad = np.nonzero(hd.cpu().numpy() != h)
    assert bad[0].size == 0, f"{name}: h differs at {list(zip(*bad))[:6]}"
    _close(a.cpu().numpy(), acc, c["V"] + c["H"], f"{name} {mode}")


# ---- 2. sampling, draws, determinism ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_h_is_the_sample_of_prop_up_and_draws_are_row_keyed(eng, name):
    from imdbn import engine as E
    from imdbn.engine import rng as R
    c = Cs.parity_case(name)
    r = device_rbm(c)
    x9 = Cs.inputs(9, c["V"], 3, False)
    margin = B.bound_step(c["W"], c["b"], c["c"], x9, "logq", PhiloxStream(c["seed"]))[2]
    assert margin >= Cs.MARGIN          # the two up propagations sum their logits in different orders
    v9 = dev(x9)
    rng = E.PhiloxRng(c["seed"])
    a9, h9 = eng.bound_step(r, v9, rng, mode="logq")
    _, hs = eng.prop_up(r, v9, sample=True, rng=E.PhiloxRng(c["seed"]))
    assert torch.equal(h9, hs)
    # determinism
    b9, k9 = eng.bound_step(r, v9, E.PhiloxRng(c["seed"]), mode="logq")
    assert torch.equal(a9, b9) and torch.equal(h9, k9)
    # one draw; the next call draws what it would after skipping the schedule
    assert rng.offset == 1 == len(R.sched_bound(c["H"]))
    _, h1 = eng.prop_up(r, v9, sample=True, rng=rng)
    skip = E.PhiloxRng(c["seed"])
    eng.skip_draws(skip, R.sched_bound(c["H"]), 9)
    _, h2 = eng.prop_up(r, v9, sample=True, rng=skip)
    assert torch.equal(h1, h2) and rng.offset == skip.offset == 2
    # the Philox key is the row: the first 5 rows of the 9-row call are the 5-row call
    a5, h5 = eng.bound_step(r, v9[:5], E.PhiloxRng(c["seed"]), mode="logq")
    assert torch.equal(a5, a9[:5]) and torch.equal(h5, h9[:5])


def test_replay_tape_matches_the_twin_fed_the_same_tape(eng):
    from imdbn import engine as E
    c = Cs.parity_case("tiny")
    want, h, margin = B.bound_step(c["W"], c["b"], c["c"], c["v"], "logq", DrawStream(REPLAY_SEED))
    print(f"replay: twin margin {margin:.3g}")
    assert margin >= Cs.MARGIN
    a, hd = eng.bound_step(device_rbm(c), dev(c["v"]), E.ReplayRng(DrawStream(REPLAY_SEED)), mode="logq")
    assert np.array_equal(hd.cpu().numpy(), h)
    _close(a.cpu().numpy(), want, c["V"] + c["H"], "replay")


def test_the_call_adds_to_a_non_zero_acc(eng):
    from imdbn import engine as E
    c, acc, _, margin = _twin("mid", "entropy")
    assert margin >= Cs.MARGIN
    start = torch.arange(c["M"], dtype=torch.float64, device=DEV) - 3.5
    a, _ = eng.bound_step(device_rbm(c), dev(c["v"]), E.PhiloxRng(c["seed"]), acc=start, mode="entropy")
    assert a is start
    _close(a.cpu().numpy(), acc + np.arange(c["M"]) - 3.5, c["V"] + c["H"], "accumulate")


# ---- 3. the whole path ------------------------------------------------------------------------------------------------
def _path_tol(layers, mag):
    units = sum(W.shape[0] + W.shape[1] for W, _, _ in layers)
    Vt, Ht = layers[-1][0].shape
    return units, (Vt + Ht) * 2.0 ** -24 * mag


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["p3", "p4"])
def test_sample_values_of_a_stack_match_the_twin(eng, name, mode):
    from imdbn.utils import likelihood as LK
    L = Cs.stack(name)
    v = Cs.inputs(Cs.PATH["B"], L[0][0].shape[0], Cs.PATH["in_seed"], False)
    S, seed = Cs.PATH["S"], Cs.PATH_SEED[name]
    want, margin, mag = B.dbn_values(L, v, S, mode, PhiloxStream(seed), 1.25)
    print(f"{name}: twin margin {margin:.3g}")
    assert margin >= Cs.MARGIN
    got = LK.dbn_sample_values(_Stack(L), dev(v), 1.25, n_samples=S, mode=mode, seed=seed)
    assert got.dtype == torch.float64 and tuple(got.shape) == (Cs.PATH["B"], S) and got.is_cuda
    units, extra = _path_tol(L, mag)
    _close(got.cpu().numpy(), want, units, f"{name} {mode}", extra)


def test_a_stack_of_one_is_log_likelihood_bit_for_bit(eng):
    from imdbn.utils import likelihood as LK
    c = Cs.parity_case("mid")
    r = device_rbm(c)
    v = dev(c["v"])
    assert torch.equal(LK.dbn_sample_values(r, v, 2.5)[:, 0], LK.log_likelihood(r, v, 2.5))


# ---- 4. against the truth ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s3", "s4"])
def test_estimates_against_the_enumerated_bound_and_likelihood(eng, name):
    from imdbn.models.idbn import iDBN
    from imdbn.utils import likelihood as LK
    L = Cs.stack(name)
    v = Cs.inputs(Cs.TRUTH["B"], L[0][0].shape[0], Cs.TRUTH["in_seed"], False)
    lp, lb, lz = B.exact_dbn_log_p(L, v), B.exact_dbn_bound(L, v), A.exact_log_z(*L[-1])
    seed, S, S2 = Cs.TRUTH_SEED[name], Cs.TRUTH["S_entropy"], Cs.TRUTH["S_logq"]
    m = iDBN.__new__(iDBN)                                             # the method needs the layers only
    m.layers = _Stack(L).layers
    tw, _, _ = B.dbn_values(L, v, S, "entropy", PhiloxStream(seed), lz)
    t_se = tw.std(1, ddof=1) / np.sqrt(S)
    got = m.log_likelihood_bound(dev(v), lz, n_samples=S, seed=seed).cpu().numpy()
    print(f"{name}: bound errors {((got - lb) / t_se).round(2)} twin se")
    assert (np.abs(got - lb) <= 5 * t_se).all()
    tq, _, _ = B.dbn_values(L, v[:1], S2, "logq", PhiloxStream(seed), lz)
    _, q_se, _ = A.weight_stats(tq[0])
    est = float(LK.dbn_log_likelihood_is(m, dev(v[:1]), lz, n_samples=S2, seed=seed)[0])
    print(f"{name}: log p_hat {est:.4f}, exact {lp[0]:.4f}, error {(est - lp[0]) / q_se:+.2f} twin se")
    assert abs(est - lp[0]) <= 5 * q_se


# ---- 5. errors --------------------------------------------------------------------------------------------------------
def _raw(eng, r, v, M, mode=0, short=0):
    """The export called directly on a sentinel-filled acc -> (EngineError message or None, acc)."""
    from imdbn.engine import native as N, rng as R
    from imdbn import engine as E
    d = eng._desc(r, False)
    acc = torch.full((max(M, 1),), -7.25, dtype=torch.float64, device=DEV)
    h = torch.empty(max(M, 1), d.H, device=DEV)
    nr, _ = eng._rng(E.PhiloxRng(1), R.sched_bound(d.H), max(M, 1), torch.device(DEV))
    ws, nbytes, stream = eng._ws_tail(torch.device(DEV), d.V, d.H, max(M, 1))
    msg = None
    try:
        eng._call("imdbn_rbm_bound_step", C.byref(d), C.c_void_p(v.data_ptr()), v.stride(0), M, mode, C.byref(nr), C.c_void_p(acc.data_ptr()),
                  C.c_void_p(h.data_ptr()), d.H, ws, nbytes - short, stream)
    except N.EngineError as e:
        msg = str(e)
    torch.cuda.synchronize()
    return msg, acc


@pytest.mark.parametrize("what,code", [("groups", -5), ("M0", -1), ("mode", -1), ("short", -2)])
def test_invalid_arguments_launch_nothing(eng, what, code):
    c = Cs.parity_case("tiny")
    v = dev(c["v"])
    r = device_rbm(c, groups=[(15, 20)] if what == "groups" else None)
    msg, acc = _raw(eng, r, v, 0 if what == "M0" else 5, mode=7 if what == "mode" else 0, short=1 if what == "short" else 0)
    print(what, "->", msg)
    assert msg is not None and f"rc={code})" in msg
    assert (acc == -7.25).all()
    if what == "mode":
        assert "7" in msg                                              # the offending value is named
    # the same workspace still serves a good call
    msg, acc = _raw(eng, device_rbm(c), v, 5)
    assert msg is None and torch.isfinite(acc).all() and not (acc == -7.25).any()


def test_python_entry_raises_engine_error(eng):
    from imdbn import engine as E
    c = Cs.parity_case("tiny")
    with pytest.raises(E.EngineError):
        eng.bound_step(device_rbm(c), dev(c["v"]), E.PhiloxRng(1), mode="mean")
    with pytest.raises(E.EngineError):
        eng.bound_step(device_rbm(c, groups=[(15, 20)]), dev(c["v"]), E.PhiloxRng(1))


# ---- 6. nothing else moved --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mid", "wide_p301"])
def test_free_energy_and_weights_are_untouched(eng, name):
    from imdbn import engine as E
    c = Cs.parity_case(name)
    r = device_rbm(c)
    v = dev(c["v"])
    g = np.random.Generator(np.random.PCG64(2))
    x = dev((g.random((c["M"], c["V"])) > 0.5).astype(np.float32))    # M rows: the workspace of the bound_step call
    W0, b0, c0, v0 = r.W.data.clone(), r.vis_bias.data.clone(), r.hid_bias.data.clone(), v.clone()
    F0 = eng.free_energy(r, x)
    eng.bound_step(r, v, E.PhiloxRng(c["seed"]))
    F1 = eng.free_energy(r, x)
    assert torch.equal(F0, F1) and torch.equal(v, v0)
    assert torch.equal(r.W.data, W0) and torch.equal(r.vis_bias.data, b0) and torch.equal(r.hid_bias.data, c0)
