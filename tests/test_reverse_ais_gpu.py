"""GPU: imdbn_rbm_reverse_ais / imdbn_rows_logmeanexp and the reverse-AIS functions of imdbn/utils/likelihood.py against the numpy
twin (tests/anneal_oracle.py) and the enumerated annealing model.

Parity: every case's seed was chosen on the CPU so that the twin's smallest Bernoulli margin |p - u| is >= 1e-5 and its smallest
categorical margin >= 1e-6 (asserted first), so every decision of the device must be the twin's: the final states u_1 are compared
exactly.  logw is held to 2 H 1e-5 + 1e-9 |logw|: an error delta = 1e-5 in a logit (the agreement the parity tests of the propagations
hold, test_parity_gpu.py) moves -F of the start state by <= delta per hidden unit, and the whole ladder,
sum_k (beta_k - beta_{k-1}) sigmoid(.) delta, by <= delta per hidden unit again.  Truth: the device estimate of every row within 5 of
the TWIN's standard errors of the enumerated log p_ann(x), its own se within twice the twin's."""
import ctypes as C

import numpy as np
import pytest
import torch

import anneal_cases as Cs
import anneal_oracle as A
from likelihood_gpu import DEV, _native, base_bias, close, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)
from oracle.draws import DrawStream, PhiloxStream

pytestmark = pytest.mark.gpu


def _twin(name):
    """(case, logw, u_1, margin, categorical margin) of a parity case under its pinned Philox seed."""
    def run():
        c = Cs.case(Cs.REVERSE, name)
        return (c,) + A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], c["groups"], c["betas"], c["x"], PhiloxStream(c["seed"]))
    return twin(("reverse_ais", name), run)


def _close(got, want, H, what):
    close(got, want, 2 * H * 1e-5 + 1e-9 * np.abs(want), what)


# ---- 1. parity with the twin ------------------------------------------------------------------------------------------
# wide: the constructor's padded pitch (float4 weight rows: k2_stream reads the hidden bit plane); wide_bA: rows 301 floats apart
# (unaligned: the fused K2 reads the bit plane); one: K = 1; rows70: two 64-row chunks
@pytest.mark.parametrize("name,pitch", [("tiny", None), ("tiny_bA", None), ("mid", None), ("mid_bA", 75), ("wide", None), ("wide_bA", 301),
                                        ("group", None), ("one", None), ("rows70", None), ("four256", None)])
def test_parity_with_the_twin(eng, name, pitch):
    from imdbn import engine as E
    from imdbn.engine import rng as R
    c, logw, u1, margin, cat_margin = _twin(name)
    print(f"{name}: twin margin {margin:.3g}, categorical margin {cat_margin:.3g}")
    assert margin >= Cs.MARGIN and cat_margin >= Cs.CAT_MARGIN
    r = device_rbm(c, pitch)
    rng = E.PhiloxRng(c["seed"])
    lw, u = eng.reverse_ais(r, dev(c["x"]), c["betas"], rng, base_vis_bias=base_bias(c), return_state=True)
    torch.cuda.synchronize()
    assert lw.dtype == torch.float64 and tuple(lw.shape) == (c["R"],) and tuple(u.shape) == (c["R"], c["V"])
    assert rng.offset == c["K"] * (2 + len(c["groups"])) == len(R.sched_reverse_ais(c["V"], c["H"], c["groups"], c["K"]))
    bad = np.nonzero(u.cpu().numpy() != u1)
    assert bad[0].size == 0, f"{name}: u_1 differs at {list(zip(*bad))[:6]}"
    _close(lw.cpu().numpy(), logw, c["H"], name)


def test_replay_tape_matches_the_twin_fed_the_same_tape(eng):
    from imdbn import engine as E
    c = Cs.case(Cs.REVERSE, Cs.REPLAY_CASE)
    want, u1, margin, _ = A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], [], c["betas"], c["x"], DrawStream(Cs.REPLAY_SEED))
    print(f"replay: twin margin {margin:.3g}")
    assert margin >= Cs.MARGIN
    lw, u = eng.reverse_ais(device_rbm(c), dev(c["x"]), c["betas"], E.ReplayRng(DrawStream(Cs.REPLAY_SEED)), base_vis_bias=base_bias(c), return_state=True)
    assert np.array_equal(u.cpu().numpy(), u1)
    _close(lw.cpu().numpy(), want, c["H"], "replay")


# ---- 2. against the truth ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bA", [False, True])
def test_estimate_against_the_enumerated_annealing_model(eng, with_bA):
    from imdbn.utils import likelihood as LK
    c = Cs.reverse_truth(with_bA)
    lp, st = A.annealing_model(c["W"], c["b"], c["c"], c["bA"], c["betas"])
    x, want = Cs.truth_rows(lp, st)
    t_logw, _, _, _ = A.reverse_ais_logw(c["W"], c["b"], c["c"], c["bA"], [], c["betas"], np.repeat(x, c["M"], 0), PhiloxStream(c["seed"]))
    _, t_se, _ = A.row_stats(t_logw, c["M"])
    res = LK.reverse_ais_log_likelihood(device_rbm(c), torch.from_numpy(x).to(DEV), n_chains=c["M"], betas=c["betas"], base_vis_bias=base_bias(c),
                                        seed=c["seed"])
    got = res["ll"].cpu().numpy()
    lme, se, ess = A.row_stats(res["logw"].cpu().numpy(), c["M"])
    print(f"b_A {with_bA}: device {got.round(4)}, exact {want.round(4)}, errors {((got - want) / t_se).round(2)} twin se; "
          f"se {se.round(4)} (twin {t_se.round(4)}), ess {ess.round(1)}")
    assert res["ll"].dtype == torch.float64 and got.shape == (c["N"],) and tuple(res["logw"].shape) == (c["N"], c["M"])
    assert (np.abs(got - want) <= 5 * t_se).all()
    assert (se <= 2 * t_se).all()
    assert np.allclose(got, lme - A.log_z_base(c["V"], c["H"], c["bA"], []), rtol=1e-12, atol=1e-12)
    assert np.allclose(res["ess"].cpu().numpy(), ess, rtol=1e-12)


# ---- 3. determinism and draws -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_bA", "mid", "wide", "group"])
def test_determinism_draw_count_and_row_keyed_draws(eng, name):
    from imdbn import engine as E
    from imdbn.engine import rng as R
    c = Cs.case(Cs.REVERSE, name)
    r = device_rbm(c)
    bA = base_bias(c)
    sched = R.sched_reverse_ais(c["V"], c["H"], c["groups"], c["K"])
    rng = E.PhiloxRng(c["seed"])
    a = eng.reverse_ais(r, dev(c["x"]), c["betas"], rng, base_vis_bias=bA)
    b = eng.reverse_ais(r, dev(c["x"]), c["betas"], E.PhiloxRng(c["seed"]), base_vis_bias=bA)
    assert torch.equal(a, b)
    assert rng.offset == len(sched)
    # the next call draws what it would after skipping the schedule
    g = np.random.Generator(np.random.PCG64(1))
    x = torch.from_numpy((g.random((6, c["V"])) > 0.5).astype(np.float32)).to(DEV)
    _, h1 = eng.prop_up(r, x, sample=True, rng=rng)
    skip = E.PhiloxRng(c["seed"])
    eng.skip_draws(skip, sched, c["R"])
    _, h2 = eng.prop_up(r, x, sample=True, rng=skip)
    assert torch.equal(h1, h2) and rng.offset == skip.offset == len(sched) + 1
    # the Philox key is the row: the first 5 engine rows of a 9-row run are the 5-row run
    x9 = torch.from_numpy(Cs.start_rows(9, c["V"], 17, c["groups"])).to(DEV)
    five = eng.reverse_ais(r, x9[:5], c["betas"], E.PhiloxRng(c["seed"]), base_vis_bias=bA)
    nine = eng.reverse_ais(r, x9, c["betas"], E.PhiloxRng(c["seed"]), base_vis_bias=bA)
    assert torch.equal(five, nine[:5])


@pytest.mark.parametrize("name", ["tiny_bA", "group"])
def test_python_function_is_chunk_invariant(eng, name):
    """11 test rows x 4 chains: one chunk of 44 engine rows against chunks of 16, 16 and 12 (all within one 64-row multiple)."""
    from imdbn import engine as E
    from imdbn.utils import likelihood as LK
    c = Cs.case(Cs.REVERSE, name)
    r = device_rbm(c)
    x = torch.from_numpy(Cs.start_rows(11, c["V"], 8, c["groups"])).to(DEV)
    kw = dict(n_chains=4, betas=c["betas"], base_vis_bias=base_bias(c), seed=6)
    one = LK.reverse_ais_log_likelihood(r, x, max_rows=4096, **kw)
    many = LK.reverse_ais_log_likelihood(r, x, max_rows=16, **kw)
    for k in ("ll", "ess", "logw"):
        assert torch.equal(one[k], many[k]), k
    assert torch.isfinite(one["ll"]).all()
    E.manual_seed(3)
    LK.reverse_ais_log_likelihood(r, x, n_chains=4, betas=c["betas"], max_rows=16)
    assert E.get_rng().offset == c["K"] * (2 + len(c["groups"]))


# ---- 4. rows_logmeanexp -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", [(3, 1), (3, 5), (2, 64), (2, 70)])
def test_rows_logmeanexp_against_numpy(eng, N, M):
    g = np.random.Generator(np.random.PCG64(10 * N + M))
    x = -800.0 * g.random((N, M))
    x[1, M // 2] = np.nan                                              # one NaN row that must stay NaN while the others do not
    lme, ess = eng.rows_logmeanexp(torch.from_numpy(x).to(DEV), M)
    torch.cuda.synchronize()
    lme, ess = lme.cpu().numpy(), ess.cpu().numpy()
    want_l, want_e = A.rows_logmeanexp(x, M)
    keep = np.arange(N) != 1
    assert lme.dtype == np.float64 and lme.shape == ess.shape == (N,)
    assert np.isnan(lme[1]) and np.isnan(ess[1]) and np.isfinite(lme[keep]).all() and np.isfinite(ess[keep]).all()
    print(f"N {N} M {M}: max |lme - numpy| {np.abs(lme[keep] - want_l[keep]).max():.3g}, max rel ess {np.abs(ess[keep] / want_e[keep] - 1).max():.3g}")
    assert (np.abs(lme[keep] - want_l[keep]) <= 1e-12).all()
    assert (np.abs(ess[keep] - want_e[keep]) <= 1e-12 * want_e[keep]).all()
    with pytest.raises(Exception):
        eng.rows_logmeanexp(torch.zeros(7, dtype=torch.float64, device=DEV), 2)


# ---- 5. errors --------------------------------------------------------------------------------------------------------
def _raw(eng, r, x, betas, R_=None, K=None, short=0, ldv=None, null=None):
    """The export called directly on a sentinel-filled logw -> (EngineError message or None, logw)."""
    from imdbn.engine import native as N, rng as R
    from imdbn import engine as E
    d = eng._desc(r, False)
    K = len(betas) - 1 if K is None else K
    R_ = x.size(0) if R_ is None else R_
    arr = (C.c_float * len(betas))(*[float(b) for b in betas])
    logw = torch.full((max(R_, 1),), -7.25, dtype=torch.float64, device=DEV)
    nr, _ = eng._rng(E.PhiloxRng(1), R.sched_reverse_ais(d.V, d.H, [], max(K, 1)), max(R_, 1), torch.device(DEV))
    ws, nbytes, stream = eng._ws_tail(torch.device(DEV), d.V, d.H, max(R_, 1))
    args = dict(v=C.c_void_p(x.data_ptr()), betas=arr, rng=C.byref(nr), logw=C.c_void_p(logw.data_ptr()))
    if null:
        args[null] = None
    msg = None
    try:
        eng._call("imdbn_rbm_reverse_ais", C.byref(d), args["v"], x.stride(0) if ldv is None else ldv, R_, K, args["betas"], None, args["rng"],
                  args["logw"] if null != "logw" else None, None, d.V, ws, nbytes - short, stream)
    except N.EngineError as e:
        msg = str(e)
    torch.cuda.synchronize()
    return msg, logw


@pytest.mark.parametrize("what,code", [("R0", -1), ("K0", -1), ("flat", -1), ("first", -1), ("last", -1), ("null_v", -1), ("null_betas", -1),
                                       ("null_rng", -1), ("ldv", -1), ("short", -2)])
def test_invalid_arguments_launch_nothing(eng, what, code):
    c = Cs.case(Cs.REVERSE, "tiny")
    r = device_rbm(c)
    x = dev(c["x"])
    betas = {"flat": [0, 0.5, 0.5, 1], "first": [0.1, 0.5, 1], "last": [0, 0.5, 0.9], "K0": [0.0]}.get(what, [0, 0.25, 0.5, 1])
    msg, logw = _raw(eng, r, x, betas, R_=0 if what == "R0" else None, short=1 if what == "short" else 0,
                     ldv=c["V"] - 1 if what == "ldv" else None, null=what[5:] if what.startswith("null_") else None)
    print(what, "->", msg)
    assert msg is not None and f"rc={code})" in msg
    assert (logw == -7.25).all()
    if what in ("flat", "first", "last"):
        assert "0.5" in msg or "0.1" in msg or "0.9" in msg          # the offending value is named
    if what == "ldv":
        assert str(c["V"] - 1) in msg
    # the same workspace still serves a good call
    msg, logw = _raw(eng, r, x, [0, 0.25, 0.5, 1])
    assert msg is None and torch.isfinite(logw).all() and not (logw == -7.25).any()


def test_null_logw_and_python_entry_raise_engine_error(eng):
    from imdbn import engine as E
    c = Cs.case(Cs.REVERSE, "tiny")
    msg, _ = _raw(eng, device_rbm(c), dev(c["x"]), [0, 0.5, 1], null="logw")
    assert msg is not None and "rc=-1)" in msg and "logw" in msg
    with pytest.raises(E.EngineError):
        eng.reverse_ais(device_rbm(c), dev(c["x"]), [0, 0.6, 0.4, 1], E.PhiloxRng(1))
    with pytest.raises(E.EngineError):
        eng.reverse_ais(device_rbm(c), dev(c["x"])[:, :7], [0, 1], E.PhiloxRng(1))


def test_rows_that_are_not_states_are_nan_and_only_they(eng):
    from imdbn import engine as E
    c = Cs.case(Cs.REVERSE, "group")
    r = device_rbm(c)
    x = c["x"].copy()
    x[1, 3] = 0.5
    x[4, 20:25] = 0.0
    x[4, 21] = x[4, 23] = 1.0
    lw = eng.reverse_ais(r, torch.from_numpy(x).to(DEV), c["betas"], E.PhiloxRng(c["seed"]), base_vis_bias=base_bias(c)).cpu().numpy()
    assert np.isnan(lw[[1, 4]]).all() and np.isfinite(np.delete(lw, [1, 4])).all()
    # the good rows are the rows of the clean run: a bad row disturbs nobody
    _, logw, _, _, _ = _twin("group")
    _close(np.delete(lw, [1, 4]), np.delete(logw, [1, 4]), c["H"], "good rows next to NaN rows")
    # a Bernoulli-only RBM: the 0/1 check alone
    c = Cs.case(Cs.REVERSE, "tiny")
    x = c["x"].copy()
    x[2, 19] = 0.5
    lw = eng.reverse_ais(device_rbm(c), torch.from_numpy(x).to(DEV), c["betas"], E.PhiloxRng(1)).cpu().numpy()
    assert np.isnan(lw[2]) and np.isfinite(np.delete(lw, 2)).all()


def test_a_wide_group_with_two_distant_ones_or_none_is_nan(eng):
    """Four groups, one 256 wide: rais_load_v counts a group's ones with lanes striding 64 -- two ones 200 columns apart, and a
    group with none, must both be marked; the other rows are those of the clean run."""
    from imdbn import engine as E
    c, logw, _, _, _ = _twin("four256")
    s, e = c["groups"][1]
    x = c["x"].copy()
    x[1, s:e] = 0.0
    x[1, s + 3] = x[1, s + 203] = 1.0
    x[4, s:e] = 0.0
    lw = eng.reverse_ais(device_rbm(c), torch.from_numpy(x).to(DEV), c["betas"], E.PhiloxRng(c["seed"]), base_vis_bias=base_bias(c)).cpu().numpy()
    assert np.isnan(lw[[1, 4]]).all() and np.isfinite(np.delete(lw, [1, 4])).all()
    _close(np.delete(lw, [1, 4]), np.delete(logw, [1, 4]), c["H"], "good rows next to NaN rows")


# ---- 6. nothing else moved --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mid_bA", "wide_bA"])
def test_parameters_free_energy_and_ais_are_untouched(eng, name):
    from imdbn import engine as E
    c = Cs.case(Cs.REVERSE, name)
    r = device_rbm(c)
    x = dev(c["x"])                                                          # R rows: the workspace of the reverse call
    W0, b0, c0 = r.W.data.clone(), r.vis_bias.data.clone(), r.hid_bias.data.clone()
    F0 = eng.free_energy(r, x)
    A0 = eng.ais(r, c["betas"], c["R"], E.PhiloxRng(3), base_vis_bias=base_bias(c))
    eng.reverse_ais(r, x, c["betas"], E.PhiloxRng(c["seed"]), base_vis_bias=base_bias(c))
    F1 = eng.free_energy(r, x)
    A1 = eng.ais(r, c["betas"], c["R"], E.PhiloxRng(3), base_vis_bias=base_bias(c))
    assert torch.equal(F0, F1) and torch.equal(A0, A1)
    assert torch.equal(r.W.data, W0) and torch.equal(r.vis_bias.data, b0) and torch.equal(r.hid_bias.data, c0)
    assert torch.equal(x.cpu(), torch.from_numpy(c["x"]))              # the caller's rows are only read
