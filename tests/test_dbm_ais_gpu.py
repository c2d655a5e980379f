"""GPU: imdbn_dbm_rowsum_layer, imdbn_dbm_ais, HipEngine.dbm_bound and DBM.log_partition against the float64 reference of
tests/dbm_ais_oracle.py on the cases of tests/dbm_ais_cases.py.

Bounds.  Row sums: ``weigh_bound`` / ``bound_layer_bound`` / ``bias_dot_bound`` of the oracle, derived in its docstring from
``dbm_oracle.pre_bound``.  States: every bit against float64 -- the replay seeds of dbm_ais_cases leave every comparison more room than
the bound of its probability (asserted on the CPU).  A whole run whose states agree accumulates the per-step bounds (``ais(bound=)``)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dbm_ais_cases as Ca
import dbm_ais_oracle as At
import dbm_cases as Ck
from imdbn.engine import native as N
from imdbn.engine import rng as R
from likelihood_gpu import DEV, _native, dev, eng, twin  # noqa: F401  (the fixtures, by name)
from test_dbm_gpu import NAN, _Fixed, _layer_on_device, _poison_intact, _stack_on_device

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
E_INVALID, E_WORKSPACE, E_RNG = -1, -2, -3          # IMDBN_E_* of include/imdbn_engine.h


def _ops(k):
    return k["W_lo"], k["x_lo"], k["W_hi"], k["x_hi"], k["bias"]


def _acc0(B):
    """A start value per row that a call must ADD to."""
    return np.arange(B, dtype=F64) * 0.5 - 3.0


# ---- 1. beta = 1 without a base: dbm_layer's bits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Ca.LAYER_CASES, ids=str)
def test_sampling_at_beta_one_without_a_base_is_dbm_layer_bit_for_bit(eng, case):
    k = Ca.layer_case(case)
    lo, hi, xl, xh, bias, bufs = _layer_on_device(k)
    want_p, want_s = eng.dbm_layer(lo, hi, xl, xh, bias, sample=True, rng=R.ReplayRng(_Fixed(k["u"])), want_p=True)
    acc, s, p = eng.dbm_rowsum_layer(lo, hi, xl, xh, bias, "sample", acc=dev(_acc0(case[3])), beta=1.0, dbeta_next=Ca.DBETA_NEXT,
                                     rng=R.ReplayRng(_Fixed(k["u"])), want_p=True)
    torch.cuda.synchronize()
    assert all(_poison_intact(v, b, o) for v, b, o in bufs), "padding was written"
    assert torch.equal(s, want_s) and torch.equal(p, want_p)
    dot = At.bias_dot(k["bias"], s.cpu().numpy())
    err = np.abs(acc.cpu().numpy() - (_acc0(case[3]) + Ca.DBETA_NEXT * dot))
    assert (err <= Ca.DBETA_NEXT * At.bias_dot_bound(k["bias"], s.cpu().numpy()) + At.EPS_D * np.abs(_acc0(case[3]))).all()


# ---- 2. WEIGH with its draw, SAMPLE at beta with a base: row sums inside the bound, states exact ----------------------------------------
@pytest.mark.parametrize("case", Ca.LAYER_CASES, ids=str)
def test_weigh_sums_stay_inside_the_bound_and_its_states_are_the_oracles(eng, case):
    k = Ca.layer_case(case)
    B = case[3]
    lo, hi, xl, xh, bias, bufs = _layer_on_device(k)
    base = dev(k["base"])
    got = []
    for run in range(2):
        acc, s, p = eng.dbm_rowsum_layer(lo, hi, xl, xh, bias, "weigh", acc=dev(_acc0(B)), beta=Ca.BETA, beta_prev=Ca.BETA_PREV, base=base,
                                         rng=R.ReplayRng(_Fixed(k["u"])), want_p=True)
        torch.cuda.synchronize()
        assert all(_poison_intact(v, b, o) for v, b, o in bufs), "padding was written"
        got.append((acc.cpu().numpy(), s.cpu().numpy(), p.cpu().numpy()))
    assert all(np.array_equal(a, b) for a, b in zip(*got)), "a second call from the same workspace differs"
    acc, s, p = got[0]
    want = At.weigh(*_ops(k), Ca.BETA, Ca.BETA_PREV, k["base"], F64)
    bound = At.weigh_bound(*_ops(k), Ca.BETA, Ca.BETA_PREV, k["base"]) + At.EPS_D * np.abs(_acc0(B))
    share = np.abs(acc - _acc0(B) - want) / bound
    wp = At.sample_p(*_ops(k), Ca.BETA, k["base"], F64)
    pshare = np.abs(p - wp) / At.sample_p_bound(*_ops(k), Ca.BETA, k["base"])
    print(f"{case}: WEIGH uses {share.max():.3g} of its bound (up to {bound.max():.3g}), p {pshare.max():.3g}")
    assert share.max() <= 1.0 and pshare.max() <= 1.0
    assert np.array_equal(s, (wp > k["u"].astype(F64)).astype(F32))
    # weigh-only: the same sums, no draw; SAMPLE at the same beta and base: the same states
    only, none_s, _ = eng.dbm_rowsum_layer(lo, hi, xl, xh, bias, "weigh", acc=dev(_acc0(B)), beta=Ca.BETA, beta_prev=Ca.BETA_PREV, base=base,
                                           sample=False)
    _, s2, p2 = eng.dbm_rowsum_layer(lo, hi, xl, xh, bias, "sample", beta=Ca.BETA, base=base, rng=R.ReplayRng(_Fixed(k["u"])), want_p=True)
    torch.cuda.synchronize()
    assert none_s is None and np.array_equal(only.cpu().numpy(), acc)
    assert np.array_equal(s2.cpu().numpy(), s) and np.array_equal(p2.cpu().numpy(), p)


# ---- 3. BOUND ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Ca.BOUND_CASES, ids=str)
def test_bound_sums_stay_inside_the_bound(eng, case):
    k = Ca.layer_case(case)
    B = case[3]
    lo, _, xl, _, bias, bufs = _layer_on_device(k)
    mu, mb = _padded_mu(k["mu"])
    got = []
    for base_lo in (None, k["base_lo"]):
        acc, s, p = eng.dbm_rowsum_layer(lo, None, xl, None, bias, "bound", acc=dev(_acc0(B)), mu=mu, base=None if base_lo is None else dev(base_lo))
        torch.cuda.synchronize()
        assert s is None and p is None and _poison_intact(mu, mb, 2) and all(_poison_intact(v, b, o) for v, b, o in bufs[:2])
        want = At.bound_layer(k["W_lo"], k["x_lo"], k["bias"], k["mu"], F64, bias_lo=base_lo)
        bound = At.bound_layer_bound(k["W_lo"], k["x_lo"], k["bias"], k["mu"], bias_lo=base_lo) + At.EPS_D * np.abs(_acc0(B))
        got.append(float((np.abs(acc.cpu().numpy() - _acc0(B) - want) / bound).max()))
        assert np.isfinite(acc.cpu().numpy()).all()
    print(f"{case}: BOUND uses {got[0]:.3g} of its bound, {got[1]:.3g} with the bias of the layer below")
    assert max(got) <= 1.0


def _padded_mu(a):
    r, c = a.shape
    buf = torch.full((r, c + 5), NAN, device=DEV)
    view = buf[:, 2:2 + c]
    view.copy_(dev(a))
    return view, buf


# ---- 4. Philox equals a tape of the same draws, at a row offset that is no multiple of 4 ---------------------------------------------------
@pytest.mark.parametrize("mode", ["weigh", "sample"])
@pytest.mark.parametrize("case", [(33, 63, 31, 16), (257, 65, 31, 65), (0, 65, 257, 16)], ids=str)
def test_philox_is_the_tape_of_its_own_draws(eng, case, mode):
    from oracle.draws import PhiloxStream
    k = Ca.layer_case(case)
    lo, hi, xl, xh, bias, _ = _layer_on_device(k, pad=False)
    B, n = case[3], case[1]
    kw = dict(beta=Ca.BETA, beta_prev=Ca.BETA_PREV, dbeta_next=Ca.DBETA_NEXT, base=dev(k["base"]), want_p=True)
    prng = R.PhiloxRng(4321, row0=3)
    a = eng.dbm_rowsum_layer(lo, hi, xl, xh, bias, mode, acc=dev(_acc0(B)), rng=prng, **kw)
    u = PhiloxStream(4321, 0, 3).uniform((B, n))
    b = eng.dbm_rowsum_layer(lo, hi, xl, xh, bias, mode, acc=dev(_acc0(B)), rng=R.ReplayRng(_Fixed(u)), **kw)
    torch.cuda.synchronize()
    assert prng.offset == 1 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert 0.0 < float(a[1].mean()) < 1.0


# ---- 5. the C entry: rows >= B and padded outputs untouched, error codes with nothing written ------------------------------------------------
def _raw(eng, k, lo, hi, xl, xh, bias, rows, mode, r, s, p, acc, base=None, mu=None, beta=Ca.BETA, beta_prev=Ca.BETA_PREV, ws_bytes=None,
         n=None, K_lo=None, K_hi=None):
    ld = lambda t: 0 if t is None else t.stride(0)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    n = k["N"] if n is None else n
    K_lo, K_hi = (k["K_lo"] if K_lo is None else K_lo), (k["K_hi"] if K_hi is None else K_hi)
    need = int(eng._lib.imdbn_dbm_rowsum_layer_ws_bytes(k["K_lo"], k["K_hi"], k["N"], rows))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    return eng._lib.imdbn_dbm_rowsum_layer(ptr(lo and lo.W), ld(lo and lo.W), K_lo, ptr(xl), ld(xl), ptr(hi and hi.W), ld(hi and hi.W), K_hi,
                                           ptr(xh), ld(xh), ptr(bias), n, rows, mode, beta, beta_prev, Ca.DBETA_NEXT, ptr(base), ptr(mu), ld(mu),
                                           None if r is None else C.byref(r), ptr(s), ld(s), ptr(p), ld(p), ptr(acc), ptr(ws),
                                           need if ws_bytes is None else ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_rows_past_B_and_the_padding_of_the_outputs_stay_untouched(eng):
    case = (257, 65, 31, 65)
    k = Ca.layer_case(case)
    lo, hi, xl, xh, bias, _ = _layer_on_device(k, pad=False)
    rows, n = 50, 65
    tape = dev(k["u"][:rows])
    r = N.Rng()
    r.mode, r.tape, r.tape_len = N.RNG_REPLAY, tape.data_ptr(), tape.numel()
    sb, pb = torch.full((65, n + 6), NAN, device=DEV), torch.full((65, n + 9), NAN, device=DEV)
    s, p = sb[:, 2:2 + n], pb[:, 4:4 + n]
    acc = torch.full((65,), NAN, dtype=torch.float64, device=DEV)
    acc[:rows] = 0.0
    assert _raw(eng, k, lo, hi, xl, xh, bias, rows, N.DBM_WEIGH, r, s, p, acc, base=dev(k["base"])) == 0
    torch.cuda.synchronize()
    assert r.draws_used == 1 and r.tape_used == rows * n
    assert _poison_intact(s[:rows], sb[:rows], 2) and _poison_intact(p[:rows], pb[:rows], 4), "padding of s / p was written"
    assert torch.isnan(sb[rows:]).all() and torch.isnan(pb[rows:]).all() and torch.isnan(acc[rows:]).all(), "a row past B was written"
    assert torch.isfinite(acc[:rows]).all() and not torch.isnan(s[:rows]).any()


def test_refusals_name_their_code_and_write_nothing(eng):
    case = (33, 63, 31, 16)
    k = Ca.layer_case(case)
    lo, hi, xl, xh, bias, _ = _layer_on_device(k, pad=False)
    B, n = 16, 63
    s, acc, mu = torch.full((B, n), NAN, device=DEV), torch.full((B,), 7.0, dtype=torch.float64, device=DEV), dev(k["mu"])
    r = N.Rng()
    r.mode, r.seed = N.RNG_PHILOX, 1
    short = N.Rng()
    tape = dev(k["u"])
    short.mode, short.tape, short.tape_len = N.RNG_REPLAY, tape.data_ptr(), B * n - 1
    W, S, Bd = N.DBM_WEIGH, N.DBM_SAMPLE, N.DBM_BOUND
    call = lambda mode, **kw: _raw(eng, k, lo, hi, xl, xh, bias, B, mode, kw.pop("r", r), kw.pop("s", s), None, kw.pop("acc", acc), **kw)
    assert call(3) == E_INVALID and call(-1) == E_INVALID
    assert call(W, n=0) == E_INVALID and call(W, K_lo=0, K_hi=0) == E_INVALID and call(W, K_lo=-1) == E_INVALID
    assert call(W, beta=1.5) == E_INVALID and call(W, beta_prev=Ca.BETA) == E_INVALID and call(W, beta=float("nan")) == E_INVALID
    assert call(W, acc=None) == E_INVALID and call(W, r=None) == E_INVALID
    assert call(S, s=None) == E_INVALID and call(S, beta=-0.1) == E_INVALID
    assert call(Bd, s=None, mu=mu) == E_INVALID, "a hi side in BOUND"
    assert call(Bd, s=None, K_hi=0) == E_INVALID, "BOUND without mu"
    assert call(Bd, K_hi=0, mu=mu) == E_INVALID, "BOUND with s"
    assert call(W, ws_bytes=255) == E_WORKSPACE and call(S, r=short) == E_RNG
    assert eng._lib.imdbn_dbm_rowsum_layer_ws_bytes(0, 0, n, B) == 0 and eng._lib.imdbn_dbm_rowsum_layer_ws_bytes(33, 31, 0, B) == 0
    torch.cuda.synchronize()
    assert torch.isnan(s).all() and bool((acc == 7.0).all()), "a refused call wrote"
    assert call(W) == 0 and call(S) == 0 and call(Bd, s=None, K_hi=0, mu=mu) == 0
    with pytest.raises(N.EngineError):
        eng.dbm_rowsum_layer(lo, hi, xl, xh, bias, "anneal")
    with pytest.raises(N.EngineError):
        eng.dbm_rowsum_layer(lo, hi, xl, xh, bias, "bound", mu=mu)
    torch.cuda.synchronize()


# ---- 6. the whole run ---------------------------------------------------------------------------------------------------------------------------
def _reference_run(sizes, M):
    Ws, bs, base = Ca.ais_case(sizes, M)
    bound = []
    logw, s = At.ais(Ws, bs, Ca.AIS_BETAS, M, Ck.Tape(Ca.AIS_SEEDS[(sizes, M)]), base, F64, bound=bound)
    return logw, s, bound[0]


@pytest.mark.parametrize("sizes,M", Ca.STACKS, ids=str)
def test_a_whole_run_ends_in_the_oracles_states_with_logw_inside_the_bound(eng, sizes, M):
    Ws, bs, base = Ca.ais_case(sizes, M)
    layers, biases = _stack_on_device(dict(Ws=Ws, bs=bs))
    got = []
    for run in range(2):
        tape = Ck.Tape(Ca.AIS_SEEDS[(sizes, M)])
        logw, states = eng.dbm_ais(layers, biases, torch.from_numpy(Ca.AIS_BETAS), M, R.ReplayRng(tape), base_bias=dev(base), return_state=True)
        torch.cuda.synchronize()
        got.append([logw.cpu().numpy()] + [s.cpu().numpy() for s in states])
    assert tape.shapes == [(M, n) for _, n in R.sched_dbm_ais(sizes, Ca.AIS_K)]
    assert all(np.array_equal(a, b) for a, b in zip(*got)), "a second run from the same workspace differs"
    want, s, bound = twin(("dbm_ais", sizes, M), lambda: _reference_run(sizes, M))
    assert all(np.array_equal(a, b.astype(F32)) for a, b in zip(got[0][1:], s[1::2])), "a final state differs from float64"
    share = np.abs(got[0][0] - want) / bound
    print(f"{sizes} M {M}: logw uses {share.max():.3g} of its bound (up to {bound.max():.3g}); logw in [{want.min():.3f}, {want.max():.3f}]")
    assert share.max() <= 1.0


def test_a_run_is_refused_before_its_first_launch(eng):
    sizes, M = (65, 33, 31), 5
    Ws, bs, base = Ca.ais_case(sizes, M)
    layers, biases = _stack_on_device(dict(Ws=Ws, bs=bs))
    for betas in ([0.1, 0.5, 1.0], [0.0, 0.5, 0.9], [0.0, 0.6, 0.5, 1.0], [0.0]):
        with pytest.raises(N.EngineError):
            eng.dbm_ais(layers, biases, betas, M, R.PhiloxRng(1))
    with pytest.raises(N.EngineError):
        eng.dbm_ais(layers, biases, [0.0, 1.0], 0, R.PhiloxRng(1))
    with pytest.raises(N.EngineError):
        eng.dbm_ais(layers, biases[:-1], [0.0, 1.0], M, R.PhiloxRng(1))
    csz = (C.c_int * 3)(*sizes)
    assert eng._lib.imdbn_dbm_ais_ws_bytes(2, csz, 0) == 0 and eng._lib.imdbn_dbm_ais_ws_bytes(0, csz, 5) == 0
    torch.cuda.synchronize()


def test_dbm_bound_is_the_float64_figure_inside_the_bound(eng):
    sizes, B = (67, 64, 33, 5), 65
    k = Ck.stack_case(sizes, B)
    layers, biases = _stack_on_device(k)
    mu, _ = eng.dbm_infer(layers, biases, dev(k["data"]), 3)
    got = eng.dbm_bound(layers, biases, dev(k["data"]), mu)
    torch.cuda.synchronize()
    mus = [m.cpu().numpy() for m in mu]
    want = At.bound_rows(k["Ws"], k["bs"], k["data"], mus, F64)
    share = np.abs(got.cpu().numpy() - want) / At.bound_rows_bound(k["Ws"], k["bs"], k["data"], mus)
    print(f"{sizes} B {B}: dbm_bound uses {share.max():.3g} of its bound")
    assert got.dtype == torch.float64 and share.max() <= 1.0


# ---- 7. the model through the real engine -----------------------------------------------------------------------------------------------------
def test_log_partition_with_philox_is_finite_and_repeats_per_seed(eng):
    from imdbn import engine as E
    from imdbn.models import DBM
    import dbm_oracle as Dt
    sizes = (8, 6, 4)
    Ws, bs, base = Ca.small_model(sizes, 0.5)
    params = {"LEARNING_RATE": 0.1, "WEIGHT_PENALTY": 0.0, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.9, "LEARNING_RATE_DYNAMIC": False, "CD": 1}
    net = DBM(list(sizes), params, device=DEV)
    for l, r in enumerate(net.layers):
        r.W.data.copy_(dev(Ws[l]))
        r.hid_bias.data.copy_(dev(bs[l + 1]))
    net.layers[0].vis_bias.data.copy_(dev(bs[0]))
    E.manual_seed(5)
    before = E.get_rng().offset
    a = net.log_partition(n_chains=64, n_betas=200, base_bias=dev(base), seed=9)
    b = net.log_partition(n_chains=64, n_betas=200, base_bias=dev(base), seed=9)
    c = net.log_partition(n_chains=64, n_betas=200, base_bias=dev(base), seed=10)
    assert E.get_rng().offset == before
    want = Dt.log_z(Ws, bs)
    print(f"log Z {a['log_z']:.4f} (se {a['se']:.4f}, ess {a['ess']:.1f}) / {c['log_z']:.4f}; exact {want:.4f}")
    assert np.isfinite(a["log_z"]) and a["log_z"] == b["log_z"] and torch.equal(a["logw"], b["logw"]) and a["log_z"] != c["log_z"]
    assert abs(a["log_z"] - want) < 0.5
    v = dev((np.random.default_rng(3).random((5, 8)) < 0.4).astype(F32))
    bound = net.log_likelihood_bound(v, want)
    assert (bound.cpu().numpy() <= Dt.log_p(Ws, bs, v.cpu().numpy(), want) + 1e-5).all()
    E.set_rng(None)
