"""GPU: imdbn_dbm_layer, HipEngine.dbm_gibbs / dbm_infer / dbm_step and imdbn.models.dbm against the float64 reference and the fp32
twin of tests/dbm_oracle.py on the cases of tests/dbm_cases.py.

Bounds.  Mean field: ``pre_bound / 4`` plus the sigmoid and damping arithmetic, as derived in dbm_oracle's docstring, elementwise;
carried through the start and the sweeps by ``infer_bounded``.  Samples: every bit against the float64 oracle -- the replay seeds of
dbm_cases leave every comparison more room than that bound (asserted on the CPU).  dbm_step: relative Frobenius error against the
float64 oracle; the fp32 twin's own error is measured on the same cases and the device gets STEP_FACTOR times the twin's figure per
quantity (its summation order differs from numpy's; measured on an MI355X: at most 1.41 times), capped by the 1e-4
parity bound of DESIGN section 5."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dbm_cases as Ck
import dbm_oracle as Dt
import oracle.rbm_oracle as O
from imdbn.engine import native as N
from imdbn.engine import rng as R
from likelihood_gpu import DEV, _native, dev, eng, twin  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NAN = float("nan")
STEP_FACTOR = 4.0
E_INVALID, E_WORKSPACE = -1, -2          # IMDBN_E_* of include/imdbn_engine.h


def _padded(a, pad_cols, off=0):
    """`a` as a view of a NaN-filled buffer: rows `pad_cols` floats longer, the data `off` columns in.  (view, buffer)"""
    r, c = a.shape
    buf = torch.full((r, c + pad_cols), NAN, device=DEV)
    view = buf[:, off:off + c]
    view.copy_(dev(a))
    return view, buf


def _poison_intact(view, buf, off=0):
    c = view.size(1)
    return bool(torch.isnan(buf[:, :off]).all() and torch.isnan(buf[:, off + c:]).all())


def _layer_on_device(k, pad=True):
    """(lo, hi, x_lo, x_hi, bias, buffers to check): weights with pitches above N / K_hi, strided x rows, all padding NaN."""
    bufs = []
    lo = hi = xl = xh = None
    if k["W_lo"] is not None:
        W, b = _padded(k["W_lo"], 5 if pad else 0)
        x, bx = _padded(k["x_lo"], 3 if pad else 0, 1 if pad else 0)
        lo, xl = SimpleNamespace(W=W), x
        bufs += [(W, b, 0), (x, bx, 1 if pad else 0)]
    if k["W_hi"] is not None:
        W, b = _padded(k["W_hi"], 7 if pad else 0)
        x, bx = _padded(k["x_hi"], 6 if pad else 0, 2 if pad else 0)
        hi, xh = SimpleNamespace(W=W), x
        bufs += [(W, b, 0), (x, bx, 2 if pad else 0)]
    return lo, hi, xl, xh, dev(k["bias"]), bufs


# ---- 5 / 7. mean-field mode against float64, poison, a second call from the same workspace ------------------------------------------
@pytest.mark.parametrize("s_lo,damp", Ck.VARIANTS)
@pytest.mark.parametrize("case", Ck.LAYER_CASES, ids=str)
def test_mean_field_stays_inside_the_derived_bound(eng, case, s_lo, damp):
    k = Ck.layer_case(*case)
    lo, hi, xl, xh, bias, bufs = _layer_on_device(k)
    got = []
    for run in range(2):
        m, mb = _padded(k["m"], 4, 3)
        res = eng.dbm_layer(lo, hi, xl, xh, bias, m=m, damp=damp, s_lo=s_lo, want_res=True)
        torch.cuda.synchronize()
        assert _poison_intact(m, mb, 3) and all(_poison_intact(v, b, o) for v, b, o in bufs), "padding was written"
        got.append((m.cpu().numpy(), res.cpu().numpy()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), "a second call from the same workspace differs"
    want, p, rres = Dt.mean_field(k["W_lo"], k["x_lo"], s_lo, k["W_hi"], k["x_hi"], 1.0, k["bias"], k["m"], damp, F64)
    dp = Dt.pre_bound(k["W_lo"], k["x_lo"], s_lo, k["W_hi"], k["x_hi"], 1.0, k["bias"]) / 4
    fm = np.abs(got[0][0] - want) / ((1 - damp) * dp + Dt.EPS_M)
    fr = np.abs(got[0][1] - rres) / (dp + Dt.EPS_P + Dt.U).max(1)
    print(f"{case} s_lo {s_lo} damp {damp}: largest share of the bound: m {fm.max():.3g}, res {fr.max():.3g} (bound up to {dp.max():.3g})")
    assert fm.max() <= 1.0 and fr.max() <= 1.0


# ---- 6 / 7. sample mode ------------------------------------------------------------------------------------------------------------------
class _Fixed:
    """A replay provider that hands out one given tensor."""

    def __init__(self, u):
        self.u = u

    def uniform(self, shape):
        assert tuple(shape) == self.u.shape
        return self.u


@pytest.mark.parametrize("case", Ck.LAYER_CASES, ids=str)
def test_replayed_samples_are_the_oracles_bit_for_bit(eng, case):
    k = Ck.layer_case(*case, binary=True, seed=Ck.SAMPLE_SEEDS[case])
    lo, hi, xl, xh, bias, bufs = _layer_on_device(k)
    got = []
    for run in range(2):
        p, s = eng.dbm_layer(lo, hi, xl, xh, bias, sample=True, rng=R.ReplayRng(_Fixed(k["u"])), want_p=True)
        torch.cuda.synchronize()
        assert all(_poison_intact(v, b, o) for v, b, o in bufs), "padding was written"
        got.append((p.cpu().numpy(), s.cpu().numpy()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    want_p = Dt.sigmoid(Dt.pre(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"], F64))
    want_s = (want_p > k["u"].astype(F64)).astype(F32)
    b = Dt.pre_bound(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"]) / 4 + Dt.EPS_P
    print(f"{case}: p uses {(np.abs(got[0][0] - want_p) / b).max():.3g} of its bound; {int((got[0][1] != want_s).sum())} bits differ")
    assert (np.abs(got[0][0] - want_p) <= b).all() and np.array_equal(got[0][1], want_s)


def _raw_sample(eng, k, lo, hi, xl, xh, bias, rows, r, s_out, p_out=None):
    """The C entry on the first `rows` rows of the operands, with the native rng struct `r`."""
    ld = lambda t: 0 if t is None else t.stride(0)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    n = k["N"]
    need = int(eng._lib.imdbn_dbm_layer_ws_bytes(k["K_lo"], k["K_hi"], n, rows))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    return eng._lib.imdbn_dbm_layer(ptr(lo and lo.W), ld(lo and lo.W), k["K_lo"], ptr(xl), ld(xl), 1.0, ptr(hi and hi.W), ld(hi and hi.W), k["K_hi"],
                                    ptr(xh), ld(xh), 1.0, ptr(bias), n, rows, 0, None, 0, 0.0, None, C.byref(r), ptr(s_out), s_out.stride(0),
                                    ptr(p_out), ld(p_out), ptr(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("row0", [0, 3])
@pytest.mark.parametrize("case", [(67, 33, 21, 5), (128, 64, 64, 64), (70, 65, 40, 5), (250, 33, 20, 5)], ids=str)
def test_philox_is_keyed_on_the_global_row(eng, case, row0):
    K_lo, n, K_hi, B = case
    k = Ck.layer_case(K_lo, n, K_hi, B + 3, binary=True)
    lo, hi, xl, xh, bias, _ = _layer_on_device(k, pad=False)
    prng = R.PhiloxRng(1234, row0=row0)
    a = eng.dbm_layer(lo, hi, xl, xh, bias, sample=True, rng=prng)
    assert prng.offset == 1
    prng2 = R.PhiloxRng(1234, row0=row0)
    b = eng.dbm_layer(lo, hi, xl, xh, bias, sample=True, rng=prng2)
    assert torch.equal(a, b), "two identical calls differ"
    # rows [3, 3 + B) of the call equal the call on those rows shifted by three
    prng3 = R.PhiloxRng(1234, row0=row0 + 3)
    c = eng.dbm_layer(lo, hi, None if xl is None else xl[3:], None if xh is None else xh[3:], bias, sample=True, rng=prng3)
    torch.cuda.synchronize()
    assert torch.equal(a[3:], c)
    # ... and the draws are the oracle's Philox stream
    from oracle.draws import PhiloxStream
    u = PhiloxStream(1234, 0, row0).uniform((B + 3, n))
    p = Dt.sigmoid(Dt.pre(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"], F64))
    bd = Dt.pre_bound(k["W_lo"], k["x_lo"], 1.0, k["W_hi"], k["x_hi"], 1.0, k["bias"]) / 4 + Dt.EPS_P
    clear = np.abs(p - u.astype(F64)) > bd
    assert np.array_equal(a.cpu().numpy()[clear], (p > u).astype(F32)[clear]) and clear.mean() > 0.99
    # draws_used / tape_used through the C entry
    r = N.Rng()
    r.mode, r.seed, r.offset, r.row0 = N.RNG_PHILOX, 1234, 0, row0
    s_out = torch.empty(B + 3, n, device=DEV)
    assert _raw_sample(eng, k, lo, hi, xl, xh, bias, B + 3, r, s_out) == 0
    torch.cuda.synchronize()
    assert r.draws_used == 1 and r.tape_used == 0 and torch.equal(s_out, a)


def test_padded_sample_outputs_are_honoured(eng):
    """lds > N and ldp > N through the C entry: s and p land in column-offset views of NaN-filled buffers, the rest stays NaN."""
    case = (250, 33, 20, 5)
    k = Ck.layer_case(*case, binary=True, seed=Ck.SAMPLE_SEEDS[case])
    lo, hi, xl, xh, bias, _ = _layer_on_device(k, pad=False)
    tape = dev(k["u"])
    r = N.Rng()
    r.mode, r.tape, r.tape_len = N.RNG_REPLAY, tape.data_ptr(), tape.numel()
    sb, pb = torch.full((5, 33 + 6), NAN, device=DEV), torch.full((5, 33 + 9), NAN, device=DEV)
    s_out, p_out = sb[:, 2:35], pb[:, 4:37]
    assert _raw_sample(eng, k, lo, hi, xl, xh, bias, 5, r, s_out, p_out) == 0
    torch.cuda.synchronize()
    assert r.draws_used == 1 and r.tape_used == 5 * 33
    assert _poison_intact(s_out, sb, 2) and _poison_intact(p_out, pb, 4), "padding of s / p was written"
    p, s = eng.dbm_layer(lo, hi, xl, xh, bias, sample=True, rng=R.ReplayRng(_Fixed(k["u"])), want_p=True)
    assert torch.equal(s_out, s) and torch.equal(p_out, p)


# ---- 7. error codes ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_code(eng):
    k = Ck.layer_case(67, 33, 21, 5)
    lo, hi, xl, xh, bias, _ = _layer_on_device(k, pad=False)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    m, s = dev(k["m"]), torch.empty(5, 33, device=DEV)
    need = int(eng._lib.imdbn_dbm_layer_ws_bytes(67, 21, 33, 5))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    r = N.Rng()
    r.mode, r.seed = N.RNG_PHILOX, 1
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(K_lo=67, K_hi=21, x_lo=xl, x_hi=xh, n=33, mm=m, ss=None, ws_bytes=need, damp=0.0):
        return eng._lib.imdbn_dbm_layer(ptr(lo.W), lo.W.stride(0), K_lo, ptr(x_lo), 67, 1.0, ptr(hi.W), hi.W.stride(0), K_hi, ptr(x_hi), 21, 1.0,
                                        ptr(bias), n, 5, 0, ptr(mm), 33, damp, None, C.byref(r), ptr(ss), 33, None, 0, ptr(ws), ws_bytes, st)

    before = m.clone()
    assert call(K_lo=0, K_hi=0) == E_INVALID and call(x_lo=None, x_hi=None) == E_INVALID
    assert call(mm=m, ss=s) == E_INVALID and call(mm=None, ss=None) == E_INVALID
    assert call(n=0) == E_INVALID and call(n=-3) == E_INVALID and call(damp=1.0) == E_INVALID
    assert call(ws_bytes=need - 1) == E_WORKSPACE
    assert eng._lib.imdbn_dbm_layer_ws_bytes(0, 0, 33, 5) == 0 and eng._lib.imdbn_dbm_layer_ws_bytes(67, 21, 0, 5) == 0
    torch.cuda.synchronize()
    assert torch.equal(m, before), "a refused call touched m"
    assert call() == 0
    with pytest.raises(N.EngineError):
        eng.dbm_layer(None, None, None, None, bias, m=m)
    with pytest.raises(N.EngineError):
        eng.dbm_layer(lo, hi, xl, xh, bias)
    torch.cuda.synchronize()


# ---- 8. dbm_gibbs and dbm_infer ------------------------------------------------------------------------------------------------------------
def _stack_on_device(k, momenta=False):
    from imdbn.models import RBM
    layers = []
    g = np.random.default_rng(77)
    for l, W in enumerate(k["Ws"]):
        V, H = W.shape
        r = RBM(V, H, Ck.LR, Ck.WEIGHT_DECAY, Ck.MOM).to(DEV)          # the constructor's padded pitch
        r.W.data.copy_(dev(W))
        r.hid_bias.data.copy_(dev(k["bs"][l + 1]))
        r.vis_bias.data.copy_(dev(k["bs"][l] if l == 0 else np.zeros_like(k["bs"][l])))
        r.W_m.zero_()
        r.hb_m, r.vb_m = torch.zeros_like(r.hid_bias.data), torch.zeros_like(r.vis_bias.data)
        layers.append(r)
    biases = [layers[0].vis_bias.data] + [r.hid_bias.data for r in layers]
    return layers, biases


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("sizes,B", Ck.STACKS, ids=str)
def test_gibbs_states_are_the_oracles(eng, sizes, B, clamp):
    k = Ck.stack_case(sizes, B)
    layers, biases = _stack_on_device(k)
    parts = [dev(p) for p in k["particles"]]
    tape = Ck.Tape(Ck.GIBBS_SEEDS[(sizes, B)])
    eng.dbm_gibbs(layers, biases, parts, Ck.GIBBS_SWEEPS, R.ReplayRng(tape), clamp_bottom=dev(k["data"]) if clamp else None)
    torch.cuda.synchronize()
    want = Dt.gibbs(k["Ws"], k["bs"], k["particles"], Ck.GIBBS_SWEEPS, Ck.Tape(Ck.GIBBS_SEEDS[(sizes, B)]), F64,
                    clamp_bottom=k["data"] if clamp else None)
    assert tape.shapes == [(B, n) for _, n in R.sched_dbm_gibbs(sizes, Ck.GIBBS_SWEEPS, clamp_bottom=clamp)]
    assert all(np.array_equal(p.cpu().numpy(), w.astype(F32)) for p, w in zip(parts, want))
    if clamp:
        assert np.array_equal(parts[0].cpu().numpy(), k["data"])


@pytest.mark.parametrize("damp", [0.0, 0.5])
@pytest.mark.parametrize("sizes,B", Ck.STACKS, ids=str)
def test_inference_stays_inside_the_accumulated_bound(eng, sizes, B, damp):
    k = Ck.stack_case(sizes, B)
    layers, biases = _stack_on_device(k)
    mu, res = eng.dbm_infer(layers, biases, dev(k["data"]), 3, damp=damp)
    torch.cuda.synchronize()
    want, wres, dmu, rb = twin(("infer", sizes, B, damp), lambda: Dt.infer_bounded(k["Ws"], k["bs"], k["data"], 3, damp))
    f = max(float((np.abs(m.cpu().numpy() - w) / d).max()) for m, w, d in zip(mu, want, dmu))
    fr = float((np.abs(res.cpu().numpy() - wres) / rb).max())
    print(f"{sizes} B {B} damp {damp}: largest share of the bound: mu {f:.3g}, res {fr:.3g}")
    assert f <= 1.0 and fr <= 1.0


# ---- 9. dbm_step -----------------------------------------------------------------------------------------------------------------------------
def _states(k, dt):
    sts = [O.RBMState.create(W, Ck.LR, Ck.WEIGHT_DECAY, Ck.MOM, hid_bias=k["bs"][l + 1],
                             vis_bias=k["bs"][l] if l == 0 else np.zeros_like(k["bs"][l])) for l, W in enumerate(k["Ws"])]
    return Dt.states_as(sts, dt)


def _model_quantities(sts):
    """name -> array of everything the model owns: W, W_m per RBM, the L + 1 layer biases and their momenta."""
    out = {}
    for l, s in enumerate(sts):
        out[f"W{l}"], out[f"W_m{l}"], out[f"b{l + 1}"], out[f"b_m{l + 1}"] = s.W, s.W_m, s.hid_bias, s.hb_m
    out["b0"], out["b_m0"] = sts[0].vis_bias, sts[0].vb_m
    return out


@pytest.mark.parametrize("sizes,B", Ck.STACKS, ids=str)
def test_two_steps_follow_the_twin(eng, sizes, B):
    k = Ck.stack_case(sizes, B)
    layers, _ = _stack_on_device(k)
    scal = Ck.STEP_SCALARS[:len(layers)]
    parts = [dev(p) for p in k["particles"]]
    ref, tw = _states(k, F64), _states(k, F32)
    rparts = tparts = k["particles"]
    for i, seed in enumerate(Ck.STEP_SEEDS[(sizes, B)]):
        out = eng.dbm_step(layers, dev(k["data"]), parts, scal, Ck.STEP_N_MF, Ck.STEP_DAMP, Ck.STEP_GIBBS_K, R.ReplayRng(Ck.Tape(seed)))
        torch.cuda.synchronize()
        r = Dt.step(ref, k["data"], rparts, scal, Ck.STEP_N_MF, Ck.STEP_DAMP, Ck.STEP_GIBBS_K, Ck.Tape(seed))
        t = Dt.step(tw, k["data"], tparts, scal, Ck.STEP_N_MF, Ck.STEP_DAMP, Ck.STEP_GIBBS_K, Ck.Tape(seed))
        rparts, tparts = r["particles"], t["particles"]
        assert all(np.array_equal(p.cpu().numpy(), w.astype(F32)) for p, w in zip(parts, rparts)), "a particle bit differs from float64"
        have = {}
        for l, rb in enumerate(layers):
            have[f"W{l}"], have[f"W_m{l}"] = rb.W.data.cpu().numpy(), rb.W_m.cpu().numpy()
            have[f"b{l + 1}"], have[f"b_m{l + 1}"] = rb.hid_bias.data.cpu().numpy(), rb.hb_m.cpu().numpy()
        have["b0"], have["b_m0"] = layers[0].vis_bias.data.cpu().numpy(), layers[0].vb_m.cpu().numpy()
        rq, tq = _model_quantities(ref), _model_quantities(tw)
        worst = 0.0
        for name in rq:
            e_dev, e_twin = Dt.rel_frobenius(have[name], rq[name]), Dt.rel_frobenius(tq[name], rq[name])
            tol = min(1e-4, STEP_FACTOR * max(e_twin, 2.0 ** -24))
            worst = max(worst, e_dev / max(e_twin, 2.0 ** -24))
            assert e_dev <= tol, f"step {i} {name}: device {e_dev:.3g}, twin {e_twin:.3g}"
        loss = float(out["recon_loss"])
        print(f"{sizes} B {B} step {i}: worst device / twin error ratio {worst:.3g}; recon_loss {loss:.7f} vs {float(r['recon_loss']):.7f}")
        assert abs(loss - float(r["recon_loss"])) <= 1e-5 * max(1.0, abs(float(r["recon_loss"])))


# ---- 10. the model through the real engine ---------------------------------------------------------------------------------------------
def _trained_idbn():
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn import engine as E
    from imdbn.models import iDBN
    g = np.random.default_rng(21)
    protos = (g.random((6, 100)) < 0.3).astype(F32)
    X = protos[g.integers(0, 6, 64)]
    X = np.where(g.random(X.shape) < 0.03, 1 - X, X).astype(F32)
    Xt = torch.from_numpy(X)
    dl = DataLoader(TensorDataset(Xt, torch.zeros(64)), batch_size=32)
    params = {"LEARNING_RATE": 0.05, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.5, "LEARNING_RATE_DYNAMIC": False, "CD": 1}
    torch.manual_seed(3)
    net = iDBN([100, 40, 20], params, dl, dl, torch.device(DEV))
    E.manual_seed(99)
    x = Xt.to(DEV)
    for rbm in net.layers:
        for ep in range(5):
            for s in (0, 32):
                rbm.train_epoch(x[s:s + 32], ep, 5, CD=1)
        x = rbm.forward(x)
    return net, Xt


def test_finetune_runs_repeats_its_bits_and_does_not_raise_the_reconstruction_error(eng):
    from imdbn import engine as E
    net, X = _trained_idbn()
    runs = []
    for _ in range(2):
        dbm = net.to_dbm()
        before = float(((dbm.reconstruct(X) - X.to(DEV)) ** 2).mean())
        E.manual_seed(7)
        first = dbm.train_step(X[:32], 0, 4, lr_scale=0.2)
        dbm.finetune(4, n_mf=10, gibbs_k=5, lr_scale=0.2, log_every=2)
        after = float(((dbm.reconstruct(X) - X.to(DEV)) ** 2).mean())
        torch.cuda.synchronize()
        runs.append((before, after, float(first["recon_loss"]), [r.W.data.clone() for r in dbm.layers], [p.clone() for p in dbm.particles]))
    print(f"reconstruction error {runs[0][0]:.5f} -> {runs[0][1]:.5f}; history {dbm.history}")
    assert runs[0][:3] == runs[1][:3] and all(torch.equal(a, b) for a, b in zip(runs[0][3] + runs[0][4], runs[1][3] + runs[1][4]))
    assert [h[0] for h in dbm.history] == [0, 2] and np.isfinite(runs[0][1])
    assert runs[0][1] <= runs[0][0]
    E.set_rng(None)
