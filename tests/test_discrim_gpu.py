"""GPU: imdbn_rbm_label_backprop_step, HipEngine.discriminative_step and iMDBN.finetune_discriminative against the float64 numpy twin
(tests/discrim_oracle.py) fed the same fp32 state.

Tolerances (tests/discrim_cases.py), derived, not measured: logp within labelgrad_cases.tol_logp; err_z element by element within
  0.25 tol_delta(H) sum_j |W_ij|  +  (H + 16) 2^-23 z (1 - z) sum_j |e_j| |W_ij|
-- every entry of e within tol_delta(H) (the label side's convention) entering column i through |W_ij| with z (1 - z) <= 1/4, plus the
product bound of test_backprop_gpu; pred on every row whose float64 top-two gap exceeds 2 eps(H).  The first test prints the largest
error / bound per case; DESIGN section 27 holds the maxima."""
import ctypes as C

import numpy as np
import pytest
import torch

import discrim_cases as Cs
import discrim_oracle as D
import labelgrad_cases as L
from likelihood_gpu import DEV, _native, close, dev, eng, twin  # noqa: F401  (the fixtures, by name)
from test_labelgrad_gpu import KEYS, _rbm, _same, _state
from test_updown_gpu import _check6, _same6, _six

pytestmark = pytest.mark.gpu

F32 = np.float32


def _twin(name, scale):
    """(case, discrim_oracle.head of it), computed once."""
    def run():
        c = L.case(name, scale)
        return c, D.head(c["W"], c["b"], c["c"], c["z"], c["K"], c["gt"])
    return twin(("discrim", name, scale), run)


def _call(eng, c, r, z=None, gt=None, apply=False, lr=L.LR, mom=L.MOM, want_pred=True):
    out = eng.label_backprop_step(r, dev(c["z"]) if z is None else z, c["K"], dev(c["gt"] if gt is None else gt), lr, mom, apply=apply,
                                  want_pred=want_pred)
    torch.cuda.synchronize()
    return out


# ---- 1. against the twin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", Cs.ALL)
def test_logp_and_err_z_match_the_twin(eng, name, scale):
    c, want = _twin(name, scale)
    r = _rbm(c)
    logp, err, pred = _call(eng, c, r)
    assert logp.dtype == torch.float64 and tuple(logp.shape) == (c["N"],) and tuple(err.shape) == (c["N"], c["Dz"]) and err.dtype == torch.float32
    close(logp.cpu().numpy(), want["logp"], L.tol_logp(c["H"], want["logp"]), f"{name} scale {scale}: logp")
    tol = Cs.tol_err_z(c["H"], want)
    e = np.abs(err.cpu().numpy().astype(np.float64) - want["err_z"])
    print(f"{name} scale {scale}: err_z max |device - twin| / bound {float((e / tol).max()):.3g} (largest error {e.max():.3g}, "
          f"largest |err_z| {np.abs(want['err_z']).max():.3g})")
    assert (e <= tol).all(), f"{name} scale {scale}: err_z {float((e / tol).max()):.3g} times the bound"


# ---- 2. pred ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", Cs.ALL)
def test_pred_is_the_twins_argmax_on_every_decided_row_whatever_gt_holds(eng, name, scale):
    c, want = _twin(name, scale)
    use = Cs.pred_rows(c["H"], want)
    assert (~use).sum() <= Cs.PRED_LEFT_OUT * c["N"]
    r = _rbm(c)
    pred = _call(eng, c, r)[2]
    assert pred.dtype == torch.int32 and tuple(pred.shape) == (c["N"],)
    assert np.array_equal(pred.cpu().numpy()[use], want["pred"][use])
    other = np.full(c["N"], -1, np.int32)                               # every label invalid: pred is still written, the same
    logp, err, pred2 = _call(eng, c, r, gt=other)
    assert torch.equal(pred, pred2) and torch.isnan(logp).all() and not err.any()
    assert _call(eng, c, r, want_pred=False)[2] is None


# ---- 3. apply=True ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", Cs.ALL)
def test_with_apply_the_six_tensors_have_the_bits_of_label_step_and_logp_those_of_label_loglik(eng, name, scale):
    c = L.case(name, scale)
    ra, rb = _rbm(c), _rbm(c)
    j, m = eng.label_loglik(ra, dev(c["z"]), c["K"], dev(c["gt"]))       # the parameters before the step
    logp = _call(eng, c, ra, apply=True)[0]
    lp = eng.label_step(rb, dev(c["z"]), c["K"], dev(c["gt"]), L.LR, L.MOM)
    torch.cuda.synchronize()
    assert torch.equal(logp, j - m) and torch.equal(logp, lp)
    assert _same(_state(ra), _state(rb)) and not _same(_state(ra), L.state(c))


# ---- 4. apply=False ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", Cs.ALL)
def test_without_apply_nothing_moves_and_err_z_has_the_bits_of_the_applying_call(eng, name, scale):
    c = L.case(name, scale)
    ra, rb = _rbm(c), _rbm(c)
    before = _state(ra)
    la, ea, pa = _call(eng, c, ra, apply=False)
    assert _same(before, _state(ra))
    lb, eb, pb = _call(eng, c, rb, apply=True)
    assert torch.equal(la, lb) and torch.equal(ea, eb) and torch.equal(pa, pb)
    assert (ea.abs().max() > 0) == (name not in L.BINARY_Z)             # a 0/1 code has z (1 - z) = 0: exact zeros
    assert not _same(before, _state(rb))


# ---- 5. other properties ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "k65", "rows67", "wide"])
def test_the_same_call_on_the_same_state_gives_the_same_bits(eng, name):
    c = L.case(name, 1.0)
    out = []
    for _ in range(2):
        r = _rbm(c)
        out.append(_call(eng, c, r, apply=True) + (_state(r),))
    assert all(torch.equal(a, b) for a, b in zip(out[0][:3], out[1][:3])) and _same(out[0][3], out[1][3])


def test_rows_with_a_label_outside_the_range_are_nan_with_a_zero_error_row_and_leave_the_other_rows_bits(eng):
    c, _ = _twin("rows67", 0.1)
    rows = [3, 40, 66]
    bad = c["gt"].copy()
    bad[rows] = [-1, c["K"], 2 ** 30]
    want = D.head(c["W"], c["b"], c["c"], c["z"], c["K"], bad)
    r = _rbm(c)
    la, ea, pa = _call(eng, c, r)
    lb, eb, pb = _call(eng, c, r, gt=bad)
    keep = torch.from_numpy(np.isfinite(want["logp"]))
    assert torch.isnan(lb[rows]).all() and not eb[rows].any() and eb[keep].abs().max() > 0
    assert torch.equal(la[keep], lb[keep]) and torch.equal(ea[keep], eb[keep]) and torch.equal(pa, pb)
    e = np.abs(eb.cpu().numpy().astype(np.float64) - want["err_z"])
    assert (e <= Cs.tol_err_z(c["H"], want)).all()
    # with apply: the step of label_step on the same labels, bit for bit
    ra, rb = _rbm(c), _rbm(c)
    _call(eng, c, ra, gt=bad, apply=True)
    eng.label_step(rb, dev(c["z"]), c["K"], dev(bad), L.LR, L.MOM)
    assert _same(_state(ra), _state(rb))


def _raw(eng, r, z, gt, K, N=None, ldz=None, Dz=None, lde=None, err=None, null=(), momentum=True, opts=True, cd_k=0, sparsity=0):
    """The export called directly on sentinel-filled outputs -> (EngineError message or None, logp, pred, err)."""
    from imdbn.engine import native as Nt
    d = eng._desc(r, True)
    if not momentum:
        d = Nt.RbmDesc.from_buffer_copy(d)
        d.W_m = None
    N = z.size(0) if N is None else N
    Dz = z.size(1) if Dz is None else Dz
    logp = torch.full((max(N, 1),), -7.25, dtype=torch.float64, device=DEV)
    pred = torch.full((max(N, 1),), -77, dtype=torch.int32, device=DEV)
    if err is None:
        err = torch.full((max(N, 1), z.size(1)), -7.25, device=DEV)
    scratch = torch.empty(max(N, 1) * (max(K, 1) + 3 * d.H), device=DEV)
    o = eng._opts(r, L.LR, L.MOM, cd_k)
    o.sparsity = sparsity
    ws, nbytes, stream = eng._ws_tail(torch.device(DEV), z.size(1), d.H, z.size(0))
    p = lambda t, nm: None if nm in null else C.c_void_p(t.data_ptr())
    msg = None
    try:
        eng._call("imdbn_rbm_label_backprop_step", C.byref(d), C.c_void_p(z.data_ptr()), z.stride(0) if ldz is None else ldz, N, Dz, K,
                  C.c_void_p(gt.data_ptr()), C.byref(o) if opts else None, p(logp, "logp"), p(pred, "pred"), p(err, "err"),
                  err.stride(0) if lde is None else lde, C.c_void_p(scratch.data_ptr()), ws, nbytes, stream)
    except Nt.EngineError as e:
        msg = str(e)
    torch.cuda.synchronize()
    return msg, logp, pred, err


@pytest.mark.parametrize("what", ["N0", "ldz", "DzK", "K1", "null_logp", "null_err", "lde", "no_momentum", "cd_k", "sparsity"])
def test_invalid_arguments_launch_nothing(eng, what):
    c = L.case("odd", 0.1)
    r = _rbm(c)
    before = _state(r)
    z, gt = dev(c["z"]), dev(c["gt"])
    kw = {"N0": dict(N=0), "ldz": dict(ldz=c["Dz"] - 1), "DzK": dict(Dz=c["Dz"] - 1), "K1": dict(K=1, Dz=c["V"] - 1),
          "null_logp": dict(null=("logp",)), "null_err": dict(null=("err",)), "lde": dict(lde=c["Dz"] - 1),
          "no_momentum": dict(momentum=False), "cd_k": dict(cd_k=1), "sparsity": dict(sparsity=1)}[what]
    msg, logp, pred, err = _raw(eng, r, z, gt, kw.pop("K", c["K"]), **kw)
    print(what, "->", msg)
    assert msg is not None and "rc=-1)" in msg
    assert {"N0": "N = 0", "ldz": f"ldz {c['Dz'] - 1}", "DzK": f"Dz + K = {c['V'] - 1}", "K1": "K = 1", "null_logp": "out_logp",
            "null_err": "err_z", "lde": f"lde {c['Dz'] - 1}", "no_momentum": "momentum", "cd_k": "cd_k 1", "sparsity": "sparsity 1"}[what] in msg
    assert (logp == -7.25).all() and (pred == -77).all() and (err == -7.25).all() and _same(before, _state(r))
    # the same workspace then serves a good call; a frozen head needs neither options nor momentum buffers, a null pred is fine
    msg, logp, pred, err = _raw(eng, r, z, gt, c["K"], opts=False, momentum=False, null=("pred",))
    assert msg is None and torch.isfinite(logp).all() and (pred == -77).all() and torch.isfinite(err).all() and _same(before, _state(r))
    msg, logp, pred, err2 = _raw(eng, r, z, gt, c["K"])
    assert msg is None and torch.isfinite(logp).all() and (pred >= 0).all() and torch.equal(err, err2) and not _same(before, _state(r))
    from imdbn import engine as E
    with pytest.raises(E.EngineError):
        eng.label_backprop_step(r, z, c["K"], gt[:-1], L.LR, L.MOM)


@pytest.mark.parametrize("name", ["odd", "wide"])
def test_strided_z_and_strided_err_z_equal_the_contiguous_call_and_padding_is_never_touched(eng, name):
    c = L.case(name, 1.0)
    N, Dz = c["N"], c["Dz"]
    ra, rb = _rbm(c), _rbm(c)
    la, ea, pa = _call(eng, c, ra, apply=True)
    big = torch.full((N + 3, Dz + 5), float("nan"), device=DEV)          # NaN beyond Dz and beyond N
    big[:N, :Dz] = dev(c["z"])
    x = big[:N, :Dz]
    out = torch.full((N + 2, Dz + 7), float("nan"), device=DEV)
    assert x.stride(0) == Dz + 5 and not x.is_contiguous()
    msg, lb, pb, _ = _raw(eng, rb, x, dev(c["gt"]), c["K"], err=out[:N, :Dz])
    assert msg is None
    assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(ea, out[:N, :Dz]) and _same(_state(ra), _state(rb))
    assert torch.isnan(big[N:]).all() and torch.isnan(big[:, Dz:]).all()
    assert torch.isnan(out[N:]).all() and torch.isnan(out[:, Dz:]).all()


# ---- 6. one discriminative_step of the small stack --------------------------------------------------------------------
def _batch(i=0):
    X, yi = Cs.toy_data()
    B = Cs.TOY["B"]
    return X[i * B:(i + 1) * B], yi[i * B:(i + 1) * B]


def _stir(m):
    """Non-zero momenta everywhere, so that a wrong momentum path shows."""
    g = torch.Generator(device="cpu").manual_seed(9)
    for r in list(m.image_idbn.layers) + [m.joint_rbm]:
        r.W_m.copy_((torch.randn(tuple(r.W.shape), generator=g) * 0.01).to(DEV))
        r.hb_m.copy_((torch.randn(r.hb_m.shape, generator=g) * 0.01).to(DEV))
        r.vb_m.copy_((torch.randn(r.vb_m.shape, generator=g) * 0.01).to(DEV))


def test_one_discriminative_step_matches_the_twin_and_the_hand_issued_engine_calls(eng):
    X, yi = _batch()
    x, y = dev(X), dev(np.eye(Cs.TOY["K"], dtype=F32)[yi])
    K, epoch = Cs.TOY["K"], 7
    m = Cs.toy_model(DEV)
    _stir(m)
    gen = m.image_idbn.untie()
    gen_before = [_six(g) for g in gen]
    before = [_six(r) for r in m.image_idbn.layers]
    layers = [Cs.layer_state(r) for r in m.image_idbn.layers]
    joint = Cs.joint_state(m.joint_rbm)
    scal = [(r._lr_mom(epoch)[0] * 0.5, r._lr_mom(epoch)[1]) for r in m.image_idbn.layers]
    hl, hm = m.joint_rbm._lr_mom(epoch)
    out = m.discriminative_step(x, y, epoch, 10, lr_scale=0.5, head_lr_scale=0.25)
    torch.cuda.synchronize()
    want, j1 = D.discriminative_step(layers, joint, X, K, yi, scal, (0.25 * hl, hm), head_wd=float(m.joint_rbm.weight_decay))
    for i, (r, s) in enumerate(zip(m.image_idbn.layers, layers)):
        _check6(r, s, f"image layer {i}")
        after = _six(r)
        assert torch.equal(after["vis_bias"], before[i]["vis_bias"]) and torch.equal(after["vb_m"], before[i]["vb_m"])
        assert not torch.equal(after["W"], before[i]["W"]) and not torch.equal(after["hid_bias"], before[i]["hid_bias"])
    got = _state(m.joint_rbm)
    H = m.joint_rbm.num_hidden
    for k in KEYS:
        close(got[k], j1[k], L.tol_param(H, j1[k], 0.25 * hl), f"joint RBM: {k}")
    assert all(_same6(_six(g), b) for g, b in zip(gen, gen_before)) and m.image_idbn.gen_layers is gen
    print(f"nll {float(out['nll']):.6f} (twin {want['nll']:.6f}), acc {float(out['acc']):.3f} (twin {want['acc']:.3f})")
    assert abs(float(out["nll"]) - want["nll"]) <= 2 * L.eps(H) + 1e-9 * abs(want["nll"])
    assert want["head"]["gap"].min() > 2 * L.eps(H) and float(out["acc"]) == want["acc"]
    # by hand, on a second model in the same state
    m2 = Cs.toy_model(DEV)
    _stir(m2)
    ls, jr = m2.image_idbn.layers, m2.joint_rbm
    a = [x] + [m2.image_idbn.represent(x, upto_layer=l) for l in range(1, len(ls) + 1)]
    logp, f, pred = eng.label_backprop_step(jr, a[-1], K, dev(yi.astype(np.int32)), 0.25 * hl, hm, apply=True, want_pred=True)
    for l in range(len(ls), 0, -1):
        f = eng.backprop_step(ls[l - 1], up=(a[l - 1], f), lr=scal[l - 1][0], mom=scal[l - 1][1], want_v=l > 1)[0]
    torch.cuda.synchronize()
    assert all(_same6(_six(p), _six(q)) for p, q in zip(list(m.image_idbn.layers) + [m.joint_rbm], list(ls) + [jr]))
    assert torch.equal(out["nll"], -torch.nanmean(logp)) and float(out["acc"]) == float((pred.cpu().numpy() == yi).mean())


# ---- 7. finetune_discriminative ---------------------------------------------------------------------------------------
def test_finetune_discriminative_lowers_the_nll_along_the_twins_trajectory_and_does_not_cost_accuracy(eng):
    from imdbn import engine as E
    epochs, K, lr_scale, head_scale = 4, Cs.TOY["K"], 1.0, 3.0
    m = Cs.toy_model(DEV)
    with E.use_rng(E.PhiloxRng(seed=8)):                                # a model worth fine-tuning: 20 epochs of CD on the image stack and
        m.image_idbn.train(20)                                          # the joint RBM's warm-up epoch
        m.train_joint(1)
    # the twin alone, float64, from the same state: its per-epoch mean NLL must fall strictly
    layers = [Cs.layer_state(r) for r in m.image_idbn.layers]
    joint = Cs.joint_state(m.joint_rbm)
    traj = []
    for ep in range(epochs):
        scal = [(r._lr_mom(ep)[0] * lr_scale, r._lr_mom(ep)[1]) for r in m.image_idbn.layers]
        hl, hm = m.joint_rbm._lr_mom(ep)
        nll = []
        for b in range(Cs.TOY["NB"]):
            X, yi = _batch(b)
            o, joint = D.discriminative_step(layers, joint, X, K, yi, scal, (head_scale * hl, hm), head_wd=float(m.joint_rbm.weight_decay))
            nll.append(o["nll"])
        traj.append(float(np.mean(nll)))
    assert all(b < a for a, b in zip(traj, traj[1:])), f"the twin alone must fall strictly: {traj}"
    top1 = m.evaluate(seed=3)["text_top1"]
    m.finetune_discriminative(epochs, lr_scale=lr_scale, head_lr_scale=head_scale, log_every=1)
    hist = m.discriminative_history
    after = m.evaluate(seed=3)["text_top1"]
    print(f"nll {hist[0][1]:.6f} -> {hist[-1][1]:.6f} (twin {traj[0]:.6f} -> {traj[-1]:.6f}); batch accuracy {hist[0][2]:.3f} -> {hist[-1][2]:.3f}; "
          f"evaluate top-1 {top1:.3f} -> {after:.3f}")
    assert [h[0] for h in hist] == list(range(epochs)) and np.isfinite(np.array(hist)).all()
    assert hist[-1][1] < hist[0][1]
    assert after >= top1
    assert not m.image_idbn.is_untied()
