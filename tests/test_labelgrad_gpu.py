"""GPU: imdbn_rbm_label_step, RBM.train_epoch_labels and iMDBN.train_joint(w_sup) against the float64 numpy twin
(tests/labelgrad_oracle.py) fed the same fp32 state.

Tolerances (tests/labelgrad_cases.py), from the project's convention for the label-side kernel -- a class value within eps = H 1e-5 of
float64, hence |dp_k| <= 2 eps p_k, and |ds| <= 2.5e-6: every entry of hpos - hneg, r and r s within tol_delta = 2 H 1e-5 + 1e-5; every
parameter and momentum entry after one step within lr tol_delta + 1e-6 (|value| + lr); logp within 2 eps + 1e-9 |value|.  The first
test prints the largest errors per case; DESIGN §22 holds the maxima."""
import ctypes as C

import numpy as np
import pytest
import torch

import labelgrad_cases as L
import labelgrad_oracle as O
from likelihood_gpu import DEV, _native, close, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL = [(n, s) for n in L.CASES for s in L.SCALES]
KEYS = ("W", "b", "c", "Wm", "bm", "cm")


def _rbm(c, st=None, wd=L.WD):
    """The joint RBM of a case on the device (the constructor's padded weight rows), its state `st` (default: the case's)."""
    st = c if st is None else st
    r = device_rbm(dict(W=st["W"], b=st["b"], c=st["c"]), groups=[(c["Dz"], c["V"])])
    r.weight_decay = wd
    r.W_m.copy_(torch.from_numpy(st["Wm"]))
    r.vb_m.copy_(torch.from_numpy(st["bm"]))
    r.hb_m.copy_(torch.from_numpy(st["cm"]))
    return r


def _state(r):
    torch.cuda.synchronize()
    return {k: t.detach().cpu().numpy().copy() for k, t in zip(KEYS, (r.W.data, r.vis_bias.data, r.hid_bias.data, r.W_m, r.vb_m, r.hb_m))}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS)


def _twin(name, scale):
    """(case, logp [N], state after one step) of the twin, computed once."""
    def run():
        c = L.case(name, scale)
        return (c,) + O.step(L.state(c), c["z"], c["K"], c["gt"], L.LR, L.MOM, L.WD)
    return twin(("labelgrad", name, scale), run)


def _step(eng, c, r, z=None, gt=None, lr=L.LR, mom=L.MOM):
    logp = eng.label_step(r, dev(c["z"]) if z is None else z, c["K"], dev(c["gt"] if gt is None else gt), lr, mom)
    torch.cuda.synchronize()
    return logp


# ---- 1. against the twin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", ALL)
def test_logp_and_all_six_tensors_after_one_step_match_the_twin(eng, name, scale):
    c, want_logp, want = _twin(name, scale)
    r = _rbm(c)
    logp = _step(eng, c, r)
    assert logp.dtype == torch.float64 and tuple(logp.shape) == (c["N"],)
    close(logp.cpu().numpy(), want_logp, L.tol_logp(c["H"], want_logp), f"{name} scale {scale}: logp")
    got = _state(r)
    for k in KEYS:
        close(got[k], want[k], L.tol_param(c["H"], want[k], L.LR), f"{name} scale {scale}: {k}")
        assert np.abs(want[k] - c[k]).max() > 0                         # the step moved it


# ---- 2. agreement with label_loglik -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", ALL)
def test_logp_has_the_bits_of_label_logliks_joint_minus_marginal(eng, name, scale):
    c = L.case(name, scale)
    r = _rbm(c)
    j, m = eng.label_loglik(r, dev(c["z"]), c["K"], dev(c["gt"]))       # the parameters before the step
    logp = _step(eng, c, r)
    assert torch.equal(logp, j - m)


# ---- 3. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "k65", "rows67", "wide"])
def test_the_same_state_stepped_twice_gives_the_same_bits(eng, name):
    c = L.case(name, 1.0)
    out = []
    for _ in range(2):
        r = _rbm(c)
        logp = _step(eng, c, r)
        out.append((logp, _state(r)))
    assert torch.equal(out[0][0], out[1][0]) and _same(out[0][1], out[1][1])


# ---- 4. invalid labels ------------------------------------------------------------------------------------------------
def test_rows_with_a_label_outside_the_range_are_nan_and_enter_no_sum(eng):
    """Two comparisons.  (a) Bit for bit: the rows with gt = -1 / gt = K stand at the END of an 8-row batch (4 valid, then 2 + 2
    invalid), weight decay 0.  Their gradient is zero, so the step equals the step on the 4 valid rows alone at lr / 2: the sums over
    rows are the same sums followed by exact zeros, and lr (G / 8) = (lr / 2) (G / 4) exactly in fp32 (powers of two).  That holds
    only if the invalid rows add nothing AND the divisor stays N = 8.  (b) Invalid rows in the middle of a batch: against the twin
    within the tolerances, and bit for bit against the same call with other finite codes in those rows."""
    c = L.case("k65", 1.0)
    K, H = c["K"], c["H"]
    g = np.random.Generator(np.random.PCG64(77))
    z = g.random((8, c["Dz"])).astype(F32)
    gt = np.array([0, 64, 7, 33, -1, K, K, -1], np.int32)
    r8, r4 = _rbm(c, wd=0.0), _rbm(c, wd=0.0)
    lp8 = _step(eng, c, r8, z=dev(z), gt=gt, lr=0.125)
    lp4 = _step(eng, c, r4, z=dev(z[:4]), gt=gt[:4], lr=0.0625)
    assert torch.isnan(lp8[4:]).all() and torch.equal(lp8[:4], lp4) and torch.isfinite(lp4).all()
    assert _same(_state(r8), _state(r4))
    # (b)
    c = L.case("rows67", 0.1)
    bad = c["gt"].copy()
    bad[[3, 40, 66]] = [-1, c["K"], 2 ** 30]
    want_logp, want = O.step(L.state(c), c["z"], c["K"], bad, L.LR, L.MOM, L.WD)
    ra, rb = _rbm(c), _rbm(c)
    la = _step(eng, c, ra, gt=bad)
    got = _state(ra)
    assert np.isnan(want_logp[[3, 40, 66]]).all() and torch.isnan(la[[3, 40, 66]]).all()
    keep = np.isfinite(want_logp)
    close(la.cpu().numpy()[keep], want_logp[keep], L.tol_logp(c["H"], want_logp[keep]), "invalid rows: logp of the others")
    for k in KEYS:
        close(got[k], want[k], L.tol_param(c["H"], want[k], L.LR), f"invalid rows: {k}")
    z2 = c["z"].copy()
    z2[[3, 40, 66]] = g.random((3, c["Dz"])).astype(F32)
    lb = _step(eng, c, rb, z=dev(z2), gt=bad)
    assert torch.equal(la[torch.from_numpy(keep)], lb[torch.from_numpy(keep)]) and _same(got, _state(rb))


# ---- 5. invalid arguments ---------------------------------------------------------------------------------------------
def _raw(eng, r, z, gt, K, N=None, ldz=None, Dz=None, null_logp=False, momentum=True):
    """The export called directly on a sentinel-filled output -> (EngineError message or None, out_logp)."""
    from imdbn.engine import native as Nt
    d = eng._desc(r, True)
    if not momentum:
        d = Nt.RbmDesc.from_buffer_copy(d)
        d.W_m = None
    N = z.size(0) if N is None else N
    Dz = z.size(1) if Dz is None else Dz
    logp = torch.full((max(N, 1),), -7.25, dtype=torch.float64, device=DEV)
    scratch = torch.empty(max(N, 1) * (max(K, 1) + 2 * d.H), device=DEV)
    o = eng._opts(r, L.LR, L.MOM, 1)
    ws, nbytes, stream = eng._ws_tail(torch.device(DEV), z.size(1), d.H, z.size(0))
    msg = None
    try:
        eng._call("imdbn_rbm_label_step", C.byref(d), C.c_void_p(z.data_ptr()), z.stride(0) if ldz is None else ldz, N, Dz, K,
                  C.c_void_p(gt.data_ptr()), C.byref(o), None if null_logp else C.c_void_p(logp.data_ptr()),
                  C.c_void_p(scratch.data_ptr()), ws, nbytes, stream)
    except Nt.EngineError as e:
        msg = str(e)
    torch.cuda.synchronize()
    return msg, logp


@pytest.mark.parametrize("what", ["N0", "ldz", "DzK", "K1", "null_logp", "no_momentum"])
def test_invalid_arguments_launch_nothing(eng, what):
    c = L.case("odd", 0.1)
    r = _rbm(c)
    before = _state(r)
    z, gt = dev(c["z"]), dev(c["gt"])
    kw = {"N0": dict(N=0), "ldz": dict(ldz=c["Dz"] - 1), "DzK": dict(Dz=c["Dz"] - 1), "K1": dict(K=1, Dz=c["V"] - 1),
          "null_logp": dict(null_logp=True), "no_momentum": dict(momentum=False)}[what]
    msg, logp = _raw(eng, r, z, gt, kw.pop("K", c["K"]), **kw)
    print(what, "->", msg)
    assert msg is not None and "rc=-1)" in msg
    assert {"N0": "N = 0", "ldz": f"ldz {c['Dz'] - 1}", "DzK": f"Dz + K = {c['V'] - 1}", "K1": "K = 1", "null_logp": "out_logp",
            "no_momentum": "momentum"}[what] in msg
    assert (logp == -7.25).all() and _same(before, _state(r))
    # the same workspace then serves a good call
    msg, logp = _raw(eng, r, z, gt, c["K"])
    assert msg is None and torch.isfinite(logp).all() and not _same(before, _state(r))
    from imdbn import engine as E
    with pytest.raises(E.EngineError):
        eng.label_step(r, z, c["K"], gt[:-1], L.LR, L.MOM)


# ---- 6. strided z -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "wide"])
def test_strided_rows_equal_contiguous_rows_and_padding_is_never_touched(eng, name):
    c = L.case(name, 1.0)
    ra, rb = _rbm(c), _rbm(c)
    la = _step(eng, c, ra)
    big = torch.full((c["N"] + 3, c["Dz"] + 5), float("nan"), device=DEV)          # NaN beyond Dz and beyond N
    big[:c["N"], :c["Dz"]] = dev(c["z"])
    x = big[:c["N"], :c["Dz"]]
    assert x.stride(0) == c["Dz"] + 5 and not x.is_contiguous()
    lb = _step(eng, c, rb, z=x)
    assert torch.equal(la, lb) and _same(_state(ra), _state(rb))
    assert torch.isnan(big[c["N"]:]).all() and torch.isnan(big[:, c["Dz"]:]).all()


# ---- 7. ascent --------------------------------------------------------------------------------------------------------
def test_twenty_five_steps_raise_the_mean_logp_along_the_twins_trajectory(eng):
    c = L.case("rows67", 0.1)
    K, H, steps, lr = c["K"], c["H"], 25, 0.05
    st = L.state(c)
    st["Wm"][:], st["bm"][:], st["cm"][:] = 0, 0, 0
    cur, traj = st, []
    for _ in range(steps + 1):
        lp, cur = O.step(cur, c["z"], K, c["gt"], lr, 0.0, 0.0)
        traj.append(lp.mean())
    assert all(b > a for a, b in zip(traj, traj[1:])), "the twin alone must rise strictly"
    r = _rbm(c, st=st, wd=0.0)
    got = []
    for _ in range(steps):
        got.append(float(_step(eng, c, r, lr=lr, mom=0.0).mean()))
    j, mg = eng.label_loglik(r, dev(c["z"]), K, dev(c["gt"]))          # where the 25th step arrived
    got.append(float((j - mg).mean()))
    err = np.abs(np.array(got) - np.array(traj))
    print(f"ascent: mean logp {got[0]:.6f} -> {got[-1]:.6f} (twin {traj[0]:.6f} -> {traj[-1]:.6f}); "
          f"max |device - twin| along the trajectory {err.max():.3g} (bound {25 * 2 * L.eps(H):.3g})")
    assert got[-1] > got[0] and got[steps - 1] > got[0]
    assert (err <= 25 * 2 * L.eps(H)).all()


# ---- 8. train_joint end to end ----------------------------------------------------------------------------------------
def _imdbn(seed=5):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import iMDBN
    g = np.random.Generator(np.random.PCG64(11))
    K, B, NB = 4, 8, 3
    yi = g.integers(0, K, B * NB)
    proto = (g.random((K, 100)) > 0.7).astype(F32)
    X = np.abs(proto[yi] - (g.random((B * NB, 100)) > 0.9).astype(F32)).astype(F32)
    dl = DataLoader(TensorDataset(torch.from_numpy(X).to(DEV), torch.from_numpy(np.eye(K, dtype=F32)[yi]).to(DEV)), batch_size=B, shuffle=False)
    params = {"LEARNING_RATE": 0.1, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95, "LEARNING_RATE_DYNAMIC": True,
              "CD": 1, "JOINT_LEARNING_RATE": 0.04, "JOINT_CD": 1, "JOINT_AUX_COND_STEPS": 10, "CROSS_GIBBS_STEPS": 5,
              "JOINT_METRICS_OVERLAP": False}
    torch.manual_seed(seed)
    return iMDBN([100, 40, 20], 16, params=params, dataloader=dl, val_loader=dl, device=torch.device(DEV), num_labels=K)


def test_train_joint_with_w_sup_equals_the_hand_issued_engine_calls(eng):
    from imdbn import engine as E
    from imdbn.utils import batches, rows_on_device
    runs = {}
    for w_sup in (0.0, 0.5):
        m = _imdbn()
        with E.use_rng(E.PhiloxRng(seed=8)):
            m.train_joint(1, w_sup=w_sup)
        runs[w_sup] = (m, _state(m.joint_rbm))
    m5, s5 = runs[0.5]
    assert "sup_nll" not in runs[0.0][0].joint_history[0]
    assert np.isfinite(m5.joint_history[0]["sup_nll"]) and m5.joint_history[0]["sup_nll"] > 0
    assert not np.array_equal(s5["W"], runs[0.0][1]["W"]) and not np.array_equal(s5["b"], runs[0.0][1]["b"])
    # by hand: the warm-up epoch of train_joint, call by call
    m = _imdbn()
    jr, K, Dz = m.joint_rbm, m.num_labels, m.Dz_img
    nll = []
    with E.use_rng(E.PhiloxRng(seed=8)):
        m.init_joint_bias_from_data(n_batches=10)
        acc = torch.zeros(5, device=DEV, dtype=torch.float64)
        for img, y in batches(m.dataloader):
            img, y = rows_on_device(img, m.device), y.to(DEV).float()
            z = m.image_idbn.represent(img)
            for _ in range(2):
                vk, km = m._clamp_y(y, z.size(0), Dz + K, Dz)
                jr.train_epoch_clamped(vk, km, 0, 1, CD=1, cond_init_steps=10, sample_h=False, sample_v=False, aux_lr_mult=0.3,
                                       use_noisy_init=True)
            lr, mom = jr._lr_mom(0)
            nll.append(-torch.nanmean(eng.label_step(jr, z, K, y.argmax(dim=1), 0.5 * lr, mom)))
            m._batch_metrics(acc, jr, z, y, img)
    assert _same(_state(jr), s5)
    assert float(torch.stack(nll).mean()) == m5.joint_history[0]["sup_nll"]
