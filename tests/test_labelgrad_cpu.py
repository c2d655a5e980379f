"""CPU-only: the numpy twin of imdbn_rbm_label_step (tests/labelgrad_oracle.py) against torch.autograd and against brute force, the
kernels' fp32 form against the twin, the host logic of RBM.train_epoch_labels / iMDBN.train_joint(w_sup) / finetune_joint_labels on a
test double of the engine, and the export's declaration and binding.

The fp32 form of the kernels, restated here (``kernel_form``): base rounded to fp32, fp32 logits o = base + U and fp32 sigmoids,
the class values in double on the widened operands, p_k and r_k rounded to fp32, hneg one fp32 fma chain over k in index order,
the label-side sums over n one fp32 fma chain in index order, the update in fp32.  Against the twin it stays inside the GPU
tolerances (labelgrad_cases.tol_*); the largest errors seen over the cases were 5.1e-7 on hpos - hneg / r / r s (case "k65" at scale
1.0, bound 1.4e-3), 1.8e-7 on logp ("rows67", bound 4e-3) and 2.3e-7 on a parameter (W of "wide", bound 1.9e-4)."""
import os
import re

import numpy as np
import pytest
import torch

import labelgrad_cases as L
import labelgrad_oracle as O
from imdbn import engine as E
from imdbn.engine import native
from labelgrad_oracle import labelgrad_double  # noqa: F401  (the fixture, by name)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
ALL = [(n, s) for n in L.CASES for s in L.SCALES]


@pytest.fixture(scope="module", autouse=True)
def _export_exists():
    """The twin restates an export: without it there is nothing these tests describe."""
    assert "imdbn_rbm_label_step" in native.SIGNATURES, "imdbn_rbm_label_step is not bound"


def _fma_chain(x, y, n):
    """acc = fma(x(i), y(i), acc) in fp32 over i = 0 .. n - 1 (the product is exact in double; one more rounding than an fma, no tighter)."""
    acc = np.zeros((), F32)
    for i in range(n):
        acc = (x(i).astype(F64) * y(i).astype(F64) + acc.astype(F64)).astype(F32)
    return acc


def kernel_form(st, z, K, gt, lr, mom, wd):
    """-> (logp [N] float64, state after the step (fp32), dict(delta, r, rs) the per-row fp32 terms): module docstring."""
    W, b, c = st["W"], st["b"], st["c"]
    N, Dz = z.shape
    H = W.shape[1]
    U = W[Dz:]
    base = (z.astype(F64) @ W[:Dz].astype(F64) + c.astype(F64)).astype(F32)
    o = (base[:, None, :] + U[None]).astype(F32)
    s = (F32(1) / (F32(1) + np.exp(-o, dtype=F32))).astype(F32)
    a = (z.astype(F64) @ b[:Dz].astype(F64))[:, None] + b[Dz:].astype(F64)[None] + \
        np.logaddexp(0.0, base.astype(F64)[:, None, :] + U.astype(F64)[None]).sum(2)
    mx = a.max(1)
    marg = mx + np.log(np.exp(a - mx[:, None]).sum(1))
    gt = np.asarray(gt).astype(np.int64)
    ok = (gt >= 0) & (gt < K)
    t = np.where(ok, gt, 0)
    n = np.arange(N)
    p = np.exp(a - marg[:, None])
    onehot = np.zeros((N, K), F64)
    onehot[n, t] = 1.0
    r = (onehot - p).astype(F32)
    p32 = p.astype(F32)
    hneg = _fma_chain(lambda k: p32[:, k, None], lambda k: s[:, k, :], K)
    hpos = s[n, t].copy()
    r[~ok], hpos[~ok], hneg[~ok] = 0, 0, 0
    G_U = _fma_chain(lambda i: r[i, :, None], lambda i: s[i], N)
    G_by = np.zeros(K, F32)
    for i in range(N):
        G_by = (G_by + r[i]).astype(F32)
    G_Wz = (z.astype(F64).T @ hpos.astype(F64) - z.astype(F64).T @ hneg.astype(F64)).astype(F32)
    G_c = (hpos.astype(F64).sum(0) - hneg.astype(F64).sum(0)).astype(F32)
    nn, lr, mom, wd = F32(N), F32(lr), F32(mom), F32(wd)
    G_W = np.concatenate([G_Wz, G_U], 0)
    Wm = (st["Wm"] * mom).astype(F32)
    Wm = (Wm + lr * (G_W / nn - wd * W).astype(F32)).astype(F32)
    cm = ((st["cm"] * mom).astype(F32) + (lr * G_c).astype(F32) / nn).astype(F32)
    G_b = np.concatenate([np.zeros(Dz, F32), G_by])
    bm = ((st["bm"] * mom).astype(F32) + (lr * G_b).astype(F32) / nn).astype(F32)
    new = dict(W=(W + Wm).astype(F32), b=(b + bm).astype(F32), c=(c + cm).astype(F32), Wm=Wm, bm=bm, cm=cm)
    return np.where(ok, a[n, t] - marg, np.nan), new, dict(delta=hpos - hneg, r=r, rs=r[:, :, None] * s)


# ---- 1. the twin's gradients against autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", [("odd", 0.1), ("odd", 1.0), ("k65", 1.0), ("one", 1.0)])
def test_twin_gradients_equal_autograd_of_the_log_softmax_of_free_energies(name, scale):
    c = L.case(name, scale)
    Dz, K, N = c["Dz"], c["K"], c["N"]
    W, b, hc = (torch.tensor(c[k].astype(F64), requires_grad=True) for k in ("W", "b", "c"))
    z = torch.tensor(c["z"].astype(F64))
    neg_F = []
    for k in range(K):
        v = torch.cat([z, torch.eye(K, dtype=torch.float64)[k].expand(N, K)], 1)
        neg_F.append(v @ b + torch.nn.functional.softplus(hc + v @ W).sum(1))
    lp = torch.log_softmax(torch.stack(neg_F, 1), 1)[torch.arange(N), torch.from_numpy(c["gt"].astype(np.int64))]
    lp.sum().backward()
    logp, G_W, G_b, G_c = O.gradients(c["W"], c["b"], c["c"], c["z"], K, c["gt"])
    assert np.abs(logp - lp.detach().numpy()).max() <= 1e-10
    for got, want, what in ((G_W, W.grad, "W"), (G_b, b.grad, "vis_bias"), (G_c, hc.grad, "hid_bias")):
        err = np.abs(got - want.numpy()).max()
        print(f"{name} scale {scale}: {what} max |twin - autograd| {err:.3g}")
        assert err <= 1e-10
    assert (G_b[:Dz] == 0).all()


# ---- 2. the twin's logp against brute force --------------------------------------------------------------------------------
def test_twin_logp_is_the_conditional_of_the_enumerated_labels_and_invalid_rows_take_no_part():
    c = L.case("odd", 1.0)
    Dz, K, N = c["Dz"], c["K"], c["N"]
    W, b, hc, z = (c[k].astype(F64) for k in ("W", "b", "c", "z"))
    F = np.stack([-(np.concatenate([z, np.tile(np.eye(K)[k], (N, 1))], 1) @ b)
                  - np.logaddexp(0.0, np.concatenate([z, np.tile(np.eye(K)[k], (N, 1))], 1) @ W + hc).sum(1) for k in range(K)], 1)
    w = np.exp(-(F - F.min(1, keepdims=True)))
    want = np.log(w[np.arange(N), c["gt"]] / w.sum(1))
    logp, G_W, G_b, G_c = O.gradients(c["W"], c["b"], c["c"], c["z"], K, c["gt"])
    assert np.abs(logp - want).max() <= 1e-10
    # invalid labels: NaN there, and the sums are those of the remaining rows
    bad = c["gt"].copy()
    bad[1], bad[3] = -1, K
    keep = np.array([0, 2, 4])
    lp2, W2, b2, c2 = O.gradients(c["W"], c["b"], c["c"], c["z"], K, bad)
    lp3, W3, b3, c3 = O.gradients(c["W"], c["b"], c["c"], c["z"][keep], K, c["gt"][keep])
    assert np.isnan(lp2[[1, 3]]).all() and np.array_equal(lp2[keep], logp[keep])
    assert np.allclose(W2, W3, rtol=0, atol=1e-12) and np.allclose(b2, b3, rtol=0, atol=1e-12) and np.allclose(c2, c3, rtol=0, atol=1e-12)
    _, new = O.step(L.state(c), c["z"], K, bad, 0.1, 0.0, 0.0)          # the divisor stays N
    assert np.allclose(new["Wm"], 0.1 * W3 / N, rtol=0, atol=1e-12)


# ---- 3. the kernels' fp32 form against the twin -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", ALL)
def test_fp32_form_stays_inside_the_gpu_tolerances(name, scale):
    c = L.case(name, scale)
    K, H, N = c["K"], c["H"], c["N"]
    q = O.rows(c["W"], c["b"], c["c"], c["z"], K, c["gt"])
    want_logp, want = O.step(L.state(c), c["z"], K, c["gt"], L.LR, L.MOM, L.WD)
    got_logp, got, terms = kernel_form(L.state(c), c["z"], K, c["gt"], L.LR, L.MOM, L.WD)
    e = {"delta": np.abs(terms["delta"] - (q["hpos"] - q["hneg"])).max(), "r": np.abs(terms["r"] - q["r"]).max(),
         "rs": np.abs(terms["rs"] - q["r"][:, :, None] * q["s"]).max()}
    ep = {k: np.abs(got[k].astype(F64) - want[k]).max() for k in want}
    print(f"{name} scale {scale}: terms {e} (bound {L.tol_delta(H):.3g}); logp {np.abs(got_logp - want_logp).max():.3g}; parameters {ep}")
    assert max(e.values()) <= L.tol_delta(H)
    assert (np.abs(got_logp - want_logp) <= L.tol_logp(H, want_logp)).all()
    for k in want:
        assert (np.abs(got[k].astype(F64) - want[k]) <= L.tol_param(H, want[k], L.LR)).all(), k
    # a sign or index error cannot hide inside the tolerance: the twin's own largest gradient entry / N is 10 x above it
    _, G_W, G_b, G_c = O.gradients(c["W"], c["b"], c["c"], c["z"], K, c["gt"])
    big = max(np.abs(G_W).max(), np.abs(G_b).max(), np.abs(G_c).max()) / N
    print(f"{name} scale {scale}: largest |G| / N {big:.3g} (10 tol_delta = {10 * L.tol_delta(H):.3g})")
    assert big >= 10 * L.tol_delta(H)


# ---- 4. host logic on the test double ---------------------------------------------------------------------------------------
class _Run:
    def __init__(self): self.logged = []
    def log(self, d): self.logged.append(dict(d))


def _model(epochs_seed=3, NB=2, B=4, K=3):
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import iMDBN
    g = np.random.Generator(np.random.PCG64(epochs_seed))
    yi = np.arange(NB * B) % K
    X = (g.random((NB * B, 20)) > 0.6).astype(F32)
    dl = DataLoader(TensorDataset(torch.from_numpy(X), torch.from_numpy(np.eye(K, dtype=F32)[yi])), batch_size=B, shuffle=False)
    params = {"LEARNING_RATE": 0.1, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95, "LEARNING_RATE_DYNAMIC": True,
              "CD": 1, "JOINT_CD": 1, "JOINT_AUX_COND_STEPS": 10, "CROSS_GIBBS_STEPS": 3}
    torch.manual_seed(1)
    return iMDBN([20, 8], 6, params=params, dataloader=dl, val_loader=dl, device=torch.device("cpu"), num_labels=K), NB, B


def test_train_joint_without_w_sup_makes_no_label_step_and_adds_no_key(labelgrad_double):
    m, NB, B = _model()
    m.wandb_run = _Run()
    with E.use_rng(E.PhiloxRng(3)):
        m.train_joint(1)
    assert not [c for c in labelgrad_double.calls if c[0] == "label_step"]
    assert "sup_nll" not in m.joint_history[0]
    assert not any("joint/sup_nll" in d for d in m.wandb_run.logged)


def test_train_joint_with_w_sup_issues_one_label_step_per_batch_after_the_generative_updates(labelgrad_double):
    m, NB, B = _model()
    m.wandb_run = _Run()
    jr = m.joint_rbm
    with E.use_rng(E.PhiloxRng(3)):
        m.train_joint(9, w_sup=0.5)                      # epochs 0-7 warm-up, epoch 8 the main phase
    upd = [c for c in labelgrad_double.calls if c[0] in ("label_step", "cd_step", "clamped_step")]
    warm = [("clamped_step",), ("clamped_step",), "L"]
    main0 = [("cd_step",), ("clamped_step",), ("clamped_step",), "L"]      # batch 0 of an epoch: + the image-clamped update
    main = [("cd_step",), ("clamped_step",), "L"]
    want = (warm * NB) * 8 + main0 + main * (NB - 1)
    assert len(upd) == len(want)
    steps = []
    for got, w in zip(upd, want):
        if w == "L":
            assert got[0] == "label_step" and got[1] == B
            steps.append(got)
        else:
            assert got[:1] == w                          # (the base double's cd_step record also carries shape, k and forward)
    for i, got in enumerate(steps):
        lr, mom = jr._lr_mom(i // NB)
        assert got[2] == pytest.approx(0.5 * lr, rel=1e-12) and got[3] == mom
    assert len(m.joint_history) == 9
    for ep, rec in enumerate(m.joint_history):
        assert np.isfinite(rec["sup_nll"]) and rec["sup_nll"] > 0
    assert [d["joint/sup_nll"] for d in m.wandb_run.logged if "joint/sup_nll" in d] == [r["sup_nll"] for r in m.joint_history]


def test_train_epoch_labels_returns_minus_the_nanmean_of_the_twins_logp(labelgrad_double):
    c = L.case("odd", 1.0)
    from bound_oracle import host_rbm
    r = host_rbm(c, groups=[(c["Dz"], c["V"])])
    r.weight_decay = L.WD
    r.W_m, r.vb_m, r.hb_m = (torch.from_numpy(c[k].copy()) for k in ("Wm", "bm", "cm"))
    bad = c["gt"].copy()
    bad[2] = c["K"]
    want_logp, want = O.step(L.state(c), c["z"], c["K"], bad, 0.25 * r._lr_mom(7)[0], r._lr_mom(7)[1], L.WD)
    E.manual_seed(5)
    nll = r.train_epoch_labels(torch.from_numpy(c["z"]), torch.from_numpy(bad), 7, 10, c["K"], lr_mult=0.25)
    assert E.get_rng().offset == 0                                      # no draws
    assert nll.dtype == torch.float64 and nll.dim() == 0 and float(nll) == pytest.approx(-np.nanmean(want_logp), rel=1e-12)
    assert np.allclose(r.W.data.numpy(), want["W"], rtol=0, atol=1e-6) and np.allclose(r.vb_m.numpy(), want["bm"], rtol=0, atol=1e-6)


def test_w_sup_is_refused_under_data_parallelism(labelgrad_double, monkeypatch):
    m, _, _ = _model()
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError, match="w_sup"):
        m.train_joint(1, w_sup=0.5)
    assert not labelgrad_double.calls


def test_finetune_joint_labels_returns_one_value_per_epoch(labelgrad_double):
    m, NB, B = _model()
    with E.use_rng(E.PhiloxRng(3)):
        m.init_joint_bias_from_data(n_batches=10)
        n0 = len(labelgrad_double.calls)
        out = m.finetune_joint_labels(3, lr_scale=0.3)
        assert E.get_rng().offset == 0
    assert [c[0] for c in labelgrad_double.calls[n0:]] == ["forward", "label_step"] * (3 * NB)     # represent(), then the step
    steps = labelgrad_double.calls[n0 + 1::2]
    assert len(out) == 3 and np.isfinite(out).all() and out == m.finetune_sup_nll
    assert len(steps) == 3 * NB and all(s[0] == "label_step" and s[1] == B for s in steps)
    for i, s in enumerate(steps):
        lr, mom = m.joint_rbm._lr_mom(i // NB)
        assert s[2] == pytest.approx(0.3 * lr, rel=1e-12) and s[3] == mom
    assert out[-1] < out[0]                                             # three epochs of ascent on 8 rows
    assert m.finetune_joint_labels(0) == []


# ---- 5. ABI -----------------------------------------------------------------------------------------------------------------
def test_export_is_declared_bound_and_in_the_built_library():
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    assert re.search(r"\bint\s+imdbn_rbm_label_step\s*\(", src)
    assert "#define IMDBN_ABI_VERSION 4" in src and native.ABI_VERSION == 4
    assert len(native.SIGNATURES["imdbn_rbm_label_step"][1]) == 13
    assert hasattr(native.lib(), "imdbn_rbm_label_step")
    from imdbn.engine.hip_engine import HipEngine
    from imdbn.models import RBM, iMDBN
    assert hasattr(HipEngine, "label_step") and hasattr(RBM, "train_epoch_labels") and hasattr(iMDBN, "finetune_joint_labels")
