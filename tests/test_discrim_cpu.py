"""CPU-only: the twin of the discriminative fine-tuning calls (tests/discrim_oracle.py) against finite differences of its own
objective, the cases' argmax rows, and the host logic of RBM.label_backprop / iMDBN.discriminative_step / finetune_discriminative
through the engine double (tests/discrim_engine_double.py).  No claim about the kernels is made here -- those are tested on the GPU in
test_discrim_gpu.py."""
import io
import os
import pickle
import re

import numpy as np
import pytest
import torch

import backprop_oracle as Bp
import discrim_cases as Cs
import discrim_oracle as D
import labelgrad_oracle as Lg
from discrim_engine_double import DiscrimOracleEngine
from imdbn import engine as E
from imdbn.engine import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.fixture
def double():
    eng = DiscrimOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)


# ---- 1. g_z is the gradient of log p(t | z) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", [("odd", 0.1), ("odd", 1.0), ("k65", 1.0), ("one", 1.0)])
def test_the_twins_g_z_is_the_central_difference_of_its_own_logp(name, scale):
    c = Cs.case(name, scale)
    K = c["K"]
    z = 0.05 + 0.9 * c["z"].astype(F64)                                 # inside (0, 1): z (1 - z) > 0 in every column
    out = D.head(c["W"], c["b"], c["c"], z, K, c["gt"])
    lp = lambda zz: Lg.rows(c["W"], c["b"], c["c"], zz, K, c["gt"])["logp"]
    h, worst = 1e-6, 0.0
    for i in range(c["Dz"]):
        zp, zm = z.copy(), z.copy()
        zp[:, i] += h
        zm[:, i] -= h
        fd = (lp(zp) - lp(zm)) / (2 * h)
        worst = max(worst, np.abs(fd - out["g_z"][:, i]).max())
    print(f"{name} scale {scale}: max |g_z - fd| {worst:.3g}")
    assert worst <= 1e-7 * (1 + np.abs(out["g_z"]).max())
    assert np.array_equal(out["err_z"], out["g_z"] * (z * (1 - z))) and np.abs(out["err_z"]).max() > 0
    # an invalid label: NaN and exact zero rows, the other rows unchanged
    bad = c["gt"].copy()
    bad[0] = K
    o2 = D.head(c["W"], c["b"], c["c"], z, K, bad)
    assert np.isnan(o2["logp"][0]) and not o2["err_z"][0].any() and not o2["e"][0].any()
    assert np.array_equal(o2["err_z"][1:], out["err_z"][1:]) and np.array_equal(o2["pred"], out["pred"])


# ---- 2. the whole chain is the gradient of the model's mean log p ----------------------------------------------------------------------
def test_with_a_frozen_head_the_twins_layer_deltas_are_the_gradient_of_the_whole_models_mean_logp():
    """lr = 1, no momentum, no weight decay, the head frozen: the deltas of W and hid_bias of both layers after one step are the
    gradient of mean log p(gt | data), checked against central differences (step 1e-6, float64) at every entry; vis_bias, the
    momenta of the visible biases and the joint RBM do not move."""
    layers, joint, x, gt = Cs.small_stack()
    K = 3
    moved = [Bp.f64_state(s) for s in layers]
    j0 = {k: v.copy() for k, v in joint.items()}
    out, j1 = D.discriminative_step(moved, joint, x, K, gt, [(1.0, 0.0)] * 2, (1.0, 0.0), train_head=False)
    assert all(np.array_equal(j1[k], j0[k]) for k in j0)
    assert out["nll"] == pytest.approx(-D.mean_logp(layers, joint, x, K, gt), rel=1e-12) and 0.0 <= out["acc"] <= 1.0
    h, worst = 1e-6, 0.0
    for li, (s, m) in enumerate(zip(layers, moved)):
        for k in ("W", "hid_bias"):
            p = getattr(s, k)
            for idx in np.ndindex(p.shape):
                keep = p[idx]
                p[idx] = keep + h
                up = D.mean_logp(layers, joint, x, K, gt)
                p[idx] = keep - h
                dn = D.mean_logp(layers, joint, x, K, gt)
                p[idx] = keep
                fd = (up - dn) / (2 * h)
                delta = getattr(m, k)[idx] - keep
                worst = max(worst, abs(delta - fd))
                assert abs(delta - fd) <= 1e-7 * abs(fd) + 1e-9, f"layer {li} {k}{idx}: {delta} vs {fd}"
        assert np.array_equal(m.vis_bias, s.vis_bias) and not m.vb_m.any()
        assert np.abs(m.W - s.W).max() > 0
    print(f"largest |delta - fd| {worst:.3g}")


def test_with_the_head_training_the_joint_state_is_the_label_steps():
    layers, joint, x, gt = Cs.small_stack()
    z = D.forward(layers, x)[-1]
    want = Lg.step(joint, z, 3, gt, 0.2, 0.5, 1e-4)[1]
    _, got = D.discriminative_step([Bp.f64_state(s) for s in layers], joint, x, 3, gt, [(0.1, 0.0)] * 2, (0.2, 0.5), head_wd=1e-4)
    assert all(np.array_equal(got[k], want[k]) for k in want)


# ---- the cases' argmax rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", Cs.ALL)
def test_the_twin_alone_decides_the_argmax_of_at_least_nine_rows_in_ten(name, scale):
    c = Cs.case(name, scale)
    out = D.head(c["W"], c["b"], c["c"], c["z"], c["K"], c["gt"])
    use = Cs.pred_rows(c["H"], out)
    print(f"{name} scale {scale}: smallest top-two gap {out['gap'].min():.3g} (2 eps = {2 * Cs.eps(c['H']):.3g}); {int((~use).sum())} of {c['N']} rows left out")
    assert (~use).sum() <= Cs.PRED_LEFT_OUT * c["N"]


# ---- 3. host logic on the engine double ---------------------------------------------------------------------------------------------
def _params(r):
    return [getattr(r, k).data.clone() for k in ("W", "hid_bias", "vis_bias")] + [getattr(r, k).clone() for k in ("W_m", "hb_m", "vb_m")]


def _model():
    m = Cs.toy_model("cpu")
    for r in list(m.image_idbn.layers) + [m.joint_rbm]:
        r.W.data = r.W.data.contiguous()
        r.W_m, r.hb_m, r.vb_m = torch.zeros_like(r.W.data), torch.zeros_like(r.hid_bias.data), torch.zeros_like(r.vis_bias.data)
    return m


def test_imdbn_discriminative_step_issues_the_documented_call_sequence_and_matches_the_twin(double):
    m = _model()
    X, yi = Cs.toy_data()
    x, y = torch.from_numpy(X[:8]), torch.from_numpy(np.eye(4, dtype=F32)[yi[:8]])
    layers = [Cs.layer_state(r) for r in m.image_idbn.layers]
    joint = Cs.joint_state(m.joint_rbm)
    before = [_params(r) for r in m.image_idbn.layers]
    E.manual_seed(3)
    out = m.discriminative_step(x, y, 7, 10, lr_scale=0.5, head_lr_scale=0.25)
    assert E.get_rng().offset == 0                                      # no draws
    scal = [(r._lr_mom(7)[0] * 0.5, r._lr_mom(7)[1]) for r in m.image_idbn.layers]
    hl, hm = m.joint_rbm._lr_mom(7)
    calls = [c for c in double.calls if c[0] in ("discriminative_step", "label_backprop_step", "backprop_step", "label_step", "cd_step")]
    assert calls[0] == ("discriminative_step",)
    assert calls[1][:3] == ("label_backprop_step", (8, 20), 4) and calls[1][3] == pytest.approx(0.25 * hl, rel=1e-12) and calls[1][4:] == (hm, True, True)
    # (call, up rows, down rows, apply, want_v, want_h): the top image layer first, want_v everywhere but at the bottom
    assert calls[2:] == [("backprop_step", (8, 40), None, True, True, False), ("backprop_step", (8, 100), None, True, False, False)]
    want, j1 = D.discriminative_step(layers, joint, X[:8], 4, yi[:8], scal, (0.25 * hl, hm), head_wd=float(m.joint_rbm.weight_decay))
    assert set(out) == {"nll", "acc"} and out["nll"].dim() == 0 and out["acc"].dim() == 0 and out["nll"].dtype == torch.float64
    assert float(out["nll"]) == pytest.approx(want["nll"], abs=1e-5) and float(out["acc"]) == want["acc"]
    for r, s, b in zip(m.image_idbn.layers, layers, before):
        np.testing.assert_allclose(r.W.data.numpy(), s.W, rtol=0, atol=2e-6)
        np.testing.assert_allclose(r.hid_bias.data.numpy(), s.hid_bias, rtol=0, atol=2e-6)
        assert torch.equal(r.vis_bias.data, b[2]) and torch.equal(r.vb_m, b[5]) and not torch.equal(r.W.data, b[0])
    np.testing.assert_allclose(m.joint_rbm.W.data.numpy(), j1["W"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(m.joint_rbm.vis_bias.data.numpy(), j1["b"], rtol=0, atol=2e-6)
    # integer labels are the one-hot rows' argmax; a frozen head is only read; monitor=False evaluates nothing
    m2 = _model()
    n0 = len(double.calls)
    jb = _params(m2.joint_rbm)
    assert m2.discriminative_step(x, torch.from_numpy(yi[:8]), 7, 10, lr_scale=0.5, train_head=False, monitor=False) is None
    # discriminative_step, the two layers' forward (the engine's own call, never prop_up), then the head
    assert [c[0] for c in double.calls[n0:n0 + 4]] == ["discriminative_step", "forward", "forward", "label_backprop_step"]
    assert double.calls[n0 + 3][5:] == (False, False)
    assert all(torch.equal(p, q) for p, q in zip(jb, _params(m2.joint_rbm)))
    for r, s in zip(m2.image_idbn.layers, m.image_idbn.layers):
        assert torch.equal(r.W.data, s.W.data)                          # the layers' step does not depend on the head's update


def test_rbm_label_backprop_uses_the_schedule_of_train_epoch_labels(double):
    m = _model()
    jr = m.joint_rbm
    z = torch.rand(5, 20, generator=torch.Generator().manual_seed(2))
    gt = torch.tensor([0, 3, 1, 4, 2])                                   # 4 = K: invalid
    before = _params(jr)
    logp, err, pred = jr.label_backprop(z, gt, 7, 10, 4, lr_mult=0.25, apply=False)
    assert all(torch.equal(p, q) for p, q in zip(before, _params(jr)))
    assert logp.dtype == torch.float64 and torch.isnan(logp[3]) and not err[3].any() and tuple(err.shape) == (5, 20) and pred.dtype == torch.int32
    jr.label_backprop(z, gt, 7, 10, 4, lr_mult=0.25)
    lr, mom = jr._lr_mom(7)
    assert double.calls[-1][3] == pytest.approx(0.25 * lr, rel=1e-12) and double.calls[-1][4:] == (mom, True, True)
    assert not torch.equal(before[0], jr.W.data)


# ---- 4. finetune_discriminative -----------------------------------------------------------------------------------------------------
def test_finetune_discriminative_is_explicit_leaves_the_model_tied_and_fills_the_history_on_watched_epochs_only(double):
    m = _model()
    keys = sorted(m.__dict__)
    assert "discriminative_history" not in m.__dict__ and not m.image_idbn.is_untied()
    m.finetune_discriminative(3, log_every=2)
    assert not m.image_idbn.is_untied() and "gen_layers" not in m.image_idbn.__dict__
    assert sorted(m.__dict__) == sorted(keys + ["discriminative_history"])
    assert sum(c[0] == "discriminative_step" for c in double.calls) == 9
    assert [c[6] for c in double.calls if c[0] == "label_backprop_step"] == [True] * 3 + [False] * 3 + [True] * 3      # want_pred = watched
    hist = m.discriminative_history
    assert [h[0] for h in hist] == [0, 2] and all(len(h) == 3 and np.isfinite(h[1:]).all() and 0.0 <= h[2] <= 1.0 for h in hist)
    assert hist[1][1] < hist[0][1]
    m.finetune_discriminative(1)
    assert len(m.discriminative_history) == 2
    # an untied stack keeps its twins as they are
    m = _model()
    gen = m.image_idbn.untie()
    gb = [_params(g) for g in gen]
    m.finetune_discriminative(1)
    assert m.image_idbn.gen_layers is gen and all(torch.equal(p, q) for b, g in zip(gb, gen) for p, q in zip(b, _params(g)))


def test_a_model_that_is_never_fine_tuned_keeps_its_attributes_and_its_pickle(double):
    m = _model()
    dump = lambda: pickle.dumps({"image_idbn": m.image_idbn.layers, "joint_rbm": m.joint_rbm})
    keys, raw = sorted(m.__dict__), dump()
    m.image_idbn.represent(torch.from_numpy(Cs.toy_data()[0][:4]))
    assert sorted(m.__dict__) == keys and dump() == raw and not any(c[0] == "discriminative_step" for c in double.calls)


# ---- 5. data parallelism ------------------------------------------------------------------------------------------------------------
def test_data_parallel_raises(double, monkeypatch):
    m = _model()
    X, yi = Cs.toy_data()
    x, y = torch.from_numpy(X[:8]), torch.from_numpy(yi[:8])
    monkeypatch.setattr(E.dp, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        m.discriminative_step(x, y, 0, 1)
    with pytest.raises(NotImplementedError):
        m.finetune_discriminative(1)
    with pytest.raises(NotImplementedError):
        double.discriminative_step(m.image_idbn.layers, m.joint_rbm, x, 4, y, [(0.1, 0.5)] * 2, (0.1, 0.5))
    with pytest.raises(NotImplementedError):
        m.joint_rbm.label_backprop(torch.zeros(8, 20), y, 0, 1, 4)
    assert not any(c[0] in ("label_backprop_step", "backprop_step") for c in double.calls)


# ---- 6. ABI -------------------------------------------------------------------------------------------------------------------------
def test_export_is_declared_bound_and_in_the_built_library():
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    assert re.search(r"\bint\s+imdbn_rbm_label_backprop_step\s*\(", src)
    assert "#define IMDBN_ABI_VERSION 4" in src and native.ABI_VERSION == 4
    assert len(native.SIGNATURES["imdbn_rbm_label_backprop_step"][1]) == 16
    assert hasattr(native.lib(), "imdbn_rbm_label_backprop_step")
    from imdbn.engine.hip_engine import HipEngine
    from imdbn.models import RBM, iMDBN
    assert hasattr(HipEngine, "label_backprop_step") and hasattr(HipEngine, "discriminative_step") and hasattr(RBM, "label_backprop")
    assert hasattr(iMDBN, "discriminative_step") and hasattr(iMDBN, "finetune_discriminative")
