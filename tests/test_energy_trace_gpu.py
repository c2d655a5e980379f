"""GPU: imdbn.utils.energy_utils tracing on the engine (imdbn_energy_trace) -- the reference's recorded traces
(energy_trace_small.npz), a row inside a panel against the same row alone, the free energies against the stacked engine call
and the fp64 oracle, odd shapes and the full joint size against the oracle, the step function, invalid arguments.

Tolerances are the ones the existing GPU tests use for the same kinds of quantity: 1e-5 absolute for label probabilities and
their L1 change (test_cross_trace_gpu.py), 1e-5 relative Frobenius for free energies (test_parity_gpu.py
test_free_energy_matches_oracle).  Derived, not new: ``deltaF_pred`` and ``margin_energy`` are differences of two free
energies, each within 1e-5 relative, so they are held to 2e-5 * max|F| absolute; ``fe_top1`` / ``fe_gap`` are entries of
softmax(-F), whose derivative with respect to any difference of two F is at most 1/2, so they are held to half of that."""
import numpy as np
import pytest
import torch

import energy_oracle as EO
import trace_oracle as TO
from golden_utils import Fixture, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_TOL = 1e-5
F_REL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    yield E.get_hip_engine()


@pytest.fixture(scope="module")
def fx():
    return Fixture("energy_trace_small.npz")


class _Model:
    pass


def _rbm(W, hb, vb, groups=None, pitch=None):
    from imdbn.models import RBM
    r = RBM(W.shape[0], W.shape[1], 0.1, 1e-4, 0.5, softmax_groups=groups).to(DEV)
    if pitch is not None:                                   # rows of `pitch` floats, the padding poisoned
        big = torch.full((W.shape[0], pitch), float("nan"), device=DEV)
        r.W.data = big[:, :W.shape[1]]
    r.W.data.copy_(torch.from_numpy(np.ascontiguousarray(W)))
    r.hid_bias.data.copy_(torch.from_numpy(hb)); r.vis_bias.data.copy_(torch.from_numpy(vb))
    return r


@pytest.fixture(scope="module")
def small():
    from imdbn.models import iDBN
    from torch.utils.data import DataLoader, TensorDataset
    w, X, Y = TO.small_model_arrays()
    m = _Model()
    m.device = torch.device(DEV)
    idbn = iDBN.__new__(iDBN)
    idbn.device = m.device
    idbn.layers = [_rbm(w[f"img{i}_W"], w[f"img{i}_hid_bias"], w[f"img{i}_vis_bias"]) for i in range(2)]
    m.image_idbn = idbn
    m.joint_rbm = _rbm(w["joint_W"], w["joint_hid_bias"], w["joint_vis_bias"], [(20, 28)])
    m.Dz_img, m.num_labels = 20, 8
    m.val_loader = DataLoader(TensorDataset(torch.from_numpy(X), torch.from_numpy(Y)), batch_size=8, shuffle=False)
    m.wandb_run = None
    return m, w, X, Y


def _close(a, b, tol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    print(f"{what}: max err {err.max() if err.size else 0.0:.3g} (tol {tol:.3g})")
    assert err.size == 0 or err.max() <= tol, f"{what}: max err {err.max():.3g} > {tol:.3g}"


def _check_case(case, fx, pre, i, keys):
    """A reference-style dict against row i of a recorded group."""
    ints, fl = fx[pre + "ints"][i], fx[pre + "floats"][i]
    assert list(case) == keys
    assert [case["steps_to_converge"], case["kstar"], case["predT"]] == ints[:3].tolist(), (pre, i)
    assert case["gt"] == (int(ints[3]) if ints[3] >= 0 else None)
    n = min(int(ints[0]), fx.meta["steps"])
    fmax = float(np.abs(fx[pre + "F"][i]).max())
    for k in ("p_top1", "p_top2", "p_gap"):
        assert len(case[k]) == n
        _close(case[k], fx[pre + k][i, :n], P_TOL, f"{pre}{i} {k}")
    if ints[3] >= 0:
        _close(case["p_gt"], fx[pre + "p_gt"][i, :n], P_TOL, f"{pre}{i} p_gt")
    else:
        assert case["p_gt"] is None
    _close(case["deltaF_pred_traj"], fx[pre + "deltaF_pred_traj"][i, :n], 2 * F_REL * fmax, f"{pre}{i} deltaF_pred_traj")
    _close([case["margin_energy"], case["deltaF_pred_final"]], fl[[0, 3]], 2 * F_REL * fmax, f"{pre}{i} margin_energy, deltaF_pred_final")
    _close([case["fe_top1_final"], case["fe_gap_final"]], fl[[1, 2]], F_REL * fmax, f"{pre}{i} fe_top1, fe_gap")
    _close([case["p_top1_final"], case["p_gap_final"]], fl[[4, 5]], P_TOL, f"{pre}{i} p_top1_final, p_gap_final")


def test_b1_wrapper_against_the_reference(fx, small):
    from imdbn.utils import energy_utils as EU
    m, _, _, _ = small
    keys = fx.meta["dict_keys"]
    m._fixed_val_case = None
    case = EU.run_and_log_fixed_case(m, epoch=0)
    assert torch.equal(m._fixed_val_case[0], torch.from_numpy(fx["fixed_img"]))
    _check_case(case, fx, "fx_", 0, keys)
    img, lbl = torch.from_numpy(fx["fixed_img"]).to(DEV), torch.from_numpy(fx["fixed_lbl"]).to(DEV)
    _check_case(EU.trace_single_img2txt(m, img, None), fx, "nl_", 0, keys)
    gi, gl = torch.from_numpy(fx["gap_img"]).to(DEV), torch.from_numpy(fx["gap_lbl"]).to(DEV)
    g = EU.trace_single_img2txt(m, gi, gl, gap_thresh=fx.meta["gap_small"])
    _check_case(g, fx, "gp_", 0, keys)
    assert g["predT"] != g["kstar"] and g["steps_to_converge"] <= fx.meta["steps"]         # converged through the gap branch
    assert EU.trace_single_img2txt(m, gi, gl)["steps_to_converge"] == fx.meta["steps"] + 1   # ... and only through it
    assert_close(EU.class_free_energies(m.joint_rbm, m.image_idbn.represent(img).clamp(1e-6, 1 - 1e-6), 8, 20).cpu().numpy(),
                 fx["fx_F"], F_REL, "class_free_energies vs the recording")


def test_panel_against_the_reference(fx, small):
    from imdbn.utils import energy_utils as EU
    m, _, _, _ = small
    T = fx.meta["steps"]
    imgs, lbls = torch.from_numpy(fx["panel_img"]).to(DEV), torch.from_numpy(fx["panel_lbl"]).to(DEV)
    o = EU.trace_img2txt_energy_batch(m, imgs, lbls, steps=T)
    ints = fx["pn_ints"]
    assert sorted(set(ints[:, 0].tolist())) == [3, 4, T + 1]
    for k, c in (("steps", 0), ("kstar", 1), ("predT", 2), ("gt", 3)):
        np.testing.assert_array_equal(o[k].cpu().numpy(), ints[:, c], err_msg=k)
    assert_close(o["F"].cpu().numpy(), fx["pn_F"], F_REL, "F vs the recording")
    h = EU._to_host(o)
    for i in range(len(ints)):
        _check_case(EU._case_dict(h, i, T, 8), fx, "pn_", i, fx.meta["dict_keys"])
        n = min(int(ints[i, 0]), T)
        _close(o["l1"][i, :n].cpu().numpy(), fx["pn_l1"][i, :n], P_TOL, f"pn_{i} l1")
        # k1 at the recorded steps: the argmax that deltaF_pred and predT come from
        assert int(o["k1"][i, n - 1]) == int(ints[i, 2])


def test_rows_alone_equal_rows_in_a_panel_and_runs_repeat(fx, small, _native):
    from imdbn.utils import energy_utils as EU
    m, _, _, _ = small
    T = fx.meta["steps"]
    imgs, lbls = torch.from_numpy(fx["panel_img"]).to(DEV), torch.from_numpy(fx["panel_lbl"]).to(DEV)
    a = EU.trace_img2txt_energy_batch(m, imgs, lbls, steps=T)
    b = EU.trace_img2txt_energy_batch(m, imgs, lbls, steps=T)
    keys = [k for k in a if a[k] is not None]
    for k in keys:
        assert torch.equal(a[k], b[k]), f"{k}: two runs differ"
    for i in (0, 5, len(imgs) - 1):
        one = EU.trace_img2txt_energy_batch(m, imgs[i:i + 1], lbls[i:i + 1], steps=T)
        for k in keys:
            assert torch.equal(one[k][0], a[k][i]), f"row {i} {k}: alone != in the panel"
    # the same at the joint size, a row in the middle of a block and of the panel, both Wy paths
    g = np.random.Generator(np.random.PCG64(21))
    for Dz, K, H in ((500, 32, 256), (45, 200, 700)):
        r, z, _ = _random_joint(g, Dz, K, H, 131)
        full = _native.energy_trace(r, z, K, 8)
        for i in (0, 66, 130):
            one = _native.energy_trace(r, z[i:i + 1].clone(), K, 8)
            for k in ("p_top1", "p_top2", "deltaF_pred", "l1", "k1", "steps", "kstar", "predT", "margin_energy", "fe_top1", "fe_gap", "F"):
                assert torch.equal(one[k][0], full[k][i]), f"{(Dz, K, H)} row {i} {k}: alone != in the panel"


def _random_joint(g, Dz, K, H, N, pitch=None, strided_z=False, wscale=0.15):
    V = Dz + K
    W = (g.standard_normal((V, H)) * wscale).astype(np.float32)
    hb = (g.standard_normal(H) * 0.2).astype(np.float32)
    vb = np.concatenate([g.standard_normal(Dz) * 0.2, g.standard_normal(K) * 1.5]).astype(np.float32)
    r = _rbm(W, hb, vb, [(Dz, V)], pitch=pitch)
    zn = g.random((N, Dz), dtype=np.float32) * 0.98 + 0.01
    if strided_z:
        big = torch.full((N, Dz + 11), float("nan"), device=DEV)
        z = big[:, 5:5 + Dz]
        z.copy_(torch.from_numpy(zn))
    else:
        z = torch.from_numpy(zn).to(DEV)
    return r, z, (W, hb, vb, zn)


def _against_oracle(eng, g, Dz, K, H, N, steps, pitch=None, strided_z=False, with_gt=True, with_y0=False, wscale=0.15, **kw):
    r, z, (W, hb, vb, zn) = _random_joint(g, Dz, K, H, N, pitch, strided_z, wscale)
    gt = (np.arange(N) * 7) % K if with_gt else None
    y0 = None
    if with_y0:
        y0 = g.random((N, K), dtype=np.float32) + 0.05
        y0 = (y0 / y0.sum(1, keepdims=True)).astype(np.float32)
    o = eng.energy_trace(r, z, K, steps, gt=torch.from_numpy(gt).to(DEV) if with_gt else None,
                         y_start=torch.from_numpy(y0).to(DEV) if with_y0 else None, want_y=True, **kw)
    torch.cuda.synchronize()
    if pitch is not None:
        assert torch.isnan(torch.as_strided(r.W.data, (Dz + K, pitch), (pitch, 1))[:, H:]).all(), "the kernel wrote into the row padding"
    e = EO.trace(W, hb, vb, zn, K, steps, gt=gt, y0=y0, **kw)
    tag = f"Dz={Dz} K={K} H={H} N={N}"
    fmax = float(np.abs(e["F"]).max())
    assert_close(o["F"].cpu().numpy(), e["F"], F_REL, f"{tag} F")
    for k, ek in (("p_top1", "p1"), ("p_top2", "p2"), ("l1", "l1")) + ((("p_gt", "p_gt"),) if with_gt else ()):
        _close(o[k].cpu(), e[ek], P_TOL, f"{tag} {k}")
    _close(o["y"].cpu(), e["y"], P_TOL, f"{tag} final y")
    _close(o["margin_energy"].cpu(), e["margin_energy"], 2 * F_REL * fmax, f"{tag} margin_energy")
    _close(o["fe_top1"].cpu(), e["fe_top1"], F_REL * fmax, f"{tag} fe_top1")
    _close(o["fe_gap"].cpu(), e["fe_gap"], F_REL * fmax, f"{tag} fe_gap")
    # decisions: exact wherever the oracle's own decision has 1e-5 of room (the bound the recorded fixture rows were chosen by)
    roomy = e["room"] > 1e-5
    print(f"{tag}: {int((~roomy).sum())} of {N} rows decided within 1e-5 of a threshold; converged {int((e['conv'] <= steps).sum())}")
    assert (~roomy).sum() <= max(1, N // 4)
    for k, ek in (("steps", "conv"), ("kstar", "kstar"), ("predT", "predT")):
        got = o[k].cpu().numpy()
        assert (got[roomy] == e[ek][roomy]).all(), (tag, k, np.nonzero(roomy & (got != e[ek]))[0])
    k1, dF = o["k1"].cpu().numpy(), o["deltaF_pred"].cpu().numpy()
    for b in np.nonzero(roomy)[0]:
        n = min(int(e["conv"][b]), steps)
        assert (k1[b, :n] == e["k1"][b, :n]).all(), (tag, "k1", b)
        _close(dF[b, :n], e["dF"][b, :n], 2 * F_REL * fmax, f"{tag} row {b} deltaF_pred")
    return o


ODD = [
    dict(Dz=20, K=8, H=16, N=1, steps=12),
    dict(Dz=37, K=2, H=50, N=67, steps=12),                          # K = 2, Dz not a multiple of 32
    dict(Dz=45, K=200, H=700, N=9, steps=6, wscale=0.03),            # Wy from global memory (small weights: with 200 labels the
                                                                     # sigmoids of larger logits saturate and the top two tie within 1e-5)
    dict(Dz=33, K=3, H=1100, N=5, steps=6),                          # base / h rows from global memory, Wy in LDS
    dict(Dz=40, K=40, H=1100, N=6, steps=6, with_y0=True),           # both from global memory; a start distribution
    dict(Dz=70, K=10, H=130, N=33, steps=12, pitch=133, strided_z=True, with_gt=False),      # padded, unaligned W pitch; strided z
    dict(Dz=64, K=32, H=256, N=16, steps=12, pitch=260, gap_thresh=0.01, eps_l1=1e-2, stable_steps=2),
]


@pytest.mark.parametrize("case", ODD, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_odd_shapes_against_the_oracle(case, _native):
    _against_oracle(_native, np.random.Generator(np.random.PCG64(100 + case["Dz"])), **case)


def test_joint_size_panel_against_the_oracle(_native):
    """532 <-> 256 with K = 32, N = 1024, 30 steps."""
    o = _against_oracle(_native, np.random.Generator(np.random.PCG64(12)), Dz=500, K=32, H=256, N=1024, steps=30)
    assert o["steps"].min() >= 1 and o["steps"].max() <= 31


def test_free_energies_against_the_stacked_engine_call(_native):
    from imdbn.utils import energy_utils as EU
    g = np.random.Generator(np.random.PCG64(8))
    for Dz, K, H, N in ((500, 32, 256, 64), (37, 5, 90, 19)):
        r, z, (W, hb, vb, zn) = _random_joint(g, Dz, K, H, N)
        F = _native.energy_trace(r, z, K, 1)["F"].cpu().numpy()
        assert_close(F, EU.class_free_energies(r, z, K, Dz).cpu().numpy(), F_REL, "F vs class_free_energies")
        assert_close(F, EO.class_free_energies(W.astype(np.float64), hb.astype(np.float64), vb.astype(np.float64), zn.astype(np.float64), K),
                     F_REL, "F vs the oracle")


def test_deterministic_step(_native):
    from imdbn import engine as E
    from imdbn.utils import energy_utils as EU
    g = np.random.Generator(np.random.PCG64(4))
    Dz, K, H, N = 500, 32, 256, 40
    r, z, (W, hb, vb, zn) = _random_joint(g, Dz, K, H, N)
    y0 = g.random((N, K), dtype=np.float32) + 0.05
    y0 = (y0 / y0.sum(1, keepdims=True)).astype(np.float32)
    v = torch.cat([z, torch.from_numpy(y0).to(DEV)], 1)
    out = EU._deterministic_img2txt_step(r, v, Dz, K)
    one = _native.energy_trace(r, z, K, 1, y_start=v[:, Dz:], want_y=True)
    assert torch.equal(out[:, :Dz], z) and torch.equal(out[:, Dz:], one["y"])
    want = EO.step(W.astype(np.float64), hb.astype(np.float64), vb.astype(np.float64), np.concatenate([zn, y0], 1).astype(np.float64), Dz, K)
    _close(out.cpu(), want, P_TOL, "one step vs the oracle")
    # the composed forms: clamp instead of softmax, sampled h, sampled label
    p = EO.sigmoid(EO.sigmoid(np.concatenate([zn, y0], 1).astype(np.float64) @ W + hb) @ W.T.astype(np.float64) + vb)[:, Dz:]
    _close(EU._deterministic_img2txt_step(r, v, Dz, K, softmax_y=False)[:, Dz:].cpu(), np.clip(p, 1e-6, 1 - 1e-6), P_TOL, "softmax_y=False")
    with E.use_rng(E.PhiloxRng(seed=5)):
        sv = EU._deterministic_img2txt_step(r, v, Dz, K, sample_v=True)
        sh = EU._deterministic_img2txt_step(r, v, Dz, K, sample_h=True)
    assert torch.equal(sv[:, :Dz], z) and torch.equal(sh[:, :Dz], z)
    lab = sv[:, Dz:]
    assert ((lab == 0) | (lab == 1)).all() and (lab.sum(1) == 1).all()
    assert torch.isfinite(sh).all() and not torch.equal(sh[:, Dz:], out[:, Dz:])
    _close(sh[:, Dz:].sum(1).cpu(), np.ones(N), P_TOL, "sample_h rows are distributions")


def test_invalid_arguments_raise(_native):
    from imdbn.engine import EngineError
    g = np.random.Generator(np.random.PCG64(2))
    r = _rbm((g.standard_normal((330, 20)) * 0.1).astype(np.float32), np.zeros(20, np.float32), np.zeros(330, np.float32))
    with pytest.raises(EngineError, match="K = 257"):
        _native.energy_trace(r, torch.rand(4, 30, device=DEV), 257, 3)                   # K > 256
    r, z, _ = _random_joint(g, 30, 8, 20, 4)
    with pytest.raises(EngineError):
        _native.energy_trace(r, z, 9, 3)                     # Dz + K > V
    with pytest.raises(EngineError):
        _native.energy_trace(r, z, 8, 0)                     # steps < 1
    with pytest.raises(EngineError):
        _native.energy_trace(r, z, 1, 3)                     # K < 2


def test_energy_panel_runs_the_fixed_panel(small):
    from imdbn.utils import conditional_steps as CS, energy_utils as EU

    class Run:
        def __init__(self):
            self.logged = []

        def log(self, d):
            self.logged.append(d)

    m, _, _, _ = small
    m._fixed_val_panel = None
    m.wandb_run = Run()
    try:
        p = EU.run_and_log_energy_panel(m, epoch=3, per_class=2)
    finally:
        run, m.wandb_run = m.wandb_run, None
    imgs, lbls = CS.build_or_get_fixed_val_panel(m, per_class=2)
    assert len(p["steps"]) == imgs.size(0) == 16
    singles = [EU.trace_single_img2txt(m, imgs[i:i + 1], lbls[i:i + 1]) for i in range(16)]
    assert p["steps"] == [c["steps_to_converge"] for c in singles]
    assert p["stats"] == CS._steps_stats(p["steps"], 30)[0]
    assert p["p_top1_final_mean"] == float(np.mean([c["p_top1_final"] for c in singles]))
    assert p["acc_kstar"] == float(np.mean([c["kstar"] == c["gt"] for c in singles]))
    assert len(run.logged) == 1 and run.logged[0]["epoch"] == 3 and "case/panel/summary" in run.logged[0]
