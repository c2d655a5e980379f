"""GPU: imdbn.utils.conditional_steps on the engine -- the reference's recorded traces (cross_trace_small.npz), batched against
per-row calls, tracing as a pure observer of the chain kernel, the decode error at full size, and a full-size panel against the
fp64 oracle."""
import numpy as np
import pytest
import torch

import trace_oracle as TO
from golden_utils import Fixture
from oracle.draws import DrawStream, PhiloxStream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    yield E.get_hip_engine()


@pytest.fixture(scope="module")
def fx():
    return Fixture("cross_trace_small.npz")


class _Model:
    pass


def _rbm(W, hb, vb, groups=None):
    from imdbn.models import RBM
    r = RBM(W.shape[0], W.shape[1], 0.1, 1e-4, 0.5, softmax_groups=groups).to(DEV)
    r.W.data.copy_(torch.from_numpy(np.ascontiguousarray(W)))
    r.hid_bias.data.copy_(torch.from_numpy(hb)); r.vis_bias.data.copy_(torch.from_numpy(vb))
    return r


def _model(w, Dz, K, zcm=None, val=None):
    from imdbn.models import iDBN
    m = _Model()
    m.device = torch.device(DEV)
    idbn = iDBN.__new__(iDBN)
    idbn.device = m.device
    n = len([k for k in w if k.startswith("img") and k.endswith("_W")])
    idbn.layers = [_rbm(w[f"img{i}_W"], w[f"img{i}_hid_bias"], w[f"img{i}_vis_bias"]) for i in range(n)]
    m.image_idbn = idbn
    m.joint_rbm = _rbm(w["joint_W"], w["joint_hid_bias"], w["joint_vis_bias"], [(Dz, Dz + K)])
    m.Dz_img, m.num_labels = Dz, K
    if zcm is not None:
        m.z_class_mean = torch.from_numpy(zcm).to(DEV)
    m.val_loader = val
    m.wandb_run = None
    return m


@pytest.fixture(scope="module")
def small():
    from torch.utils.data import DataLoader, TensorDataset
    w, X, Y = TO.small_model_arrays()
    val = DataLoader(TensorDataset(torch.from_numpy(X), torch.from_numpy(Y)), batch_size=8, shuffle=False)
    return w, val


class _Tape:
    """DrawStream re-created from a seed, its recorded categorical indices, then filler (it only feeds steps after convergence)."""

    def __init__(self, seed, cat=()):
        self.s, self.cat = DrawStream(seed), list(cat)

    def uniform(self, shape):
        return self.s.uniform(shape)

    def normal(self, shape):
        return self.s.normal(shape)

    def categorical(self, probs):
        B = probs.shape[0]
        out = np.array([self.cat.pop(0) if self.cat else 0 for _ in range(B)], np.int64)
        return out


def _replay(seed, cat=()):
    from imdbn import engine as E
    return E.use_rng(E.ReplayRng(_Tape(seed, cat)))


def _close(a, b, tol, what, rel=False):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b) / (np.abs(b) if rel else 1.0)
    assert err.size == 0 or err.max() <= tol, f"{what}: max err {err.max():.3g}"


def _check_i2t(out, fx, pre):
    sc = fx[pre + "scalars"]
    assert out["steps_to_converge"] == int(sc[0]) and out["predT"] == int(sc[1]), pre
    assert len(out["p_top1"]) == len(fx[pre + "p_top1"]) == len(out["l1"]) == len(out["top1_idx"])
    assert out["top1_idx"] == fx[pre + "top1_idx"].tolist() and out["top2_idx"] == fx[pre + "top2_idx"].tolist()
    for k in ("p_top1", "p_top2", "p_gap", "l1"):
        _close(out[k], fx[pre + k], 1e-5, pre + k)
    if int(sc[2]) >= 0:
        assert out["gt_idx"] == int(sc[2])
        _close(out["p_gt"], fx[pre + "p_gt"], 1e-5, pre + "p_gt")
    else:
        assert out["p_gt"] is None and out["gt_idx"] is None


def _check_t2i(out, fx, pre):
    assert out["steps_to_converge"] == int(fx[pre + "steps"]), pre
    _close(out["z_l2"], fx[pre + "z_l2"], 1e-5, pre + "z_l2")
    _close(out["image_mse"], fx[pre + "image_mse"], 1e-4, pre + "image_mse", rel=True)
    _close(out["best_mse"], fx[pre + "best_mse"], 1e-4, pre + "best_mse", rel=True)


def test_b1_wrappers_against_the_reference(fx, small):
    from imdbn.utils import conditional_steps as CS
    w, val = small
    T = fx.meta["max_steps"]
    m = _model(w, 20, 8, w["z_class_mean"], val)
    img, lbl = torch.from_numpy(fx["fixed_img"]).to(DEV), torch.from_numpy(fx["fixed_lbl"]).to(DEV)
    with _replay(fx.meta["seeds"]["fixed"]):
        a, b = CS.run_and_log_cross_fixed_case(m, epoch=0, max_steps=T)
    assert torch.equal(m._fixed_val_case[0], torch.from_numpy(fx["fixed_img"]))
    _check_i2t(a, fx, "fx_i2t_"); _check_t2i(b, fx, "fx_t2i_")
    with _replay(fx.meta["seeds"]["gap_i2t_"]):
        _check_i2t(CS.trace_img2txt_cross(m, img, None, max_steps=T, gap_thresh=0.02), fx, "gap_i2t_")
    for pre, fn in (("smp_i2t_", CS.trace_img2txt_cross), ("smp_t2i_", CS.trace_txt2img_cross)):
        with _replay(fx.meta["seeds"][pre], fx[pre + "cat"].tolist()):
            out = fn(m, img, lbl, max_steps=T, sample_h=True, sample_v=True)
        (_check_i2t if "i2t" in pre else _check_t2i)(out, fx, pre)
    _check_t2i(CS.trace_txt2img_cross(m, img, lbl, max_steps=T, ema_beta=0.3), fx, "ema_t2i_")
    m2 = _model(w, 20, 8, None, val)
    _check_t2i(CS.trace_txt2img_cross(m2, img, lbl, max_steps=T), fx, "nozcm_t2i_")


def test_panel_and_z_mismatch_against_the_reference(fx, small):
    from imdbn.utils import conditional_steps as CS
    w, val = small
    T = fx.meta["max_steps"]
    m = _model(w, 20, 8, w["z_class_mean"], val)
    with _replay(fx.meta["seeds"]["panel"]):
        p = CS.run_and_log_cross_panel(m, epoch=0, per_class=2, max_steps=T)
    assert p["img2txt"]["steps"] == fx["panel_i2t_steps"].tolist()
    assert p["txt2img"]["steps"] == fx["panel_t2i_steps"].tolist()
    ref = fx.meta["panel"]
    assert p["img2txt"]["stats"] == ref["img2txt"]["stats"] and p["txt2img"]["stats"] == ref["txt2img"]["stats"]
    _close(p["img2txt"]["p1_mean"], ref["img2txt"]["p1_mean"], 1e-5, "p1_mean")
    _close(p["img2txt"]["gap_mean"], ref["img2txt"]["gap_mean"], 1e-5, "gap_mean")
    _close(p["txt2img"]["best_mse_mean"], ref["txt2img"]["best_mse_mean"], 1e-4, "best_mse_mean", rel=True)

    class Run:
        def __init__(self):
            self.logged = []

        def log(self, d):
            self.logged.append(d)

    assert CS.run_and_log_z_mismatch_check(m, epoch=0, max_steps=T) is None          # no wandb_run: nothing, no draws
    m.wandb_run = Run()
    with _replay(fx.meta["seeds"]["zcheck"]):
        CS.run_and_log_z_mismatch_check(m, epoch=0, max_steps=T)
    assert len(m.wandb_run.logged) == len(fx.meta["zcheck"])
    for got, exp in zip(m.wandb_run.logged, fx.meta["zcheck"]):
        assert sorted(got) == sorted(exp)
        for k, v in exp.items():
            if isinstance(v, dict):
                for kk in v:
                    _close(got[k][kk], v[kk], 1e-5, k + "/" + kk)
            else:
                _close(got[k], v, 1e-5, k)


def test_batched_rows_equal_the_b1_calls(fx, small):
    from imdbn import engine as E
    from imdbn.utils import conditional_steps as CS
    w, val = small
    T = fx.meta["max_steps"]
    m = _model(w, 20, 8, w["z_class_mean"], val)
    imgs, lbls = torch.from_numpy(fx["panel_img"]).to(DEV), torch.from_numpy(fx["panel_lbl"]).to(DEV)
    B = imgs.size(0)
    u = DrawStream(77).uniform((B, 28))
    with _replay(77):
        i2t, t2i = CS.trace_cross_panel_batch(m, imgs, lbls, max_steps=T)
    for i in range(B):
        with E.use_rng(E.ReplayRng(type("U", (), {"uniform": lambda self, s, i=i: u[i:i + 1]})())):
            a = CS.trace_img2txt_cross_batch(m, imgs[i:i + 1], lbls[i:i + 1], max_steps=T)
        b = CS.trace_txt2img_cross_batch(m, imgs[i:i + 1], lbls[i:i + 1], max_steps=T)
        for k in ("steps", "pred", "k1", "k2"):
            assert torch.equal(a[k][0], i2t[k][i]), (i, k)
        for k in ("p_top1", "p_top2", "p_gt", "l1"):
            _close(a[k][0].cpu(), i2t[k][i].cpu(), 1e-6, f"row {i} {k}")
        assert torch.equal(b["steps"][0], t2i["steps"][i])
        for k in ("z_l2", "image_mse", "best_mse"):
            _close(b[k][0].cpu(), t2i[k][i].cpu(), 1e-6, f"row {i} {k}", rel=(k != "z_l2"))


def _slot_trace(K, B=5, T=6):
    """A label trace [T + 1, B, K] on the grid 2^-10 -- every fp32 sum of it is exact in any order -- and the truth labels, with, where K
    allows: row 0 constant with a lone maximum at gt = K - 1 (converges); row 1 the maximum tied between columns 0 and 64 (one lane, two
    slots), the rest changing; row 2 constant with the maximum tied between columns 63 and 64 (never a gap); row 3 a lone maximum and
    second place tied between columns 5 and K - 2, constant from step 3 on; row 4 (alone in the second block) changing throughout."""
    g = np.random.Generator(np.random.PCG64(40 + K))
    tr = g.integers(0, 512, (T + 1, B, K)).astype(np.float32) / 1024          # [0, 0.5)
    gt = g.integers(0, K, B).astype(np.int32)
    tr[:, 0] = tr[0, 0]; tr[:, 0, K - 1] = 0.875; gt[0] = K - 1
    if K > 64:
        tr[:, 1, 0] = tr[:, 1, 64] = 0.75
        tr[:, 2] = tr[0, 2]; tr[:, 2, 63] = tr[:, 2, 64] = 0.75
    if K > 2:
        tr[3:, 3] = tr[3, 3]
        tr[:, 3, 1] = 0.875; tr[:, 3, 5] = tr[:, 3, K - 2] = 0.625
    return tr, gt


@pytest.mark.parametrize("K", [2, 64, 65, 256])
def test_label_scan_slots_against_the_oracle(K):
    """imdbn_trace_label_scan alone, across the label slots (K = 2; one full slot; one label in the second; all four full), every
    output equal to the numpy oracle's.  The thresholds are dyadic like the trace, so no decision is a matter of rounding."""
    from imdbn import engine as E
    T, thr = 6, dict(eps_l1=2.0 ** -4, stable_steps=3, gap_thresh=0.25)
    tr, gt = _slot_trace(K, T=T)
    ys = tr[1:].astype(np.float64)
    r, steps, pred, _ = TO.label_scan(tr[0].astype(np.float64), ys, gt=gt, **thr)
    # the planted cases are there
    p1, p2 = r["p1"][None], r["p2"][None]                                   # [1, B, T] against ys [K, B, T]
    yk = ys.transpose(2, 1, 0)
    assert (steps <= T).any() and (steps == T + 1).any() and steps[0] <= T and gt[0] == K - 1
    if K > 64:
        at_k1 = np.arange(K)[:, None, None] == r["k1"][None]
        assert (np.roll(at_k1, 64, 0) & (yk == p1))[64:].any(), "no maximum tied across two slots of one lane"
        assert ((r["k1"] == 63) & (r["k2"] == 64) & (r["p1"] == r["p2"])).any(), "no maximum tied between columns 63 and 64"
    if K > 2:
        assert (((yk == p2).sum(0) >= 2) & (r["p2"] < r["p1"])).any(), "no tie for second place"
    o = E.get_hip_engine().label_scan(torch.from_numpy(tr).to(DEV), torch.from_numpy(gt).to(DEV), **thr)
    for k, ref in (("p_top1", r["p1"]), ("p_top2", r["p2"]), ("k1", r["k1"]), ("k2", r["k2"]), ("p_gt", r["p_gt"]), ("l1", r["l1"]),
                   ("steps", steps), ("pred", pred)):
        got = o[k].cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got.astype(np.float64), ref.astype(np.float64)), (K, k, got, ref)


def test_tracing_only_observes_the_chain(small):
    """chain_traced vs chain_pair with Philox and sampled steps, on the chain kernel and one launch per half step."""
    from imdbn import engine as E
    from imdbn.models.rbm import _step
    eng = E.get_hip_engine()
    g = np.random.Generator(np.random.PCG64(3))
    V, H, Dz, K, B = 532, 256, 500, 32, 40
    W = (g.standard_normal((V, H)) * 0.05).astype(np.float32)
    r = _rbm(W, (g.standard_normal(H) * 0.1).astype(np.float32), (g.standard_normal(V) * 0.1).astype(np.float32), [(Dz, Dz + K)])
    vk = torch.from_numpy(g.random((B, V), dtype=np.float32)).to(DEV)
    ma, mb = torch.zeros(B, V, device=DEV), torch.zeros(B, V, device=DEV)
    ma[:, :Dz] = 1; mb[:, Dz:] = 1
    steps = [_step(sample_h=True, vmode=1, clamp=True)] * 12
    a = {"v_known": vk, "mask": ma, "steps": steps}
    b = {"v_known": vk, "mask": mb, "steps": steps}
    traces = []
    for opt in (0, 1):
        eng.set_option("no_chain_kernel", opt)
        try:
            ra, rb = E.PhiloxRng(seed=9), E.PhiloxRng(seed=9)
            va, vb = eng.chain_pair(r, a, b, ra)
            (ta_v, ta), (tb_v, tb) = eng.chain_traced(r, dict(a, trace=(Dz, V, True)), dict(b, trace=(0, Dz, False)), rb)
            assert ra.offset == rb.offset
            assert torch.equal(va, ta_v) and torch.equal(vb, tb_v), f"no_chain_kernel={opt}"
            rc, rd = E.PhiloxRng(seed=9), E.PhiloxRng(seed=9)
            vc = eng.chain(r, vk, ma, steps, rc)
            ((td_v, _),) = eng.chain_traced(r, dict(a, trace=(Dz, V, True)), None, rd)
            assert rc.offset == rd.offset and torch.equal(vc, td_v)
            assert ta.shape == (13, B, K) and tb.shape == (12, B, Dz)
            traces.append((ta.cpu(), tb.cpu()))
        finally:
            eng.set_option("no_chain_kernel", 0)
    _close(traces[0][0], traces[1][0], 1e-6, "label trace: chain kernel vs per-launch")
    _close(traces[0][1], traces[1][1], 1e-6, "code trace: chain kernel vs per-launch")


def test_decode_sqerr_full_size_multi_chunk():
    from imdbn import engine as E
    eng = E.get_hip_engine()
    g = np.random.Generator(np.random.PCG64(5))
    sizes = [10000, 1500, 500]
    layers = [_rbm((g.standard_normal((sizes[i], sizes[i + 1])) / np.sqrt(sizes[i + 1])).astype(np.float32),
                   np.zeros(sizes[i + 1], np.float32), (g.standard_normal(sizes[i]) * 0.3).astype(np.float32)) for i in range(2)]
    T, B = 70, 128
    z = torch.from_numpy(g.random((T * B, 500), dtype=np.float32)).to(DEV)
    img = torch.from_numpy((g.random((B, 10000)) < 0.2).astype(np.float32)).to(DEV)
    rows = torch.arange(B, dtype=torch.int32, device=DEV).repeat(T)
    a = eng.decode_sqerr(layers, z, img, rows)
    b = eng.decode_sqerr(layers, z, img, rows)
    assert torch.equal(a, b), "decode error not deterministic"
    ref = torch.empty(T * B, device=DEV)
    for s in range(0, T * B, 1280):
        cur = z[s:s + 1280]
        for rbm in reversed(layers):
            cur = rbm.backward(cur)
        ref[s:s + 1280] = ((cur - img[rows[s:s + 1280].long()]) ** 2).mean(1)
    _close(a.cpu(), ref.cpu(), 1e-6, "decode_sqerr vs decode", rel=True)


def test_full_size_panel_against_the_oracle():
    """config-3 shapes: [10000, 1500, 500] image stack, 532 <-> 256 joint with K = 32, N = 128, 70 steps, both directions;
    the initial uniforms from the Philox twin."""
    from imdbn import engine as E
    from imdbn.utils import conditional_steps as CS
    g = np.random.Generator(np.random.PCG64(12))
    sizes, Dz, K, JH, N, T = [10000, 1500, 500], 500, 32, 256, 128, 70
    w = {}
    for i in range(2):
        w[f"img{i}_W"] = (g.standard_normal((sizes[i], sizes[i + 1])) * (2.0 / np.sqrt(sizes[i]))).astype(np.float32)
        w[f"img{i}_hid_bias"] = (g.standard_normal(sizes[i + 1]) * 0.5).astype(np.float32)
        w[f"img{i}_vis_bias"] = (g.standard_normal(sizes[i]) * 0.5).astype(np.float32)
    w["joint_W"] = (g.standard_normal((Dz + K, JH)) * 0.15).astype(np.float32)
    w["joint_hid_bias"] = (g.standard_normal(JH) * 0.2).astype(np.float32)
    w["joint_vis_bias"] = np.concatenate([g.standard_normal(Dz) * 0.2, g.standard_normal(K) * 1.5]).astype(np.float32)
    zcm = g.random((K, Dz), dtype=np.float32)
    m = _model(w, Dz, K, zcm)
    yi = np.arange(N) % K
    X = (g.random((N, 10000)) < 0.15).astype(np.float32)
    Y = np.eye(K, dtype=np.float32)[yi]
    with E.use_rng(E.PhiloxRng(seed=31)):
        i2t, t2i = CS.trace_cross_panel_batch(m, torch.from_numpy(X).to(DEV), torch.from_numpy(Y).to(DEV), max_steps=T)
    o = TO.SmallOracle.__new__(TO.SmallOracle)
    o.img = [(w[f"img{i}_W"].astype(np.float64), w[f"img{i}_hid_bias"].astype(np.float64), w[f"img{i}_vis_bias"].astype(np.float64)) for i in range(2)]
    o.W, o.hb, o.vb = (w["joint_W"].astype(np.float64), w["joint_hid_bias"].astype(np.float64), w["joint_vis_bias"].astype(np.float64))
    o.zcm, o.groups = zcm.astype(np.float64), [(Dz, Dz + K)]
    u = PhiloxStream(31).uniform((N, Dz + K)).astype(np.float64)
    z = o.represent(X.astype(np.float64))
    vk = np.zeros((N, Dz + K)); vk[:, :Dz] = z
    mk = np.zeros_like(vk); mk[:, :Dz] = 1
    v0 = vk * mk + (1 - mk) * u
    y0 = TO.v_probs(o.W, o.vb, TO.h_probs(o.W, o.hb, v0), o.groups)[:, Dz:]
    ys = TO.mean_field_chain(o.W, o.hb, o.vb, o.groups, v0, vk, mk, T)[:, :, Dz:]
    r, steps, pred, margin = TO.label_scan(y0, ys, gt=yi)
    close = margin <= 1e-5
    s_gpu, p_gpu = i2t["steps"].cpu().numpy(), i2t["pred"].cpu().numpy()
    bad = (~close) & ((s_gpu != steps) | (p_gpu != pred))
    assert not bad.any(), (np.nonzero(bad)[0], s_gpu[bad], steps[bad])
    _close(i2t["p_top1"].cpu(), r["p1"], 1e-5, "p_top1")
    _close(i2t["l1"].cpu(), r["l1"], 1e-5, "l1")
    vk2 = np.zeros((N, Dz + K)); vk2[:, Dz:] = Y
    m2 = np.zeros_like(vk2); m2[:, Dz:] = 1
    z0 = o.zcm[yi]
    v02 = vk2.copy(); v02[:, :Dz] = z0
    zs = TO.mean_field_chain(o.W, o.hb, o.vb, o.groups, v02, vk2, m2, T)[:, :, :Dz]
    zn, dz = TO.code_scan(zs, z0)
    mse = np.stack([TO.decode_sqerr(o.decode_layers(), zn[t], X.astype(np.float64)) for t in range(T)], 1)
    s2, best, margin2 = TO.patience_scan(dz, mse)
    close2 = margin2 <= 1e-5
    g2 = t2i["steps"].cpu().numpy()
    bad2 = (~close2) & (g2 != s2)
    assert not bad2.any(), (np.nonzero(bad2)[0], g2[bad2], s2[bad2])
    _close(t2i["z_l2"].cpu(), dz, 1e-5, "dz")
    _close(t2i["image_mse"].cpu(), mse, 1e-4, "image_mse", rel=True)
    n_close = int(close.sum() + close2.sum())
    print(f"full-size panel: {n_close} of {2 * N} rows decided within 1e-5 of a threshold; img2txt converged "
          f"{int((steps <= T).sum())}, txt2img converged {int((s2 <= T).sum())}")
    assert n_close <= N // 4
