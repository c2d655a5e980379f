"""GPU: the latent top-k search (imdbn_latent_topk / imdbn_row_stats) against the fp64 oracle at odd and full sizes, its
determinism and tie rule, and imdbn.utils.imdbn_logging on the small trained iMDBN against the reference's recorded logging
(logging_small.npz, draws replayed from the fixture's seeds)."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import logging_oracle as LO
import trace_oracle as TO
from golden_utils import Fixture
from oracle.draws import DrawStream

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
    return Fixture("logging_small.npz")


def _eng():
    from imdbn import engine as E
    return E.get_hip_engine()


def _check_topk(bank, q, metric, k, exclude=None, key=None, rows=None, tol=2e-6):
    """kernel vs oracle: indices equal wherever the oracle's deciding gap exceeds the fp32 error bound, scores close."""
    idx, sc = _eng().latent_topk(bank, q, metric, k, exclude=exclude, key=key)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    B, Q = bank.cpu().double().numpy(), q.cpu().double().numpy()
    rows = range(Q.shape[0]) if rows is None else rows
    ex = exclude.cpu().numpy() if exclude is not None else None
    kk = key.cpu().numpy() if key is not None else None
    n_exact = 0
    for r in rows:
        S = LO.scores(B, Q[r:r + 1], metric)
        oi, ov, margin = LO.topk_row(S[0], k, -1 if ex is None else int(ex[r]), kk)
        scale = float(np.abs(S).max()) + 1e-30
        if metric == 2:             # the expansion's error follows its terms, not the (cancelled) result
            scale = float(((Q[r] ** 2).sum() + (B ** 2).sum(1) + 2 * np.abs(B @ Q[r])).max())
        bound = tol * scale * (1 + np.sqrt(B.shape[1]) / 8)
        n = len(oi)
        assert (idx[r, n:] == -1).all() and np.isneginf(sc[r, n:]).all(), f"row {r}: padding"
        np.testing.assert_allclose(sc[r, :n], ov, atol=bound, err_msg=f"row {r}: scores")
        if margin > 2 * bound:
            np.testing.assert_array_equal(idx[r, :n], oi, err_msg=f"row {r} (metric {metric}): indices")
            n_exact += 1
    return n_exact


def test_topk_small_odd_sizes_against_the_oracle():
    g = np.random.Generator(np.random.PCG64(21))
    for N, D, Q, k in ((1, 37, 3, 5), (200, 37, 70, 64), (1000, 61, 33, 8), (130, 3, 129, 1)):
        wide = torch.from_numpy(g.standard_normal((N, D + 11), dtype=np.float32)).to(DEV)
        bank = wide[:, 5:5 + D]                                          # strided rows
        if N > 10:
            bank[7] = bank[3]                                            # duplicated rows tie exactly
        q = torch.from_numpy(g.standard_normal((Q, D), dtype=np.float32)).to(DEV)
        key = torch.from_numpy(g.integers(0, max(2, N // 4), (N, 2)).astype(np.float32)).to(DEV)
        ex = torch.from_numpy(g.integers(-1, N, Q).astype(np.int32)).to(DEV)
        n_exact = 0
        for metric in (0, 1, 2):
            for kk in (None, key):
                for e in (None, ex):
                    n_exact += _check_topk(bank, q, metric, k, exclude=e, key=kk)
        assert n_exact >= 0.8 * 12 * Q, (N, D, Q, k, n_exact)


def test_topk_full_size_against_the_oracle():
    g = np.random.Generator(np.random.PCG64(22))
    N, D, Q, k = 16384, 500, 13056, 64
    bank = torch.from_numpy(g.random((N, D), dtype=np.float32)).to(DEV)
    q = torch.from_numpy(g.random((Q, D), dtype=np.float32)).to(DEV)
    key = torch.from_numpy(g.integers(0, 3000, (N, 2)).astype(np.float32)).to(DEV)
    ex = torch.from_numpy(g.integers(-1, N, Q).astype(np.int32)).to(DEV)
    rows = sorted(g.choice(Q, 24, replace=False).tolist()) + [0, Q - 1]
    for metric in (0, 1, 2):
        n = _check_topk(bank, q, metric, k, exclude=ex, key=key, rows=rows, tol=4e-7)
        n += _check_topk(bank, q, metric, 8, rows=rows, tol=4e-7)
        assert n >= len(rows) // 2, (metric, n)          # of 2 len(rows) checks: the rest had a gap within the bound


def test_topk_is_deterministic_and_batch_independent():
    g = np.random.Generator(np.random.PCG64(23))
    N, D, Q = 5000, 500, 300
    bank = torch.from_numpy(g.random((N, D), dtype=np.float32)).to(DEV)
    q = torch.from_numpy(g.random((Q, D), dtype=np.float32)).to(DEV)
    key = torch.from_numpy(g.integers(0, 700, (N, 2)).astype(np.float32)).to(DEV)
    for metric in (0, 1, 2):
        a = _eng().latent_topk(bank, q, metric, 16, key=key)
        b = _eng().latent_topk(bank, q, metric, 16, key=key)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        for r in (0, 131, Q - 1):
            one = _eng().latent_topk(bank, q[r:r + 1], metric, 16, key=key)
            assert torch.equal(one[0][0], a[0][r]) and torch.equal(one[1][0].view(torch.int32), a[1][r].view(torch.int32))
        few = _eng().latent_topk(bank, q, metric, 3, key=key)          # other k: the same leading entries, same bits
        assert torch.equal(few[0], a[0][:, :3]) and torch.equal(few[1].view(torch.int32), a[1][:, :3].view(torch.int32))


def test_duplicated_rows_tie_to_the_lower_index():
    g = np.random.Generator(np.random.PCG64(24))
    base = torch.from_numpy(g.random((40, 77), dtype=np.float32)).to(DEV)
    bank = torch.cat([base, base, base[:5]], 0)                          # rows i, i + 40 (and i + 80) identical
    for metric in (0, 1, 2):
        idx, sc = _eng().latent_topk(bank, base[:5], metric, 6)
        idx, sc = idx.cpu(), sc.cpu()
        for r in range(5):
            assert idx[r, 0].item() == r and idx[r, 1].item() == r + 40 and idx[r, 2].item() == r + 80, (metric, idx[r])
            assert sc[r, 0].item() == sc[r, 1].item() == sc[r, 2].item()
        # with every row its own key, a key shared by the copies keeps only the lowest index
        key = torch.arange(85, device=DEV).remainder(40).float().repeat(2, 1).t().contiguous()
        idx, _ = _eng().latent_topk(bank, base[:5], metric, 6, key=key)
        assert (idx.cpu() < 40).all()


def test_k_limit_and_row_stats():
    from imdbn.engine import native as N
    lib = N.lib()
    bank = torch.rand(10, 4, device=DEV)
    out_i = torch.empty(1, 65, dtype=torch.int32, device=DEV)
    out_s = torch.empty(1, 65, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    for k in (65, 0):
        rc = lib.imdbn_latent_topk(p(bank), 4, 10, 4, None, p(bank), 4, 1, 1, k, None, None, p(out_i), p(out_s), p(ws), ws.numel(), None)
        assert rc == -1, (k, rc)                                         # IMDBN_E_INVALID
    with pytest.raises(N.EngineError):
        _eng().latent_topk(bank, bank[:1], "cosine", 65)
    g = np.random.Generator(np.random.PCG64(25))
    X = (g.random((777, 100)) > 0.6).astype(np.float32)
    st = _eng().row_stats(torch.from_numpy(X).to(DEV)).cpu()
    torch.testing.assert_close(st[:, 0], torch.from_numpy(X).sum(1), rtol=0, atol=0)
    torch.testing.assert_close(st[:, 1], (torch.from_numpy(X) ** 2).sum(1), rtol=0, atol=0)


# ---- the small trained iMDBN against the reference ------------------------------------------------------------------------
class _Model:
    pass


def _rbm(W, hb, vb, groups=None):
    from imdbn.models import RBM
    r = RBM(W.shape[0], W.shape[1], 0.1, 1e-4, 0.5, softmax_groups=groups).to(DEV)
    r.W.data.copy_(torch.from_numpy(np.ascontiguousarray(W)))
    r.hid_bias.data.copy_(torch.from_numpy(hb)); r.vis_bias.data.copy_(torch.from_numpy(vb))
    return r


def _small_model(steps):
    from imdbn.models import iDBN
    w, X, Y = TO.small_model_arrays()
    m = _Model()
    m.device = torch.device(DEV)
    idbn = iDBN.__new__(iDBN)
    idbn.device = m.device
    idbn.layers = [_rbm(w[f"img{i}_W"], w[f"img{i}_hid_bias"], w[f"img{i}_vis_bias"]) for i in range(2)]
    m.val_loader = DataLoader(TensorDataset(torch.from_numpy(X), torch.from_numpy(Y)), batch_size=8, shuffle=False)
    idbn.val_loader = m.val_loader
    idbn.features = {"Labels": torch.from_numpy(Y)}
    m.image_idbn = idbn
    m.joint_rbm = _rbm(w["joint_W"], w["joint_hid_bias"], w["joint_vis_bias"], [(20, 28)])
    m.Dz_img, m.num_labels, m.cross_steps = 20, 8, steps
    m.z_class_mean = torch.from_numpy(w["z_class_mean"]).to(DEV)
    m.wandb_run = None
    return m, X, Y


def _replay(seed):
    from imdbn import engine as E
    return E.use_rng(E.ReplayRng(DrawStream(seed)))


def test_vecdb_neighbours_match_the_reference(fx):
    from imdbn.utils import imdbn_logging as L
    T, k = fx.meta["steps"], fx.meta["k"]
    m, X, Y = _small_model(T)
    for ci, c in enumerate(fx.meta["cases"]):
        with _replay(c["seed"]):
            o = L.log_vecdb_neighbors_for_traj(m, sample_idx=c["sample_idx"], steps=T, k=k, metric=c["metric"], dedup=c["dedup"],
                                               exclude_self=c["exclude_self"])
        for name in ("true", "z0", "zT", "zT_l2"):
            assert o["idx_" + name][0].tolist() == fx[f"c{ci}_{name}_idx"].tolist(), (ci, name)
            np.testing.assert_allclose(o["sc_" + name][0].numpy(), fx[f"c{ci}_{name}_sc"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(o["decode"]["decode_mse"], fx[f"c{ci}_decode_mse"], rtol=1e-4)
    H = m._H_bank.cpu().numpy()
    np.testing.assert_array_equal(H, LO.row_keys(X))


def test_topk_similar_pca3_and_auto_recon_match_the_reference(fx):
    from imdbn.utils import imdbn_logging as L
    m, X, Y = _small_model(fx.meta["steps"])
    L.ensure_val_bank(m)
    for met in ("cosine", "ip", "l2"):
        i, v = L.topk_similar_in_latent(m, torch.from_numpy(fx["topk_q"]).to(DEV), k=fx.meta["k"], metric=met)
        assert i.dtype == torch.int64 and i.tolist() == fx[f"topk_{met}_idx"].tolist(), met
        np.testing.assert_allclose(v.numpy(), fx[f"topk_{met}_sc"], rtol=1e-5, atol=1e-6)
    p = fx.meta["pca3"]
    with _replay(p["seed"]):
        o = L.log_pca3_trajectory(m, p["sample_idx"], steps=fx.meta["steps"])
    np.testing.assert_allclose(o["Z_traj"], fx["pca3_Ztraj"], atol=2e-6)
    np.testing.assert_allclose(o["T3"], fx["pca3_T3"], atol=5e-5)
    np.testing.assert_allclose(o["Z3"], fx["pca3_Z3"], atol=5e-5)

    class Run:
        def __init__(self):
            self.logged = []

        def log(self, d):
            self.logged.append(d)

    m.wandb_run = Run()
    m.validation_images, m.validation_labels = torch.from_numpy(X[:8]).to(DEV), torch.from_numpy(Y[:8]).to(DEV)
    r = L.log_joint_auto_recon(m, epoch=3, num=8)
    ref = fx.meta["auto_recon"]
    assert r["text_top1"] == ref["auto_recon/text_top1"]
    assert r["text_bce"] == pytest.approx(ref["auto_recon/text_bce"], rel=1e-5)
    assert r["image_mse"] == pytest.approx(ref["auto_recon/image_mse"], rel=1e-5)
    keys = {k for d in m.wandb_run.logged for k in d}
    assert {"auto_recon/text_top1", "auto_recon/text_bce", "auto_recon/image_mse", "epoch"} <= keys


def test_trajectory_batch_equals_b1_calls_and_the_untraced_chain():
    from imdbn import engine as E
    from imdbn.utils import imdbn_logging as L
    m, X, Y = _small_model(12)
    B, T = 6, 15
    y = torch.from_numpy(Y[[0, 9, 33, 70, 101, 400]]).to(DEV)
    with E.use_rng(E.PhiloxRng(seed=31)):
        tr = L.latent_trajectory_batch(m, y, T)
    assert tr.shape == (T + 1, B, 20)
    for i in range(B):
        with E.use_rng(E.PhiloxRng(seed=31, row0=i)):
            one = L.latent_trajectory_batch(m, y[i:i + 1], T)
        assert torch.equal(one[:, 0], tr[:, i]), i
    vk = torch.cat([m.z_class_mean[y.argmax(1)], y], 1)
    km = torch.zeros_like(vk)
    km[:, 20:] = 1
    step = {"T": 1.0, "sigma": 0.0, "eta": 0.0, "sample_h": True, "vmode": 0, "clamp": True}
    v = _eng().chain(m.joint_rbm, vk, km, [step] * T, E.PhiloxRng(seed=31), init_uniform=False)
    assert torch.equal(v[:, :20], tr[-1])
