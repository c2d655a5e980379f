"""Shared by test_bimodal_logging_cpu.py (oracle engine double) and test_bimodal_logging_gpu.py: the product's iMDBN_BiModal built from
ref_bimodal_small.pkl over the validation set of bimodal_logging_small.npz, and imdbn.utils.bimodal_logging checked against that
recording of the reference."""
from __future__ import annotations

import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset, Subset

import bimodal_logging_oracle as BO
from golden_utils import GOLDEN, Fixture
from oracle.draws import DrawStream


class Run:
    def __init__(self):
        self.logged = []

    def log(self, d):
        self.logged.append(d)


class _Base(Dataset):
    def __init__(self, fx):
        self.X1, self.X2 = torch.from_numpy(fx["X1"].astype(np.float32)), torch.from_numpy(fx["X2"].astype(np.float32))
        self.labels, self.cumArea_list = fx["feat_labels"].tolist(), fx["feat_cum_area"].tolist()
        self.CH_list, self.density_list = fx["feat_convex_hull"].tolist(), fx["feat_density"].tolist()

    def __len__(self):
        return len(self.X1)

    def __getitem__(self, i):
        return self.X1[i], self.X2[i]


def fixture():
    return Fixture("bimodal_logging_small.npz")


def model(fx, dev):
    from imdbn.models import iMDBN_BiModal
    m = fx.meta
    base = _Base(fx)
    val = DataLoader(Subset(base, list(range(len(base)))), batch_size=m["batch"], shuffle=False)
    dev = torch.device(dev)
    mdl = iMDBN_BiModal(m["sizes1"], m["sizes2"], m["joint"], params=m["params"], dataloader=val, val_loader=val, device=dev)
    pl = iMDBN_BiModal.load_model(os.path.join(GOLDEN, "ref_bimodal_small.pkl"), device=dev)
    mdl.mod1_dbn.layers, mdl.mod2_dbn.layers = pl["mod1_dbn"].layers, pl["mod2_dbn"].layers
    mdl.joint_layers = pl["joint_layers"]
    mdl.joint_rbm = mdl.joint_layers[0]
    mdl.cross_steps = m["steps"]
    mdl.wandb_run = Run()
    return mdl


def replay(seed):
    from imdbn import engine as E
    return E.use_rng(E.ReplayRng(DrawStream(seed)))


def close(a, b, tol, what, rel=False):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b) / (np.abs(b) if rel else 1.0)
    print(f"{what}: max err {err.max():.3g} (tolerance {tol:g})")
    assert err.max() <= tol, f"{what}: max err {err.max():.3g} > {tol:g}"


def check_module_against_recording(fx, dev, tol=1e-5, pca_tol=5e-5, rho_tol=1e-6, probe_same=0.97):
    """Every figure is printed before it is asserted.  `tol`: embeddings, trajectories, decoded frames; `pca_tol`: projections
    (the tolerance of the recorded PCA transforms in test_imdbn_logging_*); ranks of the rows the fixture marks as decided are
    compared exactly."""
    from imdbn.utils import bimodal_logging as L
    mt = fx.meta
    T = mt["steps"]
    m = model(fx, dev)
    # embeddings and features
    E_, feats = L.compute_bimodal_joint_embeddings_and_features(m)
    assert E_.device.type == torch.device(dev).type
    close(E_.cpu(), fx["E"], tol, "joint embeddings")
    assert sorted(feats) == ["convex_hull", "cum_area", "density", "labels"]
    for k in feats:
        close(torch.as_tensor(feats[k]).cpu(), fx["feat_" + k], 1e-6, "feature " + k, rel=True)
    # probes
    p = mt["probe"]
    torch.manual_seed(4242)
    m.wandb_run = Run()
    res = L.log_bimodal_joint_linear_probe(m, epoch=p["epoch"], n_bins=p["n_bins"], steps=p["steps"])
    assert sorted(res) == sorted(p["acc"])
    same = n = 0
    for name, (acc, cm) in res.items():
        mkey = name.split("/")[1]
        yt, yp = fx[f"probe_{mkey}_true"], fx[f"probe_{mkey}_pred"]
        want = np.zeros((p["n_bins"], p["n_bins"]), np.int64)
        np.add.at(want, (yt, yp), 1)
        assert tuple(cm.shape) == (p["n_bins"], p["n_bins"]) and int(cm.sum()) == len(yt)
        assert np.array_equal(cm.sum(1).numpy(), want.sum(1)), name                     # same test rows, same binned targets
        d = int(np.abs(cm.numpy() - want).sum()) // 2                                   # predictions that differ, at least
        same, n = same + len(yt) - d, n + len(yt)
        print(f"probe {name}: acc {acc:.4f} vs {p['acc'][name]:.4f}, {d} of {len(yt)} predictions differ")
    assert same / n >= probe_same, (same, n)
    keys = {k for d in m.wandb_run.logged for k in d}
    assert {f"probe/{k}/acc" for k in p["acc"]} <= keys
    # 2-D trajectories
    for ci, c in enumerate(mt["traj"]):
        pre = f"t{ci}_"
        with replay(c["seed"]):
            o = L.log_bimodal_latent_trajectory(m, sample_idx=c["sample_idx"], steps=T, tag=f"t{ci}", n_frames=8)
        close(o["traj_h"], fx[pre + "traj_h"], tol, pre + "traj_h")
        close(o["traj_2d"], fx[pre + "traj_2d"], pca_tol, pre + "traj_2d")
        close(o["h_true_2d"], fx[pre + "h_true_2d"], pca_tol, pre + "h_true_2d")
        sel = np.unique(np.linspace(0, T, 8, dtype=int)).tolist()
        assert o["sel_idx"] == sel
        close(o["frames"], fx[pre + "frames"][sel], tol, pre + "frames")
        if ci == 0:
            close(o["H2d"], fx["H2d"], pca_tol, "H2d")
    # 3-D trajectory
    c = mt["traj3d"]
    with replay(c["seed"]):
        o = L.log_bimodal_latent_trajectory_3d(m, sample_idx=c["sample_idx"], steps=T)
    close(o["traj_z1"], fx["t3d_traj_z1"], tol, "3-D traj_z1")
    close(o["Z3"], fx["t3d_Z3"], pca_tol, "Z3")
    close(o["T3"], fx["t3d_T3"], pca_tol, "T3")
    # PCA summary + Spearman
    s = L.bimodal_pca_summary(m)
    for tagname in ("joint", "mod2"):
        for n_ in (2, 3):
            P = s[f"{tagname}_p{n_}"]
            close(P, fx[f"{tagname}_p{n_}"], pca_tol, f"{tagname} PCA-{n_}")
            ranks = np.stack([L._avg_ranks(torch.from_numpy(P[:, i]).to(dev)).cpu().numpy() for i in range(n_)], 1)
            dec = fx[f"{tagname}_p{n_}_decided"]
            assert np.array_equal(ranks[dec], fx[f"{tagname}_p{n_}_ranks"][dec]), f"{tagname} PCA-{n_}: ranks of the decided rows"
            print(f"{tagname} PCA-{n_}: {int((ranks != fx[f'{tagname}_p{n_}_ranks']).sum())} of {ranks.size} ranks differ; "
                  f"{int((~dec).sum())} rows undecided")
    for k, d in mt["correlations"].items():
        assert sorted(s["correlations"][k]) == sorted(d), k
        for kk, v in d.items():
            close(s["correlations"][k][kk], v, rho_tol, f"rho {k} {kk}")
    bad = L.embedding_correlations(torch.from_numpy(fx["joint_p2"]), {"Labels": fx["feat_labels"][:-1], "One": fx["feat_labels"][:1]})
    assert len(bad) == 4 and all(np.isnan(v) for v in bad.values())
    # snapshots
    sn = mt["snapshots"]
    m.wandb_run = Run()
    with replay(sn["seed"]):
        r = m._log_snapshots(epoch=sn["epoch"], num=sn["num"])
    for k, v in sn["mse"].items():
        close(r[k], v, 1e-4, k, rel=True)
    assert {"snap/mod1_mse", "snap/mod2_mse", "epoch"} <= {k for d in m.wandb_run.logged for k in d}
    m.wandb_run = None

    class Never:
        def uniform(self, shape):
            raise AssertionError("a draw was made")
        normal = categorical = uniform

    from imdbn import engine as E
    with E.use_rng(E.ReplayRng(Never())):
        assert m._log_snapshots(epoch=1) is None
        assert L.log_bimodal_latent_trajectory(m) is None and L.log_bimodal_latent_trajectory_3d(m) is None
    return m


def oracle_stacks(fx):
    def stack(pre, n):
        return BO.Stack([(fx[f"{pre}_{i}_W"], fx[f"{pre}_{i}_hb"], fx[f"{pre}_{i}_vb"]) for i in range(n)])
    return stack("m1", 2), stack("m2", 2), stack("j", 2)
