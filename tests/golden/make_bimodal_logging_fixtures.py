#!/usr/bin/env python3
"""Generate tests/golden/bimodal_logging_small.npz: the reference's iMDBN_BiModal side-car (imdbn/models/imdbn_bimodal.py: joint
embeddings, linear probes, MOD2->MOD1 latent trajectories in 2-D and 3-D, snapshots; the PCA + Spearman numbers its train_joint
logs through imdbn/utils/wandb_utils.py) on the trained small bimodal model of ref_bimodal_small.pkl (joint 36 <-> 24 -> 12).

Run in the build container only (needs the reference checkout, as make_fixtures.py does):

    python tests/golden/make_bimodal_logging_fixtures.py

The UNMODIFIED reference functions run on a reference ``iMDBN_BiModal`` that carries the pickled weights.  Its validation set is
the recipe of make_fixtures.case_bimodal_small (same class prototypes) drawn for 160 rows, behind a Subset-like dataset that
exposes ``labels`` / ``cumArea_list`` / ``CH_list`` / ``density_list`` / ``indices``.  ``torch.bernoulli`` (the trajectories' only
draw) is routed through a ``DrawStream`` as ``(p > U)`` and the smallest |p - U| is recorded; ``torch.rand_like`` of
``_cross_reconstruct`` goes through make_fixtures.Substitute; sklearn's ``PCA`` is a subclass that records what it fits and
transforms; ``wandb.Image``, the torchvision grid and matplotlib's figures are stubbed or unused (Agg).  The generator asserts the
margins that let tests compare exactly: |p - U| >= DRAW, the top-4 eigenvalues of every fitted covariance separated by > EIG
(relative); for the values that enter a Spearman rank see ``pick_validation_seed``: the rows that are RANK of the range away from
every other value are recorded, and their share asserted.
"""
from __future__ import annotations

import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_fixtures as MF  # noqa: E402  (reference on sys.path, wandb / torchvision stubs, scratch cwd)

import torch  # noqa: E402
import matplotlib  # noqa: E402

matplotlib.use("Agg")
import sklearn.decomposition  # noqa: E402

import bimodal_logging_oracle as BO  # noqa: E402
from oracle.draws import DrawStream  # noqa: E402
from make_logging_fixtures import Bernoulli  # noqa: E402
from imdbn.models import imdbn_bimodal as RB  # noqa: E402  (the reference module)
from imdbn.utils import wandb_utils as RW  # noqa: E402

STEPS, N_VAL, BATCH = 12, 160, 8
DRAW, EIG, RANK = 1e-4, 1e-3, 1e-4
SRC = os.path.join(HERE, "bimodal_small_100_40_20__64_30_16__j24_12.npz")
PKL = os.path.join(HERE, "ref_bimodal_small.pkl")
FUNCS = ["compute_bimodal_joint_embeddings_and_features", "log_bimodal_joint_linear_probe", "log_bimodal_latent_trajectory",
         "log_bimodal_latent_trajectory_3d"]

sys.modules["torchvision.utils"].make_grid = lambda X, nrow=8: torch.zeros(3, 2, 2)
sys.modules["wandb"].Image = lambda x, *a, **k: None


class StubRun:
    def __init__(self):
        self.logged = []

    def log(self, d):
        self.logged.append(d)


def data(vseed=1000):
    """Class prototypes of case_bimodal_small (same seed, same first draws), N_VAL rows from a stream of their own."""
    meta = json.loads(str(np.load(SRC)["meta"]))
    s = DrawStream(meta["seed"])
    K, N0 = meta["K"], meta["B"] * meta["NB"]
    proto1 = (s.uniform((K, 100)) > 0.7).astype(np.float32)
    s.uniform((N0, 100))
    proto2 = (s.uniform((K, 64)) > 0.6).astype(np.float32)
    v = DrawStream(meta["seed"] + vseed)
    yi = (np.arange(N_VAL) * 3 + (np.arange(N_VAL) // 5)) % K
    X1 = np.abs(proto1[yi] - (v.uniform((N_VAL, 100)) > 0.9).astype(np.float32)).astype(np.float32)
    X2 = np.abs(proto2[yi] - (v.uniform((N_VAL, 64)) > 0.92).astype(np.float32)).astype(np.float32)
    w = np.linspace(0.5, 1.5, 100, dtype=np.float64)
    feats = {"labels": (yi + 1).astype(np.float64), "cum_area": X1.astype(np.float64).sum(1) + 0.25 * v.uniform((N_VAL,)).astype(np.float64),
             "convex_hull": X1.astype(np.float64) @ w}
    feats["density"] = feats["cum_area"] / feats["convex_hull"]
    return meta, yi, X1, X2, feats


class Base(torch.utils.data.Dataset):
    def __init__(self, X1, X2, feats):
        self.X1, self.X2 = torch.from_numpy(X1), torch.from_numpy(X2)
        self.labels, self.cumArea_list = feats["labels"].tolist(), feats["cum_area"].tolist()
        self.CH_list, self.density_list = feats["convex_hull"].tolist(), feats["density"].tolist()

    def __len__(self):
        return len(self.X1)

    def __getitem__(self, i):
        return self.X1[i], self.X2[i]


def model(meta, X1, X2, feats):
    base = Base(X1, X2, feats)
    sub = torch.utils.data.Subset(base, list(range(len(base))))
    val = torch.utils.data.DataLoader(sub, batch_size=BATCH, shuffle=False)
    m = RB.iMDBN_BiModal(meta["sizes1"], meta["sizes2"], meta["joint"], params=meta["params"], dataloader=val, val_loader=val,
                         device=torch.device("cpu"))
    pl = RB.iMDBN_BiModal.load_model(PKL, device=torch.device("cpu"))
    m.mod1_dbn, m.mod2_dbn, m.joint_layers = pl["mod1_dbn"], pl["mod2_dbn"], pl["joint_layers"]
    m.joint_rbm = m.joint_layers[0]
    m.cross_steps = STEPS
    m.wandb_run = StubRun()
    return m


class Recorder:
    """sklearn PCA that records (fit input, fit_transform output) and every (transform input, output); mod1 decodes recorded."""

    def __init__(self, m):
        self.m, self.fits, self.transforms, self.decodes = m, [], [], []

    def __enter__(self):
        self._pca, self._dec = sklearn.decomposition.PCA, self.m.mod1_dbn.decode
        rec = self

        class PCA(self._pca):
            def fit_transform(self_, X, y=None):
                out = super().fit_transform(X, y)
                rec.fits.append((np.asarray(X, np.float64), np.asarray(out, np.float64), np.asarray(self_.explained_variance_, np.float64)))
                return out

            def transform(self_, X):
                out = super().transform(X)
                rec.transforms.append((np.asarray(X, np.float64), np.asarray(out, np.float64)))
                return out

        def decode(z):
            out = rec._dec(z)
            rec.decodes.append(out.detach().numpy().copy())
            return out

        sklearn.decomposition.PCA = RB.PCA = PCA
        self.m.mod1_dbn.decode = decode
        return self

    def __exit__(self, *a):
        sklearn.decomposition.PCA = RB.PCA = self._pca
        del self.m.mod1_dbn.decode


def check_eigs(X, what):
    X = np.asarray(X, np.float64)
    w = np.sort(np.linalg.eigvalsh(np.cov(X.T)))[::-1][:4]
    gaps = (w[:-1] - w[1:]) / w[0]
    assert gaps.min() > EIG, f"{what}: eigenvalues {w} too close"
    return float(gaps.min())


def rank_gaps(P):
    """Per column of P: every row's distance to its nearest other value, relative to the column's range: [N, C]."""
    P = np.asarray(P, np.float64)
    out = np.empty_like(P)
    for i in range(P.shape[1]):
        o = np.argsort(P[:, i])
        d = np.diff(P[o, i]) / (P[o[-1], i] - P[o[0], i])
        out[o, i] = np.minimum(np.concatenate([[np.inf], d]), np.concatenate([d, [np.inf]]))
    return out


def projections(m):
    """(E, Z2), their four sklearn projections as the PCA block of train_joint forms them, and sklearn's own float32 error.

    The reference hands sklearn float32 arrays, and sklearn then forms the covariance in float32 (X'X - n mean mean').  The top joint
    layer of the small model is barely trained: its activations vary by ~5e-3 around 0.5, so that difference cancels to a relative
    1e-3 and the float32 projections are off by up to 10 % of their size -- rounding noise of one machine, not something to pin a test
    to.  Recorded here: the same sklearn call on the same arrays cast to float64; the float32 call's distance from it is kept in
    the meta (``pca_float32_error``) for the record."""
    PCA = sklearn.decomposition.PCA
    with torch.no_grad():
        E, _ = RB.compute_bimodal_joint_embeddings_and_features(m)
        Z2 = torch.cat([m.mod2_dbn.represent(b2.view(b2.size(0), -1).float()) for _, b2 in m.val_loader], 0).numpy()
    E = E.numpy()
    P, err = {}, {}
    for tagname, X in (("joint", E), ("mod2", Z2)):
        for n in (2, 3):
            P[f"{tagname}_p{n}"] = PCA(n_components=n).fit_transform(X.astype(np.float64))
            err[f"{tagname}_p{n}"] = float(np.abs(PCA(n_components=n).fit_transform(X) - P[f"{tagname}_p{n}"]).max())
    return E, Z2, P, err


def pick_validation_seed():
    """The closest pair of N values spread over a range is about range / N^2 apart (4e-5 for the 160 rows asked for), so a set
    whose EVERY pair of projected values is RANK of the range apart does not turn up by trying seeds.  What can be had: of the
    candidate row streams, the one whose closest projected pair (over the ten projected columns) is widest; the rows that ARE
    RANK apart from every other value are recorded per column (``*_decided``), and tests compare the ranks of those exactly."""
    import contextlib
    import io
    best = (-1.0, None)
    for vseed in range(1000, 1400):
        with contextlib.redirect_stdout(io.StringIO()):
            meta0, yi, X1, X2, feats = data(vseed)
            _, _, P, _ = projections(model(meta0, X1, X2, feats))
        worst = min(float(rank_gaps(p).min()) for p in P.values())
        if worst > best[0]:
            best = (worst, vseed)
    return best


def main():
    gap, vseed = pick_validation_seed()
    print(f"validation stream {vseed}: closest projected pair {gap:.2e} of its range")
    meta0, yi, X1, X2, feats = data(vseed)
    out = {"X1": X1.astype(np.uint8), "X2": X2.astype(np.uint8), "yi": yi.astype(np.int32)}
    for k, v in feats.items():
        out["feat_" + k] = v
    meta = {"steps": STEPS, "n_val": N_VAL, "batch": BATCH, "sizes1": meta0["sizes1"], "sizes2": meta0["sizes2"], "joint": meta0["joint"], "params": meta0["params"],
            "funcs": {f: list(inspect.signature(getattr(RB, f)).parameters) for f in FUNCS},
            "snapshots_sig": list(inspect.signature(RB.iMDBN_BiModal._log_snapshots).parameters),
            "margins": {"closest_projected_pair": gap}, "vseed": vseed}
    m = model(meta0, X1, X2, feats)
    # weights of the pickled model (the tests' oracle; the GPU tests load the pickle itself)
    for name, dbn in (("m1", m.mod1_dbn), ("m2", m.mod2_dbn)):
        for i, r in enumerate(dbn.layers):
            out[f"{name}_{i}_W"], out[f"{name}_{i}_hb"], out[f"{name}_{i}_vb"] = (r.W.detach().numpy(), r.hid_bias.detach().numpy(),
                                                                                  r.vis_bias.detach().numpy())
    for i, r in enumerate(m.joint_layers):
        out[f"j_{i}_W"], out[f"j_{i}_hb"], out[f"j_{i}_vb"] = r.W.detach().numpy(), r.hid_bias.detach().numpy(), r.vis_bias.detach().numpy()

    # 1. joint embeddings + features
    with torch.no_grad():
        E, f = RB.compute_bimodal_joint_embeddings_and_features(m)
    out["E"] = E.numpy()
    assert sorted(f) == ["convex_hull", "cum_area", "density", "labels"]
    for k in f:
        np.testing.assert_allclose(f[k].numpy(), feats[k], rtol=1e-6)

    # 2. linear probes: what train_linear_classifier returned per target
    probes = []
    o_tlc = RB.train_linear_classifier

    def tlc(*a, **k):
        acc, yt, yp = o_tlc(*a, **k)
        probes.append((float(acc), np.asarray(yt, np.int32), np.asarray(yp, np.int32)))
        return acc, yt, yp

    RB.train_linear_classifier = tlc
    torch.manual_seed(4242)
    m.wandb_run = StubRun()
    RB.log_bimodal_joint_linear_probe(m, epoch=3, n_bins=5, steps=300)
    RB.train_linear_classifier = o_tlc
    names = ["cum_area", "convex_hull", "labels", "density"]
    assert len(probes) == 4
    meta["probe"] = {"epoch": 3, "n_bins": 5, "steps": 300, "acc": {f"joint/{n}": p[0] for n, p in zip(names, probes)},
                     "logged_keys": sorted({k for d in m.wandb_run.logged for k in d})}
    for n, p in zip(names, probes):
        out[f"probe_{n}_true"], out[f"probe_{n}_pred"] = p[1], p[2]

    # 3. trajectories (2-D panel) of a few samples, each from its own seed
    meta["traj"] = []
    for ci, (si, seed) in enumerate(((0, 8101), (37, 8201), (158, 8301), (500, 8401))):
        for sd in range(seed, seed + 100):
            with Bernoulli(sd) as b, Recorder(m) as r:
                RB.log_bimodal_latent_trajectory(m, sample_idx=si, steps=STEPS, tag=f"t{ci}", n_frames=8)
            if b.margin >= DRAW:
                break
        else:
            raise AssertionError("no seed with robust draws")
        assert len(r.fits) == 1 and len(r.transforms) == 2 and len(r.decodes) == STEPS + 1
        pre = f"t{ci}_"
        out[pre + "traj_h"], out[pre + "traj_2d"] = r.transforms[0][0].astype(np.float32), r.transforms[0][1]
        out[pre + "h_true"], out[pre + "h_true_2d"] = r.transforms[1][0].astype(np.float32), r.transforms[1][1]
        out[pre + "frames"] = np.clip(np.concatenate(r.decodes, 0), 0, 1).astype(np.float32)
        if ci == 0:
            out["H2d"] = r.fits[0][1]
            meta["margins"]["eig_H"] = check_eigs(r.fits[0][0], "H_all")
        meta["traj"].append({"sample_idx": si, "seed": sd, "min_draw_margin": b.margin})
        # the oracle replays the trajectory
        s_eff = min(si, N_VAL - 1)
        j = m.joint_rbm
        z2 = m.mod2_dbn.represent(torch.from_numpy(X2[s_eff:s_eff + 1])).detach().numpy()
        u = DrawStream(sd).uniform((STEPS, 1, 24)).astype(np.float64)
        th, tz, mg = BO.bimodal_trajectory(j.W.detach().numpy(), j.hid_bias.detach().numpy(), j.vis_bias.detach().numpy(), z2, 20, u)
        np.testing.assert_allclose(th[:, 0], out[pre + "traj_h"], atol=2e-6)
    # 4. 3-D trajectory
    for sd in range(8501, 8601):
        with Bernoulli(sd) as b, Recorder(m) as r:
            RB.log_bimodal_latent_trajectory_3d(m, sample_idx=11, steps=STEPS)
        if b.margin >= DRAW:
            break
    else:
        raise AssertionError("no seed with robust draws")
    assert len(r.fits) == 1 and len(r.transforms) == 1
    out["t3d_Z3"], out["t3d_traj_z1"], out["t3d_T3"] = r.fits[0][1], r.transforms[0][0].astype(np.float32), r.transforms[0][1]
    meta["margins"]["eig_Z1"] = check_eigs(r.fits[0][0], "Z1_all")
    meta["traj3d"] = {"sample_idx": 11, "seed": sd, "min_draw_margin": b.margin}

    # 5. the PCA block of train_joint (:856-912): sklearn PCA + the reference's correlation functions
    emb, Z2, P, meta["pca_float32_error"] = projections(m)
    np.testing.assert_array_equal(emb, E.numpy())
    fm = {"Cumulative Area": f["cum_area"].numpy(), "Convex Hull": f["convex_hull"].numpy(), "Labels": f["labels"].numpy(),
          "Density": f["density"].numpy()}
    meta["margins"]["eig_E"], meta["margins"]["eig_Z2"] = check_eigs(emb, "E"), check_eigs(Z2, "Z2")
    corr = {}
    run = StubRun()
    for arch, tagname, fmap in (("Joint_bimodal", "joint", fm), ("MOD2_MNIST100", "mod2", {"Labels": fm["Labels"]})):
        p2, p3 = P[tagname + "_p2"], P[tagname + "_p3"]
        for which, pp in (("p2", p2), ("p3", p3)):
            out[f"{tagname}_{which}"] = pp
            decided = rank_gaps(pp) >= RANK                    # rows whose rank in that column no 1e-4-of-range error can change
            assert decided.mean() > 0.9, (arch, which, decided.mean())
            out[f"{tagname}_{which}_decided"] = decided
            out[f"{tagname}_{which}_ranks"] = np.stack([BO.avg_ranks(pp[:, i]) for i in range(pp.shape[1])], 1)
        corr[f"{arch}/pca2"] = {k: float(v) for k, v in RW.plot_2d_embedding_and_correlations(p2, fmap, arch, "val", "pca", run).items()}
        corr[f"{arch}/pca3"] = {k: float(v) for k, v in RW.plot_3d_embedding_and_correlations(p3, fmap, arch, "val", "pca", run).items()}
        for which, pp in (("pca2", p2), ("pca3", p3)):          # the oracle's Spearman is scipy's
            mine = BO.correlations(pp, fmap)
            for k, v in corr[f"{arch}/{which}"].items():
                assert abs(mine[k] - v) < 1e-12, (k, mine[k], v)
    meta["correlations"] = corr
    # length mismatch / too short: NaN, as the reference reports
    bad = RW.plot_2d_embedding_and_correlations(out["joint_p2"], {"Labels": fm["Labels"][:-1]}, "x", "val", "pca", run)
    assert all(np.isnan(v) for v in bad.values())

    # 6. snapshots
    m.wandb_run = StubRun()
    assert m.validation_mod1 is not None
    for sd in range(8701, 8801):
        m.wandb_run = StubRun()
        s = DrawStream(sd)
        with MF.Substitute(s) as sub:
            sub._vshape = 36
            m._log_snapshots(epoch=5, num=8)
        if sub.min_margin >= DRAW:
            break
    else:
        raise AssertionError("no seed with robust draws")
    snap = {k: v for d in m.wandb_run.logged for k, v in d.items() if k.endswith("_mse")}
    assert sorted(snap) == ["snap/mod1_mse", "snap/mod2_mse"]
    meta["snapshots"] = {"seed": sd, "epoch": 5, "num": 8, "mse": snap, "min_margin": sub.min_margin}
    m.wandb_run = None
    before = len(s.log)
    with MF.Substitute(s):
        assert m._log_snapshots(epoch=5) is None
    assert len(s.log) == before                       # no wandb_run: nothing, no draws

    meta["recipe"] = ("ref_bimodal_small.pkl; prototypes of case_bimodal_small (DrawStream(seed)), rows from DrawStream(seed + vseed): "
                      "X1=|proto1[yi]-(u(N,100)>.9)|, X2=|proto2[yi]-(u(N,64)>.92)|, cum_area=sum(X1)+.25*u(N), convex_hull=X1@linspace(.5,1.5,100), "
                      "density=cum_area/convex_hull, labels=yi+1; val_loader batches of 8; torch.bernoulli(p) = (p > U), U from DrawStream(seed)")
    path = os.path.join(HERE, "bimodal_logging_small.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **out)
    print(f"wrote bimodal_logging_small.npz: {os.path.getsize(path) / 1024:.1f} KiB")
    print(json.dumps({k: meta[k] for k in ("margins", "traj", "traj3d", "snapshots", "probe")}, indent=1)[:3000])


if __name__ == "__main__":
    main()
