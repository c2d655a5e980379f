#!/usr/bin/env python3
"""Generate tests/golden/logging_small.npz: the reference's latent logging (imdbn/utils/imdbn_logging.py) on the trained small
iMDBN of imdbn_small_100_40_20_j16.npz.

Run in the build container only (needs the reference checkout, as make_fixtures.py does):

    python tests/golden/make_logging_fixtures.py

The UNMODIFIED reference functions run on the duck-typed model of make_trace_fixtures.py.  ``torch.bernoulli`` (the
trajectory's only draw) is routed through a ``DrawStream`` here, as ``(p > U)``, and the smallest |p - U| is recorded;
``panel_with_gt_and_neighbors`` / ``panel_gt_vs_decode_neighbors`` are replaced by recorders of what the reference passes
them, sklearn's ``PCA`` by a subclass that records its transforms, and the torchvision grid by an empty image.  The
generator checks with the fp64 oracle that no recorded top-k boundary is a near-tie, so tests may compare indices exactly.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_trace_fixtures as MT  # noqa: E402  (make_fixtures: reference on sys.path, wandb / torchvision stubs)

import torch  # noqa: E402
import matplotlib  # noqa: E402

matplotlib.use("Agg")
import sklearn.decomposition  # noqa: E402

import logging_oracle as LO  # noqa: E402
from oracle.draws import DrawStream  # noqa: E402
from imdbn.utils import imdbn_logging as RL  # noqa: E402  (the reference module)

STEPS, K = 12, 8
TIE = 1e-5          # smallest score gap at a recorded top-k boundary, relative to the largest |score| of the query
DRAW = 1e-4         # smallest |p - U| of a recorded trajectory

sys.modules["torchvision.utils"].make_grid = lambda X, nrow=8: torch.zeros(3, 2, 2)
sys.modules["wandb"].Image = lambda x: None


class Bernoulli:
    """torch.bernoulli(p) -> (p > U) with U from a DrawStream; records the smallest |p - U|."""

    def __init__(self, seed):
        self.s, self.margin = DrawStream(seed), float("inf")

    def __enter__(self):
        self._b = torch.bernoulli

        def bern(p, *a, **kw):
            u = torch.from_numpy(self.s.uniform(tuple(p.shape))).to(p.dtype)
            self.margin = min(self.margin, float((p - u).abs().min()))
            return (p > u).to(p.dtype)

        torch.bernoulli = bern
        return self

    def __exit__(self, *a):
        torch.bernoulli = self._b


class Recorder:
    def __init__(self):
        self.panels, self.decode, self.pca = [], [], []

    def __enter__(self):
        self._p, self._d, self._pca = RL.panel_with_gt_and_neighbors, RL.panel_gt_vs_decode_neighbors, sklearn.decomposition.PCA
        rec = self

        def panel(model, panel_title, gt_img, neighbor_imgs, neighbor_indices, neighbor_scores, tag_key):
            rec.panels.append((tag_key, neighbor_indices.numpy().astype(np.int32), neighbor_scores.numpy().astype(np.float64)))

        def decode(model, panel_title, neighbor_indices, tag_key):
            pick = neighbor_indices.to(torch.long)
            X = model._X_bank[pick].reshape(len(pick), -1).float()
            rec_ = model.image_idbn.decode(model._Z_bank[pick].float())
            rec.decode.append(((rec_ - X) ** 2).mean(1).double().numpy())

        class PCA(self._pca):
            def transform(self_, X):
                out = super().transform(X)
                rec.pca.append((np.asarray(X, np.float64), np.asarray(out, np.float64)))
                return out

        RL.panel_with_gt_and_neighbors, RL.panel_gt_vs_decode_neighbors = panel, decode
        sklearn.decomposition.PCA = PCA
        return self

    def __exit__(self, *a):
        RL.panel_with_gt_and_neighbors, RL.panel_gt_vs_decode_neighbors = self._p, self._d
        sklearn.decomposition.PCA = self._pca


def model(z, X, Y):
    m = MT.model(z, X, Y)
    m.image_idbn.val_loader = m.val_loader
    m.image_idbn.features = {"Labels": torch.from_numpy(Y)}
    m.cross_steps = STEPS
    return m


def check_ties(Z, H, q, metric, k, exclude, keyed, what):
    _, _, margin = LO.topk(Z, q, metric, k, exclude=None if exclude is None else [exclude], key=H if keyed else None)
    scale = float(np.abs(LO.scores(Z, q, metric)).max())
    assert margin[0] > TIE * scale, f"{what}: near-tie at the top-k boundary ({margin[0]:.2e}, scores up to {scale:.2e})"


def main():
    z, X, Y = MT.data()
    out, meta = {}, {"steps": STEPS, "k": K, "cases": [], "funcs": {}}
    import inspect
    for f in RL.__dict__:
        obj = getattr(RL, f)
        if inspect.isfunction(obj) and obj.__module__ == RL.__name__:
            meta["funcs"][f] = list(inspect.signature(obj).parameters)
    # 1. neighbours of z_true / z0 / zT (+ zT under l2) along a trajectory: dedup x exclude x metric
    cases = [(5, "cosine", "image", True, 7001), (17, "cosine", "index", True, 7002), (40, "ip", None, False, 7003),
             (3, "l2", "image", False, 7004), (101, "inner", "image", True, 7005), (250, "cosine", None, True, 7006)]
    for ci, (si, metric, dedup, excl, seed) in enumerate(cases):
        m = model(z, X, Y)
        for sd in range(seed, seed + 50):                         # a seed whose draws are all clear of p
            with Bernoulli(sd) as b, Recorder() as r:
                RL.log_vecdb_neighbors_for_traj(m, sample_idx=si, steps=STEPS, k=K, metric=metric, dedup=dedup, exclude_self=excl)
            if b.margin > DRAW:
                break
            del m._Z_bank
        else:
            raise AssertionError("no seed with robust draws")
        Zb, H = m._Z_bank.numpy(), m._H_bank.numpy()
        assert len(r.panels) == 4 and len(r.decode) == 1
        pre = f"c{ci}_"
        for tag, ids, sc in r.panels:
            name = tag.split("/knn_")[1].replace("_with_gt", "")
            out[pre + name + "_idx"], out[pre + name + "_sc"] = ids, sc
        out[pre + "decode_mse"] = r.decode[0]
        # the trajectory replayed in the oracle: its neighbour lists must be the reference's
        zq = {"true": m.image_idbn.represent(torch.from_numpy(X[si:si + 1])).numpy()}
        u = DrawStream(sd).uniform((STEPS, 1, 16))
        traj, _ = LO.trajectory(z["joint_W"].astype(np.float64), z["joint_hid_bias"].astype(np.float64), z["joint_vis_bias"].astype(np.float64),
                                [(20, 28)], z["z_class_mean"][Y[si:si + 1].argmax(1)], Y[si:si + 1], u)
        zq["z0"], zq["zT"] = traj[0], traj[-1]
        om = "cosine_l1" if metric == "cosine" else metric
        for name, q, met in (("true", zq["true"], om), ("z0", zq["z0"], om), ("zT", zq["zT"], om), ("zT_l2", zq["zT"], "l2")):
            check_ties(Zb, H, q, met, K, si if excl else None, dedup == "image", f"case {ci} {name}")
            ids, _, _ = LO.topk(Zb, q, met, K, exclude=[si] if excl else None, key=H if dedup == "image" else None)
            np.testing.assert_array_equal(ids[0][ids[0] >= 0], out[pre + name + "_idx"], err_msg=f"oracle vs reference, case {ci} {name}")
        meta["cases"].append({"sample_idx": si, "metric": metric, "dedup": dedup, "exclude_self": excl, "seed": sd,
                              "min_draw_margin": b.margin})
    # the image-key quirk is exercised: some neighbour list under dedup="image" skipped a colliding key
    m = model(z, X, Y)
    RL.ensure_val_bank(m)
    H = m._H_bank.numpy()
    meta["n_distinct_keys"] = int(len({(a, b) for a, b in H}))
    assert meta["n_distinct_keys"] < len(H)
    # 2. topk_similar_in_latent: no dedup, no exclusion, every metric
    g = np.random.Generator(np.random.PCG64(11))
    cand = np.concatenate([m._Z_bank.numpy()[np.arange(7, 416, 13)], g.random((32, 20), dtype=np.float32)], 0)
    tied = lambda r: any(LO.topk(m._Z_bank.numpy(), cand[r:r + 1], met, K)[2][0]         # noqa: E731
                         <= TIE * float(np.abs(LO.scores(m._Z_bank.numpy(), cand[r:r + 1], met)).max()) for met in ("cosine", "ip", "l2"))
    keep = [r for r in range(len(cand)) if not tied(r)]
    q = cand[[r for r in keep if r < 32][:3] + [r for r in keep if r >= 32][:3]]
    assert len(q) == 6
    out["topk_q"] = q
    for met in ("cosine", "ip", "l2"):
        i, v = RL.topk_similar_in_latent(m, torch.from_numpy(q), k=K, metric=met)
        out[f"topk_{met}_idx"], out[f"topk_{met}_sc"] = i.numpy().astype(np.int32), v.numpy().astype(np.float64)
        for r in range(len(q)):
            check_ties(m._Z_bank.numpy(), None, q[r:r + 1], met, K, None, False, f"topk_similar {met} row {r}")
    # 3. PCA-3 trajectory: the recorded PCA transforms (validation codes, then the trajectory)
    seed = 7101
    m = model(z, X, Y)
    for sd in range(seed, seed + 50):
        with Bernoulli(sd) as b, Recorder() as r:
            RL.log_pca3_trajectory(m, sample_idx=9, steps=STEPS)
        if b.margin > DRAW:
            break
    assert len(r.pca) == 2
    out["pca3_Ztraj"], out["pca3_T3"] = r.pca[1][0].astype(np.float32), r.pca[1][1]
    out["pca3_Z3"] = r.pca[0][1]
    meta["pca3"] = {"sample_idx": 9, "seed": sd, "min_draw_margin": b.margin}
    # 4. joint auto-reconstruction metrics
    m = model(z, X, Y)
    m.wandb_run = MT.StubRun()
    m.validation_images, m.validation_labels = torch.from_numpy(X[:8]), torch.from_numpy(Y[:8])
    RL.log_joint_auto_recon(m, epoch=3, num=8)
    meta["auto_recon"] = {k: v for d in m.wandb_run.logged for k, v in d.items() if k != "auto_recon/gt_vs_joint"}
    meta["recipe"] = ("model of make_trace_fixtures.py (imdbn_small_100_40_20_j16.npz), val_loader batches of 8; reference imdbn_logging "
                      "functions, torch.bernoulli(p) = (p > U), U from DrawStream(seed)")
    path = os.path.join(HERE, "logging_small.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **out)
    print(f"wrote logging_small.npz: {os.path.getsize(path) / 1024:.1f} KiB; distinct keys {meta['n_distinct_keys']} of {len(H)}")
    for c in meta["cases"]:
        print(c)
    print("auto_recon", meta["auto_recon"])


if __name__ == "__main__":
    main()
