"""Latent-space logging of the iMDBN on the engine (reference ``imdbn/utils/imdbn_logging.py``, alias ``imdbn/utils/logging.py``).

Under its plotting, the reference module computes three things users read:

* **latent neighbours** of a validation sample's code, of the start and of the end of its TXT->IMG trajectory, in a cached
  bank of validation codes (``ensure_val_bank``).  The reference builds the full score row per query on the CPU, sorts it and
  walks it in Python, skipping the sample itself and (``dedup="image"``) every row whose image key ``(sum, sum of squares)``
  was already seen.  Here a whole batch of queries is one ``HipEngine.latent_topk`` call: a fused scoring GEMM and
  per-query key-deduplicated top-k (``csrc/kernels_knn.hpp``), no score matrix in memory;
* **TXT->IMG latent trajectories**: h = bernoulli(p(h|v)), v = p(v|h) with the label softmax, labels re-clamped, from
  ``z_class_mean[y]`` (else from the draw-free half-step pair from the clamped labels).  The reference runs them as B = 1
  loops with a host copy per step; here a batch is one ``HipEngine.chain_traced`` call (``latent_trajectory_batch``);
* **PCA projections** of the validation codes and the trajectory (the covariance on the device in fp64, its Dz x Dz
  eigendecomposition on the host; component signs as sklearn's ``svd_flip(u_based_decision=False)``), and the joint
  auto-reconstruction metrics.

The public functions keep the reference's names, parameter lists and return values; the B = 1 functions are thin wrappers
over the batched device forms ``latent_trajectory_batch`` / ``vecdb_neighbors_batch``.  Figures (matplotlib,
``wandb.Image``, torchvision grids, the ``panel_*`` renderings) are out of scope: a ``wandb_run`` on the model receives plain
scalars and dicts, and every ``log_*`` function returns the numbers it computed as a dict.  Importing this module imports
no plotting or logging package.

Random draws: a trajectory of T steps draws one ``[B, H]`` uniform per step (the engine's ambient draw source), the
reference's ``torch.bernoulli(h_prob)`` per step for B = 1.

The bank is built once per model and cached, as in the reference: it goes stale if training continues.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from imdbn import engine as _E

__all__ = ["log_latent_trajectory_with_recon_panel", "log_pca3_trajectory", "log_pca3_trajectory_with_recon_panel",
           "panel_with_gt_and_neighbors", "panel_gt_vs_decode_neighbors", "ensure_val_bank", "find_first_val_index_with_label",
           "topk_similar_in_latent", "log_vecdb_neighbors_for_traj", "log_neighbors_images", "log_joint_auto_recon",
           "latent_trajectory_batch", "vecdb_neighbors_batch", "pca_fit"]


def _eng(model):
    return _E.get_engine(model.joint_rbm.W.data)


def _run(model):
    return getattr(model, "wandb_run", None)


def _metric_id(metric: str) -> int:
    """The reference's metric strings: "cosine", "ip" / "inner", anything else = l2."""
    return 0 if metric == "cosine" else (1 if metric in ("ip", "inner") else 2)


def _val_sample(model, sample_idx: int):
    """(x_i [1, Npix] fp32, y_i [1, K] fp32) on the model's device, or (None, None): the reference's val_loader walk."""
    seen = 0
    for imgs, lbls in model.val_loader:
        b = imgs.size(0)
        if seen + b <= sample_idx:
            seen += b
            continue
        pos = sample_idx - seen
        if pos < 0:
            break
        return (imgs[pos:pos + 1].to(model.device).reshape(1, -1).float(), lbls[pos:pos + 1].to(model.device).float())
    return None, None


def _val_codes(model):
    from imdbn.utils.probe_utils import compute_val_embeddings_and_features
    return compute_val_embeddings_and_features(model.image_idbn, upto_layer=len(model.image_idbn.layers))


def _frame_count(model, n_frames, default=8):
    cfg = getattr(model, "logging_cfg", {}) or {}
    pca_cfg = ((cfg.get("logging") or {}).get("pca_trajectory") or {})
    return int(pca_cfg.get("n_frames", default)) if n_frames is None else int(n_frames)


def _frames(n_frames: int, n: int):
    """The reference's panel frame selection: unique ints of linspace(0, n - 1, max(2, n_frames))."""
    return np.unique(np.linspace(0, n - 1, max(2, int(n_frames)), dtype=int)).tolist()


# ---- PCA ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def pca_fit(Z: torch.Tensor, n_components: int):
    """PCA of the rows of ``Z``: ``(mean [D] fp64, components [n, D] fp64)`` on Z's device.  The covariance is formed on the
    device in fp64; its D x D eigendecomposition runs on the host.  Signs follow sklearn's ``svd_flip(u_based_decision=False)``
    (the largest-magnitude entry of every component is positive), so ``pca_project`` equals sklearn's ``transform`` up to
    rounding."""
    Zd = Z.double()
    mean = Zd.mean(0)
    Zc = Zd - mean
    C = (Zc.t() @ Zc).cpu().numpy()
    w, V = np.linalg.eigh(C)
    comp = V[:, np.argsort(w)[::-1][:int(n_components)]].T.copy()
    j = np.argmax(np.abs(comp), axis=1)
    comp *= np.sign(comp[np.arange(comp.shape[0]), j])[:, None]
    return mean, torch.from_numpy(comp).to(Z.device)


def pca_project(Z: torch.Tensor, mean: torch.Tensor, comp: torch.Tensor) -> torch.Tensor:
    return (Z.double() - mean) @ comp.t()


# ---- validation bank ----------------------------------------------------------------------------------------------------
@torch.no_grad()
def ensure_val_bank(model) -> None:
    """Build and cache the validation bank on ``model.device``: ``_Z_bank`` (engine ``represent`` per batch), ``_X_bank``,
    ``_Y_bank``, ``_H_bank`` (image keys: per-row sum and sum of squares of the flattened fp32 images) and ``_Z_bank_sumsq``
    (||z||^2).  Built once, as in the reference: it goes stale if training continues (delete ``_Z_bank`` to rebuild)."""
    if hasattr(model, "_Z_bank"):
        return
    dev = model.device
    Z_list, X_list, Y_list = [], [], []
    for imgs, lbls in model.val_loader:
        x = imgs.to(dev)
        Z_list.append(model.image_idbn.represent(x.reshape(x.size(0), -1).float()))
        X_list.append(x)
        Y_list.append(lbls.to(dev))
    Z = torch.cat(Z_list, 0)
    X = torch.cat(X_list, 0)
    eng = _E.get_engine(Z)
    model._Z_bank = Z
    model._X_bank = X
    model._Y_bank = torch.cat(Y_list, 0)
    model._H_bank = eng.row_stats(X.reshape(X.size(0), -1).float())
    model._Z_bank_sumsq = eng.row_stats(Z)[:, 1].contiguous()


@torch.no_grad()
def find_first_val_index_with_label(model, k: int) -> int:
    """Index of the first validation sample of class ``k`` (-1: none); one host read per batch."""
    idx = 0
    for _, lbls in model.val_loader:
        hits = torch.nonzero(lbls.argmax(1) == int(k)).flatten()
        if hits.numel():
            return idx + int(hits[0])
        idx += lbls.size(0)
    return -1


@torch.no_grad()
def topk_similar_in_latent(model, z_query: torch.Tensor, k: int = 8, metric: str = "cosine"):
    """Top-k rows of the validation bank for every query row: CPU ``(indices int64, scores fp32)`` ``[Q, min(k, N)]``
    (no dedup, no exclusion; k <= 64)."""
    assert hasattr(model, "_Z_bank"), "Call ensure_val_bank() first."
    Z = model._Z_bank
    zq = z_query.detach().to(Z.device).float()
    if zq.dim() == 1:
        zq = zq.unsqueeze(0)
    kk = min(int(k), Z.size(0))
    idx, sc = _E.get_engine(Z).latent_topk(Z, zq, _metric_id(metric), kk, bank_sumsq=getattr(model, "_Z_bank_sumsq", None))
    return idx.long().cpu(), sc.cpu()


# ---- trajectories --------------------------------------------------------------------------------------------------------
def _start_code(model, y: torch.Tensor) -> torch.Tensor:
    """z0 [B, Dz]: z_class_mean[argmax y], else p(v | p(h | v_known))[:, :Dz] (reference :756-763)."""
    Dz = int(model.Dz_img)
    zcm = getattr(model, "z_class_mean", None)
    if zcm is not None:
        return zcm.to(y.device)[y.argmax(1)].float()
    jr = model.joint_rbm
    vk = torch.zeros(y.size(0), Dz + y.size(1), device=y.device)
    vk[:, Dz:] = y
    return jr.visible_probs(jr.forward(vk))[:, :Dz]


@torch.no_grad()
def latent_trajectory_batch(model, lbls: torch.Tensor, steps: int) -> torch.Tensor:
    """TXT->IMG trajectories of a batch of one-hot labels as ONE traced chain: ``[steps + 1, B, Dz]`` device tensor, slot 0 the
    start code, slot t the code p(v|h) of step t (h sampled, v mean-field, labels re-clamped)."""
    dev = model.device
    y = lbls.to(dev).float()
    Dz = int(model.Dz_img)
    B, V = y.size(0), Dz + y.size(1)
    z0 = _start_code(model, y)
    v0 = torch.zeros(B, V, device=dev)
    v0[:, :Dz] = z0
    v0[:, Dz:] = y
    km = torch.zeros(B, V, device=dev)
    km[:, Dz:] = 1.0
    T = int(steps)
    out = torch.empty(T + 1, B, Dz, device=dev)
    out[0] = z0
    if T > 0:
        # the start state doubles as the clamp values: re-clamping reads only the label columns of v_known
        spec = {"v_known": v0, "mask": km, "init_uniform": False, "trace": (0, Dz, False),
                "steps": [{"T": 1.0, "sigma": 0.0, "eta": 0.0, "sample_h": True, "vmode": 0, "clamp": True}] * T}
        ((_, tr),) = _eng(model).chain_traced(model.joint_rbm, spec, None, model.joint_rbm._rng(B))
        out[1:] = tr
    return out


@torch.no_grad()
def vecdb_neighbors_batch(model, sample_idx, steps: Optional[int] = None, k: int = 8, metric: str = "cosine",
                          dedup: Optional[str] = "index", exclude_self: bool = True, also_l2: bool = True, all_steps: bool = False) -> dict:
    """Neighbours of validation samples ``sample_idx`` [B] and of their TXT->IMG trajectories, as device tensors:

    * ``Z_traj`` [T+1, B, Dz], ``z_true`` [B, Dz] (``represent`` of the images);
    * ``idx`` / ``score`` [3, B, k] for the queries z_true, z0, zT under ``metric`` (padded with -1 / -inf);
    * ``idx_l2`` / ``score_l2`` [B, k] for zT under l2 (``also_l2``);
    * ``idx_steps`` / ``score_steps`` [T+1, B, k] for every trajectory step under ``metric`` (``all_steps``).

    ``metric="cosine"`` is the reference's score of this function: the inner product of L1-normalised rows (its
    ``F.normalize(x, 1)`` passes p = 1); ``topk_similar_in_latent``'s cosine is the L2 one.
    ``dedup="image"`` keeps one row per image key ``_H_bank`` (the reference's pixel sum / sum of squares: images with equal
    pixel counts collide), ``"index"`` and ``None`` keep every row; ``exclude_self`` removes the sample's own bank row."""
    ensure_val_bank(model)
    Z, X, Y = model._Z_bank, model._X_bank, model._Y_bank
    dev = Z.device
    si = torch.as_tensor(sample_idx, device=dev).reshape(-1).long()
    B = si.numel()
    T = int(model.cross_steps if steps is None else steps)
    traj = latent_trajectory_batch(model, Y[si], T)
    z_true = model.image_idbn.represent(X[si].reshape(B, -1).float()).to(dev)
    eng = _E.get_engine(Z)
    key = model._H_bank if dedup == "image" else None
    bss = getattr(model, "_Z_bank_sumsq", None)
    ex = si.int() if exclude_self else None

    def search(q, m, rep):
        return eng.latent_topk(Z, q, m, k, exclude=ex.repeat(rep) if ex is not None else None, key=key, bank_sumsq=bss)

    m = _metric_id(metric)
    if m == 0:
        # the reference's "cosine" here is F.normalize(x, 1): p = 1, an L1 normalisation (reference :784) -- kept as the spec:
        # the inner product of L1-normalised rows
        Zl1 = torch.nn.functional.normalize(Z, 1)

        def search_m(q, rep):
            return eng.latent_topk(Zl1, torch.nn.functional.normalize(q, 1), 1, k, exclude=ex.repeat(rep) if ex is not None else None,
                                   key=key)
    else:
        def search_m(q, rep):
            return search(q, m, rep)
    qs = torch.cat([z_true, traj[0], traj[-1]], 0)
    idx, sc = search_m(qs, 3)
    out = {"Z_traj": traj, "z_true": z_true, "idx": idx.view(3, B, -1), "score": sc.view(3, B, -1)}
    if also_l2:
        if m == 2:
            out["idx_l2"], out["score_l2"] = out["idx"][2], out["score"][2]
        else:
            out["idx_l2"], out["score_l2"] = search(traj[-1], 2, 1)
    if all_steps:
        i2, s2 = search_m(traj.reshape((T + 1) * B, -1), T + 1)
        out["idx_steps"], out["score_steps"] = i2.view(T + 1, B, -1), s2.view(T + 1, B, -1)
    return out


# ---- panels as numbers ---------------------------------------------------------------------------------------------------
@torch.no_grad()
def panel_with_gt_and_neighbors(model, panel_title: str, gt_img: torch.Tensor, neighbor_imgs: torch.Tensor, neighbor_indices: torch.Tensor,
                                neighbor_scores: torch.Tensor, tag_key: str):
    """The numbers of the reference's GT + neighbours figure: ranks' bank indices, scores and labels (``_Y_bank`` argmax)."""
    ids = [int(i) for i in torch.as_tensor(neighbor_indices).reshape(-1).tolist()]
    labels = [int(v) for v in model._Y_bank.argmax(1)[torch.as_tensor(ids, dtype=torch.long, device=model._Y_bank.device)].tolist()] if ids else []
    d = {"title": panel_title, "indices": ids, "scores": [float(s) for s in torch.as_tensor(neighbor_scores).reshape(-1).tolist()],
         "labels": labels}
    run = _run(model)
    if run:
        run.log({tag_key: d})
    return d


@torch.no_grad()
def panel_gt_vs_decode_neighbors(model, panel_title: str, neighbor_indices: torch.Tensor, tag_key: str):
    """The numbers of the reference's GT vs Decode(z) figure: per neighbour the MSE between its image and the decode of its code."""
    pick = torch.as_tensor(neighbor_indices).to(device=model._Z_bank.device, dtype=torch.long).reshape(-1)
    X = model._X_bank[pick].reshape(pick.numel(), -1).float()
    rec = model.image_idbn.decode(model._Z_bank[pick].float())
    mse = ((rec - X) ** 2).mean(1)
    d = {"title": panel_title, "indices": pick.tolist(), "decode_mse": mse.double().tolist()}
    run = _run(model)
    if run:
        run.log({tag_key: d})
    return d


@torch.no_grad()
def log_neighbors_images(model, indices: torch.Tensor, tag: str):
    """The reference logs a grid of the bank images of ``indices[0]``; here their bank indices and labels."""
    pick = torch.as_tensor(indices)[0].to(torch.long)
    d = {"indices": pick.tolist(), "labels": model._Y_bank.argmax(1)[pick.to(model._Y_bank.device)].tolist()}
    run = _run(model)
    if run:
        run.log({tag: d})
    return d


def _trim(idx: torch.Tensor, sc: torch.Tensor):
    """One query's padded device row -> the reference's ``[1, n]`` CPU (int64, fp32) pair."""
    i, s = idx.cpu(), sc.cpu()
    n = int((i >= 0).sum())
    return i[:n].long().unsqueeze(0), s[:n].unsqueeze(0)


@torch.no_grad()
def log_vecdb_neighbors_for_traj(model, sample_idx: int = 0, steps: Optional[int] = None, k: int = 8, metric: str = "cosine",
                                 tag: str = "vecdb", also_l2: bool = True, dedup: str = "index", exclude_self: bool = True):
    """Reference :702-891 for one validation sample: the TXT->IMG trajectory, the deduplicated neighbours of z_true / z0 / zT
    (and of zT under l2), the panels' numbers.  Returns a dict with ``Z_traj`` [T+1, Dz] (numpy), ``idx_<q>`` / ``sc_<q>``
    (``[1, n]`` CPU tensors, q in true, z0, zT, zT_l2) and ``decode`` (the GT vs Decode(z) numbers of zT's neighbours);
    None when ``sample_idx`` is outside the validation set."""
    ensure_val_bank(model)
    N = model._Z_bank.size(0)
    if not (0 <= int(sample_idx) < N):
        run = _run(model)
        if run:
            run.log({f"{tag}/warn": "sample_idx out of range"})
        return None
    o = vecdb_neighbors_batch(model, [int(sample_idx)], steps=steps, k=k, metric=metric, dedup=dedup, exclude_self=exclude_self,
                              also_l2=also_l2)
    res = {"Z_traj": o["Z_traj"][:, 0].cpu().numpy()}
    gt = model._X_bank[int(sample_idx)].reshape(1, -1).float()
    names = (("true", "Neighbors of z_true with GT", "knn_true_with_gt"), ("z0", "Neighbors of z0 with GT", "knn_z0_with_gt"),
             ("zT", "Neighbors of zT with GT", "knn_zT_with_gt"))
    for j, (nm, title, key) in enumerate(names):
        res["idx_" + nm], res["sc_" + nm] = _trim(o["idx"][j, 0], o["score"][j, 0])
    for j, (nm, title, key) in enumerate(names):
        log_neighbors_images(model, res["idx_" + nm], f"{tag}/knn_{'z_true' if nm == 'true' else nm}")
    for nm, title, key in names:
        i = res["idx_" + nm]
        panel_with_gt_and_neighbors(model, title, gt, model._X_bank[i[0].to(model._X_bank.device)], i[0], res["sc_" + nm][0], f"{tag}/{key}")
    if also_l2:
        res["idx_zT_l2"], res["sc_zT_l2"] = _trim(o["idx_l2"][0], o["score_l2"][0])
        i = res["idx_zT_l2"]
        panel_with_gt_and_neighbors(model, "Neighbors of zT (L2) with GT", gt, model._X_bank[i[0].to(model._X_bank.device)], i[0],
                                    res["sc_zT_l2"][0], f"{tag}/knn_zT_l2_with_gt")
    res["decode"] = panel_gt_vs_decode_neighbors(model, "Neighbors of zT — GT vs Decode(z)", res["idx_zT"][0], f"{tag}/knn_zT_gt_vs_decode")
    return res


# ---- PCA trajectories ------------------------------------------------------------------------------------------------------
@torch.no_grad()
def log_pca3_trajectory(model, sample_idx: int, steps: int = 40, tag: str = "pca3_traj"):
    """Reference :256-329: PCA-3 of the validation codes and the projected TXT->IMG trajectory of one sample.  Returns
    ``{"Z_traj" [T+1, Dz], "Z3" [N, 3], "T3" [T+1, 3], "mean", "components"}`` (numpy) or None."""
    run = _run(model)
    Z_val, _ = _val_codes(model)
    if Z_val is None or Z_val.numel() == 0:
        if run:
            run.log({f"{tag}/warn": "no val embeddings"})
        return None
    x_i, y_i = _val_sample(model, int(sample_idx))
    if x_i is None:
        if run:
            run.log({f"{tag}/warn": "sample not found"})
        return None
    traj = latent_trajectory_batch(model, y_i, int(steps))[:, 0]
    mean, comp = pca_fit(Z_val, 3)
    Z3, T3 = pca_project(Z_val, mean, comp), pca_project(traj, mean, comp)
    out = {"Z_traj": traj.cpu().numpy(), "Z3": Z3.cpu().numpy(), "T3": T3.cpu().numpy(), "mean": mean.cpu().numpy(),
           "components": comp.cpu().numpy()}
    if run:
        run.log({f"{tag}/pca3": {"trajectory": out["T3"].tolist()}})
    return out


def _recon_panel_common(model, sample_idx, n_comp, tag):
    run = _run(model)
    assert model.val_loader is not None, "val_loader is None"
    Z_val, feats = _val_codes(model)
    if Z_val is None or Z_val.numel() == 0:
        if run:
            run.log({f"{tag}/warn": "no val embeddings"})
        return None
    N_val = Z_val.size(0)
    sample_idx = int(max(0, min(int(sample_idx), N_val - 1)))
    mean, comp = pca_fit(Z_val, n_comp)
    x_i, y_i = _val_sample(model, sample_idx)
    if x_i is None:
        if run:
            run.log({f"{tag}/warn": "sample not found"})
        return None
    return sample_idx, Z_val, mean, comp, x_i, y_i


@torch.no_grad()
def log_pca3_trajectory_with_recon_panel(model, sample_idx: int = 0, steps: int = 40, tag: str = "pca3_traj_with_recon", n_frames: int = None,
                                         scatter_size: int = None, scatter_alpha: float = None, elev: Optional[float] = None,
                                         azim: Optional[float] = None):
    """Reference :332-540: PCA-3 of the validation codes, the sample's projected TXT->IMG trajectory and the decoded frames
    of the panel.  Returns ``{"Z3", "z_true_3d", "traj3" [T+1, 3], "Z_traj", "sel_idx", "frames" [n_sel, Npix] (clamped
    decodes), "gt_class"}`` or None.  (``scatter_size`` / ``scatter_alpha`` / ``elev`` / ``azim`` only styled the figure.)"""
    c = _recon_panel_common(model, sample_idx, 3, tag)
    if c is None:
        return None
    sample_idx, Z_val, mean, comp, x_i, y_i = c
    n_frames = _frame_count(model, n_frames)
    traj = latent_trajectory_batch(model, y_i, int(steps))[:, 0]
    sel = _frames(n_frames, traj.size(0))
    frames = model.image_idbn.decode(traj[sel]).clamp(0, 1)
    Z3 = pca_project(Z_val, mean, comp)
    out = {"Z3": Z3.cpu().numpy(), "z_true_3d": Z3[sample_idx:sample_idx + 1].cpu().numpy(),
           "traj3": pca_project(traj, mean, comp).cpu().numpy(), "Z_traj": traj.cpu().numpy(), "sel_idx": sel,
           "frames": frames.cpu().numpy(), "gt_class": int(y_i.argmax(1)[0])}
    run = _run(model)
    if run:
        run.log({f"{tag}/plot": {"sample_idx": sample_idx, "gt_class": out["gt_class"], "steps": int(steps), "sel_idx": sel,
                                 "trajectory": out["traj3"].tolist()}})
    return out


@torch.no_grad()
def log_latent_trajectory_with_recon_panel(model, sample_idx: int = 0, steps: int = 40, tag: str = "pca_traj_with_recon", n_frames: int = None,
                                           scatter_size: int = None, scatter_alpha: float = None):
    """Reference :22-253: PCA-2 of the validation codes; the trajectory is the start code, the code of the image
    ``model._cross_reconstruct`` generates, and ``min(steps // 5, 8) - 1`` linear interpolations between the two (in this order,
    as the reference has it).  Returns ``{"Z2", "z_true_2d", "traj" [n, 2], "points" [n, Dz], "sel_idx", "frames", "gt_class"}``
    or None."""
    c = _recon_panel_common(model, sample_idx, 2, tag)
    if c is None:
        return None
    sample_idx, Z_val, mean, comp, x_i, y_i = c
    n_frames = _frame_count(model, n_frames)
    z_init = _start_code(model, y_i)
    img_from_txt, _ = model._cross_reconstruct(model.image_idbn.represent(x_i), y_i, steps=steps)
    z_final = model.image_idbn.represent(img_from_txt.reshape(1, -1))
    num = min(int(steps / 5), 8)
    alphas = torch.tensor([i / num for i in range(1, num)], dtype=torch.float64, device=z_init.device)
    z_interp = ((1 - alphas)[:, None] * z_init.double() + alphas[:, None] * z_final.double()).float()
    points = torch.cat([z_init, z_final.float(), z_interp], 0)
    recon = torch.cat([model.image_idbn.decode(z_init), img_from_txt.reshape(1, -1).float()]
                      + ([model.image_idbn.decode(z_interp)] if num > 1 else []), 0).clamp(0, 1)
    sel = _frames(n_frames, points.size(0))
    Z2 = pca_project(Z_val, mean, comp)
    out = {"Z2": Z2.cpu().numpy(), "z_true_2d": Z2[sample_idx:sample_idx + 1].cpu().numpy(), "traj": pca_project(points, mean, comp).cpu().numpy(),
           "points": points.cpu().numpy(), "sel_idx": sel, "frames": recon[sel].cpu().numpy(), "gt_class": int(y_i.argmax(1)[0])}
    run = _run(model)
    if run:
        run.log({f"{tag}/plot": {"sample_idx": sample_idx, "gt_class": out["gt_class"], "steps": int(steps), "sel_idx": sel,
                                 "trajectory": out["traj"].tolist()}})
    return out


# ---- joint auto-reconstruction ----------------------------------------------------------------------------------------------
@torch.no_grad()
def log_joint_auto_recon(model, epoch: int, num: int = 8):
    """Reference :911-965: image -> code -> joint up / down -> (code, labels) -> image for the first ``num`` validation images;
    text top-1, text BCE and image MSE computed on the device and read back once.  Logs the reference's keys; returns
    ``{"text_top1", "text_bce", "image_mse"}`` (None without a ``wandb_run`` or validation images, as the reference returns)."""
    run = _run(model)
    if run is None or getattr(model, "validation_images", None) is None or getattr(model, "validation_labels", None) is None:
        return None
    imgs = model.validation_images[:num]
    lbls = model.validation_labels[:num].to(model.device).float()
    B = imgs.size(0)
    x = imgs.reshape(B, -1).to(model.device).float()
    z_top = model.image_idbn.represent(x)
    jr = model.joint_rbm
    v_recon = jr.backward(jr.forward(torch.cat([z_top, lbls], dim=1)))
    Dz = int(model.Dz_img)
    y_hat = v_recon[:, Dz:]
    rec = model.image_idbn.decode(v_recon[:, :Dz]).clamp(0, 1)
    top1 = (y_hat.argmax(1) == lbls.argmax(1)).float().mean()
    bce = torch.nn.functional.binary_cross_entropy(y_hat.clamp(1e-6, 1 - 1e-6), lbls)
    mse = ((x - rec.reshape(B, -1)) ** 2).mean()
    t1, tb, im = torch.stack([top1, bce, mse]).double().tolist()
    run.log({"auto_recon/gt_vs_joint": {"n": B}, "epoch": epoch})
    run.log({"auto_recon/text_top1": t1, "epoch": epoch})
    run.log({"auto_recon/text_bce": tb, "epoch": epoch})
    run.log({"auto_recon/image_mse": im, "epoch": epoch})
    return {"text_top1": t1, "text_bce": tb, "image_mse": im}
