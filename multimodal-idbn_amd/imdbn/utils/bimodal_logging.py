"""The observability side-car of ``iMDBN_BiModal`` on the engine (reference ``imdbn/models/imdbn_bimodal.py`` :43-419, the
PCA block of ``train_joint`` :856-912, ``_log_snapshots`` :963-1015, and the Spearman numbers of ``imdbn/utils/wandb_utils.py``).

Under its plotting, the reference computes four things users read:

* **joint embeddings** of the validation set and **linear probes** on them (``compute_bimodal_joint_embeddings_and_features``,
  ``log_bimodal_joint_linear_probe``): engine ``represent`` calls concatenated on the device, then the probe machinery of
  ``probe_utils``;
* **MOD2->MOD1 trajectories in the joint hidden space**: v0 = the clamped MOD2 code with zeros in the MOD1 columns, one
  mean-field step, then ``steps`` steps with sampled hidden units, mean-field visibles and the MOD2 code re-clamped.  The
  reference runs them as B = 1 loops with two host copies and a decode per step; here N samples are ONE
  ``HipEngine.chain_traced_vh`` call whose hidden trace is ``traj_h`` and whose visible trace over the MOD1 columns is
  ``traj_z1`` (``bimodal_trajectory_batch``), and only the frames that are shown are decoded;
* **PCA projections** of the joint hidden activations / MOD1 codes / MOD2 codes and of the trajectories
  (``imdbn_logging.pca_fit`` / ``pca_project``);
* **Spearman correlations** of every projected dimension with every feature (``embedding_correlations``): average ranks on the
  device (sort + ``unique_consecutive``), the numeric core of ``plot_{2,3}d_embedding_and_correlations``.

The reference's names and parameter lists are kept (and re-exported from ``imdbn.models.imdbn_bimodal``); the B = 1 functions
are thin wrappers over the batched forms.  Figures (matplotlib, ``wandb.Image``, torchvision grids) are out of scope: a
``wandb_run`` on the model receives plain scalars only, and every function returns the numbers it computed.  Importing this module
imports no plotting or logging package.

Random draws: a trajectory of ``steps`` steps draws one ``[N, H]`` uniform per sampled step (the engine's ambient draw source), the
reference's ``torch.bernoulli(h_prob)`` per step for B = 1; step 0 draws nothing.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from imdbn import engine as _E
from imdbn.utils.batches import batches, rows_on_device
from imdbn.utils.imdbn_logging import pca_fit, pca_project
from imdbn.utils import probe_utils as _P

__all__ = ["compute_bimodal_joint_embeddings_and_features", "log_bimodal_joint_linear_probe", "bimodal_trajectory_batch",
           "log_bimodal_latent_trajectory", "log_bimodal_latent_trajectory_3d", "embedding_correlations", "bimodal_pca_summary",
           "log_snapshots"]

_FEATS = (("Cumulative Area", "cum_area"), ("Convex Hull", "convex_hull"), ("Labels", "labels"), ("Density", "density"))


def _run(model):
    return getattr(model, "wandb_run", None)


def _eng(model):
    return _E.get_engine(model.joint_rbm.W.data)


def _val_pairs(model):
    for mod1, mod2 in batches(model.val_loader):
        yield rows_on_device(mod1, model.device), rows_on_device(mod2, model.device)


@torch.no_grad()
def _val_codes(model) -> Tuple[torch.Tensor, torch.Tensor]:
    """(Z1 [N, Dz1], Z2 [N, Dz2]): the modality codes of the whole validation loader, on the device."""
    z1, z2 = [], []
    for v1, v2 in _val_pairs(model):
        z1.append(model.mod1_dbn.represent(v1))
        z2.append(model.mod2_dbn.represent(v2))
    if not z1:
        dev = model.device
        return torch.empty(0, int(model.Dz_mod1), device=dev), torch.empty(0, int(model.Dz_mod2), device=dev)
    return torch.cat(z1, 0), torch.cat(z2, 0)


def _feats(model) -> Dict[str, torch.Tensor]:
    out = {}
    src = getattr(model, "features", None)
    if src is not None:
        for key, name in _FEATS:
            if key in src:
                out[name] = src[key]
    return out


# ---- embeddings and probes ---------------------------------------------------------------------------------------------------
@torch.no_grad()
def compute_bimodal_joint_embeddings_and_features(model):
    """Reference :43-73: ``(E [N, H_top], feats)``: the top joint layer's activations of the whole validation loader (one pass,
    engine ``represent`` calls concatenated on the device -- the reference returns a CPU tensor) and the feature dict
    ``{"cum_area", "convex_hull", "labels"[, "density"]}`` taken from ``model.features``."""
    embeds = [model.represent((v1, v2)) for v1, v2 in _val_pairs(model)]
    E = torch.cat(embeds, 0) if embeds else torch.empty(0, device=model.device)
    return E, _feats(model)


@torch.no_grad()
def log_bimodal_joint_linear_probe(model, epoch, n_bins=5, test_size=0.2, steps=1000, lr=1e-2, patience=20, min_delta=0.0,
                                   metric_prefix="joint", save_csv=False):
    """Reference :76-152: linear probes of the joint embeddings on the binned features (cum_area, convex_hull, labels, density
    when present), through ``probe_utils._run_probes`` (split seed 42).  Logs ``probe/{metric_prefix}/{mkey}/acc`` (an empty
    split: ``.../warn_empty_split/acc``); returns ``{f"{metric_prefix}/{mkey}": (acc, confusion [n_bins, n_bins])}`` (the
    reference only logs), None without embeddings."""
    E, feats = compute_bimodal_joint_embeddings_and_features(model)
    if E.numel() == 0:
        return None
    feats = {k: torch.as_tensor(v).reshape(-1).to(device=E.device, dtype=torch.float32) for k, v in feats.items()}
    res = _P._run_probes(model, E, feats, epoch, metric_prefix, n_bins, test_size, steps, lr, 42, patience, min_delta, save_csv)
    return {k: (v["acc"], v["confusion"]) for k, v in res.items()}


# ---- trajectories ---------------------------------------------------------------------------------------------------------------
def _val_rows(model, sample_idx) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rows ``sample_idx`` of the validation loader as (v1 [N, Npix1], v2 [N, Npix2]) on the device: one walk over the loader."""
    want = [int(i) for i in sample_idx]
    got1, got2 = {}, {}
    seen = 0
    for mod1, mod2 in batches(model.val_loader):
        b = mod1.size(0)
        for i in want:
            if seen <= i < seen + b and i not in got1:
                got1[i], got2[i] = mod1[i - seen:i - seen + 1], mod2[i - seen:i - seen + 1]
        seen += b
        if len(got1) == len(set(want)):
            break
    missing = [i for i in want if i not in got1]
    if missing:
        raise IndexError(f"validation samples {missing} not found ({seen} rows)")
    v1 = torch.cat([got1[i] for i in want], 0)
    v2 = torch.cat([got2[i] for i in want], 0)
    return rows_on_device(v1, model.device), rows_on_device(v2, model.device)


@torch.no_grad()
def bimodal_trajectory_batch(model, sample_idx, steps: int) -> dict:
    """The MOD2->MOD1 chains of reference :225-256 for the validation samples ``sample_idx`` [N] as ONE ``chain_traced_vh`` call:
    v0 = v_known (the MOD2 codes clamped, zeros in the MOD1 columns); step 0 is mean-field (h0 = p(h|v_known)), the ``steps``
    steps after it sample h; visibles stay mean-field and the MOD2 columns are re-clamped throughout.  Device tensors:

    * ``traj_h`` [steps + 1, N, H]: the joint hidden probabilities (h0, then what every step is about to sample);
    * ``traj_z1`` [steps + 1, N, Dz1]: the MOD1 code after every step (slot 0 = the reference's ``v_cur`` after ``h0``);
    * ``h_true`` [N, H] = p(h | [z1_true | z2_true]), ``z1_true``, ``z2_true``, and the images ``v1``."""
    v1, v2 = _val_rows(model, sample_idx)
    z1_true, z2_true = model.mod1_dbn.represent(v1), model.mod2_dbn.represent(v2)
    Dz1 = int(model.Dz_mod1)
    N_ = v1.size(0)
    vk, km = model._clamp(z2_true, Dz1, N_)
    jr = model.joint_rbm
    step = {"T": 1.0, "sigma": 0.0, "eta": 0.0, "sample_h": False, "vmode": 0, "clamp": True}
    spec = {"v_known": vk, "mask": km, "init_uniform": False, "trace": (0, Dz1, False), "trace_h": (0, int(jr.num_hidden)),
            "steps": [step] + [dict(step, sample_h=True)] * int(steps)}
    ((_, traj_z1, traj_h),) = _eng(model).chain_traced_vh(jr, spec, None, jr._rng(N_))
    return {"traj_h": traj_h, "traj_z1": traj_z1, "h_true": jr.forward(torch.cat([z1_true, z2_true], 1)),
            "z1_true": z1_true, "z2_true": z2_true, "v1": v1}


def _n_val(model) -> int:
    return sum(int(m1.size(0)) for m1, _ in batches(model.val_loader))


@torch.no_grad()
def log_bimodal_latent_trajectory(model, sample_idx: int = 0, steps: int = 50, tag: str = "trajectory", n_frames: int = 8):
    """Reference :155-334 for one validation sample: PCA-2 of the first joint layer's hidden activations of the whole validation
    set, the projected MOD2->MOD1 hidden trajectory and true point, and the decoded MOD1 frames of the panel.  Returns
    ``{"H2d" [N, 2], "traj_2d" [steps+1, 2], "h_true_2d" [1, 2], "traj_h" [steps+1, H], "sel_idx", "frames" [n_sel, Npix1]}``
    (numpy; ``frames`` are the clamped decodes of the selected steps only -- the reference decodes all ``steps + 1`` and shows
    these) or None without a ``val_loader`` / ``wandb_run``, as the reference returns.  The run receives ``{tag}/n_steps``."""
    run = _run(model)
    if model.val_loader is None or run is None:
        return None
    Z1, Z2 = _val_codes(model)
    if Z1.size(0) == 0:
        return None
    sample_idx = min(int(sample_idx), Z1.size(0) - 1)
    t = bimodal_trajectory_batch(model, [sample_idx], int(steps))
    traj_h = t["traj_h"][:, 0]
    H_all = model.joint_rbm.forward(torch.cat([Z1, Z2], 1))
    mean, comp = pca_fit(H_all, 2)
    sel = np.unique(np.linspace(0, int(steps), int(n_frames), dtype=int)).tolist()
    frames = model.mod1_dbn.decode(t["traj_z1"][sel, 0]).clamp(0, 1)
    out = {"H2d": pca_project(H_all, mean, comp).cpu().numpy(), "traj_2d": pca_project(traj_h, mean, comp).cpu().numpy(),
           "h_true_2d": pca_project(t["h_true"], mean, comp).cpu().numpy(), "traj_h": traj_h.cpu().numpy(), "sel_idx": sel,
           "frames": frames.cpu().numpy()}
    run.log({f"{tag}/n_steps": float(steps)})
    return out


@torch.no_grad()
def log_bimodal_latent_trajectory_3d(model, sample_idx: int = 0, steps: int = 50, tag: str = "trajectory"):
    """Reference :337-419: PCA-3 of the MOD1 codes of the validation set (``Z3`` [N, 3]) and the projected MOD1 trajectory (``T3``
    [steps+1, 3]); also ``traj_z1`` [steps+1, Dz1] (numpy).  None without a ``val_loader`` / ``wandb_run``.

    The reference's 3-D chain has no separate step 0: its ``traj_z[0]`` is ``v_cur`` after ``h0``, i.e. the visible result of
    the mean-field step -- slot 0 of ``bimodal_trajectory_batch``'s ``traj_z1``.  So the same ``steps + 1``-step chain serves this
    function and ``log_bimodal_latent_trajectory`` (same draws for the same sample)."""
    run = _run(model)
    if model.val_loader is None or run is None:
        return None
    Z1, _ = _val_codes(model)
    if Z1.size(0) == 0:
        return None
    sample_idx = min(int(sample_idx), Z1.size(0) - 1)
    traj = bimodal_trajectory_batch(model, [sample_idx], int(steps))["traj_z1"][:, 0]
    mean, comp = pca_fit(Z1, 3)
    out = {"Z3": pca_project(Z1, mean, comp).cpu().numpy(), "T3": pca_project(traj, mean, comp).cpu().numpy(),
           "traj_z1": traj.cpu().numpy()}
    run.log({f"{tag}/n_steps_3d": float(steps)})
    return out


# ---- Spearman ---------------------------------------------------------------------------------------------------------------------
def _avg_ranks(x: torch.Tensor) -> torch.Tensor:
    """Average ranks (1-based, ties share the mean of their positions) of a 1-D tensor, fp64, on x's device."""
    n = x.numel()
    xs, order = torch.sort(x)
    _, counts = torch.unique_consecutive(xs, return_counts=True)
    end = torch.cumsum(counts, 0).double()                        # last 1-based position of every run
    run_rank = end - (counts.double() - 1.0) / 2.0
    ranks = torch.empty(n, dtype=torch.float64, device=x.device)
    ranks[order] = torch.repeat_interleave(run_rank, counts)
    return ranks


def _spearman(a: torch.Tensor, b: torch.Tensor) -> float:
    ra, rb = _avg_ranks(a), _avg_ranks(b)
    ra, rb = ra - ra.mean(), rb - rb.mean()
    den = torch.sqrt((ra * ra).sum() * (rb * rb).sum())
    return float((ra * rb).sum() / den) if float(den) > 0 else float("nan")


@torch.no_grad()
def embedding_correlations(emb: torch.Tensor, features: dict) -> dict:
    """The numeric core of ``wandb_utils.plot_{2,3}d_embedding_and_correlations``: Spearman's rho (average ranks on ties) of every
    column of ``emb`` [N, C] with every feature, ranked on emb's device.  Keys ``f"{feat}_dim{i}"`` with i = 1 .. C as the
    reference numbers them; NaN for a feature whose length differs from N or is < 2 (and for a constant input)."""
    emb = torch.as_tensor(emb)
    out = {}
    for name, values in features.items():
        v = torch.as_tensor(np.asarray(values) if not torch.is_tensor(values) else values).reshape(-1)
        ok = v.numel() == emb.size(0) and v.numel() >= 2
        v = v.to(device=emb.device, dtype=torch.float64)
        for i in range(emb.size(1)):
            out[f"{name}_dim{i + 1}"] = _spearman(emb[:, i].double(), v) if ok else float("nan")
    return out


@torch.no_grad()
def bimodal_pca_summary(model) -> Optional[dict]:
    """The PCA block of the reference's ``train_joint`` (:856-912): PCA-2 and PCA-3 of the joint embeddings (correlated with every
    feature, named as ``model.features`` names them) and of the MOD2 codes (with "Labels" only).  Returns ``{"joint_p2", "joint_p3",
    "mod2_p2", "mod2_p3"}`` (numpy projections, absent where the reference skips: N <= 2 or fewer than 3 columns) and
    ``"correlations"``: ``{"Joint_bimodal/pca2": {...}, "Joint_bimodal/pca3", "MOD2_MNIST100/pca2", "MOD2_MNIST100/pca3"}``; the
    finite correlations go to the run as ``embeddings/val/{arch}/pca_{2,3}d/{key}``."""
    if model.val_loader is None:
        return None
    E, feats = compute_bimodal_joint_embeddings_and_features(model)
    src = getattr(model, "features", None) or {}
    feat_map = {key: src[key] for key, name in _FEATS if name in feats}
    _, Z2 = _val_codes(model)
    out, corr = {}, {}
    for arch, tagname, X, fm in (("Joint_bimodal", "joint", E, feat_map),
                                 ("MOD2_MNIST100", "mod2", Z2, {k: v for k, v in feat_map.items() if k == "Labels"})):
        if X.numel() == 0 or X.size(0) <= 2 or X.size(1) <= 2:
            continue
        for n in (2, 3):
            mean, comp = pca_fit(X, n)
            P = pca_project(X, mean, comp)
            out[f"{tagname}_p{n}"] = P.cpu().numpy()
            corr[f"{arch}/pca{n}"] = embedding_correlations(P, fm)
    out["correlations"] = corr
    run = _run(model)
    if run:
        for k, d in corr.items():
            arch, which = k.split("/")
            run.log({f"embeddings/val/{arch}/pca_{which[-1]}d/{kk}": vv for kk, vv in d.items() if vv == vv})
    return out


# ---- snapshots ------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def log_snapshots(model, epoch: int, num: int = 8):
    """Reference ``_log_snapshots`` (:963-1015) without its image grids: cross-reconstructs the first ``num`` validation pairs and
    logs ``snap/mod1_mse`` / ``snap/mod2_mse`` (means over all pixels); returns them as a dict.  Without a ``wandb_run`` or a
    validation batch nothing happens and no draws are made (None), as in the reference."""
    run = _run(model)
    if run is None or getattr(model, "validation_mod1", None) is None:
        return None
    mod1, mod2 = model.validation_mod1[:num], model.validation_mod2[:num]
    B = mod1.size(0)
    x1, x2 = mod1.reshape(B, -1).float(), mod2.reshape(B, -1).float()
    r1, r2 = model._cross_reconstruct(model.mod1_dbn.represent(x1), model.mod2_dbn.represent(x2), steps=model.cross_steps)
    m1, m2 = torch.stack([((r1.reshape(B, -1) - x1) ** 2).mean(), ((r2.reshape(B, -1) - x2) ** 2).mean()]).double().tolist()
    run.log({"snap/mod1_mse": m1, "snap/mod2_mse": m2, "epoch": epoch})
    return {"snap/mod1_mse": m1, "snap/mod2_mse": m2}
