"""Held-out cross-modal evaluation of an ``iMDBN`` and its snapshot log, on the engine (reference ``imdbn/models/imdbn.py``:
``_log_snapshots`` :714-813; the metric definitions of the ``train_joint`` batch loop :615-639 and :648-652).

``train_joint``'s online metrics are taken on training batches while the weights move.  ``evaluate_cross_modal`` asks the same
questions of a held-out split with the weights at rest: for every batch ``image_idbn.represent``, ``model._cross_reconstruct``
(unchanged: the same draws in the same order), the per-row image error and ONE ``HipEngine.cross_metrics`` call
(imdbn_cross_metrics: argmax, rank of the true label, clamped BCE, confusion counts, per-class sums) into one set of device
accumulators; the host synchronises once, after the last batch.  ``log_snapshots`` is the reference's ``_log_snapshots`` on the
same kernel, without its image grid and W&B plot objects: a ``wandb_run`` receives plain scalars only and every function returns
the numbers it computed.

The per-row image error needs no decoded image: ``_cross_reconstruct(..., _decode=False)`` hands back the code z_from_y and
``HipEngine.decode_sqerr`` decodes it straight into ``mean_c (p(v|h)_c - img_c)^2`` (imdbn_rbm_prop_down_sqerr on the bottom
layer).  That kernel has no softmax groups; with softmax groups on the bottom image layer, or with ``z_affine_*`` set, the rows
are decoded as usual and the error is taken from them.

Random draws: exactly those of ``_cross_reconstruct``, once per batch.  ``seed=None`` consumes the ambient draw source (as the
reference's ``_log_snapshots`` does); ``seed=int`` runs under a ``PhiloxRng(seed)`` of its own and leaves the caller's draw counter
where it was, so evaluating between epochs does not change training.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from imdbn import engine as _E
from imdbn.utils.batches import batches, rows_on_device

__all__ = ["evaluate_cross_modal", "log_snapshots", "row_image_error", "fused_decode_ok"]

ROW_KEYS = ("pred", "gt", "p_pred", "p_true", "rank")


def _run(model):
    return getattr(model, "wandb_run", None)


def _eng(model):
    return _E.get_engine(model.joint_rbm.W.data)


def fused_decode_ok(model) -> bool:
    """Can the decode of z_from_y end in imdbn_rbm_prop_down_sqerr?  No softmax groups on the bottom image layer, no ``z_affine_*``."""
    layers = list(model.image_idbn.layers)
    affine = hasattr(model, "z_affine_scale") and hasattr(model, "z_affine_bias")
    return bool(layers) and not (getattr(layers[0], "softmax_groups", None) or []) and not affine


@torch.no_grad()
def row_image_error(model, z: torch.Tensor, y: torch.Tensor, img: torch.Tensor, steps: Optional[int] = None,
                    fused: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One ``_cross_reconstruct(z, y, steps)`` -> ``(row_mse [B], p_y_given_img [B, K])``, ``row_mse[i]`` = the mean over the pixels of
    (img_from_txt[i] - img[i])^2.  ``fused`` None: through ``decode_sqerr`` when ``fused_decode_ok``, else from the decoded rows; the
    draws are the same either way."""
    fused = fused_decode_ok(model) if fused is None else bool(fused)
    if fused:
        z_y, p_y = model._cross_reconstruct(z, y, steps=steps, _decode=False)
        return _eng(model).decode_sqerr(model.image_idbn.layers, z_y, img), p_y
    rec, p_y = model._cross_reconstruct(z, y, steps=steps)
    return ((rec.reshape(img.size(0), -1) - img) ** 2).mean(dim=1), p_y


def _fetch(K: int, acc, conf, cls, rows) -> dict:
    """Everything in one device-to-host copy (the one synchronisation): float64 holds the int32 / int64 counts and fp32 values exactly."""
    parts = [acc, conf.double().reshape(-1), cls.reshape(-1)] + [torch.cat(rows[k]).double() if rows[k] else acc[:0] for k in ROW_KEYS]
    flat = torch.cat(parts).cpu().numpy()
    out, at = {}, 0
    for name, n in (("acc", 8), ("confusion", K * K), ("class_sums", K * 3)):
        out[name] = flat[at:at + n]; at += n
    n_rows = (flat.size - at) // len(ROW_KEYS)
    for k in ROW_KEYS:
        out[k] = flat[at:at + n_rows]; at += n_rows
    out["confusion"] = np.rint(out["confusion"]).astype(np.int64).reshape(K, K)
    out["class_sums"] = out["class_sums"].reshape(K, 3)
    for k in ("pred", "gt", "rank"):
        out[k] = np.rint(out[k]).astype(np.int64)
    for k in ("p_pred", "p_true"):
        out[k] = out[k].astype(np.float32)
    return out


@torch.no_grad()
def evaluate_cross_modal(model, loader=None, steps: Optional[int] = None, seed: Optional[int] = None,
                         max_batches: Optional[int] = None, topk: int = 3) -> Optional[dict]:
    """Cross-modal metrics of ``model`` over ``loader`` (default ``model.val_loader``; None without one): ``n``, ``text_top1``,
    ``text_top3`` (the share of rows whose true label is among the ``topk`` most probable), ``text_ce``, ``image_mse`` -- divided as
    ``train_joint`` divides its online metrics, so for the same batches they mean what ``joint_history`` means --, ``confusion``
    (int64 ``[K, K]``, rows gt, columns pred), ``per_class_acc`` / ``per_class_image_mse`` / ``per_class_n`` (a class without rows:
    NaN), ``skipped`` and the per-row ``pred``, ``gt``, ``p_pred``, ``p_true``, ``rank`` (numpy arrays).  A ragged last batch is
    fine; ``max_batches`` stops early.  Under data parallelism every rank evaluates the batches it is handed and the accumulators
    and the confusion matrix are summed over the ranks once (the per-row arrays stay the rank's own).  With a ``wandb_run`` on the
    model the four scalars are logged as ``eval/...``."""
    loader = loader if loader is not None else getattr(model, "val_loader", None)
    if loader is None:
        return None
    if seed is None:
        return _evaluate(model, loader, steps, max_batches, topk)
    with _E.use_rng(_E.PhiloxRng(int(seed), row0=int(getattr(_E.get_rng(), "row0", 0)))):
        return _evaluate(model, loader, steps, max_batches, topk)


def _evaluate(model, loader, steps, max_batches, topk) -> dict:
    dev, K = model.device, int(model.num_labels)
    eng = _eng(model)
    steps = model.cross_steps if steps is None else int(steps)
    acc = torch.zeros(8, dtype=torch.float64, device=dev)
    conf = torch.zeros(K, K, dtype=torch.int64, device=dev)
    cls = torch.zeros(K, 3, dtype=torch.float64, device=dev)
    rows = {k: [] for k in ROW_KEYS}
    npix = 1
    for b, (img, y) in enumerate(batches(loader)):
        if max_batches is not None and b >= int(max_batches):
            break
        img = rows_on_device(img, dev)
        y = y.to(dev).float()
        z = model.image_idbn.represent(img)
        row_mse, p_y = row_image_error(model, z, y, img, steps)
        npix = img.size(1)
        o = eng.cross_metrics(p_y, y=y, row_mse=row_mse, npix=npix, topk=topk, acc=acc, confusion=conf, class_sums=cls)
        for k in ROW_KEYS:
            rows[k].append(o[k])
    if _E.dp.active():                               # each rank accumulated its own batches: sums over rows, exchanged once
        pack = torch.cat([acc, conf.double().reshape(-1), cls.reshape(-1)])
        _E.dp.all_reduce_sum(pack)
        acc, conf, cls = pack[:8], pack[8:8 + K * K].reshape(K, K), pack[8 + K * K:].reshape(K, 3)
    h = _fetch(K, acc, conf, cls, rows)
    a, cs = h["acc"], h["class_sums"]
    n = max(1.0, float(a[0]))
    with np.errstate(invalid="ignore", divide="ignore"):
        per_acc = np.where(cs[:, 0] > 0, cs[:, 1] / cs[:, 0], np.nan)
        per_mse = np.where(cs[:, 0] > 0, cs[:, 2] / cs[:, 0], np.nan)
    res = {"n": int(a[0]), "text_top1": float(a[1]) / n, "text_top3": float(a[2]) / n, "text_ce": float(a[3]) / n,
           "image_mse": float(a[4]) / max(1.0, n * max(1, npix)), "confusion": h["confusion"], "per_class_acc": per_acc,
           "per_class_image_mse": per_mse, "per_class_n": np.rint(cs[:, 0]).astype(np.int64), "skipped": int(a[5])}
    res.update({k: h[k] for k in ROW_KEYS})
    run = _run(model)
    if run:
        run.log({"eval/" + k: res[k] for k in ("text_top1", "text_top3", "text_ce", "image_mse")})
    return res


@torch.no_grad()
def log_snapshots(model, epoch: int, num: int = 8) -> Optional[dict]:
    """Reference ``_log_snapshots`` (:714-813) without its image grid and W&B plot objects: cross-reconstructs the first ``num``
    validation rows, logs ``snap/image_mse`` (the mean over all pixels; the reference clamps the reconstruction to [0, 1] first, which
    leaves p(v|h) as it is) and returns it with the text ``confusion`` matrix (int64 ``[K, K]``), the ``table`` rows ``[i, gt, pred,
    p_pred, p_true]`` (plus the two names when ``class_names`` has ``num_labels`` entries; probabilities clamped to [1e-9, 1]) and
    ``pred`` / ``gt``.  Without a ``wandb_run`` or a validation batch nothing happens and no draws are made (None)."""
    run = _run(model)
    if run is None or getattr(model, "validation_images", None) is None or getattr(model, "validation_labels", None) is None:
        return None
    dev, K = model.device, int(model.num_labels)
    img = rows_on_device(model.validation_images[:num], dev)
    y = model.validation_labels[:num].to(dev).float()
    z = model.image_idbn.represent(img)
    row_mse, p_y = row_image_error(model, z, y, img, model.cross_steps)
    B, npix = img.size(0), img.size(1)
    o = _eng(model).cross_metrics(p_y, y=y, row_mse=row_mse, npix=npix, topk=min(2, K))
    h = _fetch(K, o["acc"], o["confusion"], o["class_sums"], {k: [o[k]] for k in ROW_KEYS})
    mse = float(h["acc"][4]) / float(B * npix)
    run.log({"snap/image_mse": mse, "epoch": epoch})
    names = getattr(model, "class_names", None)
    named = bool(names) and len(names) == K
    table = []
    for i in range(B):
        g, p = int(h["gt"][i]), int(h["pred"][i])
        table.append([i, g, p, float(h["p_pred"][i]), float(h["p_true"][i])] + ([names[g], names[p]] if named else []))
    return {"snap/image_mse": mse, "confusion": h["confusion"], "table": table, "pred": h["pred"], "gt": h["gt"]}
