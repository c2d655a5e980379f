"""Numpy twin of imdbn_cross_metrics (csrc/kernels_metrics.hpp) and of the two entry points of imdbn/utils/cross_eval.py.

TEST INFRASTRUCTURE ONLY.  ``metrics`` restates the kernel's definition in float64 over the float32 inputs: every decision
(first maximum, rank, top-k hit) compares the float32 numbers themselves, so it is exact; the clamps happen in float32 as in the
kernel (and in torch: ``p.clamp(1e-6, 1 - 1e-6)`` of a float32 tensor), ``1 - pt`` is the float32 difference, the logarithms and
every sum are float64.  ``evaluate`` and ``snapshot`` restate ``evaluate_cross_modal`` and ``log_snapshots`` on recorded per-batch
outputs of ``_cross_reconstruct``."""
from __future__ import annotations

import numpy as np

F32 = np.float32
CE_LO, CE_HI = F32(1e-6), F32(1.0 - 1e-6)
P_LO, P_HI = F32(1e-9), F32(1.0)


def first_max(a):
    """np.argmax returns the first maximum, as torch.argmax documents for the reference's rows (no NaN in a test)."""
    return np.argmax(np.asarray(a), axis=1).astype(np.int64)


def metrics(p, y=None, gt=None, row_mse=None, npix=1, topk=3):
    """dict(pred, gt, p_pred, p_true, rank [B]; acc [8]; confusion [K, K] int64; class_sums [K, 3]) of one call from zeroed accumulators."""
    p = np.asarray(p, F32)
    B, K = p.shape
    assert (y is None) != (gt is None)
    g = first_max(np.asarray(y, F32)) if y is not None else np.asarray(gt, np.int64)
    pred = first_max(p)
    ok = (g >= 0) & (g < K)
    gs = np.where(ok, g, 0)
    rows = np.arange(B)
    pg = p[rows, gs]
    cols = np.arange(K)[None, :]
    rank = ((p > pg[:, None]) | ((p == pg[:, None]) & (cols < gs[:, None]))).sum(1).astype(np.int64)
    pt = np.clip(p, CE_LO, CE_HI).astype(F32)
    one_minus = (F32(1.0) - pt).astype(F32)
    onehot = cols == gs[:, None]
    ce_rows = -np.where(onehot, np.log(pt.astype(np.float64)), np.log(one_minus.astype(np.float64))).sum(1)
    rm = np.zeros(B, np.float64) if row_mse is None else np.asarray(row_mse, F32).astype(np.float64)
    acc = np.zeros(8, np.float64)
    acc[0] = ok.sum()
    acc[1] = (ok & (pred == g)).sum()
    acc[2] = (ok & (rank < min(topk, K))).sum()
    acc[3] = ce_rows[ok].sum()
    acc[4] = (rm[ok] * float(npix)).sum()
    acc[5] = (~ok).sum()
    conf = np.zeros((K, K), np.int64)
    np.add.at(conf, (g[ok], pred[ok]), 1)
    cs = np.zeros((K, 3), np.float64)
    np.add.at(cs[:, 0], g[ok], 1.0)
    np.add.at(cs[:, 1], g[ok], (pred[ok] == g[ok]).astype(np.float64))
    np.add.at(cs[:, 2], g[ok], rm[ok])
    return {"pred": pred, "gt": g, "p_pred": np.clip(p[rows, pred], P_LO, P_HI), "p_true": np.where(ok, np.clip(pg, P_LO, P_HI), np.nan),
            "rank": np.where(ok, rank, -1), "acc": acc, "confusion": conf, "class_sums": cs, "ce_rows": ce_rows}


def row_mse(rec, img):
    """Per-row mean squared error of decoded rows, float64 over the float32 inputs."""
    rec, img = np.asarray(rec, F32).astype(np.float64), np.asarray(img, F32).astype(np.float64)
    return ((rec.reshape(len(img), -1) - img.reshape(len(img), -1)) ** 2).mean(1)


def evaluate(batches, topk=3):
    """``evaluate_cross_modal`` over recorded batches ``(img_from_txt, p_y_given_img, img, y)``."""
    K = np.asarray(batches[0][1]).shape[1]
    acc, conf, cs = np.zeros(8), np.zeros((K, K), np.int64), np.zeros((K, 3))
    rows = {k: [] for k in ("pred", "gt", "p_pred", "p_true", "rank")}
    npix = 1
    for rec, p_y, img, y in batches:
        npix = int(np.asarray(img).reshape(len(img), -1).shape[1])
        m = metrics(p_y, y=y, row_mse=row_mse(rec, img), npix=npix, topk=topk)
        acc += m["acc"]; conf += m["confusion"]; cs += m["class_sums"]
        for k in rows:
            rows[k].append(m[k])
    n = max(1.0, acc[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        per_acc = np.where(cs[:, 0] > 0, cs[:, 1] / cs[:, 0], np.nan)
        per_mse = np.where(cs[:, 0] > 0, cs[:, 2] / cs[:, 0], np.nan)
    out = {"n": int(acc[0]), "text_top1": acc[1] / n, "text_top3": acc[2] / n, "text_ce": acc[3] / n,
           "image_mse": acc[4] / max(1.0, n * max(1, npix)), "confusion": conf, "per_class_acc": per_acc, "per_class_image_mse": per_mse,
           "per_class_n": cs[:, 0].astype(np.int64)}
    out.update({k: np.concatenate(v) for k, v in rows.items()})
    return out


def snapshot(rec, p_y, img, y, class_names=None):
    """``log_snapshots`` on one recorded ``_cross_reconstruct``: the reconstruction clamped to [0, 1] as reference :738."""
    rec = np.clip(np.asarray(rec, F32), F32(0), F32(1))
    m = metrics(p_y, y=y)
    K = np.asarray(p_y).shape[1]
    named = bool(class_names) and len(class_names) == K
    table = [[i, int(m["gt"][i]), int(m["pred"][i]), float(m["p_pred"][i]), float(m["p_true"][i])]
             + ([class_names[int(m["gt"][i])], class_names[int(m["pred"][i])]] if named else []) for i in range(len(rec))]
    return {"snap/image_mse": float(row_mse(rec, img).mean()), "confusion": m["confusion"], "table": table, "pred": m["pred"], "gt": m["gt"],
            "ce_sum": float(m["acc"][3]), "top1": int(m["acc"][1])}
