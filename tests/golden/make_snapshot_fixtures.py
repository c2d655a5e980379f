#!/usr/bin/env python3
"""Generate tests/golden/snapshots_small.npz: the reference's ``iMDBN._log_snapshots`` (imdbn/models/imdbn.py) on the trained small
iMDBN of ref_imdbn_small.pkl / imdbn_small_100_40_20_j16.npz.

Run in the build container only (needs the reference checkout, as make_fixtures.py does):

    python tests/golden/make_snapshot_fixtures.py

The UNMODIFIED reference method runs on a reference ``iMDBN`` that carries the pickled weights and ``z_class_mean``.  Its validation
loader holds the rows of make_fixtures.case_imdbn_small in a recorded order (``perm``), so ``validation_images`` are the first 8 of
them.  ``torch.rand_like`` / ``torch.randn_like`` go through make_fixtures.Substitute and every draw is recorded; ``wandb.Image``
and the torchvision grid are stubs, ``wandb.plot.confusion_matrix`` and ``wandb.Table`` record what they are given, the run is a stub
that keeps what is logged.  Recorded besides: what ``_cross_reconstruct`` returned, and the reference's own online-metric
expressions (its :619-639: argmax, topk, F.binary_cross_entropy, F.mse_loss) evaluated by torch on those 8 rows.

The order of the rows (and with it the draw seed) is chosen so that for ALL 8 rows the reference's own fp32 ``p_top1 - p_top2`` is at
least ``ROOM``: a test may then compare every prediction exactly.  The script asserts it, writes the smallest margin into ``meta``,
and fails loudly when no candidate order has that room -- it never records a tie.
"""
from __future__ import annotations

import inspect
import json
import os
import pickle
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_trace_fixtures as TF  # noqa: E402  (make_fixtures: reference on sys.path, wandb / torchvision stubbed, scratch cwd)

MF = TF.MF

import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402
from oracle.draws import DrawStream  # noqa: E402
from imdbn.models import iMDBN  # noqa: E402  (the reference's)

ROOM = 1e-5
EPOCH, NUM = 5, 8
PKL = os.path.join(HERE, "ref_imdbn_small.pkl")
CANDIDATES = range(9101, 9165)          # order / draw seeds tried in turn

CALLS = {"cm": [], "rows": [], "cols": []}


class Table:
    def __init__(self, columns=None, **kw):
        CALLS["cols"].append(list(columns))

    def add_data(self, *row):
        CALLS["rows"].append(list(row))


_wandb = sys.modules["wandb"]
_wandb.Image = lambda x, *a, **k: None
_wandb.Table = Table
_wandb.plot = types.SimpleNamespace(confusion_matrix=lambda **kw: CALLS["cm"].append(kw) or "confusion-plot")
sys.modules["torchvision.utils"].make_grid = lambda X, nrow=8: torch.zeros(3, 2, 2)


def model(meta, X, Y):
    dl = MF._loader(X, Y, meta["B"])
    m = iMDBN(meta["sizes"], meta["joint_hidden"], params=dict(meta["params"]), dataloader=dl, val_loader=dl, device=torch.device("cpu"),
              num_labels=meta["K"])
    with open(PKL, "rb") as f:                       # (the pickle as the reference wrote it: reference classes, CPU tensors)
        pl = pickle.load(f)
    m.image_idbn.layers = pl["image_idbn"].layers
    m.joint_rbm = pl["joint_rbm"]
    m.z_class_mean = pl["z_class_mean"]
    m.wandb_run = TF.StubRun()
    return m


def run_once(meta, X, Y, seed):
    """One ``_log_snapshots`` on the rows in the order of ``seed``; returns everything recorded."""
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(len(X)).astype(np.int32)
    m = model(meta, X[perm], Y[perm])
    assert torch.equal(m.validation_images, torch.from_numpy(X[perm][:NUM]))
    cross = []
    o_cr = m._cross_reconstruct

    def cr(*a, **k):
        r = o_cr(*a, **k)
        cross.append((r[0].numpy().copy(), r[1].numpy().copy()))
        return r

    m._cross_reconstruct = cr
    for v in CALLS.values():
        v.clear()
    s = DrawStream(seed)
    with MF.Substitute(s):
        m._log_snapshots(EPOCH, NUM)
    del m._cross_reconstruct
    assert len(cross) == 1
    return perm, m, s, cross[0], {k: list(v) for k, v in CALLS.items()}


def main():
    z, X, Y = TF.data()
    meta0 = json.loads(str(z["meta"]))
    best = None
    for seed in CANDIDATES:
        perm, m, s, (rec, p_y), calls = run_once(meta0, X, Y, seed)
        top2 = np.sort(p_y, axis=1)[:, ::-1][:, :2]
        margin = float((top2[:, 0] - top2[:, 1]).min())
        wrong = int((p_y.argmax(1) != Y[perm][:NUM].argmax(1)).sum())
        print(f"seed {seed}: smallest p_top1 - p_top2 = {margin:.3e}, {wrong} of {NUM} rows mispredicted")
        if margin >= ROOM and (best is None or (best[0] == 0 and wrong > 0)):
            best = (wrong, seed)
        if best is not None and best[0] > 0:
            break
    assert best is not None, f"no row order among {len(CANDIDATES)} candidates leaves {ROOM} between the top two labels of all {NUM} rows"
    seed = best[1]
    perm, m, s, (rec, p_y), calls = run_once(meta0, X, Y, seed)
    top2 = np.sort(p_y, axis=1)[:, ::-1][:, :2]
    margin = float((top2[:, 0] - top2[:, 1]).min())
    assert margin >= ROOM, margin

    imgs, lbls = X[perm][:NUM], Y[perm][:NUM]
    K = meta0["K"]
    # what the stubs received
    assert len(calls["cm"]) == 1 and len(calls["rows"]) == NUM and calls["cols"] == [["idx", "gt_idx", "pred_idx", "p_pred", "p_y_true"]]
    cm = calls["cm"][0]
    assert cm["class_names"] == [str(i) for i in range(K)]
    rows = calls["rows"]
    logged = m.wandb_run.logged
    mse = [d for d in logged if "snap/image_mse" in d]
    assert len(mse) == 1 and mse[0]["epoch"] == EPOCH
    # the reference's online-metric expressions on the same rows, by torch
    tp, ty = torch.from_numpy(p_y), torch.from_numpy(lbls)
    gt = ty.argmax(dim=1)
    top1 = int((tp.argmax(dim=1) == gt).sum())
    top3 = int((tp.topk(k=min(3, K), dim=1).indices == gt.unsqueeze(1)).any(dim=1).sum())
    ce = float(Fn.binary_cross_entropy(tp.clamp(1e-6, 1 - 1e-6), Fn.one_hot(gt, num_classes=K).float(), reduction="sum"))
    mse_sum = float(Fn.mse_loss(torch.from_numpy(rec).view_as(torch.from_numpy(imgs)), torch.from_numpy(imgs), reduction="sum"))
    # the draws, in order: replay the stream's log
    r = DrawStream(seed)
    draws = [(r.uniform(shape) if kind == "u" else r.normal(shape)) for kind, shape in s.log]
    assert all(kind in "un" for kind, _ in s.log)
    meta = {"seed": seed, "room": ROOM, "min_margin": margin, "epoch": EPOCH, "num": NUM, "K": K, "steps": int(m.cross_steps),
            "sizes": meta0["sizes"], "joint_hidden": meta0["joint_hidden"], "params": meta0["params"], "batch": meta0["B"],
            "draw_log": [[kind, list(shape)] for kind, shape in s.log], "cm_class_names": cm["class_names"], "table_columns": calls["cols"][0],
            "logged_keys": sorted({k for d in logged for k in d}), "signature": list(inspect.signature(iMDBN._log_snapshots).parameters),
            "recipe": ("ref_imdbn_small.pkl on the rows of make_fixtures.case_imdbn_small in the order perm = PCG64(seed).permutation(N); "
                       "val_loader batches of 8; iMDBN._log_snapshots(epoch, num) with draws from DrawStream(seed); ref_metrics = top-1 hits, "
                       "top-3 hits, ce_sum, mse_sum of the reference's online-metric expressions on the 8 rows")}
    path = os.path.join(HERE, "snapshots_small.npz")
    np.savez_compressed(
        path, meta=np.array(json.dumps(meta)), perm=perm, imgs=imgs, lbls=lbls, img_from_txt=rec, p_y_given_img=p_y,
        draws=np.concatenate([d.ravel() for d in draws]).astype(np.float32),
        cm_y_true=np.asarray(cm["y_true"], np.int64), cm_preds=np.asarray(cm["preds"], np.int64),
        table_int=np.array([row[:3] for row in rows], np.int64), table_p=np.array([row[3:5] for row in rows], np.float64),
        snap_image_mse=np.float64(mse[0]["snap/image_mse"]), ref_metrics=np.array([top1, top3, ce, mse_sum], np.float64))
    print(f"wrote snapshots_small.npz: {os.path.getsize(path) / 1024:.1f} KiB; seed {seed}, smallest margin {margin:.3e}, "
          f"top-1 {top1}/{NUM}, top-3 {top3}/{NUM}, ce_sum {ce:.6f}, snap/image_mse {float(mse[0]['snap/image_mse']):.6f}")


if __name__ == "__main__":
    main()
