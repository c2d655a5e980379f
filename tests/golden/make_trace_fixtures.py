#!/usr/bin/env python3
"""Generate tests/golden/cross_trace_small.npz: the reference's convergence tracing (imdbn/utils/conditional_steps.py) on
the trained small iMDBN of imdbn_small_100_40_20_j16.npz.

Run in the build container only (needs the reference checkout, as make_fixtures.py does):

    python tests/golden/make_trace_fixtures.py

The UNMODIFIED reference functions run on a duck-typed model: ``image_idbn`` is a reference ``iDBN`` whose layers carry the
fixture's trained image weights, ``joint_rbm`` a reference ``RBM`` with the label softmax group and the trained joint
weights, ``z_class_mean`` the recorded class means, ``val_loader`` batches of 8 over the fixture's data.  Every case draws
from its own ``DrawStream`` seed (make_fixtures.Substitute), so a test re-creates each direction's draws from the seed.
"""
from __future__ import annotations

import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as MF  # noqa: E402  (puts the reference on sys.path, stubs wandb, chdirs to a scratch dir)

import torch  # noqa: E402
from oracle.draws import DrawStream  # noqa: E402
from imdbn.models import RBM, iDBN  # noqa: E402
from imdbn.utils import conditional_steps as CS  # noqa: E402

SRC = os.path.join(HERE, "imdbn_small_100_40_20_j16.npz")
MAX_STEPS = 24
FUNCS = ["_gibbs_conditional_step", "trace_img2txt_cross", "trace_txt2img_cross", "pick_fixed_val_case", "log_cross_case",
         "run_and_log_cross_fixed_case", "build_or_get_fixed_val_panel", "_steps_stats", "run_and_log_cross_panel",
         "run_and_log_z_mismatch_check"]


def data():
    """The recipe of make_fixtures.case_imdbn_small: X = |proto[yi] - flip|, one-hot Y."""
    z = np.load(SRC)
    meta = json.loads(str(z["meta"]))
    s = DrawStream(meta["seed"])
    K, N = meta["K"], meta["B"] * meta["NB"]
    yi = z["yi"]
    proto = (s.uniform((K, 100)) > 0.7).astype(np.float32)
    flip = (s.uniform((N, 100)) > 0.9).astype(np.float32)
    X = np.abs(proto[yi] - flip).astype(np.float32)
    return z, X, np.eye(K, dtype=np.float32)[yi]


class Model:
    pass


class StubRun:
    def __init__(self):
        self.logged = []

    def log(self, d):
        self.logged.append(d)


def model(z, X, Y, with_zcm=True):
    m = Model()
    m.device = torch.device("cpu")
    idbn = iDBN.__new__(iDBN)
    idbn.device = m.device
    idbn.layers = []
    for i, (V, H) in enumerate(((100, 40), (40, 20))):
        r = RBM(V, H, 0.1, 1e-4, 0.5)
        with torch.no_grad():
            r.W.copy_(torch.from_numpy(z[f"img{i}_W"])); r.hid_bias.copy_(torch.from_numpy(z[f"img{i}_hid_bias"]))
            r.vis_bias.copy_(torch.from_numpy(z[f"img{i}_vis_bias"]))
        idbn.layers.append(r)
    m.image_idbn = idbn
    jr = RBM(28, 16, 0.05, 1e-4, 0.5, softmax_groups=[(20, 28)])
    with torch.no_grad():
        jr.W.copy_(torch.from_numpy(z["joint_W"])); jr.hid_bias.copy_(torch.from_numpy(z["joint_hid_bias"]))
        jr.vis_bias.copy_(torch.from_numpy(z["joint_vis_bias"]))
    m.joint_rbm = jr
    m.Dz_img, m.num_labels = 20, 8
    if with_zcm:
        m.z_class_mean = torch.from_numpy(z["z_class_mean"])
    m.val_loader = MF._loader(X, Y, 8)
    m.wandb_run = None
    return m


def pack_i2t(out, pre):
    d = {pre + k: np.asarray(out[k], np.float64) for k in ("p_top1", "p_top2", "p_gap", "l1")}
    d[pre + "p_gt"] = np.asarray(out["p_gt"] if out["p_gt"] is not None else [], np.float64)
    d[pre + "top1_idx"] = np.asarray(out["top1_idx"], np.int32)
    d[pre + "top2_idx"] = np.asarray(out["top2_idx"], np.int32)
    d[pre + "scalars"] = np.array([out["steps_to_converge"], out["predT"], -1 if out["gt_idx"] is None else out["gt_idx"]], np.int32)
    return d


def pack_t2i(out, pre):
    return {pre + "z_l2": np.asarray(out["z_l2"], np.float64), pre + "image_mse": np.asarray(out["image_mse"], np.float64),
            pre + "steps": np.int32(out["steps_to_converge"]), pre + "best_mse": np.float64(out["best_mse"])}


def main():
    z, X, Y = data()
    out, meta = {}, {"max_steps": MAX_STEPS, "seeds": {}, "funcs": {}}
    for f in FUNCS:
        meta["funcs"][f] = list(inspect.signature(getattr(CS, f)).parameters)
    # 1. fixed case, both directions, defaults (one stream: IMG->TXT draws its [1, V] start, TXT->IMG nothing)
    m = model(z, X, Y)
    seed = 5101
    with MF.Substitute(DrawStream(seed)):
        a, b = CS.run_and_log_cross_fixed_case(m, epoch=0, max_steps=MAX_STEPS)
    img, lbl = m._fixed_val_case
    out["fixed_img"], out["fixed_lbl"] = img.numpy(), lbl.numpy()
    out.update(pack_i2t(a, "fx_i2t_")); out.update(pack_t2i(b, "fx_t2i_"))
    meta["seeds"]["fixed"] = seed
    # 2. fixed case with sample_h = sample_v = True: each direction on its own stream (the batched trace draws all max_steps)
    for pre, fn, sd in (("smp_i2t_", CS.trace_img2txt_cross, 5202), ("smp_t2i_", CS.trace_txt2img_cross, 5303)):
        s = DrawStream(sd)
        with MF.Substitute(s):
            r = fn(m, img, lbl_onehot=lbl, max_steps=MAX_STEPS, sample_h=True, sample_v=True)
        out.update(pack_i2t(r, pre) if pre.startswith("smp_i2t") else pack_t2i(r, pre))
        out[pre + "cat"] = np.concatenate(s.cat_record).astype(np.int32) if s.cat_record else np.zeros(0, np.int32)
        out[pre + "n_draws"] = np.int32(len(s.log))
        meta["seeds"][pre] = sd
    # 2b. IMG->TXT without a label and with a gap threshold this small model reaches (the default 0.25 it does not)
    with MF.Substitute(DrawStream(5252)):
        out.update(pack_i2t(CS.trace_img2txt_cross(m, img, None, max_steps=MAX_STEPS, gap_thresh=0.02), "gap_i2t_"))
    meta["seeds"]["gap_i2t_"] = 5252
    # 3. TXT->IMG with ema_beta = 0.3 and 4. without z_class_mean (no draws in either)
    with MF.Substitute(DrawStream(1)):
        out.update(pack_t2i(CS.trace_txt2img_cross(m, img, lbl, max_steps=MAX_STEPS, ema_beta=0.3), "ema_t2i_"))
        m2 = model(z, X, Y, with_zcm=False)
        out.update(pack_t2i(CS.trace_txt2img_cross(m2, img, lbl, max_steps=MAX_STEPS), "nozcm_t2i_"))
    # 5. the panel, per_class = 2 (16 samples; IMG->TXT starts are 16 [1, V] draws back to back)
    seed = 5404
    m3 = model(z, X, Y)
    with MF.Substitute(DrawStream(seed)):
        pnl = CS.run_and_log_cross_panel(m3, epoch=0, per_class=2, max_steps=MAX_STEPS)
    pi, pl = m3._fixed_val_panel
    out["panel_img"], out["panel_lbl"] = pi.numpy(), pl.numpy()
    out["panel_i2t_steps"] = np.asarray(pnl["img2txt"]["steps"], np.int32)
    out["panel_t2i_steps"] = np.asarray(pnl["txt2img"]["steps"], np.int32)
    meta["panel"] = {"img2txt": {k: pnl["img2txt"][k] for k in ("stats", "p1_mean", "gap_mean")},
                     "txt2img": {k: pnl["txt2img"][k] for k in ("stats", "best_mse_mean")}}
    meta["seeds"]["panel"] = seed
    # 6. z mismatch: returns early without a wandb_run -- a stub records what it logs
    seed = 5505
    m4 = model(z, X, Y)
    m4.wandb_run = StubRun()
    with MF.Substitute(DrawStream(seed)):
        CS.run_and_log_z_mismatch_check(m4, epoch=0, max_steps=MAX_STEPS)
    meta["zcheck"] = [{k: v for k, v in d.items()} for d in m4.wandb_run.logged]
    meta["seeds"]["zcheck"] = seed
    # _steps_stats on a list with converged and unconverged rows
    ex = [3, 7, MAX_STEPS + 1, 1, 12, MAX_STEPS, MAX_STEPS + 1, 5]
    st, mask = CS._steps_stats(ex, MAX_STEPS)
    meta["steps_stats_example"] = {"steps": ex, "stats": st, "mask": mask.tolist()}
    meta["recipe"] = ("model from imdbn_small_100_40_20_j16.npz (img*_ / joint_ weights, z_class_mean), val_loader batches of 8 over "
                      "its data; reference conditional_steps functions with draws from DrawStream(seeds[case])")
    path = os.path.join(HERE, "cross_trace_small.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **out)
    print(f"wrote cross_trace_small.npz: {os.path.getsize(path) / 1024:.1f} KiB")
    print("fixed i2t/t2i steps", a["steps_to_converge"], b["steps_to_converge"], "sampled", int(out["smp_i2t_scalars"][0]), "gap", int(out["gap_i2t_scalars"][0]),
          int(out["smp_t2i_steps"]), "ema", int(out["ema_t2i_steps"]), "nozcm", int(out["nozcm_t2i_steps"]))
    print("panel i2t", pnl["img2txt"]["steps"], "t2i", pnl["txt2img"]["steps"])
    print("zcheck", meta["zcheck"])


if __name__ == "__main__":
    main()
