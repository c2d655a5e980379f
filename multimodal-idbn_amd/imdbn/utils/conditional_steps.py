"""Cross-modal convergence tracing on the engine (reference ``imdbn/utils/conditional_steps.py``).

How many conditional-Gibbs steps does the joint RBM need before IMG->TXT (code clamped, labels free) and TXT->IMG (labels
clamped, code free) inference settles?  The reference answers with B = 1 Python loops: one sample at a time, several host
syncs per step, a full image decode per TXT->IMG step.  Here a whole batch is a few launches:

* ``HipEngine.chain_traced`` runs the chains (both directions side by side in one chain-kernel launch where it applies) and
  records p(v|h) of the label window (IMG->TXT, after a draw-free baseline step) or of the code window (TXT->IMG) at every
  step;
* ``label_scan`` / ``code_scan`` / ``patience_scan`` apply the reference's per-row stopping rules on the device;
* ``decode_sqerr`` gives the image MSE of every (step, row) code without returning the decoded images.

Every step is the reference's ``_gibbs_conditional_step`` (conditional_steps.py:16-37): h = p(h|v) at T = 1 (or a sample),
v_prob = p(v|h) with the softmax over the label group, v = v_prob (or a sample), re-clamped to the ORIGINAL known values.

The B = 1 functions keep the reference's names, signatures and return values (Python lists cut at the convergence step).
They are thin wrappers over the batched forms ``trace_img2txt_cross_batch`` / ``trace_txt2img_cross_batch`` /
``trace_cross_panel_batch``, which return device tensors.

Random draws.  With the defaults (``sample_h = sample_v = False``) the only draws are the IMG->TXT initial uniforms, one
``[B, V]`` tensor -- the very numbers the reference's B back-to-back ``[1, V]`` draws give.  With sampling, a batched trace
runs all ``max_steps`` for every row and so draws past a row's convergence point, where the reference stops drawing: the
recorded steps up to convergence are unaffected (Philox keys every row independently) but the stream position after the call
differs from the reference's.

Figures and histograms of the reference (matplotlib, ``wandb.Image``) are out of scope: a ``wandb_run`` on the model only
receives plain scalars and dicts through ``.log``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from imdbn import engine as _E

__all__ = ["_gibbs_conditional_step", "trace_img2txt_cross", "trace_txt2img_cross", "pick_fixed_val_case", "log_cross_case",
           "run_and_log_cross_fixed_case", "build_or_get_fixed_val_panel", "_steps_stats", "run_and_log_cross_panel",
           "run_and_log_z_mismatch_check", "z_mismatch_stats", "trace_img2txt_cross_batch", "trace_txt2img_cross_batch",
           "trace_cross_panel_batch"]


def _step(sample_h: bool, sample_v: bool) -> dict:
    return {"T": 1.0, "sigma": 0.0, "eta": 0.0, "sample_h": bool(sample_h), "vmode": 1 if sample_v else 0, "clamp": True}


def _eng(model):
    return _E.get_engine(model.joint_rbm.W.data)


def _flat(x: torch.Tensor, dev) -> torch.Tensor:
    x = x.to(dev)
    return x.reshape(x.size(0), -1).float() if x.dim() > 2 else x.float()


@torch.no_grad()
def _gibbs_conditional_step(rbm, v, v_known, known_mask, sample_h=False, sample_v=False):
    """One conditional step (conditional_steps.py:16-37): returns ``(v_next, v_prob)``, v_next re-clamped to ``v_known``."""
    v_next, v_prob, _, _ = rbm.gibbs_step(v, sample_h=sample_h, sample_v=sample_v)
    m = known_mask.to(v_next)
    return v_next * (1 - m) + v_known.to(v_next) * m, v_prob


# ---- the two directions as chain specs --------------------------------------------------------------------------------
def _img2txt_spec(model, imgs, K: Optional[int], max_steps, sample_h, sample_v):
    dev = model.device
    z = model.image_idbn.represent(_flat(imgs, dev))
    Dz = int(getattr(model, "Dz_img", z.size(1)))
    K = int(K if K is not None else getattr(model, "num_labels", 32))
    B, V = z.size(0), Dz + K
    vk = torch.zeros(B, V, device=dev)
    vk[:, :Dz] = z
    km = torch.zeros(B, V, device=dev)
    km[:, :Dz] = 1.0
    # v0 = vk*m + (1-m)*U inside the chain call; slot 0 of the trace is the baseline p(v | p(h | v0)) (y_prev of step 1)
    return {"v_known": vk, "mask": km, "steps": [_step(sample_h, sample_v)] * int(max_steps), "init_uniform": True,
            "trace": (Dz, V, True)}, Dz, K


def _txt2img_spec(model, lbls, max_steps, sample_h, sample_v):
    dev = model.device
    y = lbls.to(dev).float()
    Dz = int(getattr(model, "Dz_img", int(model.image_idbn.layers[-1].num_hidden)))
    K = int(getattr(model, "num_labels", y.size(1)))
    B, V = y.size(0), Dz + K
    vk = torch.zeros(B, V, device=dev)
    vk[:, Dz:] = y
    km = torch.zeros(B, V, device=dev)
    km[:, Dz:] = 1.0
    zcm = getattr(model, "z_class_mean", None)
    if zcm is not None:                     # class prior on the code (conditional_steps.py:171-176)
        z0 = zcm.to(dev)[y.argmax(dim=1)].float()
    else:                                   # draw-free mean-field half-step pair from the clamped labels (:177-184)
        jr = model.joint_rbm
        z0 = jr.visible_probs(jr.forward(vk))[:, :Dz]
    # the chain starts from [z0, y]; re-clamping reads only the label columns of v_known (masks are 0/1), so the start state
    # doubles as the clamp values
    v0 = vk.clone()
    v0[:, :Dz] = z0
    return {"v_known": v0, "mask": km, "steps": [_step(sample_h, sample_v)] * int(max_steps), "init_uniform": False,
            "trace": (0, Dz, False)}, z0.contiguous(), Dz


def _img2txt_result(eng, trace, lbls, eps_l1, stable_steps, gap_thresh):
    gt = lbls.argmax(dim=1) if lbls is not None else None
    o = eng.label_scan(trace, gt, eps_l1, stable_steps, gap_thresh)
    o["gt"] = gt
    return o


def _txt2img_result(eng, model, trace, z0, imgs, eps_z, mse_tol, patience, ema_beta):
    T, B, Dz = trace.shape
    zn, dz = eng.code_scan(trace, z0, ema_beta)
    ref = _flat(imgs, model.device)
    rows = torch.arange(B, dtype=torch.int32, device=ref.device).repeat(T)
    mse = eng.decode_sqerr(model.image_idbn.layers, zn.reshape(T * B, Dz), ref, rows).view(T, B).t().contiguous()
    steps, best = eng.patience_scan(dz, mse, eps_z, mse_tol, patience)
    return {"steps": steps, "best_mse": best, "z_l2": dz, "image_mse": mse, "z_new": zn}


@torch.no_grad()
def trace_img2txt_cross_batch(model, imgs, lbls=None, max_steps=70, sample_h=False, sample_v=False, eps_l1=1e-3, stable_steps=3,
                              gap_thresh=0.25) -> dict:
    """IMG->TXT for a batch: device tensors ``p_top1, p_top2, k1, k2, l1, p_gt`` ``[B, max_steps]`` (every step, also past
    convergence; ``p_gt`` None without labels), ``steps`` ``[B]`` (max_steps + 1 = not converged), ``pred`` ``[B]``, ``gt``."""
    eng = _eng(model)
    spec, Dz, K = _img2txt_spec(model, imgs, lbls.size(1) if lbls is not None else None, max_steps, sample_h, sample_v)
    ((_, tr),) = eng.chain_traced(model.joint_rbm, spec, None, model.joint_rbm._rng(spec["v_known"].size(0)))
    return _img2txt_result(eng, tr, lbls.to(model.device) if lbls is not None else None, eps_l1, stable_steps, gap_thresh)


@torch.no_grad()
def trace_txt2img_cross_batch(model, imgs, lbls, max_steps=70, sample_h=False, sample_v=False, eps_z=1e-3, mse_tol=1e-5, patience=3,
                              ema_beta: float = 0.0) -> dict:
    """TXT->IMG for a batch: device tensors ``z_l2``, ``image_mse`` ``[B, max_steps]``, ``steps`` ``[B]``, ``best_mse`` ``[B]``
    (inf where no step improved) and the codes ``z_new`` ``[max_steps, B, Dz]``."""
    eng = _eng(model)
    spec, z0, Dz = _txt2img_spec(model, lbls, max_steps, sample_h, sample_v)
    ((_, tr),) = eng.chain_traced(model.joint_rbm, spec, None, model.joint_rbm._rng(z0.size(0)))
    return _txt2img_result(eng, model, tr, z0, imgs, eps_z, mse_tol, patience, ema_beta)


@torch.no_grad()
def trace_cross_panel_batch(model, imgs, lbls, max_steps=70, sample_h=False, sample_v=False):
    """Both directions with the reference's default thresholds, as ONE traced chain pair (IMG->TXT first: its initial
    uniforms are the first draws, as in the reference's per-sample loop).  Returns ``(img2txt, txt2img)`` as the batch forms."""
    eng = _eng(model)
    a, _, _ = _img2txt_spec(model, imgs, lbls.size(1), max_steps, sample_h, sample_v)
    b, z0, _ = _txt2img_spec(model, lbls, max_steps, sample_h, sample_v)
    (_, tra), (_, trb) = eng.chain_traced(model.joint_rbm, a, b, model.joint_rbm._rng(z0.size(0)))
    i2t = _img2txt_result(eng, tra, lbls.to(model.device), 1e-3, 3, 0.25)
    t2i = _txt2img_result(eng, model, trb, z0, imgs, 1e-3, 1e-5, 3, 0.0)
    return i2t, t2i


# ---- the reference's B = 1 entry points ------------------------------------------------------------------------------------
def _img2txt_dict(o, i: int, max_steps: int, with_gt: bool) -> dict:
    s = int(o["steps"][i])
    n = s if s <= max_steps else max_steps
    p1 = o["p_top1"][i, :n].double().tolist()
    p2 = o["p_top2"][i, :n].double().tolist()
    return {
        "dir": "img2txt",
        "steps_to_converge": s,
        "p_top1": p1,
        "p_top2": p2,
        "p_gap": [a - b for a, b in zip(p1, p2)],
        "p_gt": o["p_gt"][i, :n].double().tolist() if with_gt else None,
        "l1": o["l1"][i, :n].double().tolist(),
        "predT": int(o["pred"][i]),
        "top1_idx": [int(k) for k in o["k1"][i, :n].tolist()],
        "top2_idx": [int(k) for k in o["k2"][i, :n].tolist()],
        "gt_idx": int(o["gt"][i]) if with_gt else None,
    }


def _txt2img_dict(o, i: int, max_steps: int) -> dict:
    s = int(o["steps"][i])
    n = s if s <= max_steps else max_steps
    return {
        "dir": "txt2img",
        "steps_to_converge": s,
        "z_l2": o["z_l2"][i, :n].double().tolist(),
        "image_mse": o["image_mse"][i, :n].double().tolist(),
        "best_mse": float(o["best_mse"][i]),
    }


@torch.no_grad()
def trace_img2txt_cross(model, img, lbl_onehot=None, max_steps=70, sample_h=False, sample_v=False, eps_l1=1e-3, stable_steps=3,
                        gap_thresh=0.25):
    """conditional_steps.py:40-130 (lists cut at the convergence step, as the reference's ``break`` cuts them)."""
    o = trace_img2txt_cross_batch(model, img, lbl_onehot, max_steps, sample_h, sample_v, eps_l1, stable_steps, gap_thresh)
    return _img2txt_dict(o, 0, int(max_steps), lbl_onehot is not None)


@torch.no_grad()
def trace_txt2img_cross(model, img, lbl_onehot, max_steps=70, sample_h=False, sample_v=False, eps_z=1e-3, mse_tol=1e-5, patience=3,
                        ema_beta: float = 0.0):
    """conditional_steps.py:133-241."""
    o = trace_txt2img_cross_batch(model, img, lbl_onehot, max_steps, sample_h, sample_v, eps_z, mse_tol, patience, ema_beta)
    return _txt2img_dict(o, 0, int(max_steps))


# ---- fixed sample / panel (host logic) ---------------------------------------------------------------------------------------
@torch.no_grad()
def pick_fixed_val_case(model, target_label: int | None = None, within_batch_index: int = 0):
    """One validation sample, cached on the model as CPU tensors so that it stays the same across epochs (:244-275)."""
    dev = model.device
    cached = getattr(model, "_fixed_val_case", None)
    if cached is not None:
        return cached[0].to(dev), cached[1].to(dev)
    if model.val_loader is None:
        raise RuntimeError("model.val_loader is None")
    pick = None
    if target_label is None:
        imgs, lbls = next(iter(model.val_loader))
        j = int(within_batch_index)
        pick = (imgs[j:j + 1].cpu(), lbls[j:j + 1].cpu())
    else:
        for imgs, lbls in model.val_loader:
            hits = torch.nonzero(lbls.argmax(dim=1) == target_label).flatten()
            if hits.numel():
                j = int(hits[0])
                pick = (imgs[j:j + 1].cpu(), lbls[j:j + 1].cpu())
                break
        if pick is None:
            imgs, lbls = next(iter(model.val_loader))
            pick = (imgs[:1].cpu(), lbls[:1].cpu())
    model._fixed_val_case = pick
    return pick[0].to(dev), pick[1].to(dev)


@torch.no_grad()
def build_or_get_fixed_val_panel(model, per_class: int = 4):
    """Up to ``per_class`` validation samples of every class, in class order, cached on the model (:392-434)."""
    dev = model.device
    cached = getattr(model, "_fixed_val_panel", None)
    if cached is not None:
        return cached[0].to(dev), cached[1].to(dev)
    if model.val_loader is None:
        raise RuntimeError("val_loader is None")
    K = int(getattr(model, "num_labels", 32))
    buckets = [[] for _ in range(K)]
    for imgs, lbls in model.val_loader:
        cls = lbls.argmax(dim=1).tolist()
        for j, c in enumerate(cls):
            if len(buckets[c]) < per_class:
                buckets[c].append((imgs[j:j + 1].cpu(), lbls[j:j + 1].cpu()))
        if per_class >= 1 and all(len(b) >= per_class for b in buckets):
            break
    chosen = [item for b in buckets for item in b]
    if not chosen:
        imgs, lbls = next(iter(model.val_loader))
        chosen = [(imgs[:1].cpu(), lbls[:1].cpu())]
    imgs_cpu = torch.cat([x for x, _ in chosen], dim=0)
    lbls_cpu = torch.cat([y for _, y in chosen], dim=0)
    model._fixed_val_panel = (imgs_cpu, lbls_cpu)
    return imgs_cpu.to(dev), lbls_cpu.to(dev)


@torch.no_grad()
def _steps_stats(steps_list, max_steps):
    """n / fraction converged / mean / p50 / p95 over the converged rows (steps <= max_steps) and the converged mask (:437-450)."""
    arr = np.asarray(steps_list, dtype=np.int32)
    mask = arr <= max_steps
    c = arr[mask]
    has = c.size > 0
    return {
        "n_total": int(arr.size),
        "n_converged": int(c.size),
        "frac_converged": float(c.size / max(1, arr.size)),
        "mean": float(c.mean()) if has else None,
        "p50": float(np.percentile(c, 50)) if has else None,
        "p95": float(np.percentile(c, 95)) if has else None,
    }, mask


def _run(model):
    return getattr(model, "wandb_run", None)


@torch.no_grad()
def log_cross_case(model, out_img2txt: dict, out_txt2img: dict, epoch: int, tag: str):
    """The summary of one fixed case (:278-362) to ``model.wandb_run`` (no figures, no tables)."""
    run = _run(model)
    if run is None:
        return
    summary = {
        "img2txt_steps": out_img2txt.get("steps_to_converge") if out_img2txt else None,
        "txt2img_steps": out_txt2img.get("steps_to_converge") if out_txt2img else None,
        "txt2img_best_mse": out_txt2img.get("best_mse") if out_txt2img else None,
        "img2txt_pred_final": out_img2txt.get("predT") if out_img2txt else None,
        "img2txt_gt": out_img2txt.get("gt_idx") if out_img2txt else None,
    }
    run.log({f"cross/{tag}/summary": summary, "epoch": epoch})


@torch.no_grad()
def run_and_log_cross_fixed_case(model, epoch: int, target_label: int | None = None, within_batch_index: int = 0, max_steps: int = 70,
                                 sample_h: bool = False, sample_v: bool = False, tag: str = "fixed_cross"):
    """Both directions on the cached fixed sample (:365-389), IMG->TXT first."""
    img, lbl = pick_fixed_val_case(model, target_label=target_label, within_batch_index=within_batch_index)
    a = trace_img2txt_cross(model, img, lbl_onehot=lbl, max_steps=max_steps, sample_h=sample_h, sample_v=sample_v)
    b = trace_txt2img_cross(model, img, lbl_onehot=lbl, max_steps=max_steps, sample_h=sample_h, sample_v=sample_v)
    log_cross_case(model, a, b, epoch=epoch, tag=tag)
    return a, b


@torch.no_grad()
def run_and_log_cross_panel(model, epoch: int, per_class: int = 4, max_steps: int = 70, sample_h: bool = False, sample_v: bool = False,
                            tag: str = "panel"):
    """Both directions over the fixed panel (:475-554) as ONE traced chain pair, one batched decode error and the scans."""
    imgs, lbls = build_or_get_fixed_val_panel(model, per_class=per_class)
    i2t, t2i = trace_cross_panel_batch(model, imgs, lbls, max_steps=max_steps, sample_h=sample_h, sample_v=sample_v)
    T = int(max_steps)
    s_i2t = [int(x) for x in i2t["steps"].tolist()]
    s_t2i = [int(x) for x in t2i["steps"].tolist()]
    # the reference's "final" values: the last entry of each cut list (the convergence step, else step max_steps)
    last = torch.clamp(i2t["steps"].long(), max=T) - 1
    rows = torch.arange(last.numel(), device=last.device)
    p1 = i2t["p_top1"][rows, last].double().tolist() if T > 0 else []
    gap = (i2t["p_top1"][rows, last].double() - i2t["p_top2"][rows, last].double()).tolist() if T > 0 else []
    best = t2i["best_mse"].double().tolist()
    st_i2t, _ = _steps_stats(s_i2t, max_steps)
    st_t2i, _ = _steps_stats(s_t2i, max_steps)
    mean_p1 = float(np.mean(p1)) if p1 else None
    mean_gap = float(np.mean(gap)) if gap else None
    mean_best = float(np.mean(best)) if best else None
    run = _run(model)
    if run is not None:
        summary = {"img2txt/" + k: st_i2t[k] for k in ("mean", "p50", "p95", "frac_converged")}
        summary.update({"txt2img/" + k: st_t2i[k] for k in ("mean", "p50", "p95", "frac_converged")})
        summary.update({"img2txt/p_top1_final_mean": mean_p1, "img2txt/p_gap_final_mean": mean_gap,
                        "txt2img/best_mse_mean": mean_best, "n_total": st_i2t["n_total"]})
        run.log({f"conv/panel/{tag}/summary": summary, "epoch": epoch})
    return {
        "img2txt": {"steps": s_i2t, "stats": st_i2t, "p1_mean": mean_p1, "gap_mean": mean_gap},
        "txt2img": {"steps": s_t2i, "stats": st_t2i, "best_mse_mean": mean_best},
    }


# ---- code mismatch ------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def z_mismatch_stats(model, max_steps: int = 20, sample_h: bool = False, sample_v: bool = False, batch=None) -> Optional[dict]:
    """What ``run_and_log_z_mismatch_check`` (:557-646) logs, as a dict: statistics of the image code ``represent(x)`` of the first
    validation batch and of the code a label-clamped chain reaches (uniform start, ``max_steps`` steps, last p(v|h)), and the mean
    per-row cosine between the two.  None when there is no validation batch."""
    dev = model.device
    if batch is None:
        try:
            batch = next(iter(model.val_loader))
        except Exception:
            return None
    imgs, lbls = batch[0].to(dev), batch[1].to(dev).float()
    B = imgs.size(0)
    z_img = model.image_idbn.represent(imgs.reshape(B, -1))
    Dz = z_img.size(1)
    K = int(getattr(model, "num_labels", lbls.size(1)))
    if sample_h or sample_v:
        # the reference runs (and discards) a TXT->IMG trace per row first; only its draws matter -- none without sampling
        trace_txt2img_cross_batch(model, imgs, lbls, max_steps=max_steps, sample_h=sample_h, sample_v=sample_v)
    vk = torch.zeros(B, Dz + K, device=dev)
    vk[:, Dz:] = lbls
    km = torch.zeros_like(vk)
    km[:, Dz:] = 1.0
    spec = {"v_known": vk, "mask": km, "steps": [_step(sample_h, sample_v)] * int(max_steps), "init_uniform": True,
            "trace": (0, Dz, False)}
    ((_, tr),) = _eng(model).chain_traced(model.joint_rbm, spec, None, model.joint_rbm._rng(B))
    z_y = tr[-1]

    def stats(t):
        return {"mean": float(t.mean()), "std": float(t.std(unbiased=False)), "q10": float(t.quantile(0.10)),
                "q90": float(t.quantile(0.90))}

    u_img = z_img / (z_img.norm(dim=1, p=2, keepdim=True) + 1e-12)
    u_y = z_y / (z_y.norm(dim=1, p=2, keepdim=True) + 1e-12)
    cos = (u_img * u_y).sum(dim=1).clamp(-1, 1)
    return {"z_img_stats": stats(z_img), "z_y_stats": stats(z_y), "cosine_mean": float(cos.mean())}


def run_and_log_z_mismatch_check(model, epoch: int, max_steps: int = 20, sample_h: bool = False, sample_v: bool = False,
                                 tag: str = "z_check"):
    """:557-646 -- returns at once without a ``wandb_run`` (no draws consumed), else logs the ``z_mismatch_stats`` dicts."""
    run = _run(model)
    if run is None:
        return None
    st = z_mismatch_stats(model, max_steps=max_steps, sample_h=sample_h, sample_v=sample_v)
    if st is None:
        return None
    run.log({f"zcheck/{tag}/z_img_stats": st["z_img_stats"], "epoch": epoch})
    run.log({f"zcheck/{tag}/z_y_stats": st["z_y_stats"], "epoch": epoch})
    run.log({f"zcheck/{tag}/cosine_mean": st["cosine_mean"], "epoch": epoch})
    return st
