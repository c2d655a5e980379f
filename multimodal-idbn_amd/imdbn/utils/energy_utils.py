"""Free energies and IMG->TXT energy tracing on the engine (reference ``imdbn/utils/energy_utils.py``).

``rbm_free_energy`` is the function the reference's evaluation tooling calls; here it is one engine call
(``imdbn_rbm_free_energy``).  ``class_free_energies`` evaluates F([z, e_k]) for every label k by stacking the K
one-hot completions of each row into one [B*K, V] batch -- the engine streams W once for the whole stack -- instead of
the reference's dense [B, K, H] broadcast.

The trace (reference :60-195) asks how many mean-field steps the label distribution y needs to settle with the image code z
clamped, and how the settled label compares with the class free energies F_k(z).  The reference traces ONE sample per call
with two full ``[1, V] x [V, H]`` products and about six host syncs per step.  Here a whole panel is one engine call
(``HipEngine.energy_trace`` -> ``imdbn_energy_trace``): z never changes, so ``z @ W[:Dz] + hid_bias`` is one propagation for
the panel, and one kernel runs every step on the label rows of W, the free energies, the top-2 curves and the stop rule.

Two quirks of the reference are kept, because they are the specification:

* the step is not ``RBM.visible_probs``: it takes the sigmoid of every visible logit and then a softmax over the SIGMOID
  OUTPUTS of the label slice (:72-79), whatever ``softmax_groups`` says.  A softmax over K values in (0, 1) cannot separate
  its top two by more than (e - 1) / (e + K - 1) (0.177 at K = 8, 0.051 at K = 32), so the default ``gap_thresh = 0.25`` is
  unreachable and rows converge only through ``pred == kstar``;
* ``pred_0`` is the argmax of the uniform start (0), so the streak can start at step 1.

``trace_single_img2txt`` keeps the reference's name, signature and dict (lists cut at the convergence step); it is a B = 1
wrapper over ``trace_img2txt_energy_batch``, which returns device tensors for every step of every row and never
synchronises.  ``run_and_log_energy_panel`` runs the fixed validation panel of ``conditional_steps`` through it.

Figures of the reference (matplotlib, ``wandb.Image``) are out of scope: a ``wandb_run`` on the model only receives plain
scalars and dicts through ``.log``.
"""
from __future__ import annotations

import numpy as np
import torch

from imdbn import engine as _E

from .conditional_steps import _steps_stats, build_or_get_fixed_val_panel, pick_fixed_val_case

__all__ = ["rbm_free_energy", "class_free_energies", "_deterministic_img2txt_step", "trace_single_img2txt",
           "trace_img2txt_energy_batch", "pick_fixed_val_case", "pick_val_case", "log_single_case_energy", "run_and_log_fixed_case",
           "run_and_log_energy_panel"]


@torch.no_grad()
def rbm_free_energy(rbm, v: torch.Tensor) -> torch.Tensor:
    """F(v) = -v.b - sum_j softplus(c_j + (vW)_j); v: [B, V] in [0, 1] (may be mean-field); returns [B]."""
    return rbm.free_energy(v)


@torch.no_grad()
def class_free_energies(joint_rbm, z_img_top: torch.Tensor, K: int, Dz: int) -> torch.Tensor:
    """F_k(z) = F([z, e_k]) for k = 0..K-1; z_img_top: [B, Dz] -> [B, K]."""
    z = z_img_top.to(joint_rbm.W.device).float()
    B = z.size(0)
    v = torch.zeros(B, K, Dz + K, device=z.device)
    v[:, :, :Dz] = z.unsqueeze(1)
    v[:, :, Dz:] = torch.eye(K, device=z.device).unsqueeze(0)
    return joint_rbm.free_energy(v.view(B * K, Dz + K)).view(B, K)


def _eng(joint_rbm):
    return _E.get_engine(joint_rbm.W.data)


# ---- one "mean-field lite" step on y (:60-88) -----------------------------------------------------------------------------
@torch.no_grad()
def _deterministic_img2txt_step(joint_rbm, v: torch.Tensor, Dz: int, K: int, softmax_y: bool = True, sample_h: bool = False,
                                sample_v: bool = False) -> torch.Tensor:
    """v -> h -> sigmoid of the visible logits, z re-clamped, y re-normalised; v: [B, Dz + K].

    With the defaults this is the trace kernel with ``steps = 1`` started from the y of ``v``.  The other flags have no caller
    in the reference; they compose engine calls: ``prop_up`` (with a Bernoulli sample of h for ``sample_h``), the raw visible
    logits of ``prop_down``, a torch tail on the ``[B, K]`` label slice, and for ``sample_v`` the categorical draw of
    ``sample_visible`` over the label group (engine Philox draws, not torch's generator)."""
    dev = joint_rbm.W.device
    v = v.to(dev).float()
    Dz, K = int(Dz), int(K)
    V = joint_rbm.W.size(0)
    eng = _eng(joint_rbm)
    if softmax_y and not sample_h and not sample_v and V == Dz + K:
        o = eng.energy_trace(joint_rbm, v[:, :Dz], K, 1, y_start=v[:, Dz:Dz + K], want_y=True)
        return torch.cat([v[:, :Dz], o["y"]], dim=1)
    B = v.size(0)
    if sample_h:
        _, h = eng.prop_up(joint_rbm, v, sample=True, rng=joint_rbm._rng(B))
    else:
        h = eng.prop_up(joint_rbm, v)
    v_next = torch.sigmoid(eng.prop_down(joint_rbm, h, logits_only=True))
    v_next[:, :Dz] = v[:, :Dz]
    y = v_next[:, Dz:Dz + K]
    y = torch.softmax(y, dim=1) if softmax_y else y.clamp(1e-6, 1 - 1e-6)
    v_next[:, Dz:Dz + K] = y
    if sample_v:
        groups = [(int(s), int(e)) for s, e in (getattr(joint_rbm, "softmax_groups", None) or [])]
        if (Dz, Dz + K) not in groups:
            raise _E.EngineError(f"sample_v needs the label columns [{Dz}, {Dz + K}) to be a softmax group of the joint RBM")
        drawn = eng.sample_visible(joint_rbm, v_next, joint_rbm._rng(B))
        v_next[:, Dz:Dz + K] = drawn[:, Dz:Dz + K]
    return v_next


# ---- the trace ---------------------------------------------------------------------------------------------------------------
def _code(model, imgs):
    dev = model.device
    x = imgs.to(dev)
    x = x.reshape(x.size(0), -1).float() if x.dim() > 2 else x.float()
    return model.image_idbn.represent(x).clamp(1e-6, 1 - 1e-6)


@torch.no_grad()
def trace_img2txt_energy_batch(model, imgs: torch.Tensor, lbls: torch.Tensor | None = None, steps: int = 30, eps_l1: float = 1e-3,
                               stable_steps: int = 3, gap_thresh: float = 0.25) -> dict:
    """The trace for a panel: device tensors ``p_top1, p_top2, p_gt, deltaF_pred, l1, k1`` ``[B, steps]`` (every step, also
    past convergence; ``p_gt`` None without labels), ``steps`` ``[B]`` (``steps + 1`` = not converged), ``kstar, predT,
    margin_energy, fe_top1, fe_gap`` ``[B]``, ``F`` ``[B, K]``, ``gt`` ``[B]`` or None.  No host synchronisation."""
    z = _code(model, imgs)
    Dz = int(getattr(model, "Dz_img", z.size(1)))
    K = int(getattr(model, "num_labels", (lbls.size(1) if lbls is not None else 32)))
    gt = lbls.to(model.device).argmax(dim=1) if lbls is not None else None
    o = _eng(model.joint_rbm).energy_trace(model.joint_rbm, z[:, :Dz], K, int(steps), gt=gt, eps_l1=eps_l1, stable_steps=stable_steps,
                                           gap_thresh=gap_thresh)
    o.pop("y")
    o["gt"] = gt
    return o


_CURVES = ("p_top1", "p_top2", "p_gt", "deltaF_pred")
_ROW = ("steps", "kstar", "predT", "margin_energy", "fe_top1", "fe_gap", "gt")


def _to_host(o: dict) -> dict:
    """Everything the dicts need, in ONE device-to-host copy (fp64: exact for the fp32 curves and the int32 columns)."""
    keys = [k for k in _CURVES + _ROW if o.get(k) is not None]
    n = o["steps"].size(0)
    flat = torch.cat([o[k].reshape(n, -1).double() for k in keys], dim=1).cpu().numpy()
    out, c = {k: None for k in _CURVES + _ROW}, 0
    for k in keys:
        w = o[k].reshape(n, -1).size(1)
        out[k] = flat[:, c:c + w]
        c += w
    return out


def _case_dict(h: dict, i: int, steps: int, K: int) -> dict:
    """Row ``i`` of the host arrays as the reference's dict (:175-195): lists cut at the convergence step."""
    s = int(h["steps"][i, 0])
    n = min(s, int(steps))
    p1, p2 = h["p_top1"][i, :n].tolist(), h["p_top2"][i, :n].tolist()
    gap = [a - b for a, b in zip(p1, p2)]
    dF = h["deltaF_pred"][i, :n].tolist()
    with_gt = h["gt"] is not None
    return {
        "deltaF_pred_traj": dF,
        "deltaF_pred_final": dF[-1] if dF else None,
        "p_top1": p1,
        "p_top2": p2,
        "p_gap": gap,
        "p_gt": h["p_gt"][i, :n].tolist() if with_gt else None,
        "p_top1_final": p1[-1] if p1 else float(1.0 / K),
        "p_gap_final": gap[-1] if gap else 0.0,
        "fe_top1_final": float(h["fe_top1"][i, 0]),
        "fe_gap_final": float(h["fe_gap"][i, 0]),
        "steps_to_converge": s,
        "kstar": int(h["kstar"][i, 0]),
        "predT": int(h["predT"][i, 0]),
        "margin_energy": float(h["margin_energy"][i, 0]),
        "gt": int(h["gt"][i, 0]) if with_gt else None,
    }


@torch.no_grad()
def trace_single_img2txt(model, img: torch.Tensor, lbl_onehot: torch.Tensor | None, steps: int = 30, eps_l1: float = 1e-3,
                         stable_steps: int = 3, gap_thresh: float = 0.25):
    """Reference :95-195 for one sample: the curves up to the convergence step, the final confidences, ``steps_to_converge``
    (``steps + 1`` = never), ``kstar`` / ``predT``, ``margin_energy`` = F(2) - F(1) and softmax(-F) top-1 / gap."""
    o = trace_img2txt_energy_batch(model, img[:1], lbl_onehot[:1] if lbl_onehot is not None else None, steps, eps_l1, stable_steps,
                                   gap_thresh)
    return _case_dict(_to_host(o), 0, int(steps), o["F"].size(1))


# ---- fixed validation case (:202-245; ``pick_fixed_val_case`` is the one of conditional_steps: same signature, same cache) --
@torch.no_grad()
def pick_val_case(model, target_label: int | None = None, batch_idx: int = 0, within_batch_index: int = 0):
    """Backward-compatible alias: ignores ``batch_idx`` and uses the cached fixed case."""
    return pick_fixed_val_case(model, target_label=target_label, within_batch_index=within_batch_index)


_SUMMARY = ("gt", "kstar", "predT", "steps_to_converge", "p_top1_final", "p_gap_final", "fe_top1_final", "fe_gap_final",
            "deltaF_pred_final", "margin_energy")


@torch.no_grad()
def log_single_case_energy(model, case_dict: dict, epoch: int, tag: str = "fixed_case"):
    """The summary of one case (:290-304) to ``model.wandb_run`` (no figures); returns silently without a run."""
    run = getattr(model, "wandb_run", None)
    if run is None:
        return
    run.log({f"case/{tag}/summary": {k: case_dict.get(k, None) for k in _SUMMARY}, "epoch": epoch})


@torch.no_grad()
def run_and_log_fixed_case(model, epoch: int, target_label: int | None = None, within_batch_index: int = 0, steps: int = 30,
                           tag: str = "fixed"):
    """The trace on the cached fixed sample (:311-324); returns the case dict."""
    img, lbl = pick_fixed_val_case(model, target_label=target_label, within_batch_index=within_batch_index)
    case = trace_single_img2txt(model, img, lbl, steps=steps)
    log_single_case_energy(model, case, epoch=epoch, tag=tag)
    return case


@torch.no_grad()
def run_and_log_energy_panel(model, epoch: int, per_class: int = 4, steps: int = 30, eps_l1: float = 1e-3, stable_steps: int = 3,
                             gap_thresh: float = 0.25, tag: str = "panel"):
    """The trace over the fixed validation panel (``build_or_get_fixed_val_panel``) as one engine call and one host copy.
    Returns ``steps`` (per row), ``stats`` (``_steps_stats``), the means of the reference's per-case finals and the
    accuracies of the two predictors (chain argmax, free-energy argmin); logs the scalars to ``model.wandb_run``."""
    imgs, lbls = build_or_get_fixed_val_panel(model, per_class=per_class)
    o = trace_img2txt_energy_batch(model, imgs, lbls, steps, eps_l1, stable_steps, gap_thresh)
    h = _to_host(o)
    T, K = int(steps), o["F"].size(1)
    cases = [_case_dict(h, i, T, K) for i in range(h["steps"].shape[0])]
    s = [c["steps_to_converge"] for c in cases]
    stats, _ = _steps_stats(s, T)
    mean = lambda k: float(np.mean([c[k] for c in cases]))
    out = {
        "steps": s,
        "stats": stats,
        "p_top1_final_mean": mean("p_top1_final"),
        "p_gap_final_mean": mean("p_gap_final"),
        "deltaF_pred_final_mean": mean("deltaF_pred_final"),
        "fe_top1_final_mean": mean("fe_top1_final"),
        "margin_energy_mean": mean("margin_energy"),
        "acc_pred": float(np.mean([c["predT"] == c["gt"] for c in cases])),
        "acc_kstar": float(np.mean([c["kstar"] == c["gt"] for c in cases])),
        "agree_pred_kstar": float(np.mean([c["predT"] == c["kstar"] for c in cases])),
    }
    run = getattr(model, "wandb_run", None)
    if run is not None:
        summary = {k: stats[k] for k in ("mean", "p50", "p95", "frac_converged", "n_total")}
        summary.update({k: v for k, v in out.items() if k not in ("steps", "stats")})
        run.log({f"case/{tag}/summary": summary, "epoch": epoch})
    return out
