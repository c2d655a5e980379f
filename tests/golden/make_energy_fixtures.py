#!/usr/bin/env python3
"""Generate tests/golden/energy_trace_small.npz: the reference's IMG->TXT energy tracing (imdbn/utils/energy_utils.py) on
the trained small iMDBN of imdbn_small_100_40_20_j16.npz.

Run in the build container only (needs the reference checkout, as make_fixtures.py does):

    python tests/golden/make_energy_fixtures.py

The UNMODIFIED reference functions run on the duck-typed model of make_trace_fixtures.model.  No draws are involved (the trace
is deterministic).  Recorded: the fixed case (``run_and_log_fixed_case``), the same sample without a label, a panel of rows
with all three outcomes (converged at step 3, at step 4, never), one row that converges through the gap branch with a small
``gap_thresh``, the class free energies and their summaries per row, what ``log_single_case_energy`` logs to a stub run, and
the function signatures / dict keys.

The recorded rows are chosen so that every decision of the reference's own fp32 run has room: ``|l1 - eps_l1|``,
``|gap - gap_thresh|`` and ``p_top1 - p_top2`` at every recorded step, and ``F(2) - F(1)``, are each at least ``ROOM``; the
script asserts it and writes the smallest margins into ``meta``.  The reference does not return l1: it is re-run here with
the reference's own ``_deterministic_img2txt_step`` and the reference's expression for it, in fp32.
"""
from __future__ import annotations

import inspect
import json
import os
import sys
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_trace_fixtures as TF  # noqa: E402  (make_fixtures: reference on sys.path, wandb stubbed, scratch cwd)

import torch  # noqa: E402
from imdbn.utils import energy_utils as EU  # noqa: E402  (the reference's)

STEPS = 30
ROOM = 1e-5
GAP_SMALL = (0.003, 0.002, 0.001, 0.0005)      # tried in this order: the largest threshold some never-converging row reaches with room
FUNCS = ["rbm_free_energy", "class_free_energies", "_deterministic_img2txt_step", "trace_single_img2txt", "pick_fixed_val_case",
         "pick_val_case", "log_single_case_energy", "run_and_log_fixed_case"]
CURVES = ("deltaF_pred_traj", "p_top1", "p_top2", "p_gap", "p_gt")


def l1_curve(m, img, n):
    """|y_t - y_{t-1}|_1 for t = 1..n, as reference :163 computes it (fp32), with the reference's step function."""
    x = img.view(img.size(0), -1).float()
    z = m.image_idbn.represent(x).clamp(1e-6, 1 - 1e-6)
    Dz, K = m.Dz_img, m.num_labels
    y = torch.full((1, K), 1.0 / K)
    v = torch.cat([z, y], dim=1)
    out = []
    for _ in range(n):
        v = EU._deterministic_img2txt_step(m.joint_rbm, v, Dz, K)
        out.append(float((v[:, Dz:Dz + K] - y).abs().sum().item()))
        y = v[:, Dz:Dz + K].clone()
    return out


def energies(m, img):
    x = img.view(img.size(0), -1).float()
    z = m.image_idbn.represent(x).clamp(1e-6, 1 - 1e-6)
    return EU.class_free_energies(m.joint_rbm, z, m.num_labels, m.Dz_img)[0].numpy()


def room(case, l1, eps_l1=1e-3, gap_thresh=0.25):
    """The smallest distance of a decision from its threshold over the recorded steps."""
    d = [case["margin_energy"]]
    for t in range(len(case["p_top1"])):
        d += [abs(l1[t] - eps_l1), abs(case["p_gap"][t] - gap_thresh), case["p_top1"][t] - case["p_top2"][t]]
    return min(d)


def pack(cases, l1s, Fs, pre):
    R, T = len(cases), STEPS
    out = {}
    for k in CURVES + ("l1",):
        a = np.full((R, T), np.nan, np.float64)
        for i, c in enumerate(cases):
            v = l1s[i] if k == "l1" else c[k]
            if v is not None:
                a[i, :len(v)] = v
        out[pre + k] = a
    out[pre + "ints"] = np.array([[c["steps_to_converge"], c["kstar"], c["predT"], -1 if c["gt"] is None else c["gt"]] for c in cases], np.int32)
    out[pre + "floats"] = np.array([[c["margin_energy"], c["fe_top1_final"], c["fe_gap_final"], c["deltaF_pred_final"], c["p_top1_final"],
                                     c["p_gap_final"]] for c in cases], np.float64)
    out[pre + "F"] = np.stack(Fs).astype(np.float32)
    return out


def main():
    z, X, Y = TF.data()
    m = TF.model(z, X, Y)
    Xt, Yt = torch.from_numpy(X), torch.from_numpy(Y)
    out, meta = {}, {"steps": STEPS, "room": ROOM, "funcs": {}, "min_room": {}}
    for f in FUNCS:
        meta["funcs"][f] = list(inspect.signature(getattr(EU, f)).parameters)

    # 1. the fixed case through the reference's entry point; a stub run and stub figures record what it logs
    run = TF.StubRun()
    m.wandb_run = run
    plt = mock.MagicMock()
    plt.subplots.side_effect = lambda *a, **k: (mock.MagicMock(), mock.MagicMock())
    with mock.patch.object(EU, "plt", plt), mock.patch.object(EU, "wandb", mock.MagicMock()):
        fixed = EU.run_and_log_fixed_case(m, epoch=7)
    m.wandb_run = None
    img, lbl = m._fixed_val_case
    meta["dict_keys"] = list(fixed)
    summ = [d for d in run.logged if "case/fixed/summary" in d]
    assert len(summ) == 1 and summ[0]["epoch"] == 7
    meta["logged_summary"] = summ[0]["case/fixed/summary"]
    l1 = l1_curve(m, img, len(fixed["p_top1"]))
    meta["min_room"]["fixed"] = room(fixed, l1)
    out["fixed_img"], out["fixed_lbl"] = img.numpy(), lbl.numpy()
    out.update(pack([fixed], [l1], [energies(m, img)], "fx_"))
    # 2. the same sample without a label
    nolbl = EU.trace_single_img2txt(m, img, None, steps=STEPS)
    assert nolbl["p_gt"] is None and nolbl["gt"] is None
    out.update(pack([nolbl], [l1], [energies(m, img)], "nl_"))

    # 3. every sample once; the panel = rows with room, all three outcomes present
    cases, l1s, rooms = [], [], []
    for i in range(len(X)):
        c = EU.trace_single_img2txt(m, Xt[i:i + 1], Yt[i:i + 1], steps=STEPS)
        l = l1_curve(m, Xt[i:i + 1], len(c["p_top1"]))
        cases.append(c); l1s.append(l); rooms.append(room(c, l))
    outcome = np.array([c["steps_to_converge"] for c in cases])
    meta["all_outcomes"] = {str(k): int((outcome == k).sum()) for k in sorted(set(outcome.tolist()))}
    ok = np.array(rooms) >= ROOM
    pick = []
    for k in sorted(set(outcome.tolist())):
        rows = [i for i in range(len(X)) if outcome[i] == k and ok[i]]
        assert rows, f"no row with outcome {k} has {ROOM} of room"
        pick += rows[:16]
    pick = sorted(pick)
    assert len(pick) >= 32 and len({int(outcome[i]) for i in pick}) >= 3, (len(pick), meta["all_outcomes"])
    assert all(cases[i]["predT"] != cases[i]["kstar"] for i in pick if outcome[i] == STEPS + 1)
    meta["min_room"]["panel"] = float(min(rooms[i] for i in pick))
    meta["panel_outcomes"] = {str(k): int(sum(outcome[i] == k for i in pick)) for k in sorted(set(outcome.tolist()))}
    out["panel_idx"] = np.array(pick, np.int32)
    out["panel_img"], out["panel_lbl"] = X[pick], Y[pick]
    out.update(pack([cases[i] for i in pick], [l1s[i] for i in pick], [energies(m, Xt[i:i + 1]) for i in pick], "pn_"))

    # 4. a row that never converges by default (predT != kstar) converges through the gap branch with a small gap_thresh
    done = False
    for g, i in ((g, i) for g in GAP_SMALL for i in np.nonzero(outcome == STEPS + 1)[0]):
        c = EU.trace_single_img2txt(m, Xt[i:i + 1], Yt[i:i + 1], steps=STEPS, gap_thresh=g)
        if c["steps_to_converge"] > STEPS or c["predT"] == c["kstar"]:
            continue
        l = l1_curve(m, Xt[i:i + 1], len(c["p_top1"]))
        r = room(c, l, gap_thresh=g)
        if r >= ROOM:
            out["gap_idx"] = np.int32(i)
            out["gap_img"], out["gap_lbl"] = X[i:i + 1], Y[i:i + 1]
            out.update(pack([c], [l], [energies(m, Xt[i:i + 1])], "gp_"))
            meta["min_room"]["gap"] = r
            meta["gap_small"] = g
            done = True
            break
    assert done, "no row converges through the gap branch with room"
    assert min(meta["min_room"].values()) >= ROOM, meta["min_room"]
    meta["smallest_margin_energy"] = float(min(out[p + "floats"][:, 0].min() for p in ("fx_", "pn_", "gp_")))
    meta["recipe"] = ("model from imdbn_small_100_40_20_j16.npz (make_trace_fixtures.model), the reference's energy_utils functions, "
                      "steps = 30; curves are NaN-padded past the convergence step; ints = steps_to_converge, kstar, predT, gt; floats = "
                      "margin_energy, fe_top1_final, fe_gap_final, deltaF_pred_final, p_top1_final, p_gap_final")
    path = os.path.join(HERE, "energy_trace_small.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **out)
    print(f"wrote energy_trace_small.npz: {os.path.getsize(path) / 1024:.1f} KiB")
    print("outcomes", meta["all_outcomes"], "panel", meta["panel_outcomes"], "room", meta["min_room"])
    print("fixed", {k: fixed[k] for k in ("steps_to_converge", "kstar", "predT", "gt", "margin_energy")})
    print("gap row", int(out["gap_idx"]), "gap_thresh", meta["gap_small"], out["gp_ints"])


if __name__ == "__main__":
    main()
