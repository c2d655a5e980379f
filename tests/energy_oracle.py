"""numpy (fp64) restatement of the IMG->TXT energy trace of imdbn/utils/energy_utils.py (reference :31-195).

The step multiplies the FULL visible vector [z, y] by W, as the reference does -- not the ``base + y @ Wy`` split the engine
kernel uses -- so the oracle does not share the kernel's shortcut."""
from __future__ import annotations

import numpy as np


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def softplus(x):
    return np.logaddexp(0.0, x)


def class_free_energies(W, hb, vb, z, K):
    """F_k(z) = F([z, e_k]) by the definition: one full free energy per completed visible vector."""
    N, Dz = z.shape
    F = np.zeros((N, K))
    for k in range(K):
        v = np.concatenate([z, np.tile(np.eye(K)[k], (N, 1))], 1)
        F[:, k] = -(v @ vb[:Dz + K]) - softplus(v @ W[:Dz + K] + hb).sum(1)
    return F


def step(W, hb, vb, v, Dz, K):
    """reference :69-88 with softmax_y, no sampling: v [N, Dz + K] -> v_next."""
    h = sigmoid(v @ W[:Dz + K] + hb)
    p = sigmoid(h @ W[:Dz + K].T + vb[:Dz + K])
    y = p[:, Dz:]
    e = np.exp(y - y.max(1, keepdims=True))
    return np.concatenate([v[:, :Dz], e / e.sum(1, keepdims=True)], 1)


def top2(y):
    """(p1, p2, k1, k2): value descending, the lower index on ties."""
    order = np.lexsort((np.arange(len(y)), -y))
    return y[order[0]], y[order[1]], int(order[0]), int(order[1])


def trace(W, hb, vb, z, K, steps, gt=None, y0=None, eps_l1=1e-3, stable_steps=3, gap_thresh=0.25):
    """All ``steps`` for every row.  Curves [N, steps]: p1, p2, p_gt, dF, l1, k1; per row: conv (steps + 1 = never), kstar, predT,
    margin_energy, fe_top1, fe_gap, F [N, K], y (final); room [N] = the smallest distance of a decision (l1 vs eps, gap vs
    gap_thresh, p1 vs p2, F(2) vs F(1)) from its threshold up to the stopping step."""
    W, hb, vb, z = (np.asarray(a, np.float64) for a in (W, hb, vb, z))
    N, Dz = z.shape
    F = class_free_energies(W, hb, vb, z, K)
    o = {k: np.zeros((N, steps)) for k in ("p1", "p2", "p_gt", "dF", "l1")}
    o["k1"] = np.zeros((N, steps), np.int64)
    o.update(F=F, conv=np.full(N, steps + 1), kstar=np.zeros(N, np.int64), predT=np.zeros(N, np.int64), margin_energy=np.zeros(N),
             fe_top1=np.zeros(N), fe_gap=np.zeros(N), room=np.full(N, np.inf), y=np.zeros((N, K)))
    for b in range(N):
        f1, f2, ks, _ = top2(-F[b])
        o["kstar"][b], o["margin_energy"][b] = ks, f1 - f2
        fe = np.exp(-F[b] - f1); fe /= fe.sum()
        q1, q2, _, _ = top2(fe)
        o["fe_top1"][b], o["fe_gap"][b] = q1, q1 - q2
        y = np.full(K, 1.0 / K) if y0 is None else np.asarray(y0[b], np.float64)
        v = np.concatenate([z[b], y])[None]
        pred, streak, done = top2(y)[2], 0, False
        room = f1 - f2
        for t in range(steps):
            v = step(W, hb, vb, v, Dz, K)
            yn = v[0, Dz:]
            p1, p2, k1, _ = top2(yn)
            l1 = np.abs(yn - y).sum()
            streak = streak + 1 if k1 == pred else 1
            pred = k1
            o["p1"][b, t], o["p2"][b, t], o["k1"][b, t], o["l1"][b, t], o["dF"][b, t] = p1, p2, k1, l1, F[b, k1] + f1
            if gt is not None:
                o["p_gt"][b, t] = yn[gt[b]]
            if not done:
                room = min(room, abs(l1 - eps_l1), abs((p1 - p2) - gap_thresh), p1 - p2)
                if l1 < eps_l1 and streak >= stable_steps and (pred == ks or p1 - p2 >= gap_thresh):
                    o["conv"][b], o["predT"][b], done = t + 1, pred, True
                    o["room"][b] = room
            y = yn
        if not done:
            o["predT"][b], o["room"][b] = pred, room
        o["y"][b] = y
    return o
