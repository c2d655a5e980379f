"""numpy (fp64) restatement of the convergence tracing of imdbn/utils/conditional_steps.py (reference :16-241):
the conditional step, the IMG->TXT label scan, the TXT->IMG code and patience scans, and the decode error."""
from __future__ import annotations

import numpy as np


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def h_probs(W, hb, v):
    return sigmoid(v @ W + hb)


def v_probs(W, vb, h, groups):
    x = h @ W.T + vb
    p = sigmoid(x)
    for s, e in groups:
        g = x[:, s:e] - x[:, s:e].max(1, keepdims=True)
        eg = np.exp(g)
        p[:, s:e] = eg / eg.sum(1, keepdims=True)
    return p


def mean_field_chain(W, hb, vb, groups, v0, vk, mask, T):
    """T mean-field conditional steps (sample_h = sample_v = False): the per-step p(v|h) [T, B, V]."""
    v = np.asarray(v0, np.float64)
    out = []
    for _ in range(T):
        p = v_probs(W, vb, h_probs(W, hb, v), groups)
        out.append(p)
        v = p * (1 - mask) + vk * mask
    return np.stack(out)


def label_scan(y0, ys, gt=None, eps_l1=1e-3, stable_steps=3, gap_thresh=0.25):
    """y0 [B, K] baseline, ys [T, B, K]: per-step p1, p2, k1, k2, p_gt, l1 [B, T]; steps, pred [B]; margin [B] = distance of the
    deciding comparison from its threshold (the smallest over the three conditions at the decisive step / over all steps)."""
    T, B, K = ys.shape
    o = {k: np.zeros((B, T)) for k in ("p1", "p2", "p_gt", "l1")}
    o["k1"], o["k2"] = np.zeros((B, T), np.int64), np.zeros((B, T), np.int64)
    steps, pred, margin = np.full(B, T + 1), np.zeros(B, np.int64), np.full(B, np.inf)
    for b in range(B):
        prev = y0[b]
        cur = int(np.argmax(prev))
        streak = 0
        done = False
        for t in range(T):
            y = ys[t, b]
            order = np.lexsort((np.arange(K), -y))          # value descending, lower index first on ties
            k1, k2 = int(order[0]), int(order[1])
            p1, p2 = y[k1], y[k2]
            l1 = np.abs(y - prev).sum()
            o["p1"][b, t], o["p2"][b, t], o["k1"][b, t], o["k2"][b, t], o["l1"][b, t] = p1, p2, k1, k2, l1
            if gt is not None:
                o["p_gt"][b, t] = y[gt[b]]
            streak = streak + 1 if k1 == cur else 1
            cur = k1
            if not done:
                if streak >= stable_steps:
                    margin[b] = min(margin[b], abs(l1 - eps_l1), abs((p1 - p2) - gap_thresh))
                if l1 < eps_l1 and streak >= stable_steps and p1 - p2 >= gap_thresh:
                    steps[b], pred[b], done = t + 1, k1, True
            prev = y
        if not done:
            pred[b] = cur
    return o, steps, pred, margin


def code_scan(zs, z0, beta=0.0):
    """zs [T, B, Dz] code trace, z0 [B, Dz]: z_new [T, B, Dz], dz [B, T]."""
    T = zs.shape[0]
    zn, dz = np.zeros_like(zs), np.zeros((zs.shape[1], T))
    prev = z0
    for t in range(T):
        z = (1 - beta) * prev + beta * zs[t] if beta > 0 else zs[t]
        dz[:, t] = np.sqrt(((z - prev) ** 2).sum(1))
        zn[t] = z
        prev = z
    return zn, dz


def patience_scan(dz, mse, eps_z=1e-3, mse_tol=1e-5, patience=3):
    """reference :217-234 per row: steps [B] (T + 1 = never), best_mse [B], margin [B] (closest decision to its threshold)."""
    B, T = dz.shape
    steps, best_o, margin = np.full(B, T + 1), np.full(B, np.inf), np.full(B, np.inf)
    for b in range(B):
        best, ni = np.inf, 0
        for t in range(T):
            m = mse[b, t]
            margin[b] = min(margin[b], abs(dz[b, t] - eps_z))
            if np.isfinite(best):
                margin[b] = min(margin[b], abs((m + 1e-12) - (best - mse_tol)) / max(best, 1e-30))
            improved = m + 1e-12 < best - mse_tol
            if dz[b, t] < eps_z:
                if improved:
                    best, ni = m, 0
                else:
                    ni += 1
                if ni >= patience:
                    steps[b] = t + 1
                    break
            else:
                if improved:
                    best = m
                ni = 0
        best_o[b] = best
    return steps, best_o, margin


def decode_sqerr(layers, z, ref):
    """layers: [(W, vb)] bottom first; z [N, Dz]; ref [N, D]: mean((decode(z) - ref)^2, 1)."""
    cur = np.asarray(z, np.float64)
    for W, vb in reversed(layers):
        cur = sigmoid(cur @ W.T + vb)
    return ((cur - ref) ** 2).mean(1)


# ---- the small trained iMDBN of imdbn_small_100_40_20_j16.npz (the model of cross_trace_small.npz) -----------------------------
def small_model_arrays():
    """(weights dict, X [416, 100], Y [416, 8]) -- the data recipe of make_fixtures.case_imdbn_small."""
    import json
    import os
    from oracle.draws import DrawStream
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imdbn_small_100_40_20_j16.npz"))
    meta = json.loads(str(z["meta"]))
    s = DrawStream(meta["seed"])
    K, N = meta["K"], meta["B"] * meta["NB"]
    yi = z["yi"]
    proto = (s.uniform((K, 100)) > 0.7).astype(np.float32)
    flip = (s.uniform((N, 100)) > 0.9).astype(np.float32)
    X = np.abs(proto[yi] - flip).astype(np.float32)
    w = {k: z[k] for k in z.files if k.startswith(("img", "joint_", "z_class_mean"))}
    return w, X, np.eye(K, dtype=np.float32)[yi]


class SmallOracle:
    """fp64 forward / decode of the small model: image stack 100 -> 40 -> 20, joint RBM 28 <-> 16 with the label group [20, 28)."""

    def __init__(self, w):
        self.img = [(w[f"img{i}_W"].astype(np.float64), w[f"img{i}_hid_bias"].astype(np.float64), w[f"img{i}_vis_bias"].astype(np.float64))
                    for i in range(2)]
        self.W, self.hb, self.vb = (w["joint_W"].astype(np.float64), w["joint_hid_bias"].astype(np.float64),
                                    w["joint_vis_bias"].astype(np.float64))
        self.zcm = w["z_class_mean"].astype(np.float64)
        self.groups = [(20, 28)]

    def represent(self, x):
        for W, hb, _ in self.img:
            x = sigmoid(x @ W + hb)
        return x

    def decode_layers(self):
        return [(W, vb) for W, _, vb in self.img]

    Dz, K = 20, 8                           # the code and label widths (StackOracle sets its own)

    def img2txt(self, x, u, T, **kw):
        """x [B, D], u [B, Dz + K] initial uniforms."""
        Dz, V = self.Dz, self.Dz + self.K
        z = self.represent(np.asarray(x, np.float64))
        B = z.shape[0]
        vk = np.zeros((B, V)); vk[:, :Dz] = z
        m = np.zeros((B, V)); m[:, :Dz] = 1
        v0 = vk * m + (1 - m) * u
        y0 = v_probs(self.W, self.vb, h_probs(self.W, self.hb, v0), self.groups)[:, Dz:]
        ys = mean_field_chain(self.W, self.hb, self.vb, self.groups, v0, vk, m, T)[:, :, Dz:]
        return label_scan(y0, ys, **kw)

    def txt2img(self, x, y, T, zcm=True, beta=0.0, **kw):
        Dz, V = self.Dz, self.Dz + self.K
        y = np.asarray(y, np.float64)
        B = y.shape[0]
        vk = np.zeros((B, V)); vk[:, Dz:] = y
        m = np.zeros((B, V)); m[:, Dz:] = 1
        if zcm:
            z0 = self.zcm[y.argmax(1)]
        else:
            z0 = v_probs(self.W, self.vb, h_probs(self.W, self.hb, vk), self.groups)[:, :Dz]
        v0 = vk.copy(); v0[:, :Dz] = z0
        zs = mean_field_chain(self.W, self.hb, self.vb, self.groups, v0, vk, m, T)[:, :, :Dz]
        zn, dz = code_scan(zs, z0, beta)
        mse = np.stack([decode_sqerr(self.decode_layers(), zn[t], np.asarray(x, np.float64)) for t in range(T)], 1)
        steps, best, margin = patience_scan(dz, mse, **kw)
        return {"z_l2": dz, "image_mse": mse, "steps": steps, "best_mse": best, "margin": margin, "z_new": zn}


# ---- fp32 twins: the kernels of csrc/kernels_trace.hpp restated in numpy, in their order of operations --------------------------
F32 = np.float32


def _butterfly(x):
    """wave_sum_all: 64 lane values [..., 64] meet in the xor butterfly 32, 16, .. 1 (fp32 addition commutes, so every lane ends with
    the value of the halving tree)."""
    x = np.asarray(x, F32)
    w = 32
    while w >= 1:
        x = (x[..., :w] + x[..., w:2 * w]).astype(F32)
        w //= 2
    return x[..., 0]


def code_scan_f32(zs, z0, beta=0.0):
    """trace_code_scan in fp32: lane l takes columns l, l + 64, ... in ascending order, the lanes meet in the butterfly, one sqrt."""
    zs, prev = np.asarray(zs, F32), np.asarray(z0, F32)
    T, B, Dz = zs.shape
    b, one = F32(beta), F32(1)
    zn, dz = np.zeros_like(zs), np.zeros((B, T), F32)
    for t in range(T):
        z = ((one - b) * prev + b * zs[t]).astype(F32) if b > 0 else zs[t]
        d = (z - prev).astype(F32)
        sq = np.zeros((B, (Dz + 63) // 64 * 64), F32)
        sq[:, :Dz] = d * d
        acc = np.zeros((B, 64), F32)
        for k in range(sq.shape[1] // 64):
            acc = (acc + sq[:, 64 * k:64 * k + 64]).astype(F32)
        dz[:, t] = np.sqrt(_butterfly(acc)).astype(F32)
        zn[t] = z
        prev = z
    return zn, dz


def row_sqerr_f32(x, ref):
    """row_sqerr in fp32: thread tid sums its columns tid, tid + 256, ... in ascending order, an 8-level halving tree, one division."""
    x, ref = np.asarray(x, F32), np.asarray(ref, F32)
    B, N = x.shape
    d = (x - ref).astype(F32)
    sq = np.zeros((B, (N + 255) // 256 * 256), F32)
    sq[:, :N] = d * d
    red = np.zeros((B, 256), F32)
    for k in range(sq.shape[1] // 256):
        red = (red + sq[:, 256 * k:256 * k + 256]).astype(F32)
    w = 128
    while w >= 1:
        red = (red[:, :w] + red[:, w:2 * w]).astype(F32)
        w //= 2
    return (red[:, 0] / F32(N)).astype(F32)


def decode_probs(layers, z):
    """float64 decode(z) of decode_sqerr: the visible probabilities of the bottom layer."""
    cur = np.asarray(z, np.float64)
    for W, vb in reversed(layers):
        cur = sigmoid(cur @ W.T + vb)
    return cur


class StackOracle(SmallOracle):
    """SmallOracle for any image stack and joint RBM: w as small_model_arrays' dict, the code Dz and K labels wide."""

    def __init__(self, w, Dz, K):
        n = len([k for k in w if k.startswith("img") and k.endswith("_W")])
        self.img = [tuple(w[f"img{i}_{k}"].astype(np.float64) for k in ("W", "hid_bias", "vis_bias")) for i in range(n)]
        self.W, self.hb, self.vb = (w[k].astype(np.float64) for k in ("joint_W", "joint_hid_bias", "joint_vis_bias"))
        self.zcm = w["z_class_mean"].astype(np.float64)
        self.Dz, self.K, self.groups = Dz, K, [(Dz, Dz + K)]
