"""numpy (fp64) restatement of the numeric core of the iMDBN_BiModal side-car (reference imdbn/models/imdbn_bimodal.py :43-419,
:856-1015; imdbn/utils/wandb_utils.py): the conditional chain of the joint RBM with its hidden AND visible probabilities recorded
per step (the general imdbn_chain_step: T, sigma, sampled hidden / visible units, softmax groups, clamp -- from given draws), the
MOD2->MOD1 trajectory built from it, PCA with sklearn's sign rule, and Spearman's rho with average ranks."""
from __future__ import annotations

import numpy as np

from logging_oracle import pca  # noqa: F401  (sklearn's svd_flip(u_based_decision=False) sign rule)
from trace_oracle import sigmoid

F64 = np.float64


def _softmax_groups(p, x, groups):
    for s, e in groups:
        g = np.exp(x[:, s:e] - x[:, s:e].max(1, keepdims=True))
        p[:, s:e] = g / g.sum(1, keepdims=True)
    return p


def step_draws(src, step, B, V, H, groups):
    """The draws of one chain step in the engine's order (imdbn.engine.rng.sched_chain): noise_h, uni_h, noise_v, uni_v, one
    categorical index per row and group."""
    d = {}
    if step["sigma"] > 0:
        d["nh"] = np.asarray(src.normal((B, H)), F64)
    if step["sample_h"]:
        d["uh"] = np.asarray(src.uniform((B, H)), F64)
    if step["sigma"] > 0:
        d["nv"] = np.asarray(src.normal((B, V)), F64)
    if step["vmode"] != 0:
        d["uv"] = np.asarray(src.uniform((B, V)), F64)
        d["cat"] = [np.asarray(src.categorical(np.zeros((B, e - s), np.float32)), np.int64) for s, e in groups]
    return d


def hidden_prob(W, hb, v, step, d):
    x = (np.asarray(v, F64) @ W + hb) / max(1e-6, step["T"])
    if step["sigma"] > 0:
        x = x + d["nh"] * step["sigma"]
    return sigmoid(x)


def visible_prob(W, vb, h, step, d, groups, mu=None):
    x = (np.asarray(h, F64) @ W.T + vb) / max(1e-6, step["T"])
    if step["sigma"] > 0:
        x = x + d["nv"] * step["sigma"]
    p = _softmax_groups(sigmoid(x), x, groups)
    if mu is not None and step["eta"] != 0.0:
        Dz = mu.shape[1]
        p[:, :Dz] = (1 - step["eta"]) * p[:, :Dz] + step["eta"] * mu
    return p


def next_state(p, vk, km, step, d, groups):
    """The visible state a step leaves, from its visible probability p (imdbn_chain_step: vmode 0 mean-field, 1 sample(p) then
    re-clamp, 2 sample(mix(p)) without re-clamping; group columns: the one-hot of the drawn index)."""
    mix = (lambda x: x * (1 - km) + vk * km) if step["clamp"] else (lambda x: x)
    if step["vmode"] == 0:
        return mix(p)
    src = p if step["vmode"] == 1 else mix(p)
    s = (src > d["uv"]).astype(p.dtype)
    for (a, b), idx in zip(groups, d["cat"]):
        s[:, a:b] = np.eye(b - a, dtype=p.dtype)[idx]
    return mix(s) if step["vmode"] == 1 else s


def chain_vh(W, hb, vb, groups, vk, km, steps, src, init_uniform=True, mu=None, baseline=False):
    """Free-running fp64 chain.  Returns (final v [B, V], vis [T (+1), B, V], hid [T, B, H], margin): vis slot t = p(v|h) of
    step t after the mu-pull (slot 0 the draw-free T = 1 baseline p(v | p(h | v0)) when `baseline`), hid slot t = p(h|v) of step t
    before sampling; margin = the smallest |p - u| over every Bernoulli decision taken."""
    W, hb, vb = np.asarray(W, F64), np.asarray(hb, F64), np.asarray(vb, F64)
    vk, km = np.asarray(vk, F64), np.asarray(km, F64)
    B, V = vk.shape
    H = W.shape[1]
    v = vk * km + (1 - km) * np.asarray(src.uniform((B, V)), F64) if init_uniform else vk.copy()
    vis, hid, margin = [], [], np.inf
    plain = {"T": 1.0, "sigma": 0.0, "eta": 0.0}
    if baseline:
        vis.append(visible_prob(W, vb, hidden_prob(W, hb, v, plain, {}), plain, {}, groups))
    for st in steps:
        d = step_draws(src, st, B, V, H, groups)
        ph = hidden_prob(W, hb, v, st, d)
        hid.append(ph)
        if st["sample_h"]:
            margin = min(margin, float(np.abs(ph - d["uh"]).min()))
            h = (ph > d["uh"]).astype(F64)
        else:
            h = ph
        pv = visible_prob(W, vb, h, st, d, groups, mu)
        vis.append(pv)
        if st["vmode"] != 0:
            free = np.ones(V, bool)
            for a, b in groups:
                free[a:b] = False
            src_p = pv if st["vmode"] == 1 else (pv * (1 - km) + vk * km if st["clamp"] else pv)
            margin = min(margin, float(np.abs(src_p - d["uv"])[:, free].min()))
        v = next_state(pv, vk, km, st, d, groups)
    return v, np.stack(vis) if vis else np.zeros((0, B, V)), np.stack(hid) if hid else np.zeros((0, B, H)), margin


def check_recorded_chain(W, hb, vb, groups, vk, km, steps, src, vis, hid, final, init_uniform=True, mu=None, baseline=False):
    """Step-by-step check of a RECORDED chain (full-width fp32 traces `vis` [T (+1), B, V], `hid` [T, B, H] and the final state):
    every step's fp64 probabilities are computed from the recorded state that ENTERED the step -- rebuilt from the recorded fp32
    probabilities and the same draws, so a Bernoulli decision that fp32 and fp64 would take differently (|p - u| at rounding level,
    not an error) cannot make the comparison diverge.  Returns (max |hid - fp64|, max |vis - fp64|, final state rebuilt equals
    `final`)."""
    W, hb, vb = np.asarray(W, F64), np.asarray(hb, F64), np.asarray(vb, F64)
    B, V = vk.shape
    H = W.shape[1]
    vk32, km32 = np.asarray(vk, np.float32), np.asarray(km, np.float32)
    if init_uniform:
        u = np.asarray(src.uniform((B, V)), np.float32)
        v = vk32 * km32 + (np.float32(1) - km32) * u
    else:
        v = vk32.copy()
    eh = ev = 0.0
    plain = {"T": 1.0, "sigma": 0.0, "eta": 0.0}
    b0 = 1 if baseline else 0
    if baseline:
        ev = max(ev, float(np.abs(visible_prob(W, vb, hidden_prob(W, hb, v, plain, {}), plain, {}, groups) - vis[0]).max()))
    for t, st in enumerate(steps):
        d = step_draws(src, st, B, V, H, groups)
        eh = max(eh, float(np.abs(hidden_prob(W, hb, v, st, d) - hid[t]).max()))
        h = (hid[t] > d["uh"].astype(np.float32)).astype(np.float32) if st["sample_h"] else hid[t]
        ev = max(ev, float(np.abs(visible_prob(W, vb, h, st, d, groups, mu) - vis[t + b0]).max()))
        d32 = {k: (x.astype(np.float32) if isinstance(x, np.ndarray) else x) for k, x in d.items()}
        v = next_state(np.asarray(vis[t + b0], np.float32), vk32, km32, st, d32, groups).astype(np.float32)
    return eh, ev, bool(np.array_equal(v, np.asarray(final, np.float32)))


class Stack:
    """A modality stack of sigmoid layers [(W, hb, vb)], fp64."""

    def __init__(self, layers):
        self.layers = [(np.asarray(W, F64), np.asarray(hb, F64), np.asarray(vb, F64)) for W, hb, vb in layers]

    def represent(self, x):
        x = np.asarray(x, F64)
        for W, hb, _ in self.layers:
            x = sigmoid(x @ W + hb)
        return x

    def decode(self, z):
        z = np.asarray(z, F64)
        for W, _, vb in reversed(self.layers):
            z = sigmoid(z @ W.T + vb)
        return z


def bimodal_trajectory(W, hb, vb, z2, Dz1, u):
    """The MOD2->MOD1 chain of reference :225-256 for rows z2 [N, Dz2] with uniforms u [steps, N, H]: (traj_h [steps+1, N, H],
    traj_z1 [steps+1, N, Dz1], margin)."""
    N = z2.shape[0]
    V = Dz1 + z2.shape[1]
    vk, km = np.zeros((N, V)), np.zeros((N, V))
    vk[:, Dz1:], km[:, Dz1:] = z2, 1.0

    class Src:
        def __init__(self):
            self.t = 0

        def uniform(self, shape):
            self.t += 1
            return u[self.t - 1]

    step = {"T": 1.0, "sigma": 0.0, "eta": 0.0, "sample_h": False, "vmode": 0, "clamp": True}
    _, vis, hid, margin = chain_vh(W, hb, vb, [], vk, km, [step] + [dict(step, sample_h=True)] * len(u), Src(), init_uniform=False)
    return hid, vis[:, :, :Dz1], margin


def avg_ranks(x):
    """1-based ranks, ties share the mean of their positions (scipy.stats.rankdata 'average')."""
    x = np.asarray(x, F64)
    order = np.argsort(x, kind="stable")
    xs = x[order]
    r = np.empty(len(x))
    i = 0
    while i < len(xs):
        j = i
        while j + 1 < len(xs) and xs[j + 1] == xs[i]:
            j += 1
        r[order[i:j + 1]] = (i + j) / 2.0 + 1.0
        i = j + 1
    return r


def spearman(a, b):
    a, b = np.asarray(a, F64).ravel(), np.asarray(b, F64).ravel()
    if len(a) != len(b) or len(a) < 2:
        return float("nan")
    ra, rb = avg_ranks(a), avg_ranks(b)
    ra, rb = ra - ra.mean(), rb - rb.mean()
    den = np.sqrt((ra * ra).sum() * (rb * rb).sum())
    return float((ra * rb).sum() / den) if den > 0 else float("nan")


def correlations(emb, features):
    emb = np.asarray(emb, F64)
    return {f"{k}_dim{i + 1}": (spearman(emb[:, i], v) if len(v) == emb.shape[0] else float("nan"))
            for k, v in features.items() for i in range(emb.shape[1])}
