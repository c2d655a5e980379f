"""Host-side description of where the engine's random draws come from.

The reference draws with ``torch.rand_like`` / ``torch.randn_like`` / ``Categorical.sample``
(rbm.py:125,131,203,208,271,333,346,352,392,395,462).  The engine never calls torch's generators;
it consumes draws in the *same order*  from one of:

``PhiloxRng``   device-side Philox-4x32-10 keyed on (seed, draw number, global row, column).
``ReplayRng``   caller-provided draws (a provider with ``uniform(shape)``, ``normal(shape)``,
                ``categorical(probs)`` returning numpy arrays) uploaded as a tape -- used by the
                parity tests to feed the draws recorded from the reference.

A *schedule* is the ordered list of draw tensors one engine call consumes:
``("u", N)`` uniform [B,N], ``("n", N)`` normal [B,N], ``("c", width)`` one categorical index per row.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

Schedule = List[Tuple[str, int]]


class PhiloxRng:
    def __init__(self, seed: int | None = None, row0: int = 0):
        self.seed = int(torch.initial_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        self.offset = 0          # number of draw tensors consumed so far
        self.row0 = int(row0)    # global index of local row 0 (data-parallel shard offset)
        # graph capture (imdbn.engine.graph.CapturedSteps): a 1-element int64 device tensor the kernels add to `offset`
        # when they RUN; set only while a capture is being recorded
        self.device_counter = None

    def advance(self, n_draws: int):
        self.offset += int(n_draws)


class ReplayRng:
    def __init__(self, provider):
        self.provider = provider

    def build(self, schedule: Schedule, B: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
        floats, cats = [], []
        for kind, n in schedule:
            if kind == "u":
                floats.append(np.ascontiguousarray(self.provider.uniform((B, n)), dtype=np.float32).ravel())
            elif kind == "n":
                floats.append(np.ascontiguousarray(self.provider.normal((B, n)), dtype=np.float32).ravel())
            elif kind == "c":
                idx = np.asarray(self.provider.categorical(np.zeros((B, n), np.float32)), dtype=np.int32)
                if idx.shape != (B,):
                    raise ValueError("categorical replay must yield one index per row")
                cats.append(idx)
            else:
                raise ValueError(kind)
        ft = torch.from_numpy(np.concatenate(floats) if floats else np.zeros(1, np.float32)).to(device)
        ct = torch.from_numpy(np.concatenate(cats) if cats else np.zeros(1, np.int32)).to(device)
        return ft, ct

    def advance(self, n_draws: int):
        pass


# ---- schedules: must mirror the consumption order in csrc/engine.hip ---------------------------
def sched_sample_visible(V: int, groups: Sequence[Tuple[int, int]]) -> Schedule:
    return [("u", V)] + [("c", e - s) for s, e in groups]


def sched_cd(V: int, H: int, groups, cd_k: int) -> Schedule:
    s: Schedule = [("u", H)]
    for _ in range(int(cd_k)):
        s += sched_sample_visible(V, groups) + [("u", H)]
    return s


def sched_pcd(V: int, H: int, groups, cd_k: int) -> Schedule:
    """imdbn_rbm_pcd_step: cd_k Gibbs steps on the particles, nothing else draws: cd_k (2 + G) draws for G groups."""
    return int(cd_k) * ([("u", H)] + sched_sample_visible(V, groups))


def sched_gauss_cd(V: int, H: int, cd_k: int, sample_v: bool) -> Schedule:
    """imdbn_rbm_gauss_cd_step: the positive-phase h, then per step the normals of v (with sample_v) and, on every step but the
    last, the next h: cd_k (1 + sample_v) draws."""
    s: Schedule = [("u", H)]
    for it in range(int(cd_k)):
        s += ([("n", V)] if sample_v else []) + ([("u", H)] if it < int(cd_k) - 1 else [])
    return s


def sched_pt(V: int, H: int, groups, n_replicas: int, n_sweeps: int) -> Schedule:
    """imdbn_rbm_pt_sweep, every tensor over all R M rows: per sweep one Gibbs step and, with R >= 2, the ("u", 1) of the exchange."""
    return int(n_sweeps) * ([("u", H)] + sched_sample_visible(V, groups) + ([("u", 1)] if int(n_replicas) >= 2 else []))


def sched_chain(V: int, H: int, groups, steps, init_uniform: bool) -> Schedule:
    s: Schedule = [("u", V)] if init_uniform else []
    for st in steps:
        if st["sigma"] > 0:
            s.append(("n", H))
        if st["sample_h"]:
            s.append(("u", H))
        if st["sigma"] > 0:
            s.append(("n", V))
        if st["vmode"] != 0:
            s += sched_sample_visible(V, groups)
    return s


def sched_clamped(V: int, H: int, groups, init_steps, cd_k: int, sample_h: bool, sample_v: bool) -> Schedule:
    s = sched_chain(V, H, groups, init_steps, True)
    for _ in range(int(cd_k)):
        if sample_h:
            s.append(("u", H))
        if sample_v:
            s += sched_sample_visible(V, groups)
    return s


def sched_ais(V: int, H: int, K: int) -> Schedule:
    """imdbn_rbm_ais over K temperatures: the initial state, then one (h, v) transition per temperature but the last."""
    return [("u", V)] + (int(K) - 1) * [("u", H), ("u", V)]


def sched_ais_groups(V: int, H: int, groups: Sequence[Tuple[int, int]], K: int) -> Schedule:
    """imdbn_rbm_ais_groups over K temperatures: the initial state (Bernoulli columns, then one categorical per softmax group), then
    one (h, v) transition per temperature but the last: (K - 1) (2 + G) + 1 + G draws for G groups."""
    sv = sched_sample_visible(V, groups)
    return sv + (int(K) - 1) * ([("u", H)] + sv)


def sched_gauss_ais(V: int, H: int, K: int) -> Schedule:
    """imdbn_rbm_gauss_ais over K temperatures: the normals of the initial state, then one (h, v) transition per temperature but the
    last, h uniform and v normal: 2 K - 1 draws."""
    return [("n", V)] + (int(K) - 1) * [("u", H), ("n", V)]


def sched_reverse_ais(V: int, H: int, groups: Sequence[Tuple[int, int]], K: int) -> Schedule:
    """imdbn_rbm_reverse_ais over K temperatures: one (h, v) transition per temperature, T_K first: K (2 + G) draws for G groups."""
    return int(K) * ([("u", H)] + sched_sample_visible(V, groups))


def sched_gauss_reverse_ais(V: int, H: int, K: int) -> Schedule:
    """imdbn_rbm_gauss_reverse_ais over K temperatures: one (h, v) transition per temperature, T_K first, h uniform and v normal:
    2 K draws."""
    return int(K) * [("u", H), ("n", V)]


def sched_bound(H: int) -> Schedule:
    """imdbn_rbm_bound_step: the one draw of h ~ q(h | v)."""
    return [("u", int(H))]


def sched_dbm_gibbs(sizes: Sequence[int], n_sweeps: int, clamp_bottom: bool = False) -> Schedule:
    """HipEngine.dbm_gibbs on layers of ``sizes`` units (bottom first): per sweep the odd layers bottom to top, one ("u", N_l) each,
    then the even layers bottom to top; layer 0 draws as ``sample_visible`` of a Bernoulli layer, or nothing when it is clamped."""
    L = len(sizes) - 1
    sweep: Schedule = [("u", int(sizes[l])) for l in range(1, L + 1, 2)]
    for l in range(0, L + 1, 2):
        if l == 0:
            sweep += [] if clamp_bottom else sched_sample_visible(int(sizes[0]), [])
        else:
            sweep.append(("u", int(sizes[l])))
    return int(n_sweeps) * sweep


def sched_mdbm_gibbs(sizes: Sequence[int], n_labels: int, n_sweeps: int, clamp_bottom: bool = False, clamp_labels: bool = False) -> Schedule:
    """HipEngine.mdbm_gibbs: ``sizes`` are the image layers ``0 .. L`` bottom first and then the joint hidden layer (index L + 1);
    the label layer is one categorical of ``n_labels``.  Per sweep the class of the joint layer (parity L + 1) bottom to top, then
    the other class bottom to top with the label's ("c", n_labels) right after layer L; a sigmoid layer draws one ("u", N_l), layer 0
    as ``sample_visible`` of a Bernoulli layer; a clamped layer draws nothing."""
    L = len(sizes) - 2
    sweep: Schedule = []
    for parity in ((L + 1) & 1, L & 1):
        for l in range(parity, L + 2, 2):
            if l == 0:
                sweep += [] if clamp_bottom else sched_sample_visible(int(sizes[0]), [])
            else:
                sweep.append(("u", int(sizes[l])))
            if l == L and not clamp_labels:
                sweep.append(("c", int(n_labels)))
    return int(n_sweeps) * sweep


def sched_dbm_ais(sizes: Sequence[int], K: int) -> Schedule:
    """imdbn_dbm_ais over K temperatures on layers of ``sizes`` units (bottom first): the start state, one ("u", N_l) per odd layer
    bottom to top, then one transition per temperature but the last: the even layers bottom to top, then the odd layers bottom to
    top."""
    L = len(sizes) - 1
    odd: Schedule = [("u", int(sizes[l])) for l in range(1, L + 1, 2)]
    even: Schedule = [("u", int(sizes[l])) for l in range(0, L + 1, 2)]
    return odd + (int(K) - 1) * (even + odd)
