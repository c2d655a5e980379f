"""HipEngine: torch tensors in, C-ABI calls out.  The only thing between ``RBM`` methods and the HIP kernels.

PyTorch is plumbing here (device memory, current stream); every arithmetic step of the hot path
runs in ``libimdbn_hip.so``.  Parameters are read from the RBM object at EVERY call (callers may
mutate or re-bind ``W``/biases behind the RBM's back); the engine holds only
scratch workspaces keyed on (device, V, H, B).

One public method per operation; what they share lives in the private helpers: ``_call``, ``_ws_tail``,
``_desc_key``, ``_reset_caches``, ``_clamped`` / ``_mu``, ``_chain_specs``, ``_cd``, ``_apply``, ``_buffer``, ``_f32`` / ``_i32``.
"""
from __future__ import annotations

import os
import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import native as N
from . import rng as R


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.size(1):
        return t
    if not t.is_contiguous():
        t = t.contiguous()
    return t


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _ref(x):
    return C.byref(x) if x is not None else None


def _f32(dev, *shape) -> torch.Tensor:
    return torch.empty(*shape, device=dev)


def _i32(dev, *shape) -> torch.Tensor:
    return torch.empty(*shape, dtype=torch.int32, device=dev)


def _on(t: Optional[torch.Tensor], dev, dtype) -> Optional[torch.Tensor]:
    """An optional side input as a contiguous `dtype` tensor on `dev`."""
    return None if t is None else t.to(device=dev, dtype=dtype).contiguous()


class HipEngine:
    name = "hip"

    def __init__(self):
        self._lib = N.lib()
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._pf: Dict[tuple, tuple] = {}           # workspace key -> (identity of the prefetched batch, slot, tensor)
        self._pf_ok: Dict[tuple, bool] = {}
        self.mode = N.PARITY_F32
        # tuning / A-B aid: IMDBN_OPTS="name=value,..." -> imdbn_set_option (include/imdbn_engine.h)
        for kv in filter(None, os.environ.get("IMDBN_OPTS", "").split(",")):
            k, _, v = kv.partition("=")
            self.set_option(k.strip(), int(v or 1))

    # ---- plumbing -----------------------------------------------------------------------------
    def _call(self, name: str, *args):
        """Call the status-returning entry `name` of the library; a non-zero status raises with the entry's name."""
        N.check(getattr(self._lib, name)(*args), name)

    def _reset_caches(self):
        """Knobs changed: workspace sizes, prefetch records and prefetch eligibility may all differ."""
        self._ws.clear(); self._pf.clear(); self._pf_ok.clear()

    def device_info(self):
        cu = C.c_int(0)
        buf = C.create_string_buffer(64)
        self._call("imdbn_device_info", C.byref(cu), buf, 64)
        return cu.value, buf.value.decode()

    def set_tuning(self, ksplit_up: int = 0, ksplit_down: int = 0):
        self._call("imdbn_set_tuning", int(ksplit_up), int(ksplit_down))
        self._reset_caches()

    def set_option(self, name: str, value: int):
        self._call("imdbn_set_option", name.encode(), int(value))
        self._reset_caches()

    # per-caller knobs (imdbn_options): a handle bound to the calling thread overrides the process defaults
    def options_create(self, **knobs):
        h = C.c_void_p(self._lib.imdbn_options_create())
        if not h:
            raise N.EngineError("imdbn_options_create failed")
        for k, v in knobs.items():
            self._call("imdbn_options_set", h, k.encode(), int(v))
        return h

    def use_options(self, handle):
        """Bind `handle` (None: the process defaults) to this thread; workspaces are re-derived (the layout may differ)."""
        self._call("imdbn_use_options", handle)
        self._reset_caches()

    def options_destroy(self, handle):
        self._lib.imdbn_options_destroy(handle)

    def rng_advance(self, counter: torch.Tensor, n: int):
        """counter[0] += n on the current stream (a node of the graph being captured)."""
        assert counter.dtype == torch.int64 and counter.numel() == 1 and counter.is_cuda
        self._call("imdbn_rng_advance", _ptr(counter), int(n), self._stream(counter.device))

    def profile(self, on: bool):
        self._call("imdbn_profile_enable", 1 if on else 0)

    def profile_read(self) -> Tuple[float, int]:
        ms, n = C.c_double(0), C.c_int(0)
        self._call("imdbn_profile_read", C.byref(ms), C.byref(n))
        return ms.value, n.value

    def debug_buffer(self, dev, V, H, B, name: str, nbytes: int) -> torch.Tensor:
        """Test aid: uint8 view of a named internal buffer of the (V, H, B) workspace (imdbn_debug_ws_offset)."""
        off = C.c_size_t(0)
        self._call("imdbn_debug_ws_offset", int(V), int(H), int(B), name.encode(), C.byref(off))
        ws = self._workspace(torch.device(dev), V, H, B)
        return ws[off.value:off.value + nbytes]

    def last_route(self) -> dict:
        """Test aid: the kernel family the last up and the last down propagation of this thread launched, as the launchers
        recorded it (imdbn_debug_last_route): ``{"up": name or None, "up_epilogue": "lean" | "general", "down": name or None,
        "down_epilogue": ..., "finish_groups": bool}``; the names are ``native.ROUTE_UP`` / ``native.ROUTE_DOWN``."""
        r = (C.c_int * 5)()
        self._call("imdbn_debug_last_route", r)
        return {"up": N.ROUTE_UP[r[0]] if r[0] >= 0 else None, "up_epilogue": "general" if r[1] else "lean",
                "down": N.ROUTE_DOWN[r[2]] if r[2] >= 0 else None, "down_epilogue": "general" if r[3] else "lean",
                "finish_groups": bool(r[4])}

    def last_chain(self) -> dict:
        """Test aid: how the last chain call of this thread ran (imdbn_debug_last_chain): ``{"route": "per_launch" | "kernel" |
        "kernel_pair" or None, "rows": batch rows per block, "blocks": blocks of the launch (both 0 per launch), "recs": records of
        chain 0, a traced baseline included}``; the names are ``native.CHAIN_ROUTE``."""
        r = (C.c_int * 4)()
        self._call("imdbn_debug_last_chain", r)
        return {"route": N.CHAIN_ROUTE[r[0]] if r[0] >= 0 else None, "rows": r[1], "blocks": r[2], "recs": r[3]}

    def last_cd(self) -> dict:
        """Test aid: how the last CD pass of this thread ran (imdbn_debug_last_cd): ``{"pos_up": up family of the positive-phase K1,
        "first_down": down family of the first K2, "last_up": up family of the last K1 (names as in ``last_route``, None before the
        first pass), "next": where the next batch was prepared (``native.CD_NEXT``), "slot": prefetch slot the data were read from
        (0: none), "adaptive": the preparation decided per 64-column item}``."""
        r = (C.c_int * 6)()
        self._call("imdbn_debug_last_cd", r)
        return {"pos_up": N.ROUTE_UP[r[0]] if r[0] >= 0 else None, "first_down": N.ROUTE_DOWN[r[1]] if r[1] >= 0 else None,
                "last_up": N.ROUTE_UP[r[2]] if r[2] >= 0 else None, "next": N.CD_NEXT[r[3]], "slot": r[4], "adaptive": bool(r[5])}

    def _workspace(self, dev, V, H, B):
        # one workspace per (device, shape, STREAM): two same-shape RBMs driven from two streams must not share scratch
        key = (dev, V, H, B, torch.cuda.current_stream(dev).cuda_stream if torch.device(dev).type == "cuda" else 0)
        ws = self._ws.get(key)
        if ws is None:
            need = int(self._lib.imdbn_ws_bytes(V, H, B))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            self._ws[key] = ws
        return ws

    def _ws_tail(self, dev, V, H, B):
        """``(workspace, bytes, stream)``: the last three arguments of every entry that takes a workspace."""
        ws = self._workspace(dev, V, H, B)
        return _ptr(ws), ws.numel(), self._stream(dev)

    def _buffer(self, key: tuple, make, at_least: int = 0) -> torch.Tensor:
        """Get-or-create a reusable buffer in the workspace dict (re-made when smaller than `at_least` elements)."""
        buf = self._ws.get(key)
        if buf is None or buf.numel() < at_least:
            buf = self._ws[key] = make()
        return buf

    @staticmethod
    def _stream(dev):
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def _desc_key(self, rbm, need_momentum: bool):
        """What a cached descriptor of `rbm` is valid for: the addresses / pitches of the parameter and momentum tensors as
        they are NOW, the softmax groups and the mode.  None: parameters missing, nothing is cached."""
        p, dct = rbm._parameters, rbm.__dict__
        Wp, hbp, vbp = p.get("W"), p.get("hid_bias"), p.get("vis_bias")
        if Wp is None or hbp is None or vbp is None:
            return None
        Wm, hbm, vbm = dct.get("W_m"), dct.get("hb_m"), dct.get("vb_m")
        g = dct.get("softmax_groups")
        return (Wp.data_ptr(), Wp.stride(0), Wp.shape, hbp.data_ptr(), vbp.data_ptr(),
                Wm.data_ptr() if isinstance(Wm, torch.Tensor) else 0, hbm.data_ptr() if isinstance(hbm, torch.Tensor) else 0,
                vbm.data_ptr() if isinstance(vbm, torch.Tensor) else 0, Wm.stride(0) if isinstance(Wm, torch.Tensor) and Wm.dim() == 2 else 0,
                tuple(map(tuple, g)) if g else (), self.mode, need_momentum)

    def _desc(self, rbm, need_momentum: bool) -> N.RbmDesc:
        """The native descriptor of `rbm`.  Built (and validated) once per state of the parameter tensors: callers may re-bind
        or move W / biases / momentum buffers at any time (SURVEY b-1), so the cached descriptor is keyed on their addresses."""
        need_momentum = bool(need_momentum)
        key = self._desc_key(rbm, need_momentum)
        if key is not None:
            cache = rbm.__dict__.get("_imdbn_desc")
            hit = cache.get(need_momentum) if cache is not None else None
            if hit is not None and hit[0] == key:
                return hit[1]
        d = self._build_desc(rbm, need_momentum)
        key = self._desc_key(rbm, need_momentum)        # re-homing may have replaced the momentum buffers: key on what is there now
        if key is not None:
            rbm.__dict__.setdefault("_imdbn_desc", {})[need_momentum] = (key, d)
        return d

    def _build_desc(self, rbm, need_momentum: bool) -> N.RbmDesc:
        W = rbm.W.data
        if not W.is_cuda:
            raise N.EngineError("HipEngine needs CUDA/HIP tensors (RBM.W is on %s)" % W.device)
        if W.dtype != torch.float32 or W.dim() != 2 or W.stride(1) != 1:
            raise N.EngineError("RBM.W must be fp32 [V,H] with unit inner stride")
        V, H = W.shape
        d = N.RbmDesc()
        d.W, d.ldw, d.V, d.H = W.data_ptr(), W.stride(0), V, H
        hb, vb = rbm.hid_bias.data, rbm.vis_bias.data
        for t, n, nm in ((hb, H, "hid_bias"), (vb, V, "vis_bias")):
            if t.device != W.device or t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
                raise N.EngineError(f"RBM.{nm} must be contiguous fp32 [{n}] on {W.device}")
        d.hid_bias, d.vis_bias = hb.data_ptr(), vb.data_ptr()
        if need_momentum:
            # momentum buffers are plain attributes, not moved by .to() (rbm.py:77-79): re-home them
            for nm, ref in (("W_m", W), ("hb_m", hb), ("vb_m", vb)):
                m = getattr(rbm, nm, None)
                if m is None or m.shape != ref.shape:
                    m = torch.zeros_like(ref)
                elif m.device != ref.device or m.dtype != torch.float32:
                    m = m.to(device=ref.device, dtype=torch.float32)
                if nm != "W_m" and not m.is_contiguous():
                    m = m.contiguous()
                setattr(rbm, nm, m)
            if rbm.W_m.stride(0) != W.stride(0) or rbm.W_m.stride(1) != 1:
                # the C ABI has one leading dimension for W and W_m: re-home W_m with W's pitch (values kept)
                m2 = torch.empty_strided(tuple(W.shape), tuple(W.stride()), dtype=torch.float32, device=W.device)
                m2.copy_(rbm.W_m)
                rbm.W_m = m2
            d.W_m, d.hb_m, d.vb_m = rbm.W_m.data_ptr(), rbm.hb_m.data_ptr(), rbm.vb_m.data_ptr()
        groups = list(getattr(rbm, "softmax_groups", None) or [])
        if len(groups) > N.MAX_GROUPS:
            raise N.EngineError(f"at most {N.MAX_GROUPS} softmax groups supported")
        d.n_groups = len(groups)
        for i, (s, e) in enumerate(groups):
            d.group_start[i], d.group_end[i] = int(s), int(e)
        d.mode = self.mode
        return d

    @staticmethod
    def _groups(rbm):
        return [(int(s), int(e)) for s, e in (getattr(rbm, "softmax_groups", None) or [])]

    def _rng(self, rng, schedule: R.Schedule, B: int, dev):
        """native rng struct + keep-alive tensors"""
        r = N.Rng()
        keep = None
        if isinstance(rng, R.ReplayRng):
            ft, ct = rng.build(schedule, B, dev)
            r.mode = N.RNG_REPLAY
            r.tape, r.tape_len = ft.data_ptr(), ft.numel()
            r.cat_tape, r.cat_len = ct.data_ptr(), ct.numel()
            keep = (ft, ct)
        elif isinstance(rng, R.PhiloxRng):
            r.mode = N.RNG_PHILOX
            r.seed, r.offset, r.row0 = rng.seed, rng.offset, rng.row0
            if rng.device_counter is not None:          # a capture is being recorded: draw number = offset + *counter at run time
                r.dev_offset = rng.device_counter.data_ptr()
        else:
            raise N.EngineError("rng must be PhiloxRng or ReplayRng")
        return r, keep

    @staticmethod
    def _done(rng, r: N.Rng, schedule):
        if r.draws_used != len(schedule):
            raise N.EngineError(f"draw schedule mismatch: engine consumed {r.draws_used}, host planned {len(schedule)}")
        rng.advance(r.draws_used)

    def skip_draws(self, rng, schedule: R.Schedule, B: int):
        """Consume draws without computing (dead refinement passes of _cross_reconstruct)."""
        if isinstance(rng, R.ReplayRng):
            rng.build(schedule, B, "cpu")
        else:
            rng.advance(len(schedule))

    @staticmethod
    def _steps(steps: Sequence[dict]):
        arr = (N.ChainStep * max(1, len(steps)))()
        for i, s in enumerate(steps):
            arr[i].T, arr[i].sigma, arr[i].eta = float(s["T"]), float(s["sigma"]), float(s["eta"])
            arr[i].sample_h, arr[i].vmode, arr[i].clamp = int(s["sample_h"]), int(s["vmode"]), int(s["clamp"])
        return arr

    @staticmethod
    def _clamped(v_known, mask):
        """The clamped operands as fp32 with ONE row stride (the C ABI has one leading dimension for both)."""
        vk, km = _f32c(v_known), _f32c(mask)
        if vk.stride(0) != km.stride(0):
            vk, km = vk.contiguous(), km.contiguous()
        return vk, km

    @staticmethod
    def _mu(mu):
        """The optional prior mean: ``(fp32 tensor to keep alive or None, (address, ld, Dz))``; all zero without one."""
        if mu is None:
            return None, (0, 0, 0)
        t = _f32c(mu)
        return t, (t.data_ptr(), t.stride(0), t.size(1))

    # ---- propagations -------------------------------------------------------------------------
    def prop_up(self, rbm, v, T=1.0, sample=False, rng=None):
        d = self._desc(rbm, False)
        v = _f32c(v)
        B, dev = v.size(0), v.device
        out = torch.empty(B, d.H, device=dev)
        smp = torch.empty(B, d.H, device=dev) if sample else None
        sched = [("u", d.H)] if sample else []
        r, keep = self._rng(rng, sched, B, dev) if sample else (None, None)
        self._call("imdbn_rbm_prop_up", C.byref(d), _ptr(v), v.stride(0), B, float(T), _ref(r), _ptr(out), out.stride(0), _ptr(smp), d.H,
                   *self._ws_tail(dev, d.V, d.H, B))
        if sample:
            self._done(rng, r, sched)
            return out, smp
        return out

    def forward(self, rbm, v, data_binary=None):
        """forward(v) at T = 1 (imdbn_rbm_forward): the streaming K1 reads 0/1 pieces of the batch as a bit plane."""
        d = self._desc(rbm, False)
        x = _f32c(v)
        B, dev = x.size(0), x.device
        out = torch.empty(B, d.H, device=dev)
        binary = self._hint(v, data_binary)         # the caller's tensor: the fp32 form `x` may be a copy without the tag
        self._call("imdbn_rbm_forward", C.byref(d), _ptr(x), x.stride(0), B, binary, _ptr(out), out.stride(0),
                   *self._ws_tail(dev, d.V, d.H, B))
        return out

    def free_energy(self, rbm, v):
        d = self._desc(rbm, False)
        v = _f32c(v)
        B, dev = v.size(0), v.device
        out = torch.empty(B, device=dev)
        self._call("imdbn_rbm_free_energy", C.byref(d), _ptr(v), v.stride(0), B, _ptr(out), *self._ws_tail(dev, d.V, d.H, B))
        return out

    def _anneal(self, name: str, rbm, d, sched_fn, n_rows: int, betas, rng, base_vis_bias, return_state: bool, v=None, logvar=None):
        """The shared body of ``ais``, ``ais_groups``, ``reverse_ais``, ``gauss_ais`` and ``gauss_reverse_ais``: the entry
        ``imdbn_rbm_<name>`` over ``n_rows`` chains under the draw schedule ``sched_fn(K)``; ``v``: the start states of the calls that
        take them; ``logvar``: the checked log-variances of the Gaussian calls -- the forward one's entry takes ``logvar, betas, K, M``
        where the others take ``M, K, betas``."""
        dev = rbm.W.device if v is None else v.device
        b = [float(x) for x in (betas.tolist() if hasattr(betas, "tolist") else betas)]
        K, M = len(b) - 1, int(n_rows)
        arr = (C.c_float * max(1, len(b)))(*b)
        bA = _on(base_vis_bias, dev, torch.float32)
        if bA is not None and bA.numel() != d.V:
            raise N.EngineError(f"{name}: base_vis_bias must have {d.V} elements")
        logw = torch.empty(max(M, 1), dtype=torch.float64, device=dev)
        state = torch.empty(max(M, 1), d.V, device=dev) if return_state else None
        sched = sched_fn(max(K, 1))
        r, keep = self._rng(rng, sched, max(M, 1), dev)
        start = () if v is None else (_ptr(v), v.stride(0))
        if logvar is None:
            head = (*start, M, K, arr)
        else:
            head = (_ptr(logvar), arr, K, M) if v is None else (_ptr(logvar), *start, M, K, arr)
        self._call("imdbn_rbm_" + name, C.byref(d), *head, _ptr(bA), C.byref(r), _ptr(logw), _ptr(state), d.V,
                   *self._ws_tail(dev, d.V, d.H, max(M, 1)))
        self._done(rng, r, sched)
        return (logw, state) if return_state else logw

    def ais(self, rbm, betas, n_chains: int, rng, base_vis_bias: Optional[torch.Tensor] = None, return_state: bool = False):
        """Annealed importance sampling (imdbn_rbm_ais): ``n_chains`` chains from the base-rate model (visible biases
        ``base_vis_bias``, None = zeros) to ``rbm`` through the temperatures ``betas`` (0 = betas[0] < ... < betas[K] = 1).
        Returns the log importance weights, a float64 device tensor ``[n_chains]`` (and the final states ``[n_chains, V]`` with
        ``return_state``); log Z ~= H log 2 + sum softplus(base_vis_bias) + logmeanexp(logw).  No host sync."""
        d = self._desc(rbm, False)
        return self._anneal("ais", rbm, d, lambda K: R.sched_ais(d.V, d.H, K), n_chains, betas, rng, base_vis_bias, return_state)

    def ais_groups(self, rbm, betas, n_chains: int, rng, base_vis_bias: Optional[torch.Tensor] = None, return_state: bool = False):
        """``ais`` for an RBM whose visible layer has softmax groups (imdbn_rbm_ais_groups): inside a group the columns of
        ``base_vis_bias`` are the logits of a categorical, every state holds exactly one 1 per group, and
        log Z ~= H log 2 + sum_{i outside groups} softplus(b_A,i) + sum_g logsumexp(b_A[g]) + logmeanexp(logw).  Same returns as
        ``ais``; without groups it is ``ais`` bit for bit.  No host sync."""
        d = self._desc(rbm, False)
        return self._anneal("ais_groups", rbm, d, lambda K: R.sched_ais_groups(d.V, d.H, self._groups(rbm), K), n_chains, betas, rng,
                            base_vis_bias, return_state)

    def reverse_ais(self, rbm, v_rows, betas, rng, base_vis_bias: Optional[torch.Tensor] = None, return_state: bool = False):
        """Reverse annealed importance sampling (imdbn_rbm_reverse_ais): one chain per row of ``v_rows`` ``[R, V]`` (0/1; the caller
        replicates a test row once per chain) runs the AIS transitions of ``ais_groups`` backwards through ``betas``, T_K first.
        Returns the per-chain log weights, a float64 device tensor ``[R]`` (and the final states u_1 ``[R, V]`` with
        ``return_state``): ``-log Z_A + logmeanexp`` over a test row's chains is a stochastic lower bound on log p_ann(row), log Z_A
        as ``ais_groups`` states it.  A row that is not 0/1, or whose softmax group does not hold exactly one 1, gets NaN.  RBMs
        with softmax groups are accepted.  No host sync."""
        d = self._desc(rbm, False)
        if not v_rows.is_cuda or v_rows.dim() != 2 or v_rows.size(1) != d.V:
            raise N.EngineError(f"reverse_ais needs a HIP tensor v_rows [R, {d.V}]")
        v = _f32c(v_rows)
        return self._anneal("reverse_ais", rbm, d, lambda K: R.sched_reverse_ais(d.V, d.H, self._groups(rbm), K), v.size(0), betas, rng,
                            base_vis_bias, return_state, v=v)

    def rows_logmeanexp(self, logw: torch.Tensor, n_chains: int):
        """``(lme, ess)`` per test row of the chain weights ``logw`` (float64, ``N * n_chains`` elements, row n owns the chains
        ``n * n_chains ...``; imdbn_rows_logmeanexp): float64 device tensors ``[N]``, ``lme = log mean exp`` and
        ``ess = (sum w)^2 / sum w^2``.  A NaN stays in its row.  No host sync."""
        M = int(n_chains)
        if not logw.is_cuda or logw.dtype != torch.float64 or M < 1 or logw.numel() % M != 0:
            raise N.EngineError(f"rows_logmeanexp needs a float64 HIP tensor of N * {M} elements")
        x = logw.contiguous()
        n, dev = x.numel() // M, x.device
        lme = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        ess = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        self._call("imdbn_rows_logmeanexp", _ptr(x), n, M, _ptr(lme), _ptr(ess), self._stream(dev))
        return lme, ess

    def label_loglik(self, rbm, z: torch.Tensor, K: int, gt: torch.Tensor):
        """Both label-side values of the joint RBM ``rbm`` per row of the code ``z`` ``[N, Dz]`` (imdbn_rbm_label_loglik; the labels
        sit in the visible columns ``[Dz, Dz + K)``): ``(joint, marg)``, float64 device tensors ``[N]`` with
        ``joint = -F([z, e_gt])`` (NaN where ``gt`` is outside ``[0, K)``) and ``marg = log sum_y exp(-F([z, y]))``.  One up
        propagation and one kernel, no host sync."""
        d = self._desc(rbm, False)
        if not z.is_cuda or z.dim() != 2:
            raise N.EngineError("label_loglik needs a HIP tensor z [N, Dz]")
        z = _f32c(z)
        n, Dz = z.shape
        dev = z.device
        g = _on(gt, dev, torch.int32)
        if g is None or g.numel() != n:
            raise N.EngineError("label_loglik: gt must hold one label per row of z")
        joint = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        marg = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        self._call("imdbn_rbm_label_loglik", C.byref(d), _ptr(z), z.stride(0), n, Dz, int(K), _ptr(g), _ptr(joint), _ptr(marg),
                   *self._ws_tail(dev, Dz, d.H, max(n, 1)))       # the propagation is (Dz, H, N): its workspace, not (V, H, N)
        return joint, marg

    def label_step(self, rbm, z: torch.Tensor, K: int, gt: torch.Tensor, lr: float, mom: float) -> torch.Tensor:
        """One ascent step on ``mean log p(gt | z)`` of the joint RBM ``rbm`` over ``[z (Dz) | labels (K)]`` (imdbn_rbm_label_step):
        every parameter and momentum buffer is updated in place with learning rate ``lr``, momentum ``mom`` and the RBM's weight
        decay.  Returns ``log p(gt | z)`` under the parameters on entry, a float64 device tensor ``[N]`` (NaN where ``gt`` is
        outside ``[0, K)``; such a row enters no gradient).  One up propagation, two kernels and the update path, no draws, no
        host sync."""
        d = self._desc(rbm, True)
        if not z.is_cuda or z.dim() != 2:
            raise N.EngineError("label_step needs a HIP tensor z [N, Dz]")
        z = _f32c(z)
        n, Dz = z.shape
        dev = z.device
        g = _on(gt, dev, torch.int32)
        if g is None or g.numel() != n:
            raise N.EngineError("label_step: gt must hold one label per row of z")
        K = int(K)
        o = self._opts(rbm, lr, mom, 1)
        logp = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        need = max(n, 1) * (max(K, 0) + 2 * d.H)
        scratch = self._buffer(("label_step", dev, torch.cuda.current_stream(dev).cuda_stream), lambda: _f32(dev, need), need)
        self._call("imdbn_rbm_label_step", C.byref(d), _ptr(z), z.stride(0), n, Dz, K, _ptr(g), C.byref(o), _ptr(logp), _ptr(scratch),
                   *self._ws_tail(dev, Dz, d.H, max(n, 1)))       # the propagation and the update are (Dz, H, N), as label_loglik
        return logp

    def pseudo_loglik(self, rbm, v: torch.Tensor, return_sites: bool = False):
        """Exact pseudo-log-likelihood per row of ``v`` ``[N, V]`` (0/1, one-hot softmax groups; imdbn_rbm_pseudo_loglik):
        ``PLL = sum_sites log p(v_site | v_rest)``, a float64 device tensor ``[N]``; with ``return_sites`` also the per-column terms,
        fp32 ``[N, V]`` (a group's term at its observed column, 0 in the group's other columns).  A row that is not 0/1, or a group
        without exactly one 1, is NaN in both.  One up propagation and three kernels, no draws, no host sync."""
        d = self._desc(rbm, False)
        if not v.is_cuda or v.dim() != 2 or v.size(1) != d.V:
            raise N.EngineError(f"pseudo_loglik needs a HIP tensor v [N, {d.V}]")
        v = _f32c(v)
        n, dev = v.size(0), v.device
        pll = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        site = torch.empty(max(n, 1), d.V, device=dev) if return_sites else None
        self._call("imdbn_rbm_pseudo_loglik", C.byref(d), _ptr(v), v.stride(0), n, _ptr(pll), _ptr(site), d.V,
                   *self._ws_tail(dev, d.V, d.H, max(n, 1)))
        return (pll, site) if return_sites else pll

    def exact_log_z(self, rbm, logvar=None, side="auto", marginals=False, max_bits=24):
        """Exact log Z by enumerating one side of ``rbm`` on the device (imdbn_rbm_exact_logz).  ``side``:
        ``"hidden"``, ``"visible"`` or ``"auto"`` -- the smaller side (ties: hidden); hidden whenever the visible layer has softmax
        groups or is Gaussian (``logvar`` ``[V]`` given), because such a layer cannot be enumerated.  Returns ``{"log_z": 0-d float64
        device tensor, "log_w_max": the log of the largest state weight (0-d float64), "side": "hidden" | "visible", "bits": n,
        "vis_mean", "hid_mean"}``; the means are the exact model marginals, fp32 ``[V]`` / ``[H]`` (E[v_i] for Gaussian visibles), with
        ``marginals``, else None.  ``max_bits`` guards the cost (2^n states times the other side's width): a wider enumerated side
        raises; the library itself stops at 30.  No draws, no host sync."""
        d = self._desc(rbm, False)
        dev = rbm.W.device
        z = None if logvar is None else self._logvar("exact_log_z: logvar", logvar, d.V, dev)
        if side not in ("auto", "hidden", "visible"):
            raise N.EngineError(f"exact_log_z: side must be 'auto', 'hidden' or 'visible', got {side!r}")
        if side == "auto":
            side = "hidden" if (z is not None or d.n_groups > 0 or d.H <= d.V) else "visible"
        n = d.H if side == "hidden" else d.V
        if n > int(max_bits):
            raise N.EngineError(f"exact_log_z: n = {n} units on the enumerated ({side}) side is above max_bits = {int(max_bits)}: "
                                f"2^{n} states; pass max_bits={n} to allow it (the library's limit is 30)")
        code = 1 if side == "hidden" else 2
        need = int(self._lib.imdbn_exact_scratch_bytes(d.V, d.H, code))
        scratch = self._buffer(("exact", dev, d.V, d.H, code, torch.cuda.current_stream(dev).cuda_stream),
                               lambda: torch.empty(max(need, 256), dtype=torch.uint8, device=dev), need)
        out = torch.empty(2, dtype=torch.float64, device=dev)
        vm = torch.empty(d.V, device=dev) if marginals else None
        hm = torch.empty(d.H, device=dev) if marginals else None
        self._call("imdbn_rbm_exact_logz", C.byref(d), _ptr(z), code, _ptr(out), _ptr(vm), _ptr(hm), _ptr(scratch), scratch.numel(),
                   self._stream(dev))
        return {"log_z": out[0], "log_w_max": out[1], "side": side, "bits": n, "vis_mean": vm, "hid_mean": hm}

    def bound_step(self, rbm, v, rng, acc: Optional[torch.Tensor] = None, mode: str = "entropy"):
        """One directed layer of the DBN lower bound (imdbn_rbm_bound_step): draws ``h ~ q(h | v)`` and adds
        ``log p(v | h)`` plus the entropy of q (``mode="entropy"``) or ``-log q(h | v)`` (``mode="logq"``) to ``acc``, a float64
        device tensor ``[M]`` (created zeroed when None).  Returns ``(acc, h)``, ``h`` fp32 0/1 ``[M, H]``.  No host sync."""
        return self._bound("bound_step", self._desc(rbm, False), None, v, rng, acc, mode)

    def _bound(self, name: str, d, logvar, v, rng, acc, mode: str):
        """The shared body of ``bound_step`` and ``gauss_bound_step``: the entry ``imdbn_rbm_<name>``; ``logvar``: the checked
        log-variances of the Gaussian call, which its entry takes in front of ``v``."""
        v = _f32c(v)
        M, dev = v.size(0), v.device
        if mode not in ("entropy", "logq"):
            raise N.EngineError(f"{name}: mode must be 'entropy' or 'logq', got {mode!r}")
        if acc is None:
            acc = torch.zeros(max(M, 1), dtype=torch.float64, device=dev)
        elif acc.dtype != torch.float64 or acc.device != dev or acc.numel() != M or not acc.is_contiguous():
            raise N.EngineError(f"{name}: acc must be a contiguous float64 [{M}] tensor on {dev}")
        h = torch.empty(max(M, 1), d.H, device=dev)
        sched = R.sched_bound(d.H)
        r, keep = self._rng(rng, sched, max(M, 1), dev)
        z = () if logvar is None else (_ptr(logvar),)
        self._call("imdbn_rbm_" + name, C.byref(d), *z, _ptr(v), v.stride(0), M, N.BOUND_LOGQ if mode == "logq" else N.BOUND_ENTROPY,
                   C.byref(r), _ptr(acc), _ptr(h), h.stride(0), *self._ws_tail(dev, d.V, d.H, max(M, 1)))
        self._done(rng, r, sched)
        return acc, h

    def prop_down(self, rbm, h, T=1.0, logits_only=False):
        d = self._desc(rbm, False)
        h = _f32c(h)
        B, dev = h.size(0), h.device
        out = torch.empty(B, d.V, device=dev)
        self._call("imdbn_rbm_prop_down", C.byref(d), _ptr(h), h.stride(0), B, float(T), 1 if logits_only else 0, _ptr(out), out.stride(0),
                   *self._ws_tail(dev, d.V, d.H, B))
        return out

    def sample_visible(self, rbm, v_prob, rng):
        d = self._desc(rbm, False)
        p = _f32c(v_prob)
        B, dev = p.size(0), p.device
        out = torch.empty(B, d.V, device=dev)
        sched = R.sched_sample_visible(d.V, self._groups(rbm))
        r, keep = self._rng(rng, sched, B, dev)
        self._call("imdbn_rbm_sample_visible", C.byref(d), _ptr(p), p.stride(0), B, C.byref(r), _ptr(out), out.stride(0), self._stream(dev))
        self._done(rng, r, sched)
        return out

    def gibbs_step(self, rbm, v, sample_h, sample_v, rng):
        d = self._desc(rbm, False)
        v = _f32c(v)
        B, dev = v.size(0), v.device
        v_next, v_prob = torch.empty(B, d.V, device=dev), torch.empty(B, d.V, device=dev)
        h, h_prob = torch.empty(B, d.H, device=dev), torch.empty(B, d.H, device=dev)
        sched = ([("u", d.H)] if sample_h else []) + (R.sched_sample_visible(d.V, self._groups(rbm)) if sample_v else [])
        r, keep = self._rng(rng, sched, B, dev)
        self._call("imdbn_rbm_gibbs_step", C.byref(d), _ptr(v), v.stride(0), B, int(bool(sample_h)), int(bool(sample_v)), C.byref(r),
                   _ptr(v_next), _ptr(v_prob), _ptr(h), _ptr(h_prob), *self._ws_tail(dev, d.V, d.H, B))
        self._done(rng, r, sched)
        return v_next, v_prob, h, h_prob

    # ---- CD updates ---------------------------------------------------------------------------
    @staticmethod
    def _opts(rbm, lr, mom, cd_k, sparsity=False, sample_h=False, sample_v=False, reclamp=True) -> N.CdOpts:
        o = N.CdOpts()
        o.cd_k, o.lr, o.momentum, o.weight_decay = int(cd_k), float(lr), float(mom), float(rbm.weight_decay)
        o.sparsity, o.sparsity_target = int(bool(sparsity)), float(getattr(rbm, "sparsity_factor", 0.0))
        o.sample_h, o.sample_v, o.reclamp_negative = int(bool(sample_h)), int(bool(sample_v)), int(bool(reclamp))
        return o

    @staticmethod
    def binary_hint(x: torch.Tensor) -> int:
        """What the HOST knows about the values of the batch `x` (imdbn_cd_opts.data_binary): ``N.DATA_BINARY`` / ``N.DATA_REAL``
        when the tensor carries the tag ``_imdbn_binary`` (``imdbn.datasets.DeviceLoader`` batches and sequential
        ``TensorDataset`` loaders: True; engine outputs -- probabilities -- : False), else ``N.DATA_UNKNOWN``.

        Unknown is the normal case (a training loop that builds a fresh tensor per step, idbn.py:199-203) and costs nothing:
        the device decides per 64-column piece of the batch, from the exactness map its own preparation writes, whether the
        positive phase reads it as a bit plane or as bf16 terms -- the same numbers either way, so results never depend on what
        the host knew or on what ran before.  The host never inspects a batch (no reduction, no synchronisation)."""
        tag = getattr(x, "_imdbn_binary", None)
        if tag is None:
            return N.DATA_UNKNOWN
        return N.DATA_BINARY if tag else N.DATA_REAL

    @staticmethod
    def _hint(x: torch.Tensor, given) -> int:
        """`given`: None (ask the tensor's tag), a bool (True: asserted 0/1; False: nothing known) or an N.DATA_* code."""
        if given is None:
            return HipEngine.binary_hint(x)
        if isinstance(given, bool):
            return N.DATA_BINARY if given else N.DATA_UNKNOWN
        return int(given)

    @staticmethod
    def _ident(t: torch.Tensor):
        """What must be unchanged for prefetched operand forms of `t` to be still valid (best effort: writes through
        ``.data`` or raw pointers do not bump the version -- the caller of ``next_data=`` promises not to do that)."""
        return (t.data_ptr(), t.untyped_storage().data_ptr(), t._version, tuple(t.shape), t.stride(0))

    def prefetch_ok(self, d, B) -> bool:
        key = (d.V, d.H, B, d.ldw, (d.W or 0) & 15, (d.W_m or 0) & 15)
        ok = self._pf_ok.get(key)
        if ok is None:
            ok = self._pf_ok[key] = bool(self._lib.imdbn_rbm_prefetch_ok(C.byref(d), B))
        return ok

    def _prefetch_opts(self, o, d, x, next_data):
        """Fill the next-batch fields of the options of a CD pass on batch `x` (imdbn_cd_opts.next_* / data_slot); returns the
        key of the prefetch state and the accepted hint (None: none) -- ``_cd`` records ``self._pf[key]`` after the call."""
        B, dev = x.size(0), x.device
        key = (dev, d.V, d.H, B, torch.cuda.current_stream(dev).cuda_stream)
        st = self._pf.pop(key, None)
        if st is not None and st[0] == self._ident(x):
            o.data_slot = st[1]
        nxt = None
        if (next_data is not None and next_data.dtype == torch.float32 and next_data.device == dev and next_data.dim() == 2
                and tuple(next_data.shape) == tuple(x.shape) and next_data.stride(1) == 1 and self.prefetch_ok(d, B)):
            nxt = next_data
            o.next_data, o.ld_next, o.next_slot = nxt.data_ptr(), nxt.stride(0), (2 if o.data_slot == 1 else 1)
            o.next_binary = self.binary_hint(next_data)
        return key, nxt

    def _cd(self, name: str, rbm, d, data, o, rng, data_binary, *outs, next_data=None, prefetch: bool = True, particles=None,
            nullable_chains: bool = False):
        """The CD pass behind cd_step / cd_stats / cd_factors / cd_factors_wire / pcd_step / centered_step: entry `name`(desc,
        batch, ld, B, [particles, ld,] opts, rng, *outs, workspace tail).  `d` is the caller's descriptor (each method asks for its
        own ``need_momentum``), `o` its options.  With `prefetch` (cd_factors, pcd_step and centered_step have none) this is the one
        place that consumes and records the next-batch state: the record of this shape is popped before the call, the new one
        stored only after the call and its draw count came out right.  `particles`: the persistent chains of pcd_step /
        centered_step, whose draws are theirs alone; `nullable_chains`: the entry takes the pair also when there are none (NULL, 0)."""
        x = _f32c(data)
        B, dev = x.size(0), x.device
        o.data_binary = self._hint(data, data_binary)       # the caller's tensor: a fp32 copy `x` has lost the tag
        groups = self._groups(rbm)
        sched = R.sched_cd(d.V, d.H, groups, o.cd_k) if particles is None else R.sched_pcd(d.V, d.H, groups, o.cd_k)
        r, keep = self._rng(rng, sched, B, dev)
        tail = self._ws_tail(dev, d.V, d.H, B)
        key, nxt = self._prefetch_opts(o, d, x, next_data) if prefetch else (None, None)
        chains = ((None, 0) if nullable_chains else ()) if particles is None else (_ptr(particles), particles.stride(0))
        self._call(name, C.byref(d), _ptr(x), x.stride(0), B, *chains, C.byref(o), C.byref(r), *outs, *tail)
        self._done(rng, r, sched)
        if nxt is not None:                      # the strong reference keeps the address from being recycled
            self._pf[key] = (self._ident(nxt), int(o.next_slot), nxt)

    def cd_step(self, rbm, data, lr, mom, cd_k, rng, next_data=None, data_binary=None, forward=False):
        """One CD-k update.  ``next_data``: the batch the NEXT cd_step of this shape will get -- its operand forms are
        then prepared by extra blocks of this call's first negative-phase launch and the
        next call skips its own preparation when it is handed that very tensor, unmodified.
        ``forward``: also return ``forward(data)`` under the updated weights (one more propagation in the same call)."""
        d = self._desc(rbm, True)
        B, dev = data.size(0), data.device
        o = self._opts(rbm, lr, mom, cd_k, sparsity=getattr(rbm, "sparsity", False))
        loss = torch.empty(1, device=dev)
        fwd = None
        if forward:
            fwd = torch.empty(B, d.H, device=dev)
            o.fwd_out, o.ld_fwd = fwd.data_ptr(), fwd.stride(0)
        self._cd("imdbn_rbm_cd_step", rbm, d, data, o, rng, data_binary, _ptr(loss), next_data=next_data)
        if forward:
            return loss.reshape(()), fwd
        return loss.reshape(())

    @staticmethod
    def _chains(who: str, t: torch.Tensor, V: int) -> torch.Tensor:
        """Persistent chains are updated IN PLACE: the caller's tensor goes to the engine as it is, never as a copy."""
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.size(1) == V
                and t.size(0) >= 1 and t.stride(1) == 1 and t.stride(0) >= V):
            raise N.EngineError(f"{who} needs its chains as an fp32 HIP tensor [rows, {V}] with unit inner stride (updated in place)")
        return t

    def pcd_step(self, rbm, data, particles, lr, mom, cd_k, rng, data_binary=None, monitor: bool = True):
        """One persistent-CD update (imdbn_rbm_pcd_step): the update of ``cd_step`` with the negative phase run for ``cd_k`` Gibbs
        steps (0: none) on ``particles`` ``[B, V]`` (fp32 0/1, updated in place) instead of from the data.  Returns the mean-field
        reconstruction error ``mean((data - visible_probs(forward(data)))^2)`` as a 0-d device tensor, or None with
        ``monitor=False`` (that propagation is then not launched).  No host sync."""
        d = self._desc(rbm, True)
        p = self._chains("pcd_step", particles, d.V)
        if p.size(0) != data.size(0) or p.device != data.device:
            raise N.EngineError(f"pcd_step: {p.size(0)} chains on {p.device} for a batch of {data.size(0)} rows on {data.device}")
        o = self._opts(rbm, lr, mom, cd_k, sparsity=getattr(rbm, "sparsity", False))
        loss = torch.empty(1, device=data.device) if monitor else None
        self._cd("imdbn_rbm_pcd_step", rbm, d, data, o, rng, data_binary, _ptr(loss), prefetch=False, particles=p)
        return loss.reshape(()) if monitor else None

    @staticmethod
    def _offsets(who: str, t: torch.Tensor, n: int, dev) -> torch.Tensor:
        """Centering offsets are updated IN PLACE, as the chains are."""
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == n
                and t.is_contiguous()):
            raise N.EngineError(f"{who} must be a contiguous fp32 [{n}] tensor on {dev} (updated in place)")
        return t

    def centered_step(self, rbm, data, particles, lr, mom, cd_k, rng, mu, lam, slide, mode, data_binary=None, monitor: bool = True):
        """One centered update (imdbn_rbm_centered_step): the phases of ``cd_step`` (``particles=None``, CD-``cd_k``
        from the data) or of ``pcd_step`` (``particles`` ``[B, V]``, advanced in place by ``cd_k`` >= 0 Gibbs steps), then the
        update with the centered gradient around the offsets ``mu`` ``[V]`` / ``lam`` ``[H]`` (fp32, updated in place: they first
        slide by ``slide`` in [0, 1] towards the batch means -- ``mode`` 0: of the data, 1: of data and model).  Returns the loss
        of the phases' call as a 0-d device tensor, or None with ``monitor=False``.  No host sync."""
        d = self._desc(rbm, True)
        dev = data.device
        p = None
        if particles is not None:
            p = self._chains("centered_step", particles, d.V)
            if p.size(0) != data.size(0) or p.device != dev:
                raise N.EngineError(f"centered_step: {p.size(0)} chains on {p.device} for a batch of {data.size(0)} rows on {dev}")
        mu, lam = self._offsets("centered_step: mu", mu, d.V, dev), self._offsets("centered_step: lam", lam, d.H, dev)
        o = self._opts(rbm, lr, mom, cd_k, sparsity=getattr(rbm, "sparsity", False))
        loss = torch.empty(1, device=dev) if monitor else None
        need = int(self._lib.imdbn_centered_scratch_floats(d.V, d.H))
        scratch = self._buffer(("centered", dev, d.V, d.H, torch.cuda.current_stream(dev).cuda_stream),
                               lambda: torch.empty(need, dtype=torch.float32, device=dev), need)
        self._cd("imdbn_rbm_centered_step", rbm, d, data, o, rng, data_binary, _ptr(mu), _ptr(lam), float(slide), int(mode), _ptr(loss),
                 _ptr(scratch), prefetch=False, particles=p, nullable_chains=True)
        return loss.reshape(()) if monitor else None

    # ---- extended mean field (imdbn_rbm_tap_*) ----------------------------------------
    @staticmethod
    def _magnetisations(who: str, mv, mh, B: int, V: int, H: int, dev):
        """Magnetisations are updated IN PLACE, as the chains are: a tensor that would have to be copied is refused."""
        for nm, t, n in (("mv", mv, V), ("mh", mh, H)):
            if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.dim() == 2 and t.size(0) == B
                    and t.size(1) == n and t.stride(1) == 1 and (B == 1 or t.stride(0) >= n)):
                raise N.EngineError(f"{who}: {nm} must be an fp32 tensor [{B}, {n}] on {dev} with unit inner stride (updated in place)")
        return mv, mh

    def _tap_ws(self, dev, V, H, B):
        """``(workspace, bytes, stream)`` of the TAP entries: the workspace of the shape plus the split-K slabs and row partials."""
        need = int(self._lib.imdbn_rbm_tap_ws_bytes(V, H, B))
        ws = self._buffer(("tap_ws", dev, V, H, B, torch.cuda.current_stream(dev).cuda_stream),
                          lambda: torch.empty(need, dtype=torch.uint8, device=dev), need)
        return _ptr(ws), ws.numel(), self._stream(dev)

    def tap_iterate(self, rbm, mv, mh, n_iters, damp=0.5, order=2, want_gamma=True, want_res=True):
        """``n_iters`` >= 0 TAP iterations (imdbn_rbm_tap_iterate) on the magnetisations ``mv`` ``[B, V]`` /
        ``mh`` ``[B, H]`` (fp32, updated in place; row views with a pitch are taken as they are).  Returns ``(gamma, res)``: the
        free energy Gamma of every row as it stands after them (float64 ``[B]``; log Z ~ -Gamma at a fixed point) and the residual of
        the last iteration (fp32 ``[B]``), or None for the one not wanted.  ``order`` 1: naive mean field.  No host sync."""
        d = self._desc(rbm, False)
        dev = rbm.W.data.device
        B = mv.size(0) if isinstance(mv, torch.Tensor) and mv.dim() == 2 else 0
        self._magnetisations("tap_iterate", mv, mh, B, d.V, d.H, dev)
        gamma = torch.empty(B, dtype=torch.float64, device=dev) if want_gamma else None
        res = torch.empty(B, dtype=torch.float32, device=dev) if want_res else None
        self._call("imdbn_rbm_tap_iterate", C.byref(d), _ptr(mv), max(mv.stride(0), d.V), _ptr(mh), max(mh.stride(0), d.H), B, int(n_iters), float(damp),
                   int(order), _ptr(gamma), _ptr(res), *self._tap_ws(dev, d.V, d.H, B))
        return gamma, res

    def tap_step(self, rbm, data, mv, mh, lr, mom, n_iters, damp=0.5, order=2, data_binary=None, monitor=True):
        """One TAP update (imdbn_rbm_tap_step): the positive phase of ``cd_step``, ``n_iters`` >= 0 iterations on
        the persistent magnetisations ``mv`` / ``mh`` (updated in place) as the negative phase, the deterministic gradient and the
        update rule of ``cd_step``.  Returns the mean-field reconstruction error of the data as a 0-d device tensor, or None with
        ``monitor=False`` (that propagation is then not launched).  No draws, no host sync."""
        d = self._desc(rbm, True)
        x = _f32c(data)
        B, dev = x.size(0), x.device
        self._magnetisations("tap_step", mv, mh, B, d.V, d.H, dev)
        o = self._opts(rbm, lr, mom, 0, sparsity=getattr(rbm, "sparsity", False))
        o.data_binary = self._hint(data, data_binary)
        loss = torch.empty(1, device=dev) if monitor else None
        need = int(self._lib.imdbn_rbm_tap_scratch_floats(d.V, d.H))
        scratch = self._buffer(("tap", dev, d.V, d.H, torch.cuda.current_stream(dev).cuda_stream),
                               lambda: torch.empty(need, dtype=torch.float32, device=dev), need)
        self._call("imdbn_rbm_tap_step", C.byref(d), _ptr(x), x.stride(0), B, _ptr(mv), max(mv.stride(0), d.V), _ptr(mh), max(mh.stride(0), d.H), C.byref(o),
                   int(n_iters), float(damp), int(order), _ptr(loss), _ptr(scratch), scratch.numel(), *self._tap_ws(dev, d.V, d.H, B))
        return loss.reshape(()) if monitor else None

    # ---- deep Boltzmann machine (imdbn_dbm_layer) --------------------------------------
    def dbm_layer(self, lo, hi, x_lo, x_hi, bias, m=None, damp=0.0, s_lo=1.0, s_hi=1.0, sample=False, rng=None, want_p=False,
                  want_res=False):
        """One half-step of a layer between two RBMs (imdbn_dbm_layer): ``pre = s_lo x_lo W_lo + s_hi x_hi
        W_hi^T + bias`` with ``W_lo`` the ``W`` of ``lo`` (the layer is its hidden side) and ``W_hi`` the ``W`` of ``hi`` (the layer
        is its visible side); either RBM may be None with its ``x`` (a one-sided form), not both.  ``bias`` ``[N]`` is the layer's.
        Mean field (``sample=False``): ``m`` ``[B, N]`` fp32 is updated in place, ``m <- damp m + (1 - damp) sigmoid(pre)``;
        returns the rows' ``max |sigmoid(pre) - m_old|`` (fp32 ``[B]``) with ``want_res``, else None.  Sample: one ``("u", N)``
        draw of ``rng``; returns ``s = 1[sigmoid(pre) > U]``, or ``(p, s)`` with ``want_p``.  No host sync."""
        return self._dbm_layer(lo, hi, x_lo, x_hi, bias, m, damp, s_lo, s_hi, sample, rng, want_p, want_res)

    @staticmethod
    def _dbm_operands(who: str, lo, hi, x_lo, x_hi, bias):
        """The checked operands of a DBM layer call: ``(dev, n, B, Wl, Wh, xl, xh, b, kl, kh, ld)``; ``ld(t)``: the pitch of an optional
        tensor (0 for None).  ``lo`` / ``hi``: an RBM, or a 2-D fp32 view with unit inner stride standing for its ``W`` (a row block
        ``joint.W.data[:Dz]``: the layer is those rows)."""
        if lo is None and hi is None:
            raise N.EngineError(f"{who}: needs the RBM below, the RBM above or both")
        Wl, Wh = (None if r is None else (r if isinstance(r, torch.Tensor) else r.W.data) for r in (lo, hi))      # an RBM, or a view of a W
        first = Wl if Wl is not None else Wh
        dev = first.device
        n = Wl.size(1) if Wl is not None else Wh.size(0)
        for nm, W in (("lo", Wl), ("hi", Wh)):
            if W is not None and not (W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and W.stride(1) == 1 and W.device == dev):
                raise N.EngineError(f"{who}: {nm}.W must be fp32 [V, H] with unit inner stride on {dev}")
        if Wl is not None and Wh is not None and Wh.size(0) != n:
            raise N.EngineError(f"{who}: lo has {n} hidden units, hi has {Wh.size(0)} visible units")
        xs = []
        for nm, W, x, k in (("x_lo", Wl, x_lo, None if Wl is None else Wl.size(0)), ("x_hi", Wh, x_hi, None if Wh is None else Wh.size(1))):
            if W is None:
                xs.append(None)
                continue
            if x is None:
                raise N.EngineError(f"{who}: {nm} is missing")
            x = _f32c(x)
            if x.dim() != 2 or x.size(1) != k or x.device != dev:
                raise N.EngineError(f"{who}: {nm} must be [B, {k}] on {dev}")
            xs.append(x)
        xl, xh = xs
        B = (xl if xl is not None else xh).size(0)
        if xl is not None and xh is not None and xh.size(0) != B:
            raise N.EngineError(f"{who}: x_lo and x_hi need the same rows")
        b = bias.data if isinstance(bias, torch.nn.Parameter) else bias
        if not (isinstance(b, torch.Tensor) and b.device == dev and b.dtype == torch.float32 and b.numel() == n and b.is_contiguous()):
            raise N.EngineError(f"{who}: bias must be a contiguous fp32 [{n}] tensor on {dev}")
        ld = lambda t: 0 if t is None else max(t.stride(0), t.size(1))
        kl, kh = (0 if xl is None else xl.size(1)), (0 if xh is None else xh.size(1))
        return dev, n, B, Wl, Wh, xl, xh, b, kl, kh, ld

    def _dbm_layer(self, lo, hi, x_lo, x_hi, bias, m, damp, s_lo, s_hi, sample, rng, want_p, want_res, s_out=None):
        """``dbm_layer``; ``s_out``: an fp32 ``[B, N]`` tensor with unit inner stride that receives the samples in place of a fresh
        one (``dbm_gibbs`` writes a layer's new state straight into its particles: a layer is never its own input)."""
        if bool(sample) == (m is not None):
            raise N.EngineError("dbm_layer: mean field takes m (updated in place), sample=True takes none")
        dev, n, B, Wl, Wh, xl, xh, b, kl, kh, ld = self._dbm_operands("dbm_layer", lo, hi, x_lo, x_hi, bias)
        need = int(self._lib.imdbn_dbm_layer_ws_bytes(kl, kh, n, B))
        ws = self._buffer(("dbm_ws", dev, kl, kh, n, B, torch.cuda.current_stream(dev).cuda_stream),
                          lambda: torch.empty(max(need, 256), dtype=torch.uint8, device=dev), need)
        res = p = smp = r = None
        sched = [("u", n)] if sample else []
        if sample:
            smp = torch.empty(B, n, device=dev) if s_out is None else s_out
            if not (smp.device == dev and smp.dtype == torch.float32 and smp.dim() == 2 and smp.size(0) == B and smp.size(1) == n
                    and smp.stride(1) == 1 and (B == 1 or smp.stride(0) >= n)):
                raise N.EngineError(f"dbm_layer: the sample output must be an fp32 tensor [{B}, {n}] on {dev} with unit inner stride")
            p = torch.empty(B, n, device=dev) if want_p else None
            r, keep = self._rng(rng, sched, B, dev)
        else:
            if not (isinstance(m, torch.Tensor) and m.device == dev and m.dtype == torch.float32 and m.dim() == 2 and m.size(0) == B
                    and m.size(1) == n and m.stride(1) == 1 and (B == 1 or m.stride(0) >= n)):
                raise N.EngineError(f"dbm_layer: m must be an fp32 tensor [{B}, {n}] on {dev} with unit inner stride (updated in place)")
            res = torch.empty(B, device=dev) if want_res else None
        self._call("imdbn_dbm_layer", _ptr(Wl), ld(Wl), kl, _ptr(xl), ld(xl), float(s_lo), _ptr(Wh), ld(Wh), kh, _ptr(xh), ld(xh), float(s_hi),
                   _ptr(b), n, B, self.mode, _ptr(m), ld(m), float(damp), _ptr(res), _ref(r), _ptr(smp), ld(smp), _ptr(p), ld(p),
                   _ptr(ws), ws.numel(), self._stream(dev))
        if sample:
            self._done(rng, r, sched)
            return (p, smp) if want_p else smp
        return res

    @staticmethod
    def _dbm_check(who: str, layers, biases):
        L = len(layers)
        if L < 1 or len(biases) != L + 1:
            raise N.EngineError(f"{who}: {L} RBMs need {L + 1} layer biases, got {len(biases)}")
        return L

    def dbm_gibbs(self, layers, biases, particles, n_sweeps, rng, clamp_bottom=None):
        """``n_sweeps`` block-Gibbs sweeps of a DBM on ``particles``, the list of its ``L + 1`` 0/1 state
        tensors ``[M, N_l]``, in place: the odd layers given the even ones, bottom to top, then the even layers given the odd ones.
        ``layers``: the ``L`` RBMs bottom first; ``biases``: the ``L + 1`` layer biases, ``biases[0]`` being ``layers[0].vis_bias``
        (layer 0 goes through ``prop_down`` + ``sample_visible``, which read it there).  Draws per sweep: ``rng.sched_dbm_gibbs``.
        With ``clamp_bottom`` ``[M, N_0]`` layer 0 is held at that tensor and draws nothing.  Returns ``particles``.  No host sync."""
        L = self._dbm_check("dbm_gibbs", layers, biases)
        if len(particles) != L + 1:
            raise N.EngineError(f"dbm_gibbs: {L} RBMs need {L + 1} state tensors, got {len(particles)}")
        if clamp_bottom is not None:
            particles[0].copy_(clamp_bottom)
        for _ in range(int(n_sweeps)):
            for parity in (1, 0):
                for l in range(parity, L + 1, 2):
                    if l == 0:
                        if clamp_bottom is None:
                            particles[0].copy_(self.sample_visible(layers[0], self.prop_down(layers[0], particles[1]), rng))
                        continue
                    hi = layers[l] if l < L else None
                    self._dbm_layer(layers[l - 1], hi, particles[l - 1], particles[l + 1] if l < L else None, biases[l], None, 0.0, 1.0, 1.0,
                                    True, rng, False, False, s_out=particles[l])
        return particles

    def dbm_infer(self, layers, biases, v, n_mf, damp=0.0, init=None, want_res=True):
        """Mean-field posterior of a DBM given the bottom layer ``v`` ``[B, N_0]``.  Start (``init`` None): the
        bottom-up pass ``mu_l = sigmoid(s mu_{l-1} W_{l-1} + b_l)`` with ``s = 2`` below the top layer and ``s = 1`` at it
        (Salakhutdinov & Hinton 2009, section 3.1), the one-sided form of ``dbm_layer``; else ``init``, the ``L`` tensors
        ``[B, N_l]`` (updated in place).  Then ``n_mf`` sweeps over the layers ``1 .. L`` in order, each from its freshest
        neighbours, damped by ``damp``.  Returns ``([mu_1 .. mu_L], res)``: ``res`` fp32 ``[B]``, the largest ``|sigmoid - mu_old|``
        over the layers of the last sweep (zeros with ``n_mf = 0``), or None without ``want_res``.  No host sync."""
        L = self._dbm_check("dbm_infer", layers, biases)
        x = _f32c(v)
        B, dev = x.size(0), x.device
        if init is None:
            mu = []
            for l in range(1, L + 1):
                m = torch.zeros(B, biases[l].numel(), device=dev)
                self.dbm_layer(layers[l - 1], None, x if l == 1 else mu[-1], None, biases[l], m=m, s_lo=2.0 if l < L else 1.0)
                mu.append(m)
        else:
            mu = list(init)
            if len(mu) != L:
                raise N.EngineError(f"dbm_infer: init needs {L} tensors, got {len(mu)}")
        res = torch.zeros(B, device=dev) if want_res else None
        for it in range(int(n_mf)):
            last = want_res and it == int(n_mf) - 1
            for l in range(1, L + 1):
                r = self.dbm_layer(layers[l - 1], layers[l] if l < L else None, x if l == 1 else mu[l - 2], mu[l] if l < L else None,
                                   biases[l], m=mu[l - 1], damp=damp, want_res=last)
                if last:
                    res = r if l == 1 else torch.maximum(res, r)
        return mu, res

    def dbm_step(self, layers, data, particles, epoch_scalars, n_mf, damp, gibbs_k, rng, monitor=True):
        """One training step of a DBM (Salakhutdinov & Hinton 2009) on one stream, no host sync.  ``layers``: the
        ``L`` RBMs bottom first; the model's biases live in them (layer 0: ``layers[0].vis_bias``, layer l >= 1:
        ``layers[l-1].hid_bias``).  (1) ``dbm_infer`` on ``data`` (``n_mf`` sweeps, ``damp``); (2) ``gibbs_k`` sweeps of
        ``dbm_gibbs`` on ``particles`` (``L + 1`` tensors of as many rows as ``data``, in place); (3) when every phase tensor exists,
        one ``assoc_update`` per RBM l from ``(pos_l, pos_{l+1}, neg_l, neg_{l+1})`` -- ``pos_0 = data``, ``pos_l = mu_l``, ``neg``
        the particles -- with ``epoch_scalars[l] = (lr, mom)``, the RBM's weight decay and no sparsity term.  The update also moves
        ``layers[l].vis_bias`` for l >= 1, which is no parameter of the model and is never read.  Returns ``{"mu", "particles",
        "res", "recon_loss"}``; ``recon_loss``: the mean squared error of ``sigmoid(mu_1 W_0^T + b_0)`` against the data under the
        parameters on entry, a 0-d device tensor, or None with ``monitor=False`` (that propagation is then not launched)."""
        from . import dp
        if dp.active():
            raise NotImplementedError("dbm_step has no data-parallel split")
        L = len(layers)
        if L < 1 or len(epoch_scalars) != L or len(particles) != L + 1:
            raise N.EngineError(f"dbm_step: {L} RBMs need {L} (lr, mom) pairs and {L + 1} particle tensors")
        x = _f32c(data)
        if any(p.size(0) != x.size(0) for p in particles):
            raise N.EngineError("dbm_step: the particles need as many rows as the data")
        biases = [layers[0].vis_bias.data] + [r.hid_bias.data for r in layers]
        mu, res = self.dbm_infer(layers, biases, x, n_mf, damp=damp)
        recon = None
        if monitor:
            recon = (self.prop_down(layers[0], mu[0]) - x).square().mean()
        self.dbm_gibbs(layers, biases, particles, gibbs_k, rng)
        pos = [x] + mu
        for l, rbm in enumerate(layers):
            lr, mom = epoch_scalars[l]
            self._assoc(rbm, pos[l], pos[l + 1], particles[l], particles[l + 1], lr, mom, False)
        return {"mu": mu, "particles": particles, "res": res, "recon_loss": recon}

    # ---- multimodal deep Boltzmann machine (imdbn_dbm_group_layer) ----------------------
    def dbm_group_layer(self, lo, hi, x_lo, x_hi, bias, groups, m=None, damp=0.0, sample=False, rng=None, want_p=False, want_res=False,
                        s_out=None):
        """One half-step of a DBM layer of categorical units (imdbn_dbm_group_layer): ``pre = x_lo W_lo + x_hi
        W_hi^T + bias`` as ``dbm_layer`` forms it; ``lo`` / ``hi``: an RBM or a 2-D fp32 view with unit inner stride standing for its
        ``W`` (the label layer passes ``hi = joint.W.data[Dz:]`` alone).  ``groups``: ``(start, end)`` pairs that tile ``[0, N)`` in
        order, at most ``MAX_GROUPS`` of width 2 to 256; ``p`` is the softmax of ``pre`` within each.  Mean field: ``m`` ``[B, N]``
        fp32 (a column block of a wider tensor is fine) is updated in place, ``m <- damp m + (1 - damp) p``; returns the rows' ``max
        |p - m_old|`` with ``want_res``, else None.  Sample: one ``("c", width)`` draw of ``rng`` per group; returns the one-hot rows
        (written into ``s_out`` when given), or ``(p, s)`` with ``want_p``.  No host sync."""
        from . import dp
        if dp.active():
            raise NotImplementedError("dbm_group_layer has no data-parallel split")
        if bool(sample) == (m is not None):
            raise N.EngineError("dbm_group_layer: mean field takes m (updated in place), sample=True takes none")
        dev, n, B, Wl, Wh, xl, xh, b, kl, kh, ld = self._dbm_operands("dbm_group_layer", lo, hi, x_lo, x_hi, bias)
        gs = [(int(s), int(e)) for s, e in groups]
        if not 1 <= len(gs) <= N.MAX_GROUPS or gs[0][0] != 0 or gs[-1][1] != n or any(a[1] != c[0] for a, c in zip(gs, gs[1:])):
            raise N.EngineError(f"dbm_group_layer: 1 to {N.MAX_GROUPS} groups must tile [0, {n}) in order, got {gs}")
        ends = (C.c_int * len(gs))(*[e for _, e in gs])
        need = int(self._lib.imdbn_dbm_group_layer_ws_bytes(kl, kh, n, B))
        ws = self._buffer(("dbm_group_ws", dev, kl, kh, n, B, torch.cuda.current_stream(dev).cuda_stream),
                          lambda: torch.empty(max(need, 256), dtype=torch.uint8, device=dev), need)
        block = lambda t: (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.dim() == 2 and t.size(0) == B
                           and t.size(1) == n and t.stride(1) == 1 and (B == 1 or t.stride(0) >= n))
        res = p = smp = r = None
        sched = [("c", e - s) for s, e in gs] if sample else []
        if sample:
            smp = torch.empty(B, n, device=dev) if s_out is None else s_out
            if not block(smp):
                raise N.EngineError(f"dbm_group_layer: the sample output must be an fp32 tensor [{B}, {n}] on {dev} with unit inner stride")
            p = torch.empty(B, n, device=dev) if want_p else None
            r, keep = self._rng(rng, sched, B, dev)
        else:
            if not block(m):
                raise N.EngineError(f"dbm_group_layer: m must be an fp32 tensor [{B}, {n}] on {dev} with unit inner stride (updated in place)")
            res = torch.empty(B, device=dev) if want_res else None
        self._call("imdbn_dbm_group_layer", _ptr(Wl), ld(Wl), kl, _ptr(xl), ld(xl), 1.0, _ptr(Wh), ld(Wh), kh, _ptr(xh), ld(xh), 1.0,
                   _ptr(b), n, B, self.mode, len(gs), ends, _ptr(m), ld(m), float(damp), _ptr(res), _ref(r), _ptr(smp), ld(smp), _ptr(p), ld(p),
                   _ptr(ws), ws.numel(), self._stream(dev))
        if sample:
            self._done(rng, r, sched)
            return (p, smp) if want_p else smp
        return res

    @staticmethod
    def _mdbm_check(who: str, image_layers, joint, biases):
        """``(L, Dz, K, J)`` of a multimodal DBM: ``L`` image RBMs, the joint RBM over ``[z_img (Dz) | y (K, one softmax group)]`` with
        ``J`` hidden units, and the ``L + 3`` layer biases ``b_0 .. b_L, b_J, b_Y``."""
        L = len(image_layers)
        if L < 1 or len(biases) != L + 3:
            raise N.EngineError(f"{who}: {L} image RBMs and the joint RBM need {L + 3} layer biases, got {len(biases)}")
        Dz = image_layers[-1].W.size(1)
        V, J = joint.W.shape
        K = V - Dz
        if [tuple(map(int, g)) for g in (getattr(joint, "softmax_groups", None) or [])] != [(Dz, V)]:
            raise N.EngineError(f"{who}: the joint RBM's visible side must be [z_img ({Dz}) | y] with y its one softmax group")
        return L, Dz, K, J

    def mdbm_infer(self, image_layers, joint, biases, v, y, n_mf, damp=0.0, want_res=True):
        """Mean-field posterior of a multimodal DBM given the image ``v`` ``[B, N_0]`` and, with ``y`` a one-hot
        ``[B, K]``, the label; with ``y`` None the labels are free and start at ``softmax(b_Y)``.  Start: the doubled-weights pass of
        ``dbm_infer`` up to ``z`` (``s = 2`` at every image layer), then ``J`` from ``[mu_L | y]`` with ``s = 1``.  Then ``n_mf``
        Gauss-Seidel sweeps over the layers ``1 .. L`` (``z`` hears from the image stack and, through the rows ``[0, Dz)`` of the joint
        ``W``, from ``J``), ``J``, and ``Y`` when free.  Returns ``([mu_1 .. mu_L, mu_J, mu_Y], res)``: ``mu_L`` and ``mu_Y`` are the
        column blocks of ONE ``[B, Dz + K]`` tensor, the joint RBM's visible row (``mu_L._base``); ``res`` as ``dbm_infer``'s.  No
        host sync."""
        from . import dp
        if dp.active():
            raise NotImplementedError("mdbm_infer has no data-parallel split")
        L, Dz, K, J = self._mdbm_check("mdbm_infer", image_layers, joint, biases)
        x = _f32c(v)
        B, dev = x.size(0), x.device
        free = y is None
        zy = torch.zeros(B, Dz + K, device=dev)
        mz, my = zy[:, :Dz], zy[:, Dz:]
        Wz, Wy = joint.W.data[:Dz], joint.W.data[Dz:]
        mj = torch.zeros(B, J, device=dev)
        if free:                                  # softmax(b_Y) by the layer's own kernel: a silent J leaves pre = b_Y exactly
            self.dbm_group_layer(None, Wy, None, mj, biases[L + 2], [(0, K)], m=my)
        else:
            my.copy_(y)
        mu = [torch.zeros(B, biases[l].numel(), device=dev) for l in range(1, L)] + [mz]
        for l in range(1, L + 1):
            self._dbm_layer(image_layers[l - 1], None, x if l == 1 else mu[l - 2], None, biases[l], mu[l - 1], 0.0, 2.0, 1.0, False, None,
                            False, False)
        self._dbm_layer(joint, None, zy, None, biases[L + 1], mj, 0.0, 1.0, 1.0, False, None, False, False)
        res = torch.zeros(B, device=dev) if want_res else None
        for it in range(int(n_mf)):
            last = want_res and it == int(n_mf) - 1
            rs = []
            for l in range(1, L + 1):
                rs.append(self._dbm_layer(image_layers[l - 1], image_layers[l] if l < L else Wz, x if l == 1 else mu[l - 2],
                                          mu[l] if l < L else mj, biases[l], mu[l - 1], damp, 1.0, 1.0, False, None, False, last))
            rs.append(self._dbm_layer(joint, None, zy, None, biases[L + 1], mj, damp, 1.0, 1.0, False, None, False, last))
            if free:
                rs.append(self.dbm_group_layer(None, Wy, None, mj, biases[L + 2], [(0, K)], m=my, damp=damp, want_res=last))
            if last:
                res = torch.stack(rs).amax(0)
        return mu + [mj, my], res

    def mdbm_gibbs(self, image_layers, joint, biases, particles, n_sweeps, rng, clamp_bottom=None, clamp_labels=None):
        """``n_sweeps`` block-Gibbs sweeps of a multimodal DBM on ``particles``, in place: the ``L + 2`` tensors
        ``[s_0 .. s_{L-1}, zy, s_J]`` with ``zy`` ``[M, Dz + K]`` holding ``z_img`` and the one-hot label side by side.  Two-colouring:
        ``J`` is one class with the layers of parity ``L + 1``; ``Y`` goes with layer ``L``.  Per sweep the class of ``J`` bottom to
        top, then the other class bottom to top with ``Y`` right after layer ``L``.  Draws: ``rng.sched_mdbm_gibbs``.  With
        ``clamp_bottom`` ``[M, N_0]`` / ``clamp_labels`` one-hot ``[M, K]`` that layer is held and draws nothing.  Returns
        ``particles``.  No host sync."""
        from . import dp
        if dp.active():
            raise NotImplementedError("mdbm_gibbs has no data-parallel split")
        L, Dz, K, J = self._mdbm_check("mdbm_gibbs", image_layers, joint, biases)
        if len(particles) != L + 2:
            raise N.EngineError(f"mdbm_gibbs: {L} image RBMs and the joint RBM need {L + 2} state tensors, got {len(particles)}")
        zy = particles[L]
        if zy.dim() != 2 or zy.size(1) != Dz + K:
            raise N.EngineError(f"mdbm_gibbs: particles[{L}] must be [M, {Dz + K}], z_img and the label side by side")
        state = lambda l: zy[:, :Dz] if l == L else particles[l]
        Wz, Wy = joint.W.data[:Dz], joint.W.data[Dz:]
        if clamp_bottom is not None:
            particles[0].copy_(clamp_bottom)
        if clamp_labels is not None:
            zy[:, Dz:].copy_(clamp_labels)
        for _ in range(int(n_sweeps)):
            for parity in ((L + 1) & 1, L & 1):
                for l in range(parity, L + 2, 2):
                    if l == 0:
                        if clamp_bottom is None:
                            particles[0].copy_(self.sample_visible(image_layers[0], self.prop_down(image_layers[0], state(1)), rng))
                    elif l <= L:
                        self._dbm_layer(image_layers[l - 1], image_layers[l] if l < L else Wz, state(l - 1), state(l + 1), biases[l], None, 0.0,
                                        1.0, 1.0, True, rng, False, False, s_out=state(l))
                        if l == L and clamp_labels is None:
                            self.dbm_group_layer(None, Wy, None, particles[L + 1], biases[L + 2], [(0, K)], sample=True, rng=rng,
                                                 s_out=zy[:, Dz:])
                    else:
                        self._dbm_layer(joint, None, zy, None, biases[L + 1], None, 0.0, 1.0, 1.0, True, rng, False, False,
                                        s_out=particles[L + 1])
        return particles

    def mdbm_step(self, image_layers, joint, data, labels, particles, epoch_scalars, n_mf, damp, gibbs_k, rng, monitor=True):
        """One training step of a multimodal DBM (Srivastava & Salakhutdinov 2012) on one stream, no host sync.
        The biases live in the RBMs: ``b_0 = image_layers[0].vis_bias``, ``b_l = image_layers[l-1].hid_bias``, ``b_J =
        joint.hid_bias``, ``b_Y = joint.vis_bias[Dz:]``.  (1) ``mdbm_infer`` on ``(data, labels)`` with the label clamped; (2)
        ``gibbs_k`` sweeps of ``mdbm_gibbs`` on ``particles`` (as many rows as ``data``, in place); (3) one ``assoc_update`` per image
        RBM as ``dbm_step`` does, and one for the joint RBM from ``([mu_L | y], mu_J, [s_L | s_Y], s_J)``, with ``epoch_scalars[l] =
        (lr, mom)`` (the joint RBM last), every RBM's own weight decay and no sparsity term.  The update also moves
        ``image_layers[l].vis_bias`` for l >= 1 and ``joint.vis_bias[:Dz]``, which are no parameters of the model and are never read.
        Returns ``{"mu", "particles", "res", "recon_loss"}`` as ``dbm_step``."""
        from . import dp
        if dp.active():
            raise NotImplementedError("mdbm_step has no data-parallel split")
        L = len(image_layers)
        if L < 1 or len(epoch_scalars) != L + 1 or len(particles) != L + 2:
            raise N.EngineError(f"mdbm_step: {L} image RBMs and the joint RBM need {L + 1} (lr, mom) pairs and {L + 2} particle tensors")
        x = _f32c(data)
        if any(p.size(0) != x.size(0) for p in particles):
            raise N.EngineError("mdbm_step: the particles need as many rows as the data")
        Dz = image_layers[-1].W.size(1)
        biases = ([image_layers[0].vis_bias.data] + [r.hid_bias.data for r in image_layers]
                  + [joint.hid_bias.data, joint.vis_bias.data[Dz:]])
        mu, res = self.mdbm_infer(image_layers, joint, biases, x, labels, n_mf, damp=damp)
        recon = None
        if monitor:
            recon = (self.prop_down(image_layers[0], mu[0]) - x).square().mean()
        self.mdbm_gibbs(image_layers, joint, biases, particles, gibbs_k, rng)
        pos = [x] + mu[:L]
        for l, rbm in enumerate(image_layers):
            lr, mom = epoch_scalars[l]
            self._assoc(rbm, pos[l], pos[l + 1], particles[l], particles[l + 1][:, :Dz] if l + 1 == L else particles[l + 1], lr, mom, False)
        lr, mom = epoch_scalars[L]
        self._assoc(joint, mu[L - 1]._base, mu[L], particles[L], particles[L + 1], lr, mom, False)      # _base: the [mu_L | y] row
        return {"mu": mu, "particles": particles, "res": res, "recon_loss": recon}

    # ---- the DBM as a density model (imdbn_dbm_rowsum_layer, imdbn_dbm_ais) ------------
    _DBM_MODES = {"weigh": N.DBM_WEIGH, "sample": N.DBM_SAMPLE, "bound": N.DBM_BOUND}

    def dbm_rowsum_layer(self, lo, hi, x_lo, x_hi, bias, mode, acc=None, beta=1.0, beta_prev=0.0, dbeta_next=0.0, base=None, mu=None,
                         sample=True, rng=None, want_p=False, s_out=None):
        """One layer of a DBM with a row sum for its epilogue (imdbn_dbm_rowsum_layer); the operands and
        ``pre`` are ``dbm_layer``'s with ``s_lo = s_hi = 1``.  ``acc``: a float64 ``[B]`` device tensor the call ADDS to (None: a
        fresh one of zeros, except in ``"sample"`` mode, which then sums nothing).  ``mode``:
        ``"weigh"``  ``acc += sum_n sp(e_n(beta)) - sp(e_n(beta_prev))``, ``e(t) = t pre + (1 - t) base`` (``base`` ``[N]``, None =
        zeros); with ``sample`` the units are also drawn at ``beta`` (one ``("u", N)`` draw of ``rng``).
        ``"sample"`` ``s = 1[sigmoid(beta pre + (1 - beta) base) > U]``; ``acc += dbeta_next sum_n bias_n s_n``.
        ``"bound"``  from below only (``hi`` None): ``acc += sum_n mu_n pre_n + h(mu_n)`` for the magnetisations ``mu`` ``[B, N]``;
        here ``base`` is the bias of the layer BELOW, whose ``sum_k base_k x_lo[., k]`` is added too.
        Returns ``(acc, s, p)``: ``s`` the drawn states (``s_out`` when given) and ``p`` their probabilities with ``want_p``, None
        where nothing was drawn.  No host sync."""
        if mode not in self._DBM_MODES:
            raise N.EngineError(f"dbm_rowsum_layer: mode must be one of {sorted(self._DBM_MODES)}, got {mode!r}")
        dev, n, B, Wl, Wh, xl, xh, b, kl, kh, ld = self._dbm_operands("dbm_rowsum_layer", lo, hi, x_lo, x_hi, bias)
        draws = mode == "sample" or (mode == "weigh" and bool(sample))
        if mode == "bound" and (Wh is not None or mu is None):
            raise N.EngineError("dbm_rowsum_layer: the bound is one-sided from below and needs mu")
        nb = kl if mode == "bound" else n
        bA = _on(base, dev, torch.float32)
        if bA is not None and bA.numel() != nb:
            raise N.EngineError(f"dbm_rowsum_layer: base must have {nb} elements")
        if mu is not None:
            mu = _f32c(mu)
            if mu.dim() != 2 or mu.size(0) != B or mu.size(1) != n or mu.device != dev:
                raise N.EngineError(f"dbm_rowsum_layer: mu must be [{B}, {n}] on {dev}")
        if acc is None and mode != "sample":
            acc = torch.zeros(B, dtype=torch.float64, device=dev)
        if acc is not None and not (acc.device == dev and acc.dtype == torch.float64 and acc.numel() == B and acc.is_contiguous()):
            raise N.EngineError(f"dbm_rowsum_layer: acc must be a contiguous float64 [{B}] tensor on {dev}")
        need = int(self._lib.imdbn_dbm_rowsum_layer_ws_bytes(kl, kh, n, B))
        ws = self._buffer(("dbm_rowsum_ws", dev, kl, kh, n, B, torch.cuda.current_stream(dev).cuda_stream),
                          lambda: torch.empty(max(need, 256), dtype=torch.uint8, device=dev), need)
        smp = p = r = None
        sched = [("u", n)] if draws else []
        if draws:
            smp = torch.empty(B, n, device=dev) if s_out is None else s_out
            if not (smp.device == dev and smp.dtype == torch.float32 and smp.dim() == 2 and smp.size(0) == B and smp.size(1) == n
                    and smp.stride(1) == 1 and (B == 1 or smp.stride(0) >= n)):
                raise N.EngineError(f"dbm_rowsum_layer: the sample output must be an fp32 tensor [{B}, {n}] on {dev} with unit inner stride")
            p = torch.empty(B, n, device=dev) if want_p else None
            r, keep = self._rng(rng, sched, B, dev)
        self._call("imdbn_dbm_rowsum_layer", _ptr(Wl), ld(Wl), kl, _ptr(xl), ld(xl), _ptr(Wh), ld(Wh), kh, _ptr(xh), ld(xh), _ptr(b), n, B,
                   self._DBM_MODES[mode], float(beta), float(beta_prev), float(dbeta_next), _ptr(bA), _ptr(mu), ld(mu), _ref(r),
                   _ptr(smp), ld(smp), _ptr(p), ld(p), _ptr(acc), _ptr(ws), ws.numel(), self._stream(dev))
        if draws:
            self._done(rng, r, sched)
        return acc, smp, p

    def dbm_ais(self, layers, biases, betas, n_chains: int, rng, base_bias: Optional[torch.Tensor] = None, return_state: bool = False):
        """Annealed importance sampling of a DBM over its odd layers, the even ones summed out (imdbn_dbm_ais; Salakhutdinov &
        Hinton 2009, section 4.1): ``n_chains`` chains from the base model (no weights, zero biases but layer
        0's ``base_bias``, None = zeros) through ``betas`` (0 = betas[0] < ... < betas[K] = 1) in ONE call.  Returns the log
        importance weights, a float64 device tensor ``[n_chains]`` (and the final states of the odd layers, bottom first, with
        ``return_state``); log Z ~= sum_{l >= 1} N_l log 2 + sum softplus(base_bias) + logmeanexp(logw).  Draws:
        ``rng.sched_dbm_ais``.  No host sync."""
        L = self._dbm_check("dbm_ais", layers, biases)
        if L > N.DBM_MAX_LAYERS:
            raise N.EngineError(f"dbm_ais: at most {N.DBM_MAX_LAYERS} RBMs, got {L}")
        Ws = [r.W.data for r in layers]
        dev = Ws[0].device
        sizes = [Ws[0].size(0)] + [W.size(1) for W in Ws]
        bs = [b.data if isinstance(b, torch.nn.Parameter) else b for b in biases]
        for l, W in enumerate(Ws):
            if not (W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and W.stride(1) == 1 and W.device == dev and W.size(0) == sizes[l]):
                raise N.EngineError(f"dbm_ais: layers[{l}].W must be fp32 [{sizes[l]}, H] with unit inner stride on {dev}")
        for l, b in enumerate(bs):
            if not (isinstance(b, torch.Tensor) and b.device == dev and b.dtype == torch.float32 and b.numel() == sizes[l] and b.is_contiguous()):
                raise N.EngineError(f"dbm_ais: biases[{l}] must be a contiguous fp32 [{sizes[l]}] tensor on {dev}")
        bt = [float(x) for x in (betas.tolist() if hasattr(betas, "tolist") else betas)]
        K, M = len(bt) - 1, int(n_chains)
        arr = (C.c_float * max(1, len(bt)))(*bt)
        bA = _on(base_bias, dev, torch.float32)
        if bA is not None and bA.numel() != sizes[0]:
            raise N.EngineError(f"dbm_ais: base_bias must have {sizes[0]} elements")
        logw = torch.empty(max(M, 1), dtype=torch.float64, device=dev)
        states = [torch.empty(max(M, 1), sizes[l], device=dev) if return_state and l % 2 == 1 else None for l in range(L + 1)]
        csz = (C.c_int * (L + 1))(*sizes)
        need = int(self._lib.imdbn_dbm_ais_ws_bytes(L, csz, max(M, 1)))
        ws = self._buffer(("dbm_ais_ws", dev, tuple(sizes), M, torch.cuda.current_stream(dev).cuda_stream),
                          lambda: torch.empty(max(need, 256), dtype=torch.uint8, device=dev), need)
        sched = R.sched_dbm_ais(sizes, max(K, 1))
        r, keep = self._rng(rng, sched, max(M, 1), dev)
        ptrs = lambda ts, n: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
        self._call("imdbn_dbm_ais", L, ptrs(Ws, L), (C.c_int64 * L)(*[max(W.stride(0), W.size(1)) for W in Ws]), csz, ptrs(bs, L + 1),
                   _ptr(bA), arr, K, M, C.byref(r), _ptr(logw), ptrs(states, L + 1), (C.c_int64 * (L + 1))(*sizes), _ptr(ws), ws.numel(),
                   self._stream(dev))
        self._done(rng, r, sched)
        return (logw, [s for s in states if s is not None]) if return_state else logw

    def dbm_bound(self, layers, biases, v, mus):
        """``b_0 v + sum_{l >= 1} sum_n mu_{l,n} (mu_{l-1} W_{l-1} + b_l)_n + h(mu_{l,n})`` per row of ``v`` ``[B, N_0]``, ``mu_0 = v``:
        the variational bound on log p(v) of a DBM for the factorised posterior ``mus`` (``L`` tensors, as ``dbm_infer`` returns
        them) WITHOUT its ``- log Z``.  ``L`` ``dbm_rowsum_layer`` calls in bound mode on one float64 ``[B]``
        accumulator.  No host sync."""
        L = self._dbm_check("dbm_bound", layers, biases)
        if len(mus) != L:
            raise N.EngineError(f"dbm_bound: {L} RBMs need {L} magnetisation tensors, got {len(mus)}")
        x = _f32c(v)
        acc = None
        for l in range(1, L + 1):
            acc, _, _ = self.dbm_rowsum_layer(layers[l - 1], None, x if l == 1 else mus[l - 2], None, biases[l], "bound", acc=acc,
                                              base=biases[0] if l == 1 else None, mu=mus[l - 1])
        return acc

    # ---- Gaussian visible units (imdbn_rbm_gauss_*) ---------------------------------
    @staticmethod
    def _logvar(who: str, t, n: int, dev) -> torch.Tensor:
        """The log-variances (and their momentum) go to the engine as they are: the update writes them in place."""
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == n
                and t.is_contiguous()):
            raise N.EngineError(f"{who} must be a contiguous fp32 [{n}] tensor on {dev}")
        return t

    def gauss_forward(self, rbm, logvar, v, T=1.0, sample=False, rng=None):
        """p(h | v) of a Gaussian-visible RBM (imdbn_rbm_gauss_prop_up): ``sigmoid(((v exp(-logvar)) W + c) / T)``; with ``sample``
        also ``1[p > U]`` (one ("u", H) draw): ``(p, h)``.  No host sync."""
        d = self._desc(rbm, False)
        v = _f32c(v)
        B, dev = v.size(0), v.device
        z = self._logvar("gauss_forward: logvar", logvar, d.V, dev)
        out = torch.empty(B, d.H, device=dev)
        smp = torch.empty(B, d.H, device=dev) if sample else None
        sched = [("u", d.H)] if sample else []
        r, keep = self._rng(rng, sched, B, dev) if sample else (None, None)
        self._call("imdbn_rbm_gauss_prop_up", C.byref(d), _ptr(z), _ptr(v), v.stride(0), B, float(T), _ref(r), _ptr(out), out.stride(0),
                   _ptr(smp), d.H, *self._ws_tail(dev, d.V, d.H, B))
        if sample:
            self._done(rng, r, sched)
            return out, smp
        return out

    def gauss_backward(self, rbm, logvar, h, sample=False, rng=None):
        """The mean of p(v | h) of a Gaussian-visible RBM (imdbn_rbm_gauss_prop_down): ``b + h W^T``, the bits of
        ``prop_down(logits_only=True)``; with ``sample`` also ``mean + exp(logvar / 2) n`` (one ("n", V) draw): ``(mean, v)``."""
        d = self._desc(rbm, False)
        h = _f32c(h)
        B, dev = h.size(0), h.device
        z = self._logvar("gauss_backward: logvar", logvar, d.V, dev)
        out = torch.empty(B, d.V, device=dev)
        smp = torch.empty(B, d.V, device=dev) if sample else None
        sched = [("n", d.V)] if sample else []
        r, keep = self._rng(rng, sched, B, dev) if sample else (None, None)
        self._call("imdbn_rbm_gauss_prop_down", C.byref(d), _ptr(z), _ptr(h), h.stride(0), B, _ref(r), _ptr(out), out.stride(0),
                   _ptr(smp), d.V, *self._ws_tail(dev, d.V, d.H, B))
        if sample:
            self._done(rng, r, sched)
            return out, smp
        return out

    def gauss_sample_visible(self, rbm, logvar, mean, rng):
        """v ~ N(mean, exp(logvar)) for a caller's ``mean`` ``[B, V]`` (imdbn_rbm_gauss_sample_visible): one ("n", V) draw."""
        d = self._desc(rbm, False)
        m = _f32c(mean)
        B, dev = m.size(0), m.device
        z = self._logvar("gauss_sample_visible: logvar", logvar, d.V, dev)
        out = torch.empty(B, d.V, device=dev)
        sched = [("n", d.V)]
        r, keep = self._rng(rng, sched, B, dev)
        self._call("imdbn_rbm_gauss_sample_visible", C.byref(d), _ptr(z), _ptr(m), m.stride(0), B, C.byref(r), _ptr(out), out.stride(0),
                   self._stream(dev))
        self._done(rng, r, sched)
        return out

    def gauss_free_energy(self, rbm, logvar, v):
        """F(v) = sum (v - b)^2 / (2 sigma^2) - sum softplus(c + (v / sigma^2) W) per row, fp32 ``[B]`` (imdbn_rbm_gauss_free_energy)."""
        d = self._desc(rbm, False)
        v = _f32c(v)
        B, dev = v.size(0), v.device
        z = self._logvar("gauss_free_energy: logvar", logvar, d.V, dev)
        out = torch.empty(B, device=dev)
        self._call("imdbn_rbm_gauss_free_energy", C.byref(d), _ptr(z), _ptr(v), v.stride(0), B, _ptr(out), *self._ws_tail(dev, d.V, d.H, B))
        return out

    def gauss_ais(self, rbm, logvar, betas, n_chains: int, rng, base_vis_bias: Optional[torch.Tensor] = None, return_state: bool = False):
        """Annealed importance sampling over Gaussian visibles (imdbn_rbm_gauss_ais): ``n_chains`` chains from the
        base-rate model (no weights, the variances of ``logvar``, visible bias ``base_vis_bias``; None = the RBM's own ``vis_bias``,
        not zeros) to ``rbm`` through the temperatures ``betas`` (0 = betas[0] < ... < betas[K] = 1).  Returns the log importance
        weights, a float64 device tensor ``[n_chains]`` (and the final states ``[n_chains, V]`` with ``return_state``);
        log Z ~= H log 2 + (V / 2) log 2 pi + sum(logvar) / 2 + logmeanexp(logw).  No host sync."""
        d = self._desc(rbm, False)
        dev = rbm.W.device
        z = self._logvar("gauss_ais: logvar", logvar, d.V, dev)
        return self._anneal("gauss_ais", rbm, d, lambda K: R.sched_gauss_ais(d.V, d.H, K), n_chains, betas, rng, base_vis_bias,
                            return_state, logvar=z)

    def gauss_reverse_ais(self, rbm, logvar, v_rows, betas, rng, base_vis_bias: Optional[torch.Tensor] = None, return_state: bool = False):
        """Reverse annealed importance sampling over Gaussian visibles (imdbn_rbm_gauss_reverse_ais): one chain per
        row of ``v_rows`` ``[R, V]`` (real; the caller replicates a test row once per chain) runs the transitions of ``gauss_ais``
        backwards through ``betas``, T_K first.  Returns the per-chain log weights, a float64 device tensor ``[R]`` (and the final
        states u_1 ``[R, V]`` with ``return_state``): ``-log Z_A + logmeanexp`` over a test row's chains is a stochastic lower bound on
        the log-density log p_ann(row), log Z_A as ``gauss_ais`` states it.  ``base_vis_bias`` None = the RBM's own ``vis_bias``.  A
        row holding a non-finite element gets NaN.  No host sync."""
        d = self._desc(rbm, False)
        if not v_rows.is_cuda or v_rows.dim() != 2 or v_rows.size(1) != d.V:
            raise N.EngineError(f"gauss_reverse_ais needs a HIP tensor v_rows [R, {d.V}]")
        v = _f32c(v_rows)
        z = self._logvar("gauss_reverse_ais: logvar", logvar, d.V, v.device)
        return self._anneal("gauss_reverse_ais", rbm, d, lambda K: R.sched_gauss_reverse_ais(d.V, d.H, K), v.size(0), betas, rng,
                            base_vis_bias, return_state, v=v, logvar=z)

    def gauss_bound_step(self, rbm, logvar, v, rng, acc: Optional[torch.Tensor] = None, mode: str = "entropy"):
        """The bottom bracket of the DBN lower bound under a Gaussian visible layer (imdbn_rbm_gauss_bound_step):
        draws ``h ~ q(h | v) = Bernoulli(sigmoid(c + (v exp(-logvar)) W))`` and adds ``log N(v; b + h W^T, exp(logvar))`` plus the
        entropy of q (``mode="entropy"``) or ``-log q(h | v)`` (``mode="logq"``) to ``acc``, a float64 device tensor ``[M]`` (created
        zeroed when None).  Returns ``(acc, h)``, ``h`` fp32 0/1 ``[M, H]``: what ``bound_step`` of the layer above takes.  No host
        sync."""
        d = self._desc(rbm, False)
        v = _f32c(v)
        z = self._logvar("gauss_bound_step: logvar", logvar, d.V, v.device)
        return self._bound("gauss_bound_step", d, z, v, rng, acc, mode)

    def gauss_cd_step(self, rbm, logvar, logvar_m, data, lr, mom, cd_k, rng, lr_z, z_lo=float("-inf"), z_hi=float("inf"),
                      sample_v=True, monitor: bool = True):
        """One CD-``cd_k`` update of a Gaussian-visible RBM with learned variances (imdbn_rbm_gauss_cd_step):
        the parameters and momentum buffers of ``rbm`` and -- with ``lr_z != 0`` -- ``logvar`` / ``logvar_m`` ``[V]`` (fp32, updated
        in place, ``logvar`` clamped into ``[z_lo, z_hi]``).  ``sample_v``: the negative visible state is drawn from N(mean,
        sigma^2), else it is the mean.  Returns ``mean((data - mean_last)^2)`` as a 0-d device tensor, or None with
        ``monitor=False``.  No host sync."""
        d = self._desc(rbm, True)
        x = _f32c(data)
        B, dev = x.size(0), x.device
        z = self._logvar("gauss_cd_step: logvar", logvar, d.V, dev)
        zm = self._logvar("gauss_cd_step: logvar_m", logvar_m, d.V, dev)
        o = self._opts(rbm, lr, mom, cd_k, sparsity=getattr(rbm, "sparsity", False))
        loss = torch.empty(1, device=dev) if monitor else None
        need = int(self._lib.imdbn_gauss_scratch_floats(d.V, d.H, B))
        scratch = self._buffer(("gauss", dev, d.V, d.H, B, torch.cuda.current_stream(dev).cuda_stream),
                               lambda: torch.empty(need, dtype=torch.float32, device=dev), need)
        sched = R.sched_gauss_cd(d.V, d.H, o.cd_k, sample_v)
        r, keep = self._rng(rng, sched, B, dev)
        self._call("imdbn_rbm_gauss_cd_step", C.byref(d), _ptr(z), _ptr(zm), _ptr(x), x.stride(0), B, C.byref(o), float(lr_z), float(z_lo),
                   float(z_hi), int(bool(sample_v)), C.byref(r), _ptr(loss), _ptr(scratch), *self._ws_tail(dev, d.V, d.H, B))
        self._done(rng, r, sched)
        return loss.reshape(()) if monitor else None

    def pt_sweep(self, rbm, state, betas, n_sweeps: int, rng, swap_try: Optional[torch.Tensor] = None,
                 swap_acc: Optional[torch.Tensor] = None):
        """``n_sweeps`` parallel-tempering sweeps (imdbn_rbm_pt_sweep) over ``state`` ``[R M, V]`` (fp32 0/1, updated in place), R =
        ``len(betas)`` replicas of M chains, replica r in the rows ``[r M, (r + 1) M)`` at inverse temperature ``betas[r]``
        (0 < betas[0] < ... < betas[R - 1] = 1): per sweep one Gibbs step of every replica at its temperature, then the exchange
        between the neighbouring replicas of the sweep's parity.  Returns ``(swap_try, swap_acc)``, int64 device tensors
        ``[max(R - 1, 1)]`` the call ADDS its proposals and acceptances per pair to (created zeroed when None).  No host sync."""
        d = self._desc(rbm, False)
        x = self._chains("pt_sweep", state, d.V)
        b = [float(t) for t in (betas.tolist() if hasattr(betas, "tolist") else betas)]
        Rn, dev = len(b), x.device
        if Rn < 1 or x.size(0) % Rn != 0:
            raise N.EngineError(f"pt_sweep: {x.size(0)} rows do not divide into {Rn} replicas")
        M = x.size(0) // Rn
        arr = (C.c_float * Rn)(*b)
        cnt = []
        for nm, t in (("swap_try", swap_try), ("swap_acc", swap_acc)):
            if t is None:
                t = torch.zeros(max(Rn - 1, 1), dtype=torch.int64, device=dev)
            elif t.dtype != torch.int64 or t.device != dev or t.numel() != max(Rn - 1, 1) or not t.is_contiguous():
                raise N.EngineError(f"pt_sweep: {nm} must be a contiguous int64 [{max(Rn - 1, 1)}] tensor on {dev}")
            cnt.append(t)
        sched = R.sched_pt(d.V, d.H, self._groups(rbm), Rn, n_sweeps)
        r, keep = self._rng(rng, sched, Rn * M, dev)
        # the replicas' steps run on M rows, the exchange on all of them: one workspace that serves both layouts
        need = max(int(self._lib.imdbn_ws_bytes(d.V, d.H, Rn * M)), int(self._lib.imdbn_ws_bytes(d.V, d.H, M)))
        ws = self._buffer(("pt_sweep", dev, d.V, d.H, torch.cuda.current_stream(dev).cuda_stream),
                          lambda: torch.empty(need, dtype=torch.uint8, device=dev), need)
        self._call("imdbn_rbm_pt_sweep", C.byref(d), _ptr(x), x.stride(0), Rn, M, arr, int(n_sweeps), C.byref(r), _ptr(cnt[0]), _ptr(cnt[1]),
                   _ptr(ws), ws.numel(), self._stream(dev))
        self._done(rng, r, sched)
        return cnt[0], cnt[1]

    def assoc_update(self, rbm, vpos, hpos, vneg, hneg, lr, mom):
        """The weight / bias update alone (rbm.py:209-224) from the four phase tensors (imdbn_rbm_assoc_update)."""
        self._assoc(rbm, vpos, hpos, vneg, hneg, lr, mom, getattr(rbm, "sparsity", False))

    def _assoc(self, rbm, vpos, hpos, vneg, hneg, lr, mom, sparsity):
        d = self._desc(rbm, True)
        ts = [_f32c(t) for t in (vpos, hpos, vneg, hneg)]
        B, dev = ts[0].size(0), ts[0].device
        o = self._opts(rbm, lr, mom, 1, sparsity=sparsity)
        self._call("imdbn_rbm_assoc_update", C.byref(d), _ptr(ts[0]), ts[0].stride(0), _ptr(ts[1]), ts[1].stride(0), _ptr(ts[2]),
                   ts[2].stride(0), _ptr(ts[3]), ts[3].stride(0), B, C.byref(o), *self._ws_tail(dev, d.V, d.H, B))

    # ---- up-down fine-tuning of a stack ----------------------------------------------------------------
    def delta_step(self, rbm, direction, x, target, lr=0.0, mom=0.0, apply=True, rowlp=True):
        """One delta-rule step of the directed layer ``rbm`` (imdbn_rbm_delta_step): ``direction`` ``"up"`` (``x`` ``[B, V]``
        predicts ``target`` ``[B, H]`` through ``W`` and ``hid_bias``) or ``"down"`` (``x`` ``[B, H]`` predicts ``target`` ``[B, V]``
        through ``W^T`` and ``vis_bias``).  With ``apply`` the weights and the predicting bias move by ``lr``, ``mom`` and the RBM's
        weight decay (the other bias and its momentum are untouched); with ``rowlp`` the call returns ``log p(target | x)`` per row
        under the parameters on entry, a float64 device tensor ``[B]``, else None.  No draws, no host sync."""
        if direction not in ("up", "down"):
            raise N.EngineError(f"delta_step: direction must be 'up' or 'down', got {direction!r}")
        if not apply and not rowlp:
            raise N.EngineError("delta_step: apply=False and rowlp=False leave nothing to do")
        d = self._desc(rbm, bool(apply))
        up = direction == "up"
        n_in, n_out = (d.V, d.H) if up else (d.H, d.V)
        x, t = _f32c(x), _f32c(target)
        if x.dim() != 2 or t.dim() != 2 or x.size(1) != n_in or t.size(1) != n_out or x.size(0) != t.size(0) or x.device != t.device:
            raise N.EngineError(f"delta_step({direction}): needs x [B, {n_in}] and target [B, {n_out}] on one device")
        B, dev = x.size(0), x.device
        o = self._opts(rbm, lr, mom, 0) if apply else None
        lp = torch.empty(max(B, 1), dtype=torch.float64, device=dev) if rowlp else None
        self._call("imdbn_rbm_delta_step", C.byref(d), N.DELTA_UP if up else N.DELTA_DOWN, _ptr(x), x.stride(0), _ptr(t), t.stride(0), B,
                   _ref(o), _ptr(lp), *self._ws_tail(dev, d.V, d.H, max(B, 1)))
        return lp

    def updown_step(self, rec_layers, gen_layers, data, epoch_scalars, CD, particles, rng, monitor: bool = True):
        """One up-down (contrastive wake-sleep) step of a stack (Hinton, Osindero & Teh 2006): ``rec_layers`` the L RBMs bottom
        first (recognition weights of the directed layers, and the undirected top RBM), ``gen_layers`` the L - 1 generative twins.
        On one stream, no host sync: the wake pass up the recognition weights (``("u", H_l)`` per layer), ``pcd_step`` of the top
        RBM on the top wake state, the sleep pass down the generative weights from the particles after that call (``("u", V_l)``
        per layer, every sample drawn before any update), then the generative delta steps on the wake states and the recognition
        delta steps on the sleep states.  ``epoch_scalars``: ``(lr, mom)`` per layer; twin l uses entry l.  ``particles``: None (a
        fresh copy of the top wake state: CD-``CD`` from it), ``"persistent"`` (the top RBM's own chains, ``RBM._negative_chains``)
        or a ``[B, V_top]`` tensor advanced in place.  Returns ``{"wake": [s_1 ..], "sleep": [s'_0 ..], "particles", "wake_nll",
        "sleep_nll", "top_loss"}``; the three monitors are 0-d device scalars, None with ``monitor=False``."""
        from . import dp
        if dp.active():
            raise NotImplementedError("updown_step has no data-parallel split")
        L = len(rec_layers)
        if L < 1 or len(gen_layers) != L - 1 or len(epoch_scalars) != L:
            raise N.EngineError(f"updown_step: {L} layers need {max(L - 1, 0)} generative twins and {L} (lr, mom) pairs")
        top = rec_layers[-1]
        wake = [_f32c(data)]
        for rbm in rec_layers[:-1]:
            wake.append(self.prop_up(rbm, wake[-1], sample=True, rng=rng)[1])
        s_top = wake[-1]
        k = int(CD)
        if particles is None:
            particles = s_top.clone()
        elif isinstance(particles, str):
            particles, k = top._negative_chains(self, s_top, None, k, "updown_step")
        lr, mom = epoch_scalars[-1]
        top_loss = self.pcd_step(top, s_top, particles, lr, mom, k, rng, monitor=monitor)
        sleep = [particles]
        for g in reversed(gen_layers):
            sleep.insert(0, self.sample_visible(g, self.prop_down(g, sleep[0]), rng))
        lp_w = [self.delta_step(g, "down", wake[l + 1], wake[l], *epoch_scalars[l], rowlp=monitor) for l, g in enumerate(gen_layers)]
        lp_s = [self.delta_step(r, "up", sleep[l], sleep[l + 1], *epoch_scalars[l], rowlp=monitor) for l, r in enumerate(rec_layers[:-1])]
        out = {"wake": wake[1:], "sleep": sleep[:-1], "particles": particles, "wake_nll": None, "sleep_nll": None, "top_loss": top_loss}
        if monitor:
            zero = torch.zeros((), dtype=torch.float64, device=s_top.device)
            out["wake_nll"] = -torch.stack(lp_w).sum(0).mean() if lp_w else zero
            out["sleep_nll"] = -torch.stack(lp_s).sum(0).mean() if lp_s else zero
        return out

    # ---- backprop fine-tuning of the unrolled stack as a deep autoencoder -------------------------------
    def backprop_step(self, rbm, up=None, down=None, lr=0.0, mom=0.0, apply=True, want_v=False, want_h=False):
        """One back-propagation step through the sigmoid layer ``rbm`` (imdbn_rbm_backprop_step).  ``up`` = ``(x_v, e_h)``: the
        layer's input ``[B, V]`` in the upward direction and the error at its hidden pre-activations ``[B, H]``; ``down`` =
        ``(x_h, e_v)``: its input ``[B, H]`` in the downward direction and the error at its visible pre-activations ``[B, V]``.
        Errors are ascent directions.  Returns ``(err_v, err_h)``: ``(e_h W^T) x_v (1 - x_v)`` with ``want_v`` (needs ``up``) and
        ``(e_v W) x_h (1 - x_h)`` with ``want_h`` (needs ``down``), from the parameters on entry; a part not asked for is None.
        With ``apply`` the weights move along ``(x_v^T e_h + e_v^T x_h) / B`` and the bias of every pair present along its error's
        column mean, by ``lr``, ``mom`` and the RBM's weight decay.  No draws, no host sync."""
        if up is None and down is None:
            raise N.EngineError("backprop_step: needs an up pair, a down pair or both")
        if (want_v and up is None) or (want_h and down is None):
            raise N.EngineError("backprop_step: want_v needs the up pair, want_h the down pair")
        if not apply and not want_v and not want_h:
            raise N.EngineError("backprop_step: apply=False without want_v or want_h leaves nothing to do")
        d = self._desc(rbm, bool(apply))
        pairs = []
        for nm, pair, n_x, n_e in (("up", up, d.V, d.H), ("down", down, d.H, d.V)):
            if pair is None:
                pairs.append((None, None))
                continue
            x, e = _f32c(pair[0]), _f32c(pair[1])
            if x.dim() != 2 or e.dim() != 2 or x.size(1) != n_x or e.size(1) != n_e or x.size(0) != e.size(0) or x.device != e.device:
                raise N.EngineError(f"backprop_step: the {nm} pair needs x [B, {n_x}] and e [B, {n_e}] on one device")
            pairs.append((x, e))
        first = pairs[0][0] if pairs[0][0] is not None else pairs[1][0]
        B, dev = first.size(0), first.device
        if any(x is not None and (x.size(0) != B or x.device != dev) for x, _ in pairs):
            raise N.EngineError("backprop_step: the two pairs need the same rows on one device")
        o = self._opts(rbm, lr, mom, 0) if apply else None
        err_v = torch.empty(B, d.V, device=dev) if want_v else None
        err_h = torch.empty(B, d.H, device=dev) if want_h else None
        ld = lambda t: 0 if t is None else t.stride(0)
        (xv, eh), (xh, ev) = pairs
        self._call("imdbn_rbm_backprop_step", C.byref(d), _ptr(xv), ld(xv), _ptr(eh), ld(eh), _ptr(xh), ld(xh), _ptr(ev), ld(ev), B, _ref(o),
                   _ptr(err_v), ld(err_v), _ptr(err_h), ld(err_h), *self._ws_tail(dev, d.V, d.H, max(B, 1)))
        return err_v, err_h

    def autoencoder_step(self, rec_layers, gen_layers, data, epoch_scalars, monitor: bool = True):
        """One backprop step on the reconstruction cross-entropy of the stack unrolled into an encoder and a decoder (Hinton &
        Salakhutdinov 2006): ``rec_layers`` the L RBMs bottom first (the encoder; the top RBM is tied: its weights also open the
        decoder), ``gen_layers`` the L - 1 generative twins (the rest of the decoder).  On one stream, no host sync, no draws:
        ``a_0 = data``, ``a_l = forward`` of layer l; ``d_L = a_L`` and ``d_{l-1}`` the deterministic ``backward`` through the top
        RBM (l = L) or twin l - 1 -- ``d_0`` is ``iDBN.reconstruct(data)``, bit for bit; ``e_0 = data - d_0``.  Then down the
        decoder ``backprop_step(gen[l-1], down=(d_l, e_{l-1}))`` for l = 1 .. L - 1, the top RBM with both pairs
        ``up=(a_{L-1}, f_L), down=(a_L, e_{L-1})`` -- ``f_L`` from an evaluate-only call on the same parameters -- and
        ``backprop_step(rec[l-1], up=(a_{l-1}, f_l))`` for l = L - 1 .. 1.  ``epoch_scalars``: ``(lr, mom)`` per layer; twin l uses
        entry l.  Returns ``{"recon": d_0, "code": a_L, "xent", "mse"}``: ``xent`` is minus the batch mean of the rows'
        ``sum_j data_j z_j - softplus(z_j)`` on the decoder's output logits ``z`` in float64, ``mse`` the mean of ``e_0^2``; both
        0-d device scalars on the parameters on entry, None with ``monitor=False`` (nothing is then computed for them)."""
        from . import dp
        if dp.active():
            raise NotImplementedError("autoencoder_step has no data-parallel split")
        L = len(rec_layers)
        if L < 1 or len(gen_layers) != L - 1 or len(epoch_scalars) != L:
            raise N.EngineError(f"autoencoder_step: {L} layers need {max(L - 1, 0)} generative twins and {L} (lr, mom) pairs")
        top = rec_layers[-1]
        x = _f32c(data)
        a = [x]
        for rbm in rec_layers:
            cur = a[-1] if len(a) > 1 else data             # the caller's tensor carries the 0/1 tag, its fp32 form may be a copy
            out = self.forward(rbm, cur, data_binary=self.binary_hint(cur))
            out._imdbn_binary = False
            a.append(out)
        down = list(gen_layers) + [top]                     # the layer a top-down pass goes through below level l + 1
        dec = [None] * L + [a[L]]
        for l in range(L, 0, -1):
            dec[l - 1] = self.prop_down(down[l - 1], dec[l])
        xent = mse = None
        if monitor:                                         # before any update: the output layer's parameters on entry
            xent = -self.delta_step(down[0], "down", dec[1], x, apply=False).mean()
        e = x - dec[0]
        if monitor:
            mse = (e * e).mean()
        for l in range(1, L):
            e = self.backprop_step(gen_layers[l - 1], down=(dec[l], e), lr=epoch_scalars[l - 1][0], mom=epoch_scalars[l - 1][1], want_h=True)[1]
        lr, mom = epoch_scalars[L - 1]
        f = self.backprop_step(top, down=(a[L], e), apply=False, want_h=True)[1]
        f = self.backprop_step(top, up=(a[L - 1], f), down=(a[L], e), lr=lr, mom=mom, want_v=L > 1)[0]
        for l in range(L - 1, 0, -1):
            f = self.backprop_step(rec_layers[l - 1], up=(a[l - 1], f), lr=epoch_scalars[l - 1][0], mom=epoch_scalars[l - 1][1], want_v=l > 1)[0]
        return {"recon": dec[0], "code": a[L], "xent": xent, "mse": mse}

    # ---- backprop fine-tuning of a stack with a Gaussian bottom layer ------------------------------------
    def gauss_backprop_step(self, rbm, logvar, logvar_m, data, up=None, down=None, lr=0.0, mom=0.0, lr_z=0.0, z_lo=float("-inf"),
                            z_hi=float("inf"), apply=True, want_h=False, monitor=False):
        """One back-propagation step through the Gaussian visible layer ``rbm`` (imdbn_rbm_gauss_backprop_step).  ``data`` ``[B, V]``
        is the layer's real-valued input; ``up`` = ``e_h`` ``[B, H]``, the error at its hidden pre-activations (the layer as the
        encoder's input, operand ``data exp(-logvar)``); ``down`` = ``x_h`` ``[B, H]``, the layer's input in the downward direction
        (the layer as the decoder's output, mean ``m = vis_bias + x_h W^T``, error ``(data - m) exp(-logvar)``).  Returns
        ``(err_h, nll, mse)``: ``(e_0 W) x_h (1 - x_h)`` with ``want_h`` and, with ``monitor``, the Gaussian negative log-density
        ``J`` of ``data`` under the mean (without the ``log 2 pi / 2`` constant) and ``mean((data - m)^2)`` as 0-d device scalars --
        both need ``down``, all from the parameters on entry; a part not asked for is None.  With ``apply`` the weights move along
        ``(u^T e_h + e_0^T x_h) / B``, the bias of every pair present along its error's column mean, by ``lr``, ``mom`` and the RBM's
        weight decay, and -- with ``lr_z != 0`` -- ``logvar`` / ``logvar_m`` ``[V]`` (fp32, in place, ``logvar`` clamped into
        ``[z_lo, z_hi]``) by ``lr_z``.  No draws, no host sync."""
        if up is None and down is None:
            raise N.EngineError("gauss_backprop_step: needs an up pair, a down pair or both")
        if (want_h or monitor) and down is None:
            raise N.EngineError("gauss_backprop_step: want_h and monitor need the down pair")
        if not apply and not want_h and not monitor:
            raise N.EngineError("gauss_backprop_step: apply=False without want_h or monitor leaves nothing to do")
        d = self._desc(rbm, bool(apply))
        x = _f32c(data)
        if x.dim() != 2 or x.size(1) != d.V:
            raise N.EngineError(f"gauss_backprop_step: needs data [B, {d.V}]")
        B, dev = x.size(0), x.device
        z = self._logvar("gauss_backprop_step: logvar", logvar, d.V, dev)
        learn_z = bool(apply) and float(lr_z) != 0.0
        zm = self._logvar("gauss_backprop_step: logvar_m", logvar_m, d.V, dev) if learn_z else None
        ops = []
        for nm, t in (("up", up), ("down", down)):
            if t is not None:
                t = _f32c(t)
                if t.dim() != 2 or t.size(1) != d.H or t.size(0) != B or t.device != dev:
                    raise N.EngineError(f"gauss_backprop_step: the {nm} pair needs [{B}, {d.H}] rows on {dev}")
            ops.append(t)
        eh, xh = ops
        o = self._opts(rbm, lr, mom, 0) if apply else None
        err_h = torch.empty(B, d.H, device=dev) if want_h else None
        loss = torch.empty(2, device=dev) if monitor else None
        need = int(self._lib.imdbn_gauss_backprop_scratch_floats(d.V, d.H, B))
        scratch = self._buffer(("gauss_backprop", dev, d.V, d.H, B, torch.cuda.current_stream(dev).cuda_stream),
                               lambda: torch.empty(need, dtype=torch.float32, device=dev), need)
        ld = lambda t: 0 if t is None else t.stride(0)
        self._call("imdbn_rbm_gauss_backprop_step", C.byref(d), _ptr(z), _ptr(zm), _ptr(x), x.stride(0), _ptr(eh), ld(eh), _ptr(xh), ld(xh), B,
                   _ref(o), float(lr_z) if learn_z else 0.0, float(z_lo), float(z_hi), _ptr(err_h), ld(err_h), _ptr(loss), _ptr(scratch),
                   *self._ws_tail(dev, d.V, d.H, B))
        return err_h, (loss[0] if monitor else None), (loss[1] if monitor else None)

    def gauss_autoencoder_step(self, rec_layers, gen_layers, data, epoch_scalars, monitor: bool = True):
        """``autoencoder_step`` for a stack whose bottom layer is a ``GaussianRBM`` with linear-Gaussian visibles (Hinton &
        Salakhutdinov 2006): the loss is the Gaussian negative log-density ``J = mean_b sum_i (data - d_0)^2 exp(-zeta) / 2 + zeta / 2``
        of the data under the reconstruction ``d_0``, ``zeta`` the log-variance of the decoder's bottom layer (twin 0; with one layer
        the RBM's own ``logvar``, tied).  On one stream, no host sync, no draws: ``a_1 = gauss_forward`` of layer 0, ``a_l = forward``
        above; ``d_L = a_L``, ``d_{l-1}`` the deterministic ``backward`` through the top RBM or twin l - 1 and ``d_0 = gauss_backward``
        through twin 0 -- ``iDBN.reconstruct(data)``, bit for bit.  Then ``gauss_backprop_step(gen[0], down=d_1, want_h=True)`` (the
        output layer), the middle twins, the top RBM and the encoder as ``autoencoder_step`` runs them, and last
        ``gauss_backprop_step(rec[0], up=f_1)``.  With one layer: an evaluate-only call with ``want_h``, then one call with both
        pairs.  ``epoch_scalars``: ``(lr, mom)`` per layer, twin l uses entry l; every Gaussian layer learns its ``logvar`` with
        ``lr_sigma_mult`` times that ``lr`` inside its own clamps.  Returns ``{"recon": d_0, "code": a_L, "nll": J, "mse"}``, the
        monitors 0-d device scalars on the parameters on entry, None with ``monitor=False``."""
        from . import dp
        if dp.active():
            raise NotImplementedError("gauss_autoencoder_step has no data-parallel split")
        L = len(rec_layers)
        if L < 1 or len(gen_layers) != L - 1 or len(epoch_scalars) != L:
            raise N.EngineError(f"gauss_autoencoder_step: {L} layers need {max(L - 1, 0)} generative twins and {L} (lr, mom) pairs")
        top, enc = rec_layers[-1], rec_layers[0]
        out_layer = gen_layers[0] if L > 1 else enc
        x = _f32c(data)
        a = [x, self.gauss_forward(enc, enc._z(), x)]
        a[1]._imdbn_binary = False
        for rbm in rec_layers[1:]:
            out = self.forward(rbm, a[-1], data_binary=self.binary_hint(a[-1]))
            out._imdbn_binary = False
            a.append(out)
        down = list(gen_layers) + [top]
        dec = [None] * L + [a[L]]
        for l in range(L, 1, -1):
            dec[l - 1] = self.prop_down(down[l - 1], dec[l])
        dec[0] = self.gauss_backward(out_layer, out_layer._z(), dec[1])
        gz = lambda r, lr: dict(lr_z=r.lr_sigma_mult * lr, z_lo=r.logvar_min, z_hi=r.logvar_max)
        lr, mom = epoch_scalars[0]
        if L == 1:
            f, nll, mse = self.gauss_backprop_step(enc, enc._z(), enc._zm(), x, down=a[1], apply=False, want_h=True, monitor=monitor)
            self.gauss_backprop_step(enc, enc._z(), enc._zm(), x, up=f, down=a[1], lr=lr, mom=mom, **gz(enc, lr))
            return {"recon": dec[0], "code": a[1], "nll": nll, "mse": mse}
        e, nll, mse = self.gauss_backprop_step(out_layer, out_layer._z(), out_layer._zm(), x, down=dec[1], lr=lr, mom=mom, want_h=True,
                                               monitor=monitor, **gz(out_layer, lr))
        for l in range(2, L):
            e = self.backprop_step(gen_layers[l - 1], down=(dec[l], e), lr=epoch_scalars[l - 1][0], mom=epoch_scalars[l - 1][1], want_h=True)[1]
        f = self.backprop_step(top, down=(a[L], e), apply=False, want_h=True)[1]
        f = self.backprop_step(top, up=(a[L - 1], f), down=(a[L], e), lr=epoch_scalars[L - 1][0], mom=epoch_scalars[L - 1][1], want_v=True)[0]
        for l in range(L - 1, 1, -1):
            f = self.backprop_step(rec_layers[l - 1], up=(a[l - 1], f), lr=epoch_scalars[l - 1][0], mom=epoch_scalars[l - 1][1], want_v=True)[0]
        self.gauss_backprop_step(enc, enc._z(), enc._zm(), x, up=f, lr=lr, mom=mom, **gz(enc, lr))
        return {"recon": dec[0], "code": a[L], "nll": nll, "mse": mse}

    # ---- discriminative fine-tuning of a stack through the joint RBM's exact class posterior ------------
    def label_backprop_step(self, rbm, z: torch.Tensor, K: int, gt: torch.Tensor, lr: float = 0.0, mom: float = 0.0, apply: bool = True,
                            want_pred: bool = False):
        """``log p(gt | z)`` of the joint RBM ``rbm`` over ``[z (Dz) | labels (K)]`` as an output layer
        (imdbn_rbm_label_backprop_step).  Returns ``(logp, err_z, pred)``, all from the parameters on entry: ``logp`` the float64
        ``[N]`` of ``label_step`` (the same bits; NaN where ``gt`` is outside ``[0, K)``), ``err_z`` ``[N, Dz]`` =
        ``d log p / d z * z (1 - z)`` -- the ``e_h`` of ``backprop_step`` for the layer that produced ``z``; an exact zero row for an
        invalid label -- and, with ``want_pred``, ``pred`` int32 ``[N]`` = ``argmax_k`` of the class values (else None).  With
        ``apply`` the update of ``label_step`` (the same bits in all six tensors); without it no parameter is written.  No
        draws, no host sync."""
        d = self._desc(rbm, bool(apply))
        if not z.is_cuda or z.dim() != 2:
            raise N.EngineError("label_backprop_step needs a HIP tensor z [N, Dz]")
        z = _f32c(z)
        n, Dz = z.shape
        dev = z.device
        g = _on(gt, dev, torch.int32)
        if g is None or g.numel() != n:
            raise N.EngineError("label_backprop_step: gt must hold one label per row of z")
        K = int(K)
        o = self._opts(rbm, lr, mom, 0) if apply else None
        logp = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        pred = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if want_pred else None
        err = torch.empty(max(n, 1), Dz, device=dev)
        need = max(n, 1) * (max(K, 0) + 3 * d.H)
        scratch = self._buffer(("label_backprop_step", dev, torch.cuda.current_stream(dev).cuda_stream), lambda: _f32(dev, need), need)
        self._call("imdbn_rbm_label_backprop_step", C.byref(d), _ptr(z), z.stride(0), n, Dz, K, _ptr(g), _ref(o), _ptr(logp), _ptr(pred),
                   _ptr(err), err.stride(0), _ptr(scratch), *self._ws_tail(dev, Dz, d.H, max(n, 1)))
        return logp, err, pred

    def discriminative_step(self, layers, joint, data, K, gt, epoch_scalars, head_scalars, train_head: bool = True, monitor: bool = True):
        """One backprop step on ``-mean log p(gt | data)`` of a stack read as a classifier (Hinton & Salakhutdinov 2006; Larochelle
        & Bengio 2008): ``layers`` the L RBMs of the image stack bottom first (their recognition half: ``W`` and ``hid_bias``),
        ``joint`` the joint RBM over ``[code | K labels]`` whose exact class posterior is the output layer.  On one stream, no host
        sync, no draws: ``a_0 = data``, ``a_l = forward`` of layer l; ``label_backprop_step(joint, a_L)`` (with ``train_head`` the
        step of ``label_step`` at ``head_scalars = (lr, mom)``, else the head is frozen) gives ``f_L``; then
        ``backprop_step(layers[l-1], up=(a_{l-1}, f_l), want_v=l > 1)`` for l = L .. 1 with ``epoch_scalars[l-1] = (lr, mom)``.
        Returns ``{"code": a_L, "nll", "acc"}``: ``nll = -nanmean(logp)`` (float64) and ``acc`` the share of the rows with a valid
        label whose argmax class is the label, 0-d device scalars on the parameters on entry; None with ``monitor=False``.  Only
        ``layers`` and ``joint`` are written: no generative twin is read or touched."""
        from . import dp
        if dp.active():
            raise NotImplementedError("discriminative_step has no data-parallel split")
        L = len(layers)
        if L < 1 or len(epoch_scalars) != L:
            raise N.EngineError(f"discriminative_step: {L} layers need {L} (lr, mom) pairs")
        a = [_f32c(data)]
        for rbm in layers:
            cur = a[-1] if len(a) > 1 else data             # the caller's tensor carries the 0/1 tag, its fp32 form may be a copy
            out = self.forward(rbm, cur, data_binary=self.binary_hint(cur))
            out._imdbn_binary = False
            a.append(out)
        g = _on(gt, a[L].device, torch.int32)
        lr, mom = head_scalars
        logp, f, pred = self.label_backprop_step(joint, a[L], K, g, lr, mom, apply=bool(train_head), want_pred=bool(monitor))
        nll = acc = None
        if monitor:
            ok = (g >= 0) & (g < int(K))
            nll = -torch.nanmean(logp)
            acc = ((pred == g) & ok).sum().double() / ok.sum().double()
        for l in range(L, 0, -1):
            f = self.backprop_step(layers[l - 1], up=(a[l - 1], f), lr=epoch_scalars[l - 1][0], mom=epoch_scalars[l - 1][1], want_v=l > 1)[0]
        return {"code": a[L], "nll": nll, "acc": acc}

    # ---- RCCL through the C ABI (a binder without torch.distributed; the classes use torch.distributed) ---------------
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self._call("imdbn_comm_unique_id", buf)
        return buf.raw

    def comm_init(self, world: int, rank: int, uid: bytes):
        comm = C.c_void_p(0)
        self._call("imdbn_comm_init", C.byref(comm), int(world), int(rank), C.create_string_buffer(uid, 128))
        return comm

    def comm_destroy(self, comm):
        self._call("imdbn_comm_destroy", comm)

    def comm_allreduce_sum(self, comm, t: torch.Tensor):
        assert t.dtype == torch.float32 and t.is_contiguous()
        self._call("imdbn_allreduce_sum_f32", comm, _ptr(t), t.numel(), self._stream(t.device))
        return t

    def comm_allgather(self, comm, send: torch.Tensor, recv: torch.Tensor):
        assert send.is_contiguous() and recv.is_contiguous() and recv.numel() * recv.element_size() % (send.numel() * send.element_size()) == 0
        self._call("imdbn_allgather_bytes", comm, _ptr(send), _ptr(recv), send.numel() * send.element_size(), self._stream(send.device))
        return recv

    def packed_floats(self, V, H) -> int:
        return int(self._lib.imdbn_packed_delta_floats(V, H))

    def packed_buffer(self, rbm) -> torch.Tensor:
        """Reusable all-reduce buffer for this RBM's shape (every entry but the <=3 pad floats is rewritten by
        cd_stats, so no per-step zeroing)."""
        W = rbm.W.data
        V, H = W.shape
        return self._buffer(("packed", W.device, V, H), lambda: torch.zeros(self.packed_floats(V, H), device=W.device))

    def cd_stats(self, rbm, data, cd_k, rng, out: Optional[torch.Tensor] = None, data_binary=None, next_data=None):
        """The shard's packed statistics (data-parallel all-reduce exchange); ``next_data``: the next-batch hint of ``cd_step``."""
        d = self._desc(rbm, True)       # (imdbn_rbm_prefetch_ok wants the full descriptor)
        packed = out if out is not None else torch.zeros(self.packed_floats(d.V, d.H), device=data.device)
        self._cd("imdbn_rbm_cd_stats", rbm, d, data, self._opts(rbm, 0.0, 0.0, cd_k), rng, data_binary, _ptr(packed), next_data=next_data)
        return packed

    # ---- data-parallel factor exchange (include/imdbn_engine.h) --------------------------------------
    def factor_block(self, V, H, B):
        """(offset, bytes) of the factor block inside the workspace of an (V, H, B) call."""
        off, nb = C.c_size_t(0), C.c_size_t(0)
        self._call("imdbn_factor_block", int(V), int(H), int(B), C.byref(off), C.byref(nb))
        return int(off.value), int(nb.value)

    def factor_mode_ok(self, rbm, B) -> bool:
        W = rbm.W.data
        return (W.is_cuda and 1 <= B <= 64 and W.shape[1] % 4 == 0 and W.stride(0) % 4 == 0 and W.data_ptr() % 16 == 0
                and not self._groups(rbm))

    def cd_factors(self, rbm, data, cd_k, rng, data_binary=None) -> torch.Tensor:
        """The CD pass of this rank's rows; returns the factor block (a uint8 VIEW of the workspace: consume it --
        e.g. all-gather it -- before the next engine call on this RBM shape)."""
        d = self._desc(rbm, False)
        B, dev = data.size(0), data.device
        self._cd("imdbn_rbm_cd_factors", rbm, d, data, self._opts(rbm, 0.0, 0.0, cd_k), rng, data_binary, prefetch=False)
        off, nb = self.factor_block(d.V, d.H, B)
        return self._workspace(dev, d.V, d.H, B)[off:off + nb]

    def cd_factors_wire(self, rbm, data, cd_k, rng, binary: bool, next_data=None, data_binary=None) -> torch.Tensor:
        """The CD pass of this rank's rows straight into the wire form of its factor block (imdbn_rbm_cd_factors_wire =
        cd_factors + pack_factors in one call), with the next-batch hint of ``cd_step``.  Returns a reusable buffer."""
        d = self._desc(rbm, True)       # (imdbn_rbm_prefetch_ok wants the full descriptor)
        out = self._wire_buffer("wire1", rbm, data.size(0), 1, binary)[0]
        self._cd("imdbn_rbm_cd_factors_wire", rbm, d, data, self._opts(rbm, 0.0, 0.0, cd_k), rng, data_binary,
                 int(bool(binary)), _ptr(out), next_data=next_data)
        return out

    def _apply(self, name: str, rbm, dev, lr, mom, sparsity, *args):
        """The update behind the apply_* methods: entry `name`(desc, *args, opts, loss, stream); returns the 0-d loss.
        ``sparsity`` None: the RBM's own setting."""
        d = self._desc(rbm, True)
        o = self._opts(rbm, lr, mom, 1, sparsity=getattr(rbm, "sparsity", False) if sparsity is None else sparsity)
        loss = torch.empty(1, device=dev)
        self._call(name, C.byref(d), *args, C.byref(o), _ptr(loss), self._stream(dev))
        return loss.reshape(())

    def apply_wire(self, rbm, wires: torch.Tensor, rows_per_rank, global_B, binary: bool, lr, mom):
        """The update from the gathered wire blocks (imdbn_rbm_apply_wire = unpack_factors(planes_only) + apply_factors_wire)."""
        world = int(wires.size(0))
        assert wires.dtype == torch.uint8 and wires.dim() == 2 and wires.is_contiguous()
        planes = self.gather_buffer(rbm, rows_per_rank, world)
        return self._apply("imdbn_rbm_apply_wire", rbm, wires.device, lr, mom, None, _ptr(wires), int(wires.stride(0)), world,
                           int(rows_per_rank), int(global_B), int(bool(binary)), _ptr(planes), int(planes.stride(0)))

    def gather_buffer(self, rbm, B, world) -> torch.Tensor:
        """Reusable [world, block bytes] uint8 buffer for the all-gather of the factor blocks."""
        W = rbm.W.data
        _, nb = self.factor_block(W.shape[0], W.shape[1], B)
        return self._buffer(("gather", W.device, W.shape[0], W.shape[1], B, world),
                            lambda: torch.empty(world, nb, dtype=torch.uint8, device=W.device))

    # wire form of the factor block (include/imdbn_engine.h): bit-packed visible planes
    def compact_bytes(self, V, H, B, binary: bool) -> int:
        nb = C.c_size_t(0)
        self._call("imdbn_factor_compact_bytes", int(V), int(H), int(B), int(bool(binary)), C.byref(nb))
        return int(nb.value)

    def _wire_buffer(self, tag, rbm, B, world, binary) -> torch.Tensor:
        W = rbm.W.data
        V, H = W.shape
        # zeros: the block trailer's `bad` mark must not match a pack epoch by accident (include/imdbn_engine.h)
        return self._buffer((tag, W.device, V, H, B, world, bool(binary)),
                            lambda: torch.zeros(world, self.compact_bytes(V, H, B, binary), dtype=torch.uint8, device=W.device))

    def pack_factors(self, rbm, block: torch.Tensor, B, binary: bool) -> torch.Tensor:
        """This rank's factor block -> its compact wire form (a reusable buffer)."""
        W = rbm.W.data
        out = self._wire_buffer("wire1", rbm, B, 1, binary)[0]
        self._call("imdbn_rbm_pack_factors", int(W.shape[0]), int(W.shape[1]), int(B), int(bool(binary)), _ptr(block), _ptr(out),
                   self._stream(W.device))
        return out

    def compact_gather_buffer(self, rbm, B, world, binary: bool) -> torch.Tensor:
        return self._wire_buffer("wireN", rbm, B, world, binary)

    def unpack_factors(self, rbm, compact: torch.Tensor, B, binary: bool, planes_only: bool = False) -> torch.Tensor:
        """[world, compact bytes] gathered wire blocks -> [world, block bytes] full blocks for apply_factors
        (``planes_only``: just the visible planes, for apply_factors_wire)."""
        W = rbm.W.data
        world = int(compact.size(0))
        full = self.gather_buffer(rbm, B, world)
        assert compact.dtype == torch.uint8 and compact.dim() == 2 and compact.is_contiguous()
        self._call("imdbn_rbm_unpack_factors", int(W.shape[0]), int(W.shape[1]), int(B), int(bool(binary)), _ptr(compact),
                   int(compact.stride(0)), world, _ptr(full), int(full.stride(0)), int(bool(planes_only)), self._stream(W.device))
        return full

    def apply_factors_wire(self, rbm, wires: torch.Tensor, planes: torch.Tensor, rows_per_rank, global_B, lr, mom):
        """apply_factors with the blocks' head read from the gathered wire blocks and the visible planes from `planes`."""
        return self._apply("imdbn_rbm_apply_factors_wire", rbm, wires.device, lr, mom, None, _ptr(wires), int(wires.stride(0)),
                           _ptr(planes), int(planes.stride(0)), int(wires.size(0)), int(rows_per_rank), int(global_B))

    def apply_factors(self, rbm, gathered, rows_per_rank, global_B, lr, mom):
        assert gathered.dtype == torch.uint8 and gathered.dim() == 2 and gathered.is_contiguous()
        return self._apply("imdbn_rbm_apply_factors", rbm, gathered.device, lr, mom, None, _ptr(gathered), int(gathered.size(0)),
                           int(gathered.stride(0)), int(rows_per_rank), int(global_B))

    def apply_delta(self, rbm, packed, global_B, lr, mom, sparsity: Optional[bool] = None):
        return self._apply("imdbn_rbm_apply_delta", rbm, packed.device, lr, mom, sparsity, _ptr(packed), int(global_B))

    # ---- chains -------------------------------------------------------------------------------
    def chain(self, rbm, v_known, mask, steps: List[dict], rng, init_uniform=True, mu=None):
        d = self._desc(rbm, False)
        vk, km = self._clamped(v_known, mask)
        B, dev = vk.size(0), vk.device
        out = torch.empty(B, d.V, device=dev)
        sched = R.sched_chain(d.V, d.H, self._groups(rbm), steps, init_uniform)
        r, keep = self._rng(rng, sched, B, dev)
        mu_t, mu_args = self._mu(mu)
        self._call("imdbn_rbm_chain", C.byref(d), _ptr(vk), _ptr(km), vk.stride(0), B, int(bool(init_uniform)), len(steps),
                   self._steps(steps), *mu_args, C.byref(r), _ptr(out), out.stride(0), *self._ws_tail(dev, d.V, d.H, B))
        self._done(rng, r, sched)
        return out

    def _chain_specs(self, who: str, rbm, d, chains, traced: bool):
        """Chain dicts ``dict(v_known, mask, steps, init_uniform=True, mu=None, trace=None, trace_h=None)`` (None after the first: no
        such chain) -> ``(B, dev, specs, traces, results, sched, keep, hidden)``: per chain its N.ChainSpec and N.ChainTrace (None unless
        `traced` and the dict has a ``trace``) and ``(final_v, trace tensor or None)``; the schedules concatenated in chain order (ONE rng
        per engine call); `keep` holds everything the structs point into and must live until the C call has returned; `hidden` = per
        chain ``(N.ChainTrace, [steps, B, c1 - c0] tensor)`` of its ``trace_h=(c0, c1)`` window, ``(None, None)`` without one."""
        specs, traces, results, sched, keep, hidden = [], [], [], [], [], []
        B = dev = None
        for ch in chains:
            if ch is None:
                specs.append(None); traces.append(None); hidden.append((None, None)); continue
            vk, km = self._clamped(ch["v_known"], ch["mask"])
            if B is None:
                B, dev = vk.size(0), vk.device
            elif vk.size(0) != B:
                raise N.EngineError(f"{who}: the two chains need the same batch size")
            steps, init_uniform = ch["steps"], bool(ch.get("init_uniform", True))
            out = torch.empty(B, d.V, device=dev)
            mu_t, mu_args = self._mu(ch.get("mu"))
            arr = self._steps(steps)
            sp = N.ChainSpec()
            sp.v_known, sp.mask, sp.ldk = vk.data_ptr(), km.data_ptr(), vk.stride(0)
            sp.init_uniform, sp.n_steps, sp.steps = int(init_uniform), len(steps), arr
            sp.mu, sp.ldmu, sp.Dz = mu_args
            sp.out_v, sp.ldo = out.data_ptr(), out.stride(0)
            tr, tt = None, None
            if traced and ch.get("trace") is not None:
                c0, c1, base = (int(x) for x in ch["trace"])
                tr = torch.empty(len(steps) + (1 if base else 0), B, c1 - c0, device=dev)
                tt = N.ChainTrace()
                tt.c0, tt.c1, tt.with_baseline = c0, c1, 1 if base else 0
                tt.out, tt.ld_row, tt.step_stride = tr.data_ptr(), tr.stride(1), tr.stride(0)
            hr, ht = None, None
            if traced and ch.get("trace_h") is not None:
                c0, c1 = (int(x) for x in ch["trace_h"])
                hr = torch.empty(len(steps), B, max(c1 - c0, 0), device=dev)
                ht = N.ChainTrace()
                ht.c0, ht.c1, ht.with_baseline = c0, c1, 0
                ht.out, ht.ld_row, ht.step_stride = hr.data_ptr(), hr.stride(1), hr.stride(0)
            specs.append(sp); traces.append(tt); results.append((out, tr)); keep.append((vk, km, mu_t, arr)); hidden.append((ht, hr))
            sched += R.sched_chain(d.V, d.H, self._groups(rbm), steps, init_uniform)
        return B, dev, specs, traces, results, sched, keep, hidden

    def chain_pair(self, rbm, a: dict, b: dict, rng):
        """Two independent chains of `rbm` on batches of the same size as one engine call (imdbn_rbm_chain_pair); each of `a`, `b` =
        dict(v_known, mask, steps, init_uniform=True, mu=None).  Same draws, same results as ``chain(a)`` then ``chain(b)``."""
        d = self._desc(rbm, False)
        B, dev, specs, _, results, sched, keep, _ = self._chain_specs("chain_pair", rbm, d, (a, b), False)
        r, keep_r = self._rng(rng, sched, B, dev)
        self._call("imdbn_rbm_chain_pair", C.byref(d), B, C.byref(specs[0]), C.byref(specs[1]), C.byref(r), *self._ws_tail(dev, d.V, d.H, B))
        self._done(rng, r, sched)
        return results[0][0], results[1][0]

    def chain_traced(self, rbm, a: dict, b: Optional[dict], rng):
        """``chain(a)`` (b None) or ``chain_pair(a, b)`` recording, per step, p(v|h) of a column window (imdbn_rbm_chain_traced).  Each
        chain dict may carry ``trace=(c0, c1, with_baseline)``; returns one ``(final_v, trace)`` per chain, ``trace`` = ``[slots, B,
        c1 - c0]`` (slots = steps + with_baseline; slot 0 of a baseline = p(v | p(h | v0)) at T = 1) or None.  Same draws, same final
        states as the untraced calls."""
        d = self._desc(rbm, False)
        B, dev, specs, traces, results, sched, keep, _ = self._chain_specs("chain_traced", rbm, d, (a, b), True)
        r, keep_r = self._rng(rng, sched, B, dev)
        self._call("imdbn_rbm_chain_traced", C.byref(d), B, _ref(specs[0]), _ref(traces[0]), _ref(specs[1]), _ref(traces[1]), C.byref(r),
                   *self._ws_tail(dev, d.V, d.H, B))
        self._done(rng, r, sched)
        return results

    def chain_traced_vh(self, rbm, a: dict, b: Optional[dict], rng):
        """``chain_traced`` that also records hidden probabilities (imdbn_rbm_chain_traced_vh).  Besides ``trace``, a chain dict may
        carry ``trace_h=(c0, c1)``, a window of HIDDEN columns; returns one ``(final_v, trace, trace_h)`` per chain, ``trace_h`` =
        ``[steps, B, c1 - c0]`` (slot t = p(h|v) of step t with that step's T and noise, before sampling; never a baseline slot) or
        None.  Same draws, same final states, same visible traces as ``chain_traced``."""
        d = self._desc(rbm, False)
        B, dev, specs, traces, results, sched, keep, hidden = self._chain_specs("chain_traced_vh", rbm, d, (a, b), True)
        r, keep_r = self._rng(rng, sched, B, dev)
        self._call("imdbn_rbm_chain_traced_vh", C.byref(d), B, _ref(specs[0]), _ref(traces[0]), _ref(hidden[0][0]), _ref(specs[1]),
                   _ref(traces[1]), _ref(hidden[1][0]), C.byref(r), *self._ws_tail(dev, d.V, d.H, B))
        self._done(rng, r, sched)
        present = [h for sp, h in zip(specs, hidden) if sp is not None]
        return [(out, tr, hr) for (out, tr), (_, hr) in zip(results, present)]

    def label_scan(self, trace: torch.Tensor, gt: Optional[torch.Tensor], eps_l1: float, stable_steps: int, gap_thresh: float) -> dict:
        """IMG->TXT scan of a label trace ``[T + 1, B, K]`` (slot 0 = baseline): per-step ``[B, T]`` p_top1 / p_top2 / k1 / k2 / p_gt / l1
        and per-row ``steps`` (T + 1 = not converged) / ``pred`` (imdbn_trace_label_scan)."""
        S, B, K = trace.shape
        T = S - 1
        if trace.stride(2) != 1:
            trace = trace.contiguous()
        dev = trace.device
        o = {"p_top1": _f32(dev, B, T), "p_top2": _f32(dev, B, T), "k1": _i32(dev, B, T), "k2": _i32(dev, B, T),
             "p_gt": _f32(dev, B, T) if gt is not None else None, "l1": _f32(dev, B, T), "steps": _i32(dev, B), "pred": _i32(dev, B)}
        g = _on(gt, dev, torch.int32)
        self._call("imdbn_trace_label_scan", _ptr(trace), trace.stride(0), trace.stride(1), T, B, K, _ptr(g), float(eps_l1),
                   int(stable_steps), float(gap_thresh), _ptr(o["p_top1"]), _ptr(o["p_top2"]), _ptr(o["k1"]), _ptr(o["k2"]),
                   _ptr(o["p_gt"]), _ptr(o["l1"]), _ptr(o["steps"]), _ptr(o["pred"]), self._stream(dev))
        return o

    def code_scan(self, trace: torch.Tensor, z_init: torch.Tensor, ema_beta: float):
        """TXT->IMG code scan of a z trace ``[T, B, Dz]``: ``(z_new [T, B, Dz], dz [B, T])`` (imdbn_trace_code_scan)."""
        T, B, Dz = trace.shape
        if trace.stride(2) != 1:
            trace = trace.contiguous()
        z0 = _f32c(z_init)
        dev = trace.device
        zn, dz = _f32(dev, T, B, Dz), _f32(dev, B, T)
        self._call("imdbn_trace_code_scan", _ptr(trace), trace.stride(0), trace.stride(1), T, B, Dz, _ptr(z0), z0.stride(0),
                   float(ema_beta), _ptr(zn), _ptr(dz), self._stream(dev))
        return zn, dz

    def patience_scan(self, dz: torch.Tensor, mse: torch.Tensor, eps_z: float, mse_tol: float, patience: int):
        """TXT->IMG stop rule over ``dz``, ``mse`` ``[B, T]``: ``(steps [B] int32, best_mse [B])`` (imdbn_trace_patience_scan)."""
        dz, mse = dz.float().contiguous(), mse.float().contiguous()
        B, T = dz.shape
        dev = dz.device
        steps, best = _i32(dev, B), _f32(dev, B)
        self._call("imdbn_trace_patience_scan", _ptr(dz), _ptr(mse), T, B, float(eps_z), float(mse_tol), int(patience), _ptr(steps),
                   _ptr(best), self._stream(dev))
        return steps, best

    def decode_sqerr(self, idbn_layers, z: torch.Tensor, ref: torch.Tensor, ref_row: Optional[torch.Tensor] = None,
                     chunk: int = 1024) -> torch.Tensor:
        """``((decode(z) - ref[ref_row])**2).mean(1)`` without the decoded images: the layers above the bottom one decode with
        ``prop_down`` (RBM.backward), the bottom layer with imdbn_rbm_prop_down_sqerr.  Rows go in chunks of ``chunk``."""
        layers = list(idbn_layers)
        dev = layers[0].W.device
        z = z.to(device=dev, dtype=torch.float32)
        R_ = _f32c(ref.to(device=dev))
        n = z.size(0)
        rows = _on(ref_row, dev, torch.int32) if ref_row is not None else torch.arange(n, dtype=torch.int32, device=dev)
        out = torch.empty(n, device=dev)
        d = self._desc(layers[0], False)
        for s in range(0, n, int(chunk)):
            e = min(n, s + int(chunk))
            cur = z[s:e]
            for rbm in reversed(layers[1:]):
                cur = self.prop_down(rbm, cur)
            cur = _f32c(cur)
            B = e - s
            rr = rows[s:e]
            self._call("imdbn_rbm_prop_down_sqerr", C.byref(d), _ptr(cur), cur.stride(0), B, _ptr(R_), R_.stride(0), _ptr(rr),
                       _ptr(out[s:e]), *self._ws_tail(dev, d.V, d.H, B))
        return out

    def energy_trace(self, rbm, z: torch.Tensor, K: int, steps: int, gt: Optional[torch.Tensor] = None,
                     y_start: Optional[torch.Tensor] = None, eps_l1: float = 1e-3, stable_steps: int = 3, gap_thresh: float = 0.25,
                     want_y: bool = False) -> dict:
        """IMG->TXT energy trace of a panel of clamped codes ``z`` ``[N, Dz]`` on the joint RBM (imdbn_energy_trace): one K1
        propagation and one label kernel, no host sync.  Device tensors: per step ``[N, steps]`` ``p_top1, p_top2, p_gt`` (None
        without ``gt``), ``deltaF_pred, l1, k1``; per row ``steps`` (``steps + 1`` = not converged), ``kstar, predT, margin_energy,
        fe_top1, fe_gap``; ``F`` ``[N, K]``; ``y`` ``[N, K]`` after the last step when ``want_y``.  ``y_start`` None = uniform."""
        d = self._desc(rbm, False)
        if not z.is_cuda or z.dim() != 2:
            raise N.EngineError("energy_trace needs a HIP tensor z [N, Dz]")
        z = _f32c(z)
        n, Dz = z.shape
        dev = z.device
        K, T = int(K), int(steps)
        if n < 1 or T < 1:
            raise N.EngineError(f"energy_trace: N = {n}, steps = {T} (both must be >= 1)")
        o = {"p_top1": _f32(dev, n, T), "p_top2": _f32(dev, n, T), "p_gt": _f32(dev, n, T) if gt is not None else None,
             "deltaF_pred": _f32(dev, n, T), "l1": _f32(dev, n, T), "k1": _i32(dev, n, T), "steps": _i32(dev, n), "kstar": _i32(dev, n),
             "predT": _i32(dev, n), "margin_energy": _f32(dev, n), "fe_top1": _f32(dev, n), "fe_gap": _f32(dev, n),
             "F": _f32(dev, n, max(K, 1)), "y": _f32(dev, n, max(K, 1)) if want_y else None}
        g = _on(gt, dev, torch.int32)
        y0 = _f32c(y_start.to(dev)) if y_start is not None else None
        if (g is not None and g.numel() != n) or (y0 is not None and (y0.dim() != 2 or y0.size(0) != n or y0.size(1) != K)):
            raise N.EngineError("energy_trace: gt [N] and y_start [N, K] must match z")
        out = N.EnergyOut()
        alias = {"steps_to_converge": "steps", "y_final": "y"}      # the struct's field names are the dict's keys, but for these two
        for field, _ in N.EnergyOut._fields_:
            t = o[alias.get(field, field)]
            setattr(out, field, t.data_ptr() if t is not None else None)
        self._call("imdbn_energy_trace", C.byref(d), _ptr(z), z.stride(0), n, Dz, K, T, _ptr(g), _ptr(y0),
                   y0.stride(0) if y0 is not None else 0, float(eps_l1), int(stable_steps), float(gap_thresh), C.byref(out),
                   *self._ws_tail(dev, Dz, d.H, n))       # phase A is a (Dz, H, N) propagation: its workspace, not (V, H, N)
        return o

    def cross_metrics(self, p: torch.Tensor, y: Optional[torch.Tensor] = None, gt: Optional[torch.Tensor] = None,
                      row_mse: Optional[torch.Tensor] = None, npix: int = 1, topk: int = 3, acc: Optional[torch.Tensor] = None,
                      confusion: Optional[torch.Tensor] = None, class_sums: Optional[torch.Tensor] = None) -> dict:
        """Label metrics of ``p`` = p(y | img) ``[B, K]`` against the truth ``y`` ``[B, K]`` (first maximum per row) or ``gt`` ``[B]``
        (imdbn_cross_metrics): per row ``pred, gt, p_pred, p_true, rank``; ``acc`` ``[8]`` float64 (rows, top-1 hits, top-k hits,
        ce_sum, mse_sum = sum row_mse * npix, skipped rows), ``confusion`` ``[K, K]`` int64 (rows gt, columns pred), ``class_sums``
        ``[K, 3]`` float64 (rows, top-1 hits, sum of row_mse per true class).  The three accumulators are ADDED to: pass the ones a
        loop over batches shares, whatever is not passed is allocated as zeros.  ``p`` may be a column view of a wider tensor.
        Returns device tensors; no host sync."""
        if not p.is_cuda or p.dim() != 2:
            raise N.EngineError("cross_metrics needs a HIP tensor p [B, K]")
        p = _f32c(p)
        B, K = p.shape
        dev = p.device
        yt = _f32c(y.to(dev)) if y is not None else None
        g, rm = _on(gt, dev, torch.int32), _on(row_mse, dev, torch.float32)
        if (yt is not None and tuple(yt.shape) != (B, K)) or (g is not None and g.numel() != B) or (rm is not None and rm.numel() != B):
            raise N.EngineError("cross_metrics: y [B, K], gt [B] and row_mse [B] must match p")
        zeros = lambda shape, dt: torch.zeros(*shape, dtype=dt, device=dev)
        acc = zeros((8,), torch.float64) if acc is None else acc
        confusion = zeros((max(K, 1), max(K, 1)), torch.int64) if confusion is None else confusion
        class_sums = zeros((max(K, 1), 3), torch.float64) if class_sums is None else class_sums
        for t, shape, dt, nm in ((acc, (8,), torch.float64, "acc"), (confusion, (K, K), torch.int64, "confusion"),
                                 (class_sums, (K, 3), torch.float64, "class_sums")):
            if t.device != dev or t.dtype != dt or (K >= 2 and tuple(t.shape) != shape) or not t.is_contiguous():
                raise N.EngineError(f"cross_metrics: {nm} must be a contiguous {dt} tensor {list(shape)} on {dev}")
        o = {"pred": _i32(dev, B), "gt": _i32(dev, B), "p_pred": _f32(dev, B), "p_true": _f32(dev, B), "rank": _i32(dev, B),
             "acc": acc, "confusion": confusion, "class_sums": class_sums}
        out = N.CrossMetricsOut()
        for field, _ in N.CrossMetricsOut._fields_:
            setattr(out, field, o[field].data_ptr())
        need = (4 * B + 255) // 256 * 256 + (128 << 10)
        ws = self._buffer(("cross_metrics", dev, torch.cuda.current_stream(dev).cuda_stream),
                          lambda: torch.empty(need, dtype=torch.uint8, device=dev), at_least=need)
        self._call("imdbn_cross_metrics", _ptr(p), p.stride(0), B, K, _ptr(yt), yt.stride(0) if yt is not None else 0, _ptr(g), _ptr(rm),
                   int(npix), int(topk), C.byref(out), _ptr(ws), ws.numel(), self._stream(dev))
        return o

    # ---- unit moments (imdbn/utils/unit_tuning.py) --------------------------------------------------------------------------
    def unit_moments(self, act: torch.Tensor, cls: Optional[torch.Tensor] = None, n_classes: int = 0, x: Optional[torch.Tensor] = None,
                     acc: Optional[dict] = None) -> dict:
        """Sufficient statistics of the activations ``act`` ``[B, H]`` for per-unit tuning curves and regressions
        (imdbn_unit_moments): with ``cls`` ``[B]`` (a class in ``[0, n_classes)`` per row) ``cls_sum``, ``cls_sumsq`` ``[K, H]`` float64
        and ``cls_count`` ``[K]`` int64; with regressors ``x`` ``[B, R]`` (R <= 8) and z = [1, x]: ``xa`` ``[R + 1, H]`` = sum z a,
        ``aa`` ``[H]`` = sum a^2, ``xx`` ``[R + 1, R + 1]`` = sum z z^T, all float64; ``rows`` ``[2]`` int64 = rows used, rows skipped (a
        class outside the range or a non-finite regressor).  ``acc`` is an earlier result: it is ADDED to (a loop over the batches of
        a split leaves one result); without it the dict is allocated as zeros.  ``act`` may be a row view with ``stride(1) == 1``
        of a wider tensor; it is not copied.  Returns device tensors; no host sync."""
        if not act.is_cuda or act.dim() != 2:
            raise N.EngineError("unit_moments needs a HIP tensor act [B, H]")
        act = _f32c(act)
        B, H = act.shape
        dev = act.device
        K = int(n_classes) if cls is not None else 0
        c = _on(cls, dev, torch.int32)
        xt = None
        if x is not None:
            xt = _on(x.reshape(B, -1) if x.dim() != 2 else x, dev, torch.float32)
        R = 0 if xt is None else xt.size(1)
        if (c is not None and c.numel() != B) or (xt is not None and xt.size(0) != B):
            raise N.EngineError("unit_moments: cls [B] and x [B, R] must match act")
        if R == 0:
            xt = None
        shapes = {"cls_sum": ((K, H), torch.float64), "cls_sumsq": ((K, H), torch.float64), "cls_count": ((K,), torch.int64),
                  "xa": ((R + 1, H), torch.float64), "aa": ((H,), torch.float64), "xx": ((R + 1, R + 1), torch.float64),
                  "rows": ((2,), torch.int64)}
        if acc is None:
            acc = {k: torch.zeros(*shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
        for k, (shape, dt) in shapes.items():
            t = acc.get(k)
            if t is None or t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise N.EngineError(f"unit_moments: acc[{k!r}] must be a contiguous {dt} tensor {list(shape)} on {dev}")
        need = int(self._lib.imdbn_unit_moments_ws_bytes(B, H, K, R))
        ws = self._buffer(("unit_moments", dev, torch.cuda.current_stream(dev).cuda_stream),
                          lambda: torch.empty(need, dtype=torch.uint8, device=dev), at_least=need)
        self._call("imdbn_unit_moments", _ptr(act), act.stride(0), B, H, _ptr(c), K, _ptr(xt), R if xt is not None else 0, R,
                   _ptr(acc["cls_sum"]) if K else None, _ptr(acc["cls_sumsq"]) if K else None, _ptr(acc["cls_count"]) if K else None,
                   _ptr(acc["xa"]), _ptr(acc["aa"]), _ptr(acc["xx"]), _ptr(acc["rows"]), _ptr(ws), ws.numel(), self._stream(dev))
        return acc

    # ---- latent nearest-neighbour search (imdbn/utils/imdbn_logging.py) ----------------------------------------------------
    LATENT_METRICS ={"cosine": 0, "inner": 1, "ip": 1, "l2": 2}

    def row_stats(self, x: torch.Tensor) -> torch.Tensor:
        """``[N, 2]`` fp32 device tensor: per-row sum and sum of squares of ``x`` (rows flattened), in a fixed order
        (imdbn_row_stats; exact integers for 0/1 rows).  No host sync."""
        if not x.is_cuda:
            raise N.EngineError("row_stats needs a HIP tensor")
        x = _f32c(x.reshape(x.size(0), -1))
        n, d = x.shape
        out = torch.empty(2, n, device=x.device)
        self._call("imdbn_row_stats", _ptr(x), x.stride(0), n, d, _ptr(out[0]), _ptr(out[1]), self._stream(x.device))
        return out.t()

    def _topk_workspace(self, dev, N_: int, Q: int, k: int) -> torch.Tensor:
        """Workspace of imdbn_latent_topk: the header's minimum plus room for up to ceil(N / 64) bank chunks of about 2048
        blocks in all (fewer chunks: fewer blocks, the same result)."""
        A = lambda b: (int(b) + 255) // 256 * 256
        chunks = min(max(1, -(-2048 // -(-Q // 64))), -(-N_ // 64))
        need = A(4 * Q) + A(4 * N_) + chunks * 2 * A(4 * Q * k)
        return self._buffer(("topk", dev, torch.cuda.current_stream(dev).cuda_stream),
                            lambda: torch.empty(need, dtype=torch.uint8, device=dev), at_least=need)

    def latent_topk(self, bank: torch.Tensor, queries: torch.Tensor, metric, k: int, exclude: Optional[torch.Tensor] = None,
                    key: Optional[torch.Tensor] = None, bank_sumsq: Optional[torch.Tensor] = None):
        """Per query row the first ``k`` bank rows in rank order (imdbn_latent_topk): ``(idx [Q, k] int32, score [Q, k] fp32)``
        device tensors, padded with -1 / -inf.  ``metric``: 0 / "cosine", 1 / "inner" / "ip", 2 / "l2"; ``exclude`` [Q]
        (-1: none) removes one bank row per query; ``key`` [N, 2] keeps only the best-ranked row of every equal key pair;
        ``bank_sumsq`` [N] = ``row_stats(bank)[:, 1]`` (computed when None).  No host sync."""
        m = self.LATENT_METRICS[metric] if isinstance(metric, str) else int(metric)
        if not (bank.is_cuda and queries.is_cuda):
            raise N.EngineError("latent_topk needs HIP tensors")
        dev = bank.device
        B_ = _f32c(bank)
        Qt = _f32c(queries.to(dev))
        if B_.dim() != 2 or Qt.dim() != 2 or Qt.size(1) != B_.size(1):
            raise N.EngineError(f"latent_topk: bank {tuple(B_.shape)} and queries {tuple(Qt.shape)} must be [N, D] and [Q, D]")
        n, d = B_.shape
        q = Qt.size(0)
        k = int(k)
        ex, ky, bss = _on(exclude, dev, torch.int32), _on(key, dev, torch.float32), _on(bank_sumsq, dev, torch.float32)
        if (ex is not None and ex.numel() != q) or (ky is not None and ky.shape != (n, 2)) or (bss is not None and bss.numel() != n):
            raise N.EngineError("latent_topk: exclude [Q], key [N, 2] and bank_sumsq [N] must match the bank and queries")
        idx, sc = _i32(dev, q, max(k, 1)), _f32(dev, q, max(k, 1))
        ws = self._topk_workspace(dev, n, q, max(1, min(k, 64)))
        self._call("imdbn_latent_topk", _ptr(B_), B_.stride(0), n, d, _ptr(bss), _ptr(Qt), Qt.stride(0), q, m, k, _ptr(ex), _ptr(ky),
                   _ptr(idx), _ptr(sc), _ptr(ws), ws.numel(), self._stream(dev))
        return idx, sc

    # ---- pairwise free-energy scores (imdbn/utils/retrieval.py) -------------------------------------------------------------
    def pair_scores(self, rbm, z1: torch.Tensor, z2: torch.Tensor, gt_q: Optional[torch.Tensor] = None,
                    gt_n: Optional[torch.Tensor] = None, k: int = 0, return_scores: bool = False) -> dict:
        """Every query ``z1`` ``[Q, D1]`` against every candidate ``z2`` ``[N, D2]`` under the joint RBM ``rbm`` over
        ``[z1 | z2]`` (imdbn_rbm_pair_scores): ``S[q, n] = -F([z1_q | z2_n])``.  With ``gt_q`` ``[Q]``: ``rank_q`` (int32, the 0-based
        place of candidate ``gt_q[q]`` in a stable descending sort of row q; -1 for an entry outside ``[0, N)``) and ``score_q``
        (``S[q, gt_q[q]]``, NaN there); with ``gt_n`` ``[N]``: ``rank_n`` / ``score_n`` over the columns; with ``k > 0``: ``top_idx`` /
        ``top_score`` ``[Q, k]`` padded with -1 / -inf; with ``return_scores``: ``scores`` ``[Q, N]``.  Device tensors, no host sync."""
        d = self._desc(rbm, False)
        if not (z1.is_cuda and z2.is_cuda) or z1.dim() != 2 or z2.dim() != 2 or z1.size(1) < 1 or z1.size(1) + z2.size(1) != d.V:
            raise N.EngineError(f"pair_scores needs HIP tensors z1 [Q, D1] and z2 [N, D2] with D1 + D2 = {d.V}")
        dev = z1.device
        z1, z2 = _f32c(z1), _f32c(z2.to(dev))
        (Q, D1), n = z1.shape, z2.size(0)
        k = int(k)
        gq, gn = _on(gt_q, dev, torch.int32), _on(gt_n, dev, torch.int32)
        if (gq is not None and gq.numel() != Q) or (gn is not None and gn.numel() != n):
            raise N.EngineError("pair_scores: gt_q [Q] and gt_n [N] must match z1 and z2")
        o = {}
        if gq is not None:
            o["rank_q"], o["score_q"] = _i32(dev, max(Q, 1)), _f32(dev, max(Q, 1))
        if gn is not None:
            o["rank_n"], o["score_n"] = _i32(dev, max(n, 1)), _f32(dev, max(n, 1))
        if k > 0:
            o["top_idx"], o["top_score"] = _i32(dev, max(Q, 1), k), _f32(dev, max(Q, 1), k)
        if return_scores:
            o["scores"] = _f32(dev, max(Q, 1), max(n, 1))
        out = N.PairOut()
        for name, t in o.items():
            setattr(out, name, t.data_ptr())
        out.lds = max(n, 1)
        # the header's minimum plus room for the candidate chunks of about 2048 blocks (fewer chunks: fewer blocks, the same result)
        A = lambda b: (int(b) + 255) // 256 * 256
        kk = min(max(k, 0), 64)
        chunks = min(max(1, -(-2048 // -(-max(Q, 1) // 64))), -(-max(n, 1) // 64))
        need = int(self._lib.imdbn_pair_ws_bytes(d.V, d.H, max(Q, 1), max(n, 1), kk)) + (chunks - 1) * (A(4 * Q) + (2 * A(4 * Q * kk) if kk else 0))
        ws = self._buffer(("pair", dev, torch.cuda.current_stream(dev).cuda_stream),
                          lambda: torch.empty(need, dtype=torch.uint8, device=dev), at_least=need)
        self._call("imdbn_rbm_pair_scores", C.byref(d), D1, _ptr(z1), z1.stride(0), Q, _ptr(z2), z2.stride(0), n, _ptr(gq), _ptr(gn), k,
                   C.byref(out), _ptr(ws), ws.numel(), self._stream(dev))
        return o

    # ---- clamped CD (the joint RBM's update) ----------------------------------------------------------------------------
    def _clamped_cd(self, name: str, rbm, d, v_known, mask, init_steps, mu, o, sample_h, sample_v, rng, out: torch.Tensor):
        """clamped_step / clamped_stats: entry `name`(desc, v_known, mask, ld, B, init steps, mu, opts, rng, out, workspace tail)."""
        vk, km = self._clamped(v_known, mask)
        B, dev = vk.size(0), vk.device
        sched = R.sched_clamped(d.V, d.H, self._groups(rbm), init_steps, o.cd_k, sample_h, sample_v)
        r, keep = self._rng(rng, sched, B, dev)
        mu_t, mu_args = self._mu(mu)
        self._call(name, C.byref(d), _ptr(vk), _ptr(km), vk.stride(0), B, len(init_steps), self._steps(init_steps), *mu_args,
                   C.byref(o), C.byref(r), _ptr(out), *self._ws_tail(dev, d.V, d.H, B))
        self._done(rng, r, sched)

    def clamped_step(self, rbm, v_known, mask, init_steps: List[dict], mu, lr, mom, cd_k, sample_h, sample_v, reclamp, rng):
        d = self._desc(rbm, True)
        o = self._opts(rbm, lr, mom, cd_k, sparsity=False, sample_h=sample_h, sample_v=sample_v, reclamp=reclamp)
        loss = torch.empty(1, device=v_known.device)
        self._clamped_cd("imdbn_rbm_clamped_step", rbm, d, v_known, mask, init_steps, mu, o, sample_h, sample_v, rng, loss)
        return loss.reshape(())

    def clamped_stats(self, rbm, v_known, mask, init_steps: List[dict], mu, cd_k, sample_h, sample_v, reclamp, rng,
                      out: Optional[torch.Tensor] = None):
        """Data-parallel half of clamped_step: the shard's packed statistics (apply with apply_delta(sparsity=False))."""
        d = self._desc(rbm, False)
        o = self._opts(rbm, 0.0, 0.0, cd_k, sparsity=False, sample_h=sample_h, sample_v=sample_v, reclamp=reclamp)
        packed = out if out is not None else torch.zeros(self.packed_floats(d.V, d.H), device=v_known.device)
        self._clamped_cd("imdbn_rbm_clamped_stats", rbm, d, v_known, mask, init_steps, mu, o, sample_h, sample_v, rng, packed)
        return packed
