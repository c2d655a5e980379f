"""RBM with the reference's class surface, backed by the MI355X CD engine.

API mirror of the reference ``imdbn/models/rbm.py`` (same constructor, method names, keyword
defaults, attribute names and pickle state -- SURVEY.md 8b-1 / Appendix C), but every method body
is host-side scalar logic plus ONE call into the native engine (``imdbn.engine``): no ATen
arithmetic on the hot path.  Reference line numbers are cited per method.

Deliberate differences: random draws come from the engine's RNG source
(``imdbn.engine.get_rng()``: device Philox by default, recorded draws in the parity tests) instead
of torch's global generator; all returned tensors are grad-less.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from imdbn import engine as _E


def _row_pitch(h: int) -> int:
    """Row pitch in elements: H rounded up to 128 floats (512 B: the row segment one half-wave of the update kernel
    reads and writes) or else to 32 floats (128 B), whichever costs < 7 % extra memory."""
    forced = int(os.environ.get("IMDBN_ROW_PITCH_ABS", "0"))       # layout experiments: an absolute pitch (>= h, multiple of 4)
    if forced >= h and forced % 4 == 0:
        return forced
    for q in (int(os.environ.get("IMDBN_ROW_PITCH", "128")), 32):
        p = (h + q - 1) // q * q
        if (p - h) * 16 <= h:
            return p
    return h


def _step(T=1.0, sigma=0.0, eta=0.0, sample_h=False, vmode=0, clamp=True) -> dict:
    return {"T": float(T), "sigma": float(sigma), "eta": float(eta), "sample_h": bool(sample_h),
            "vmode": int(vmode), "clamp": bool(clamp)}


class RBM(nn.Module):
    """Bernoulli RBM with optional softmax groups on the visible layer (reference rbm.py:24-79)."""

    def __init__(
        self,
        num_visible: int,
        num_hidden: int,
        learning_rate: float,
        weight_decay: float,
        momentum: float,
        dynamic_lr: bool = False,
        final_momentum: float = 0.97,
        sparsity: bool = False,
        sparsity_factor: float = 0.05,
        softmax_groups: Optional[List[Tuple[int, int]]] = None,
    ):
        super().__init__()
        self.num_visible = int(num_visible)
        self.num_hidden = int(num_hidden)
        self.lr = float(learning_rate)
        self.weight_decay = float(weight_decay)
        self.momentum = float(momentum)
        self.dynamic_lr = bool(dynamic_lr)
        self.final_momentum = float(final_momentum)
        self.sparsity = bool(sparsity)
        self.sparsity_factor = float(sparsity_factor)
        self.softmax_groups = softmax_groups or []

        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")      # rbm.py:69
        # Same law as the reference (randn / sqrt(V), rbm.py:70-72).  On the GPU the rows of W and W_m are
        # allocated with a pitch padded to 128 B: shape, values and semantics are unchanged (W is a [V,H]
        # view with stride (pitch, 1)), but every 512-B row segment the kernels touch is cache-line aligned
        # (H = 1500 would otherwise straddle 5 lines instead of 4: ~25 % over-fetch, profiles/r01_pmc_*).
        pitch = _row_pitch(self.num_hidden) if device.type == "cuda" else self.num_hidden
        w_full = torch.randn(self.num_visible, pitch, device=device) / math.sqrt(max(1, self.num_visible))
        self.W = nn.Parameter(w_full[:, :self.num_hidden], requires_grad=False)
        self.hid_bias = nn.Parameter(torch.zeros(self.num_hidden, device=device), requires_grad=False)
        self.vis_bias = nn.Parameter(torch.zeros(self.num_visible, device=device), requires_grad=False)
        # momentum buffers: plain attributes, exactly as in the reference (rbm.py:77-79)
        self.W_m = torch.zeros(self.num_visible, pitch, device=device)[:, :self.num_hidden]
        self.hb_m = torch.zeros_like(self.hid_bias)
        self.vb_m = torch.zeros_like(self.vis_bias)

    # ---- pickle state ----------------------------------------------------
    def __getstate__(self):
        """The reference's plain attribute state.  On the GPU ``W`` / ``W_m`` are views of row-padded buffers; a pickle
        must not carry that storage: they are written as contiguous ``[V, H]`` tensors (stride ``(H, 1)``), exactly what
        the reference class -- or this one -- expects to unpickle."""
        state = self.__dict__.copy()
        state.pop("_imdbn_desc", None)                 # the engine's cached native descriptor (raw addresses): never part of the state
        # persistent chains, their swap counters and the centering offsets: a loaded model restarts its chains and re-initialises its offsets
        # (and the magnetisations of train_epoch_tap)
        for k in ("_pcd", "_pcd_replicas", "_pt_try", "_pt_acc", "_ctr_mu", "_ctr_lam", "_tap_mv", "_tap_mh"):
            state.pop(k, None)
        params = state["_parameters"].copy()
        W = params.get("W")
        if W is not None and not W.is_contiguous():
            params["W"] = nn.Parameter(W.data.contiguous(), requires_grad=W.requires_grad)
        state["_parameters"] = params
        Wm = state.get("W_m")
        if isinstance(Wm, torch.Tensor) and not Wm.is_contiguous():
            state["W_m"] = Wm.contiguous()
        return state

    # ---- helpers ------------------------------------------------------------------------------
    def _eng(self):
        return _E.get_engine(self.W.data)

    def _in(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(device=self.W.device, dtype=torch.float32)

    def _mu(self):
        mp = getattr(self, "_mu_pull", None)                                        # rbm.py:359
        if mp is None:
            return None, 0.0
        return self._in(mp["mu_k"]), float(mp.get("eta0", 0.15))

    def _lr_mom(self, epoch: int):
        lr = self.lr / (1 + 0.01 * epoch) if self.dynamic_lr else self.lr          # rbm.py:194
        mom = self.momentum if epoch <= 5 else self.final_momentum                  # rbm.py:195
        return lr, mom

    # ---- propagations (rbm.py:81-178) ---------------------------------------------------------
    @torch.no_grad()
    def forward(self, v: torch.Tensor, T: float = 1.0) -> torch.Tensor:
        """p(h|v) = sigmoid((v W + c)/max(1e-6,T))   (rbm.py:92)."""
        eng = self._eng()
        if T == 1.0:
            # the same path as the forward fused into train_epoch(return_forward=True): bit-identical results
            out = eng.forward(self, self._in(v), data_binary=eng.binary_hint(v))
        else:
            out = eng.prop_up(self, self._in(v), T=T)
        out._imdbn_binary = False      # probabilities: the next layer's update makes no bit plane of them (HipEngine.binary_hint)
        return out

    @torch.no_grad()
    def _visible_logits(self, h: torch.Tensor, T: float = 1.0) -> torch.Tensor:
        """(h W^T + b)/max(1e-6,T)   (rbm.py:96)."""
        return self._eng().prop_down(self, self._in(h), T=T, logits_only=True)

    @torch.no_grad()
    def visible_probs(self, h: torch.Tensor, T: float = 1.0) -> torch.Tensor:
        """p(v|h) with softmax over each group (rbm.py:109-116)."""
        return self._eng().prop_down(self, self._in(h), T=T)

    @torch.no_grad()
    def free_energy(self, v: torch.Tensor) -> torch.Tensor:
        """F(v) = -v.b - sum_j softplus(c_j + (vW)_j), shape [B] (imdbn/utils/energy_utils.py:19-28).

        The reference's ``RBM`` has no such method (``iMDBN._cross_reconstruct`` probes for it with ``hasattr``,
        imdbn.py:455, and falls back to zeros); here it exists and feeds the opt-in live best-of-K selection
        (``iMDBN.live_best_of_k``)."""
        return self._eng().free_energy(self, self._in(v))

    @torch.no_grad()
    def log_partition(self, **kw) -> dict:
        """AIS estimate of log Z (``imdbn.utils.likelihood.estimate_log_partition``; binary visibles, no softmax groups)."""
        from imdbn.utils.likelihood import estimate_log_partition
        return estimate_log_partition(self, **kw)

    def log_partition_exact(self, **kw) -> dict:
        """Exact log Z by on-device enumeration of the smaller side (``imdbn.utils.likelihood.exact_log_partition``; at most
        ``max_bits`` = 24 units there, softmax groups accepted)."""
        from imdbn.utils.likelihood import exact_log_partition
        return exact_log_partition(self, **kw)

    def exact_marginals(self, **kw):
        """``(vis_mean [V], hid_mean [H])``: the exact model marginals p(v_i = 1), p(h_j = 1) -- what a persistent or tempered
        particle cloud should reproduce (``imdbn.utils.likelihood.exact_log_partition(marginals=True)``)."""
        from imdbn.utils.likelihood import exact_log_partition
        res = exact_log_partition(self, marginals=True, **kw)
        return res["vis_mean"], res["hid_mean"]

    @torch.no_grad()
    def pseudo_log_likelihood(self, v: torch.Tensor, return_sites: bool = False):
        """Exact pseudo-log-likelihood sum_sites log p(v_site | v_rest) per row, float64 ``[B]``
        (``imdbn.utils.likelihood.pseudo_log_likelihood``; softmax groups accepted, no partition function, no draws)."""
        from imdbn.utils.likelihood import pseudo_log_likelihood
        return pseudo_log_likelihood(self, v, return_sites=return_sites)

    @torch.no_grad()
    def log_likelihood(self, v: torch.Tensor, log_z) -> torch.Tensor:
        """log p(v) = -F(v) - log Z per row, float64 ``[B]`` (``imdbn.utils.likelihood.log_likelihood``)."""
        from imdbn.utils.likelihood import log_likelihood
        return log_likelihood(self, v, log_z)

    @torch.no_grad()
    def log_likelihood_conservative(self, v: torch.Tensor, **kw) -> dict:
        """Reverse-AIS lower bound on log p(v) per row under the annealing model: ``{"ll", "ess", "logw"}``
        (``imdbn.utils.likelihood.reverse_ais_log_likelihood``; no AIS estimate of log Z enters)."""
        from imdbn.utils.likelihood import reverse_ais_log_likelihood
        return reverse_ais_log_likelihood(self, v, **kw)

    @torch.no_grad()
    def sample_visible(self, v_prob: torch.Tensor) -> torch.Tensor:
        """Bernoulli over all columns, one categorical per softmax group (rbm.py:125-135)."""
        return self._eng().sample_visible(self, self._in(v_prob), self._rng(v_prob.size(0)))

    @torch.no_grad()
    def backward(self, h: torch.Tensor, return_logits: bool = False) -> torch.Tensor:
        """Decoder alias of visible_probs at T=1 (rbm.py:148-151)."""
        if return_logits:
            return self._visible_logits(h)
        return self.visible_probs(h)

    @torch.no_grad()
    def backward_sample(self, h: torch.Tensor) -> torch.Tensor:
        """rbm.py:156."""
        return self.sample_visible(self.visible_probs(h))

    @torch.no_grad()
    def gibbs_step(self, v: torch.Tensor, sample_h: bool = True, sample_v: bool = True):
        """One v -> h -> v' step; returns (v_next, v_prob, h, h_prob)   (rbm.py:174-178)."""
        return self._eng().gibbs_step(self, self._in(v), sample_h, sample_v, self._rng(v.size(0)))

    def _rng(self, B: int):
        """The ambient draw source; under data parallelism Philox draws are keyed on the GLOBAL batch row
        (rank r owns rows [r*B, (r+1)*B)), so a sharded call equals the unsharded one."""
        rng = _E.get_rng()
        if _E.dp.active() and isinstance(rng, _E.PhiloxRng):
            rng.row0 = _E.dp.rank() * int(B)
        return rng

    # ---- CD-k update (rbm.py:180-227) -----------------------------------------------------------
    @torch.no_grad()
    def train_epoch(self, data: torch.Tensor, epoch: int, max_epochs: int, CD: int = 1,
                    next_data: Optional[torch.Tensor] = None, return_forward: bool = False):
        """One CD-k update on one mini-batch (the name is the reference's); returns the 0-d MSE loss.

        ``next_data`` (extension, optional): the batch the following ``train_epoch`` call will receive.  Its operand
        forms are prepared by extra blocks of one of this call's launches; hand that same tensor, unmodified, to the next
        call and it skips its own preparation (results are bit-identical either way; a modified, different or
        ineligible tensor is simply prepared again).

        ``return_forward`` (extension): return ``(loss, self.forward(data))`` -- the pair of calls of the layer loop
        (idbn.py:195-204) -- with the forward pass run inside the same engine call where it can be (the batch's operand
        forms are still in the workspace); bit-identical to the two separate calls.

        With data parallelism enabled (``imdbn.engine.dp.enable()``) ``data`` is this rank's shard
        of the global batch: the ranks exchange their factor blocks (or all-reduce the statistics, see
        ``imdbn.engine.dp.enable``) once and every replica applies the same update with 1/global_batch
        (SURVEY.md 8e).
        """
        lr, mom = self._lr_mom(epoch)
        eng, x = self._eng(), self._in(data)
        rng = self._rng(x.size(0))
        # 0/1 batches (binary images) are read as bit planes by the positive phase; what a batch contains is found out on the
        # device (imdbn_cd_opts.data_binary = unknown) unless the caller's tensor object carries a loader's tag (``_in`` makes a
        # fresh view every call)
        hint = eng.binary_hint(data)
        dp = _E.dp
        if dp.active():
            B, world = x.size(0), dp.world_size()
            dp.validate_rows(B, x.device)
            if dp.mode() == "factors" and eng.factor_mode_ok(self, B):
                # exchange the factors (~7 MB per rank at 10000 x 1500; 2 MB in wire form) instead of the fp32 statistics (60 MB).
                # Three calls per step: CD pass into the wire form (the visible planes as bits: the sample always, the data when
                # declared binary; with the next-batch hint), all-gather, update
                binary = dp.binary_data()
                wire = eng.cd_factors_wire(self, x, CD, rng, binary, next_data=next_data, data_binary=hint)
                wires = dp.all_gather_blocks(eng.compact_gather_buffer(self, B, world, binary), wire)
                loss = eng.apply_wire(self, wires, B, B * world, binary, lr, mom)
            else:
                packed = eng.cd_stats(self, x, CD, rng, out=eng.packed_buffer(self), data_binary=hint, next_data=next_data)
                dp.all_reduce_sum(packed)
                loss = eng.apply_delta(self, packed, B * world, lr, mom)
            return (loss, self.forward(data)) if return_forward else loss
        if not return_forward:
            return eng.cd_step(self, x, lr, mom, CD, rng, next_data=next_data, data_binary=hint)
        loss, h = eng.cd_step(self, x, lr, mom, CD, rng, next_data=next_data, data_binary=hint, forward=True)
        h._imdbn_binary = False
        return loss, h

    # ---- persistent chains: PCD-k and parallel tempering (extension) --------------------
    @torch.no_grad()
    def train_epoch_persistent(self, data: torch.Tensor, epoch: int, max_epochs: int, CD: int = 1, betas=None, monitor: bool = True):
        """One persistent-CD update on one mini-batch (Tieleman 2008): ``train_epoch`` with the negative phase run on chains that
        live across calls instead of restarting from the data.  Learning rate and momentum follow ``train_epoch``'s schedule.

        The chains are ``self._pcd``, ``[R * B, V]`` 0/1 with replica r in the rows ``[r B, (r + 1) B)``: created on first use as
        ``sample_visible(data)`` per replica (and again when a batch outgrows them or the number of replicas changes), never
        pickled.  A batch shorter than the chains uses and advances the first rows of every replica only.

        ``betas=None``: ``CD`` Gibbs steps on the chains, then the update (PCD-k).  ``betas`` (R >= 2 inverse temperatures,
        ``0 < betas[0] < ... < betas[R - 1] = 1``): ``CD`` parallel-tempering sweeps over all replicas -- a Gibbs step each at its
        temperature, then Metropolis exchanges between neighbours (Desjardins et al. 2010) -- and the update from the ``beta = 1``
        replica as it stands.  ``pt_swap_rates()`` reports the exchanges.

        Returns the 0-d mean-field reconstruction error ``mean((data - visible_probs(forward(data)))^2)`` (a persistent chain does
        not reconstruct the batch), or None with ``monitor=False`` -- the reconstruction is then not computed.  No reference
        counterpart; no data-parallel split."""
        if _E.dp.active():
            raise NotImplementedError("train_epoch_persistent has no data-parallel split")
        lr, mom = self._lr_mom(epoch)
        eng, x = self._eng(), self._in(data)
        particles, k = self._negative_chains(eng, x, betas, CD, "train_epoch_persistent")
        return eng.pcd_step(self, x, particles, lr, mom, k, self._rng(x.size(0)), data_binary=eng.binary_hint(data), monitor=monitor)

    def _negative_chains(self, eng, x: torch.Tensor, betas, CD: int, who: str):
        """The persistent chains behind one update on the batch ``x`` (train_epoch_persistent, train_epoch_centered): creates
        ``self._pcd`` where needed and returns ``(particles, k)``, the ``[b, V]`` view of the chains the update's negative phase
        runs on and the Gibbs steps it still has to make on them -- ``CD`` without ``betas``; with them the ``CD`` tempering
        sweeps run here and the ``beta = 1`` replica is used as it stands (``k = 0``)."""
        b, V = x.size(0), self.num_visible
        bl = None if betas is None else [float(t) for t in (betas.tolist() if hasattr(betas, "tolist") else betas)]
        if bl is not None and len(bl) < 2:
            raise ValueError(f"{who}: betas needs at least two inverse temperatures (None: plain PCD)")
        Rn = 1 if bl is None else len(bl)
        chains = self.__dict__.get("_pcd")
        if (chains is None or chains.device != x.device or chains.size(1) != V or chains.size(0) % Rn != 0
                or chains.size(0) // Rn < b or getattr(self, "_pcd_replicas", Rn) != Rn):
            chains = self._pcd = torch.cat([self.sample_visible(x) for _ in range(Rn)], 0).contiguous()
            self._pcd_replicas = Rn
            self._pt_try = self._pt_acc = None
        Bc = chains.size(0) // Rn
        if bl is None:
            return chains[:b], CD
        # a short batch: the first b rows of every replica, as one [R b, V] tensor of their own for the sweep
        short = b < Bc
        state = chains.view(Rn, Bc, V)[:, :b].reshape(Rn * b, V) if short else chains
        self._pt_try, self._pt_acc = eng.pt_sweep(self, state, bl, CD, self._rng(Rn * b), self._pt_try, self._pt_acc)
        if short:
            chains.view(Rn, Bc, V)[:, :b] = state.view(Rn, b, V)
        return chains[(Rn - 1) * Bc:(Rn - 1) * Bc + b], 0

    def pt_swap_rates(self):
        """Accepted / proposed exchanges per neighbouring pair of replicas since the chains were created: a float64 CPU tensor
        ``[R - 1]`` (NaN for a pair never proposed; None before the first tempered update).  ONE host read, on request only."""
        t, a = self.__dict__.get("_pt_try"), self.__dict__.get("_pt_acc")
        if t is None or a is None:
            return None
        ta = torch.stack([t, a]).cpu().double()
        return torch.where(ta[0] > 0, ta[1] / ta[0].clamp(min=1.0), torch.full_like(ta[0], float("nan")))

    # ---- centered update: the centering trick / enhanced gradient (extension) -------------
    @torch.no_grad()
    def train_epoch_centered(self, data: torch.Tensor, epoch: int, max_epochs: int, CD: int = 1, persistent: bool = False, betas=None,
                             slide: float = 0.01, offsets: str = "data", monitor: bool = True):
        """One update on one mini-batch with the centered gradient (Montavon & Mueller 2012; Cho, Raiko & Ilin 2011; Melchior,
        Fischer & Wiskott 2016): the RBM is centered around the offsets ``mu`` (visible) and ``lam`` (hidden), which follow the
        batch means by ``slide`` in [0, 1] per call -- ``offsets="data"``: the means of the data and of p(h | data); ``"enhanced"``:
        the average of those and the model's.  The stored parameters stay the normal ones (a centered RBM is the normal RBM with
        the biases ``b - W lam`` and ``c - W^T mu``), so every other method and the pickle are unaffected.  Learning rate and
        momentum follow ``train_epoch``'s schedule.

        The phases are ``train_epoch``'s (CD-``CD`` from the data) or, with ``persistent=True`` or ``betas``, those of
        ``train_epoch_persistent`` on the same chains ``self._pcd`` (``betas``: ``CD`` tempering sweeps, then the update from the
        ``beta = 1`` replica).  The offsets live in ``self._ctr_mu`` / ``self._ctr_lam`` (``centering_offsets()``): created on first
        use, or after a device change, by running that call with ``slide = 1`` from zeros -- the first batch's means --, never
        pickled.

        Returns the 0-d loss of the phases' method, or None with ``monitor=False``.  No reference counterpart; no data-parallel
        split."""
        if _E.dp.active():
            raise NotImplementedError("train_epoch_centered has no data-parallel split")
        if offsets not in ("data", "enhanced"):
            raise ValueError(f"train_epoch_centered: offsets = {offsets!r}, must be 'data' or 'enhanced'")
        lr, mom = self._lr_mom(epoch)
        eng, x = self._eng(), self._in(data)
        particles, k = (self._negative_chains(eng, x, betas, CD, "train_epoch_centered") if (persistent or betas is not None)
                        else (None, CD))
        mu, lam = self.__dict__.get("_ctr_mu"), self.__dict__.get("_ctr_lam")
        if mu is None or lam is None or mu.device != x.device or lam.device != x.device:
            mu = self._ctr_mu = torch.zeros(self.num_visible, dtype=torch.float32, device=x.device)
            lam = self._ctr_lam = torch.zeros(self.num_hidden, dtype=torch.float32, device=x.device)
            slide = 1.0
        return eng.centered_step(self, x, particles, lr, mom, k, self._rng(x.size(0)), mu, lam, float(slide),
                                 1 if offsets == "enhanced" else 0, data_binary=eng.binary_hint(data), monitor=monitor)

    def centering_offsets(self):
        """``(mu [V], lam [H])``, the offsets of train_epoch_centered as they stand (the live tensors), or None before its first call."""
        mu, lam = self.__dict__.get("_ctr_mu"), self.__dict__.get("_ctr_lam")
        return None if mu is None or lam is None else (mu, lam)

    # ---- extended mean field: TAP training and log Z (extension; imdbn/utils/tap.py) -------
    def train_epoch_tap(self, data: torch.Tensor, epoch: int, max_epochs: int, **kw):
        """One deterministic TAP update on one mini-batch (``imdbn.utils.tap.train_epoch_tap``: ``n_iters``, ``damp``, ``order``, ``monitor``)."""
        from imdbn.utils.tap import train_epoch_tap
        return train_epoch_tap(self, data, epoch, max_epochs, **kw)

    def log_partition_tap(self, **kw) -> dict:
        """``-Gamma*``, the TAP approximation of log Z at any layer size (``imdbn.utils.tap.tap_log_partition``)."""
        from imdbn.utils.tap import tap_log_partition
        return tap_log_partition(self, **kw)

    # ---- supervised step on the labels (extension) ---------------------------------------
    @torch.no_grad()
    def train_epoch_labels(self, z: torch.Tensor, gt: torch.Tensor, epoch: int, max_epochs: int, num_labels: int,
                           lr_mult: float = 1.0):
        """One ascent step on ``mean log p(gt | z)`` of a joint RBM over ``[z | one-hot label]`` (the last ``num_labels`` visible
        columns): the exact gradient of the hybrid objective of Larochelle & Bengio (2008), applied to every parameter with the
        learning rate (times ``lr_mult``) and momentum schedule of ``train_epoch``.  ``gt``: integer labels ``[B]``; a label
        outside ``[0, num_labels)`` takes no part.  Returns the 0-d device scalar ``-nanmean(log p(gt | z))`` (float64) under the
        parameters before the step.  No reference counterpart (its ``w_sup`` is unused); no draws."""
        if _E.dp.active():
            raise NotImplementedError("train_epoch_labels (w_sup) has no data-parallel split")
        lr, mom = self._lr_mom(epoch)
        logp = self._eng().label_step(self, self._in(z), int(num_labels), gt, float(lr_mult) * lr, mom)
        return -torch.nanmean(logp)

    @torch.no_grad()
    def label_backprop(self, z: torch.Tensor, gt: torch.Tensor, epoch: int, max_epochs: int, num_labels: int, lr_mult: float = 1.0,
                       apply: bool = True):
        """``log p(gt | z)`` of a joint RBM over ``[z | one-hot label]`` as an output layer (extension): returns
        ``(logp, err_z, pred)`` of the engine's ``label_backprop_step`` -- ``err_z`` is the error at the pre-activations that
        produced ``z``, ready for ``backprop_step`` of the layer below -- all under the parameters on entry.  With ``apply`` the
        step of ``train_epoch_labels`` (the same schedule, the same bits); without it the RBM is only read.  No draws."""
        if _E.dp.active():
            raise NotImplementedError("label_backprop has no data-parallel split")
        lr, mom = self._lr_mom(epoch)
        return self._eng().label_backprop_step(self, self._in(z), int(num_labels), gt, float(lr_mult) * lr, mom, apply=bool(apply),
                                               want_pred=True)

    # ---- schedules (rbm.py:229-238) -------------------------------------------------------------
    def _lin_schedule(self, t, t_max, start, end):
        if t_max <= 1:
            return float(end)
        alpha = min(max(t / (t_max - 1), 0.0), 1.0)
        return float(start + (end - start) * alpha)

    def _hot_steps(self, n_steps, hot_frac):
        return int(max(0, min(n_steps, round(hot_frac * n_steps))))

    def _nmf_steps(self, n_steps, T0, T1, sigma0, sharpen_last, T_cold_plus, eta0) -> List[dict]:
        """Host scalars of rbm.py:337-341,362 for each step of noisy mean-field annealing."""
        n = int(n_steps)
        steps = []
        for t in range(n):
            Tt = self._lin_schedule(t, n, T0, T1)
            if (n - t) <= max(1, int(sharpen_last)):
                Tt = T_cold_plus
            frac = max(0.0, 1.0 - (t / max(1, n - 1)))
            steps.append(_step(T=Tt, sigma=sigma0 * frac, eta=eta0 * frac, sample_h=False, vmode=0, clamp=True))
        return steps

    # ---- chains (rbm.py:240-400) ---------------------------------------------------------------
    @torch.no_grad()
    def conditional_gibbs_annealed(
        self,
        v_known: torch.Tensor,
        known_mask: torch.Tensor,
        n_steps: int = 40,
        T0: float = 2.5,
        T1: float = 1.0,
        sample_h_until: int = 20,
        sample_v_every: int = 0,
        final_meanfield: bool = True,
    ):
        """rbm.py:270-298."""
        n = int(n_steps)
        hot = int(max(0, min(n_steps, sample_h_until)))
        steps = []
        for t in range(n):
            Tt = self._lin_schedule(t, n, T0, T1)
            if (n - t) <= 3:
                Tt = min(0.9, Tt)
            sv = (t < hot) and (sample_v_every > 0) and (t % sample_v_every == 0)
            steps.append(_step(T=Tt, sample_h=(t < hot), vmode=1 if sv else 0, clamp=True))
        if final_meanfield:
            steps.append(_step(T=1.0, clamp=True))
        return self._eng().chain(self, self._in(v_known), self._in(known_mask), steps, self._rng(v_known.size(0)))

    @torch.no_grad()
    def noisy_meanfield_annealed(
        self,
        v_known: torch.Tensor,
        known_mask: torch.Tensor,
        n_steps: int = 72,
        T0: float = 3.0,
        T1: float = 1.0,
        sigma0: float = 0.9,
        hot_frac: float = 0.7,
        sharpen_last: int = 3,
        T_cold_plus: float = 0.9,
    ):
        """rbm.py:332-367 (``hot_frac`` is accepted and, as in the reference, has no effect)."""
        mu, eta0 = self._mu()
        steps = self._nmf_steps(n_steps, T0, T1, sigma0, sharpen_last, T_cold_plus, eta0 if mu is not None else 0.0)
        return self._eng().chain(self, self._in(v_known), self._in(known_mask), steps, self._rng(v_known.size(0)), mu=mu)

    @torch.no_grad()
    def conditional_gibbs(
        self,
        v_known: torch.Tensor,
        known_mask: torch.Tensor,
        n_steps: int = 30,
        sample_h: bool = False,
        sample_v: bool = False,
    ) -> torch.Tensor:
        """rbm.py:391-400; the last entry is the reference's final UN-clamped pass (:400)."""
        steps = [_step(sample_h=sample_h, vmode=1 if sample_v else 0, clamp=True) for _ in range(int(n_steps))]
        steps.append(_step(clamp=False))
        return self._eng().chain(self, self._in(v_known), self._in(known_mask), steps, self._rng(v_known.size(0)))

    @torch.no_grad()
    def _chain_pair(self, gibbs: dict, nmf: dict):
        """``conditional_gibbs(**gibbs)`` and ``noisy_meanfield_annealed(**nmf)`` (run in that order by the reference,
        imdbn.py:424-449) as ONE engine call: the two chains are independent (they share only the read-only weights), so they
        run side by side in one launch.  Same draws in the same order, same results as the two calls.  Returns (v_gibbs, v_nmf)."""
        g = dict(n_steps=30, sample_h=False, sample_v=False); g.update(gibbs)
        n = dict(n_steps=72, T0=3.0, T1=1.0, sigma0=0.9, hot_frac=0.7, sharpen_last=3, T_cold_plus=0.9); n.update(nmf)
        steps_g = [_step(sample_h=g["sample_h"], vmode=1 if g["sample_v"] else 0, clamp=True) for _ in range(int(g["n_steps"]))]
        steps_g.append(_step(clamp=False))                                          # rbm.py:400
        mu, eta0 = self._mu()
        steps_n = self._nmf_steps(n["n_steps"], n["T0"], n["T1"], n["sigma0"], n["sharpen_last"], n["T_cold_plus"], eta0 if mu is not None else 0.0)
        a = {"v_known": self._in(g["v_known"]), "mask": self._in(g["known_mask"]), "steps": steps_g}
        b = {"v_known": self._in(n["v_known"]), "mask": self._in(n["known_mask"]), "steps": steps_n, "mu": mu}
        return self._eng().chain_pair(self, a, b, self._rng(a["v_known"].size(0)))

    # ---- clamped CD (rbm.py:402-483) -------------------------------------------------------------
    @torch.no_grad()
    def train_epoch_clamped(
        self,
        v_known: torch.Tensor,
        known_mask: torch.Tensor,
        epoch: int,
        max_epochs: int,
        CD: int = 1,
        cond_init_steps: int = 50,
        sample_h: bool = True,
        sample_v: bool = False,
        reclamp_negative: bool = True,
        aux_lr_mult: float = 0.3,
        use_noisy_init: bool = True,
    ):
        """Auxiliary clamped CD update; returns the 0-d loss mean((v+ - v-)^2)."""
        lr, mom = self._lr_mom(epoch)
        mu = None
        if use_noisy_init:                                                          # rbm.py:443-448
            mu, eta0 = self._mu()
            init = self._nmf_steps(max(10, int(cond_init_steps)), 3.0, 1.0, 0.9, 2, 0.9, eta0 if mu is not None else 0.0)
        else:                                                                       # rbm.py:450-453
            init = [_step(sample_h=sample_h, vmode=1 if sample_v else 0, clamp=True) for _ in range(int(cond_init_steps))]
            init.append(_step(clamp=False))
        eng, vk, km = self._eng(), self._in(v_known), self._in(known_mask)
        rng = self._rng(vk.size(0))
        dp = _E.dp
        if dp.active():
            # this rank's rows of the global batch; one all-reduce of the packed statistics
            B = vk.size(0)
            dp.validate_rows(B, vk.device)
            packed = eng.clamped_stats(self, vk, km, init, mu, CD, sample_h, sample_v, reclamp_negative, rng, out=eng.packed_buffer(self))
            dp.all_reduce_sum(packed)
            return eng.apply_delta(self, packed, B * dp.world_size(), aux_lr_mult * lr, mom, sparsity=False)
        return eng.clamped_step(self, vk, km, init, mu, aux_lr_mult * lr, mom, CD, sample_h, sample_v, reclamp_negative, rng)
