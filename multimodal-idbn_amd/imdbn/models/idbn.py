"""iDBN: stack of engine-backed RBMs with the reference's class surface.

Mirror of the reference ``imdbn/models/idbn.py`` for the parts on the hot path (SURVEY.md 8a:
a12-a14): constructor, the interleaved greedy ``train`` loop (:195-204), ``represent`` (:307-323),
``reconstruct`` (:325-344), ``decode`` (:346-359), ``save_model`` (:361-373).  The wandb / PCA /
linear-probe tail of ``train`` (:206-305) is the reference's observability side-car and is out of
scope; ``wandb_run`` is accepted and only receives the epoch loss.
"""
from __future__ import annotations

import os
import pickle
from typing import List, Optional

import torch

from imdbn.models.grbm import GaussianRBM
from imdbn.models.rbm import RBM
from imdbn.utils import batches, rows_on_device
from imdbn.utils.tap import tap_layer_ok, tap_params


def binary_input(v: torch.Tensor) -> bool:
    """Whether a layer's input can seed persistent chains: anything but the probabilities an engine propagation returned (those
    carry ``_imdbn_binary = False``, RBM.forward)."""
    return getattr(v, "_imdbn_binary", None) is not False


class iDBN:
    def __init__(
        self,
        layer_sizes: List[int],
        params: dict,
        dataloader,
        val_loader,
        device,
        wandb_run=None,
        logging_config_path: Optional[str] = None,
    ):
        self.layers: List[RBM] = []
        self.params = params
        self.dataloader = dataloader
        self.val_loader = val_loader
        self.device = device
        self.wandb_run = wandb_run
        self.logging_cfg = {}

        # fields the reference's utilities expect (idbn.py:113-116)
        self.text_flag = False
        self.arch_str = "-".join(map(str, layer_sizes))
        self.arch_dir = os.path.join("logs-idbn", f"architecture_{self.arch_str}")
        os.makedirs(self.arch_dir, exist_ok=True)

        self.cd_k = int(self.params.get("CD", 1))                                   # idbn.py:118
        self.sparsity_last = bool(self.params.get("SPARSITY", False))
        self.sparsity_factor = float(self.params.get("SPARSITY_FACTOR", 0.1))

        try:                                                                        # idbn.py:123-126
            self.val_batch, self.val_labels = next(iter(val_loader))
        except Exception:
            self.val_batch, self.val_labels = None, None
        # validation features for the evaluation side-car (idbn.py:129-144): a Subset over a base dataset that carries
        # per-sample lists; any other loader leaves `features` at None, as in the reference
        self.features = None
        try:
            indices = val_loader.dataset.indices
            base = val_loader.dataset.dataset
            feats = {
                "Cumulative Area": torch.tensor([base.cumArea_list[i] for i in indices], dtype=torch.float32),
                "Convex Hull": torch.tensor([base.CH_list[i] for i in indices], dtype=torch.float32),
                "Labels": torch.tensor([base.labels[i] for i in indices], dtype=torch.float32),
            }
            density = getattr(base, "density_list", None)
            if density is not None:
                feats["Density"] = torch.tensor([density[i] for i in indices], dtype=torch.float32)
            self.features = feats
        except Exception:
            pass

        # extension, off by default: params["GAUSSIAN_VISIBLE"] makes layer 0 a GaussianRBM (real-valued inputs with
        # learned variances; params["GAUSSIAN_LR_SIGMA_MULT"], ["GAUSSIAN_LOGVAR_MIN"], ["GAUSSIAN_LOGVAR_MAX"] are its arguments)
        self.gaussian_visible = bool(self.params.get("GAUSSIAN_VISIBLE", False))
        for i in range(len(layer_sizes) - 1):                                       # idbn.py:149-161
            gauss = dict(lr_sigma_mult=float(self.params.get("GAUSSIAN_LR_SIGMA_MULT", 1.0)),
                         logvar_min=float(self.params.get("GAUSSIAN_LOGVAR_MIN", float("-inf"))),
                         logvar_max=float(self.params.get("GAUSSIAN_LOGVAR_MAX", float("inf")))) if (self.gaussian_visible and i == 0) else None
            rbm = (RBM if gauss is None else GaussianRBM)(
                num_visible=layer_sizes[i],
                num_hidden=layer_sizes[i + 1],
                learning_rate=self.params["LEARNING_RATE"],
                weight_decay=self.params["WEIGHT_PENALTY"],
                momentum=self.params["INIT_MOMENTUM"],
                dynamic_lr=self.params["LEARNING_RATE_DYNAMIC"],
                final_momentum=self.params["FINAL_MOMENTUM"],
                sparsity=(self.sparsity_last and i == len(layer_sizes) - 2),
                sparsity_factor=self.sparsity_factor,
                **(gauss or {}),
            ).to(self.device)
            self.layers.append(rbm)

    def _layers_to_monitor(self) -> List[int]:
        layers = {len(self.layers)}
        if len(self.layers) > 1:
            layers.add(1)
        return sorted(layers)

    def _layer_tag(self, idx: int) -> str:
        return f"layer{idx}"

    def train(self, epochs: int, log_every_pca: int = 25, log_every_probe: int = 10):
        """Interleaved greedy layer-wise training (idbn.py:195-204): on every batch each layer
        is updated by CD and then feeds the next layer with p(h|v) from its UPDATED weights.

        The reference does ``float(loss)`` after every update (a device->host sync per RBM
        update, idbn.py:204); here losses stay on the device and are fetched once per epoch
        (values identical).  ``self.loss_history`` keeps them.
        """
        self.loss_history = []
        # extension, off by default: params["PERSISTENT"] trains the layers whose input is binary -- a batch of the
        # loader, never another layer's probabilities -- with persistent chains (RBM.train_epoch_persistent: PCD-k, or parallel
        # tempering over params["PT_BETAS"]); every other layer keeps CD-k
        persistent, pt_betas = bool(self.params.get("PERSISTENT", False)), self.params.get("PT_BETAS")
        # extension, off by default: params["CENTERED"] (True: slide 0.01; a float: the slide) routes every layer's
        # update through RBM.train_epoch_centered with the offsets of params["CENTERED_OFFSETS"] ("data" / "enhanced"); persistent
        # chains keep the gate above
        centered = self.params.get("CENTERED", False)
        centered = None if centered is None or centered is False else (0.01 if centered is True else float(centered))
        ctr_offsets = self.params.get("CENTERED_OFFSETS", "data")
        # extension, off by default: params["TAP"] (True: 3 iterations, order 2, damp 0.5; a dict: n_iters / order / damp)
        # trains every Bernoulli layer without softmax groups by RBM.train_epoch_tap; not together with PERSISTENT or CENTERED
        tap = tap_params(self.params)
        if tap is not None:
            from imdbn import engine as _E
            if _E.dp.active():
                raise NotImplementedError("iDBN.train: params['TAP'] has no data-parallel split")
        for epoch in range(int(epochs)):
            losses = []
            # one batch of lookahead: the first layer prepares the operand forms of the following batch during its
            # weight update (RBM.train_epoch next_data=); the batches and their order are unchanged
            dev_batch = lambda item: None if item is None else rows_on_device(item[0], self.device)
            it = iter(batches(self.dataloader))
            cur = dev_batch(next(it, None))
            while cur is not None:
                nxt = dev_batch(next(it, None))
                v = cur
                last = len(self.layers) - 1
                for li, rbm in enumerate(self.layers):
                    # update + forward of the same batch as one engine call; the top layer's forward (computed and
                    # dropped by the reference, idbn.py:203) has no side effect and is not run
                    if isinstance(rbm, GaussianRBM):      # its own CD update; no persistent or centered form
                        loss = rbm.train_epoch(v, epoch, epochs, CD=self.cd_k)
                        if li < last:
                            v = rbm.forward(v)
                    elif tap is not None and tap_layer_ok(rbm):
                        loss = rbm.train_epoch_tap(v, epoch, epochs, n_iters=tap[0], order=tap[1], damp=tap[2])
                        if li < last:
                            v = rbm.forward(v)
                    elif centered is not None:
                        chains = persistent and binary_input(v)
                        loss = rbm.train_epoch_centered(v, epoch, epochs, CD=self.cd_k, persistent=chains, betas=pt_betas if chains else None,
                                                        slide=centered, offsets=ctr_offsets)
                        if li < last:
                            v = rbm.forward(v)
                    elif persistent and binary_input(v):
                        loss = rbm.train_epoch_persistent(v, epoch, epochs, CD=self.cd_k, betas=pt_betas)
                        if li < last:
                            v = rbm.forward(v)
                    elif li < last:
                        loss, v = rbm.train_epoch(v, epoch, epochs, CD=self.cd_k, next_data=nxt if li == 0 else None, return_forward=True)
                    else:
                        loss = rbm.train_epoch(v, epoch, epochs, CD=self.cd_k, next_data=nxt if li == 0 else None)
                    losses.append(loss)
                cur = nxt
            if losses:
                ep = torch.stack([l.reshape(()) for l in losses]).float().cpu()
                self.loss_history.append(ep)
                if self.wandb_run:
                    self.wandb_run.log({"idbn/loss": float(ep.mean()), "epoch": epoch})

    @torch.no_grad()
    def represent(self, x: torch.Tensor, upto_layer: Optional[int] = None) -> torch.Tensor:
        """idbn.py:319-323."""
        v = rows_on_device(x, self.device)
        L = len(self.layers) if (upto_layer is None) else max(0, min(len(self.layers), int(upto_layer)))
        for i in range(L):
            v = self.layers[i].forward(v)
        return v

    @torch.no_grad()
    def reconstruct(self, x: torch.Tensor) -> torch.Tensor:
        """idbn.py:336-344."""
        cur = rows_on_device(x, self.device)
        for rbm in self.layers:
            cur = rbm.forward(cur)
        for rbm in reversed(self._down_layers()):
            cur = rbm.backward(cur)
        return cur

    @torch.no_grad()
    def decode(self, top: torch.Tensor) -> torch.Tensor:
        """idbn.py:356-359."""
        cur = top.to(self.device)
        for rbm in reversed(self._down_layers()):
            cur = rbm.backward(cur)
        return cur

    # ---- up-down fine-tuning of the whole stack (extension; Hinton, Osindero & Teh 2006) ----------------
    def _no_gaussian(self, who: str):
        """The fine-tuning passes and the bounds treat every layer as Bernoulli: refused on a stack with a Gaussian layer."""
        if any(isinstance(r, GaussianRBM) for r in self.layers):
            raise ValueError(f"iDBN.{who}: needs Bernoulli visible units; layer 0 of this stack is a GaussianRBM (DESIGN section 29)")

    def is_untied(self) -> bool:
        return self.__dict__.get("gen_layers") is not None

    def _down_layers(self) -> List[RBM]:
        """The RBMs a top-down pass goes through, bottom first: the generative twins of an untied model under its top RBM, else
        ``layers``."""
        gen = self.__dict__.get("gen_layers")
        return self.layers if gen is None else list(gen) + [self.layers[-1]]

    @torch.no_grad()
    def untie(self) -> List[RBM]:
        """Give every directed layer (all but the top RBM) generative weights of its own: ``self.gen_layers[l]`` is an ``RBM`` of
        the shape, row pitch, device and hyper-parameters of ``layers[l]`` holding copies of its ``W`` and ``vis_bias`` (the two
        parameters a top-down pass reads) and zero momenta; ``layers`` stay the recognition weights.  Idempotent.  ``__init__`` does
        not create the attribute: a model that is never untied keeps its attribute set and its pickle."""
        self._no_gaussian("untie")                     # first: a Gaussian stack is refused whether or not gaussian_untie has run
        gen = self.__dict__.get("gen_layers")
        if gen is not None:
            return gen
        gen = []
        for r in self.layers[:-1]:
            g = RBM.__new__(RBM)                      # not the constructor: it would draw an initial W from torch's generator
            torch.nn.Module.__init__(g)
            for k in ("num_visible", "num_hidden", "lr", "weight_decay", "momentum", "dynamic_lr", "final_momentum", "sparsity_factor"):
                setattr(g, k, getattr(r, k))
            g.sparsity, g.softmax_groups = False, []
            dev = r.W.device
            W = torch.empty_strided(tuple(r.W.shape), tuple(r.W.stride()), dtype=torch.float32, device=dev)
            W.copy_(r.W.data)
            g.W = torch.nn.Parameter(W, requires_grad=False)
            g.hid_bias = torch.nn.Parameter(r.hid_bias.data.clone(), requires_grad=False)
            g.vis_bias = torch.nn.Parameter(r.vis_bias.data.clone(), requires_grad=False)
            g.W_m = torch.empty_strided(tuple(W.shape), tuple(W.stride()), dtype=torch.float32, device=dev).zero_()
            g.hb_m, g.vb_m = torch.zeros_like(g.hid_bias.data), torch.zeros_like(g.vis_bias.data)
            gen.append(g)
        self.gen_layers = gen
        return gen

    @torch.no_grad()
    def updown_step(self, data: torch.Tensor, epoch: int, max_epochs: int, CD: int = 1, persistent: bool = False, lr_scale: float = 1.0,
                    monitor: bool = True):
        """One up-down step on one mini-batch (unties the model on first use): the engine's ``updown_step`` -- wake pass, CD-``CD``
        on the top RBM from the top wake state (``persistent``: PCD on the top RBM's own chains), sleep pass, the generative delta
        rule on the wake states and the recognition delta rule on the sleep states.  Every layer uses its own RBM's learning-rate
        and momentum schedule (``lr`` times ``lr_scale``) and weight decay.  Returns ``{"wake_nll", "sleep_nll", "top_loss"}`` as
        0-d device scalars -- minus the mean over the batch of the summed log-probabilities of the generative / recognition
        predictions before this call's update, and the top RBM's mean-field reconstruction error -- or None with
        ``monitor=False`` (nothing is then evaluated for them).  No host sync; no data-parallel split."""
        from imdbn import engine as _E
        self._no_gaussian("updown_step")
        if _E.dp.active():
            raise NotImplementedError("updown_step has no data-parallel split")
        gen = self.untie()
        x = rows_on_device(data, self.device)
        scalars = []
        for r in self.layers:
            lr, mom = r._lr_mom(epoch)
            scalars.append((lr * float(lr_scale), mom))
        out = self.layers[-1]._eng().updown_step(self.layers, gen, x, scalars, int(CD), "persistent" if persistent else None,
                                                 self.layers[-1]._rng(x.size(0)), monitor=monitor)
        return {k: out[k] for k in ("wake_nll", "sleep_nll", "top_loss")} if monitor else None

    def finetune_updown(self, epochs: int, CD: int = 1, persistent: bool = False, lr_scale: float = 0.1, log_every: int = 0):
        """``epochs`` passes of ``updown_step`` over ``self.dataloader`` (explicit only: ``train`` never calls it and no
        ``params`` key turns it on).  ``log_every`` > 0: the monitors of every ``log_every``-th epoch are evaluated, fetched in ONE
        host read after the epoch's last batch and appended to ``self.updown_history`` as ``(epoch, wake_nll, sleep_nll,
        top_loss)`` batch means; otherwise nothing is evaluated and the host never reads."""
        self.updown_history = getattr(self, "updown_history", [])
        for epoch in range(int(epochs)):
            watch = int(log_every) > 0 and epoch % int(log_every) == 0
            mons = []
            for item in batches(self.dataloader):
                m = self.updown_step(rows_on_device(item[0], self.device), epoch, epochs, CD=CD, persistent=persistent, lr_scale=lr_scale,
                                     monitor=watch)
                if watch:
                    mons.append(torch.stack([m["wake_nll"].double(), m["sleep_nll"].double(), m["top_loss"].double()]))
            if mons:
                w, s, t = torch.stack(mons).mean(0).cpu().tolist()
                self.updown_history.append((epoch, w, s, t))
                if self.wandb_run:
                    self.wandb_run.log({"idbn/wake_nll": w, "idbn/sleep_nll": s, "idbn/top_loss": t, "epoch": epoch})

    # ---- backprop fine-tuning of the unrolled stack as a deep autoencoder (extension; Hinton & Salakhutdinov 2006) ----
    @torch.no_grad()
    def autoencoder_step(self, data: torch.Tensor, epoch: int, max_epochs: int, lr_scale: float = 1.0, monitor: bool = True):
        """One backprop step on one mini-batch (unties the model on first use): the engine's ``autoencoder_step`` -- the stack
        unrolled into an encoder (``layers``) and a decoder (the top RBM's own weights, then the generative twins), the gradient
        of the reconstruction cross-entropy of ``reconstruct(data)`` sent back through every sigmoid layer.  Every layer uses its
        own RBM's learning-rate and momentum schedule (``lr`` times ``lr_scale``) and weight decay.  Returns ``{"xent", "mse"}``
        as 0-d device scalars -- the batch mean of the rows' cross-entropy between ``data`` and its reconstruction, and the mean
        squared reconstruction error, both before this call's update -- or None with ``monitor=False`` (nothing is then evaluated
        for them).  No host sync; no data-parallel split."""
        from imdbn import engine as _E
        self._no_gaussian("autoencoder_step")
        if _E.dp.active():
            raise NotImplementedError("autoencoder_step has no data-parallel split")
        gen = self.untie()
        x = rows_on_device(data, self.device)
        scalars = []
        for r in self.layers:
            lr, mom = r._lr_mom(epoch)
            scalars.append((lr * float(lr_scale), mom))
        out = self.layers[-1]._eng().autoencoder_step(self.layers, gen, x, scalars, monitor=monitor)
        return {k: out[k] for k in ("xent", "mse")} if monitor else None

    def finetune_autoencoder(self, epochs: int, lr_scale: float = 0.1, log_every: int = 0):
        """``epochs`` passes of ``autoencoder_step`` over ``self.dataloader`` (explicit only: ``train`` never calls it and no
        ``params`` key turns it on).  ``log_every`` > 0: the monitors of every ``log_every``-th epoch are evaluated, fetched in ONE
        host read after the epoch's last batch and appended to ``self.autoencoder_history`` as ``(epoch, xent, mse)`` batch means;
        otherwise nothing is evaluated and the host never reads."""
        self.autoencoder_history = getattr(self, "autoencoder_history", [])
        for epoch in range(int(epochs)):
            watch = int(log_every) > 0 and epoch % int(log_every) == 0
            mons = []
            for item in batches(self.dataloader):
                m = self.autoencoder_step(rows_on_device(item[0], self.device), epoch, epochs, lr_scale=lr_scale, monitor=watch)
                if watch:
                    mons.append(torch.stack([m["xent"].double(), m["mse"].double()]))
            if mons:
                x, s = torch.stack(mons).mean(0).cpu().tolist()
                self.autoencoder_history.append((epoch, x, s))
                if self.wandb_run:
                    self.wandb_run.log({"idbn/autoencoder_xent": x, "idbn/autoencoder_mse": s, "epoch": epoch})

    # ---- backprop fine-tuning of a stack with a Gaussian bottom layer (extension; Hinton & Salakhutdinov 2006) ----
    @torch.no_grad()
    def gaussian_untie(self) -> List[RBM]:
        """``untie`` for a stack built with ``GAUSSIAN_VISIBLE``: the twin of layer 0 is a ``GaussianRBM`` (built without its
        constructor: no torch draws) holding copies of the layer's ``W``, ``vis_bias`` and ``logvar`` -- the decoder's own
        log-variance --, zero momenta (``logvar_m`` included) and the layer's ``lr_sigma_mult``, ``logvar_min`` and ``logvar_max``;
        the twins above are ``untie``'s.  Idempotent; ``ValueError`` on a stack without a Gaussian bottom layer."""
        gen = self.__dict__.get("gen_layers")
        if gen is not None:
            return gen
        if not (self.layers and isinstance(self.layers[0], GaussianRBM)):
            raise ValueError("iDBN.gaussian_untie: needs a stack whose layer 0 is a GaussianRBM (params['GAUSSIAN_VISIBLE']); use untie")
        gen = []
        for r in self.layers[:-1]:
            gauss = isinstance(r, GaussianRBM)
            cls = GaussianRBM if gauss else RBM
            g = cls.__new__(cls)                      # not the constructor: it would draw an initial W from torch's generator
            torch.nn.Module.__init__(g)
            for k in ("num_visible", "num_hidden", "lr", "weight_decay", "momentum", "dynamic_lr", "final_momentum", "sparsity_factor"):
                setattr(g, k, getattr(r, k))
            g.sparsity, g.softmax_groups = False, []
            dev = r.W.device
            W = torch.empty_strided(tuple(r.W.shape), tuple(r.W.stride()), dtype=torch.float32, device=dev)
            W.copy_(r.W.data)
            g.W = torch.nn.Parameter(W, requires_grad=False)
            g.hid_bias = torch.nn.Parameter(r.hid_bias.data.clone(), requires_grad=False)
            g.vis_bias = torch.nn.Parameter(r.vis_bias.data.clone(), requires_grad=False)
            g.W_m = torch.empty_strided(tuple(W.shape), tuple(W.stride()), dtype=torch.float32, device=dev).zero_()
            g.hb_m, g.vb_m = torch.zeros_like(g.hid_bias.data), torch.zeros_like(g.vis_bias.data)
            if gauss:
                g.lr_sigma_mult, g.logvar_min, g.logvar_max = r.lr_sigma_mult, r.logvar_min, r.logvar_max
                g.logvar = torch.nn.Parameter(r.logvar.data.clone(), requires_grad=False)
                g.logvar_m = torch.zeros_like(g.logvar.data)
            gen.append(g)
        self.gen_layers = gen
        return gen

    @torch.no_grad()
    def gaussian_autoencoder_step(self, data: torch.Tensor, epoch: int, max_epochs: int, lr_scale: float = 1.0, monitor: bool = True):
        """``autoencoder_step`` for a stack built with ``GAUSSIAN_VISIBLE`` (unties the model with ``gaussian_untie`` on first use):
        the engine's ``gauss_autoencoder_step`` -- the decoder's bottom layer is linear-Gaussian, the loss the Gaussian negative
        log-density of ``data`` under ``reconstruct(data)`` with the decoder's learned variances.  Every layer uses its own RBM's
        learning-rate and momentum schedule (``lr`` times ``lr_scale``) and weight decay, every Gaussian layer ``lr_sigma_mult``
        times that rate for its ``logvar``, inside its clamps.  Returns ``{"nll", "mse"}`` as 0-d device scalars -- the batch mean of
        ``sum_i (data - recon)^2 exp(-zeta) / 2 + zeta / 2`` and the mean squared reconstruction error, both before this call's
        update -- or None with ``monitor=False``.  No host sync; no data-parallel split."""
        from imdbn import engine as _E
        if _E.dp.active():
            raise NotImplementedError("gaussian_autoencoder_step has no data-parallel split")
        gen = self.gaussian_untie()
        x = rows_on_device(data, self.device)
        scalars = []
        for r in self.layers:
            lr, mom = r._lr_mom(epoch)
            scalars.append((lr * float(lr_scale), mom))
        out = self.layers[-1]._eng().gauss_autoencoder_step(self.layers, gen, x, scalars, monitor=monitor)
        return {k: out[k] for k in ("nll", "mse")} if monitor else None

    def finetune_gaussian_autoencoder(self, epochs: int, lr_scale: float = 0.1, log_every: int = 0):
        """``epochs`` passes of ``gaussian_autoencoder_step`` over ``self.dataloader`` (explicit only).  ``log_every`` > 0: the
        monitors of every ``log_every``-th epoch are evaluated, fetched in ONE host read after the epoch's last batch and appended
        to ``self.gaussian_autoencoder_history`` as ``(epoch, nll, mse)`` batch means; otherwise the host never reads."""
        self.gaussian_autoencoder_history = getattr(self, "gaussian_autoencoder_history", [])
        for epoch in range(int(epochs)):
            watch = int(log_every) > 0 and epoch % int(log_every) == 0
            mons = []
            for item in batches(self.dataloader):
                m = self.gaussian_autoencoder_step(rows_on_device(item[0], self.device), epoch, epochs, lr_scale=lr_scale, monitor=watch)
                if watch:
                    mons.append(torch.stack([m["nll"].double(), m["mse"].double()]))
            if mons:
                x, s = torch.stack(mons).mean(0).cpu().tolist()
                self.gaussian_autoencoder_history.append((epoch, x, s))
                if self.wandb_run:
                    self.wandb_run.log({"idbn/gaussian_autoencoder_nll": x, "idbn/gaussian_autoencoder_mse": s, "epoch": epoch})

    @torch.no_grad()
    def log_likelihood_bound(self, v: torch.Tensor, log_z_top, **kw) -> torch.Tensor:
        """Variational lower bound on log p(v) of the whole stack per row, float64 ``[B]``
        (``imdbn.utils.likelihood.dbn_lower_bound``; ``log_z_top`` = log Z of the top RBM)."""
        self._no_gaussian("log_likelihood_bound")
        from imdbn.utils.likelihood import dbn_lower_bound
        return dbn_lower_bound(self, v, log_z_top, **kw)

    def log_likelihood_bound_conservative(self, v: torch.Tensor, **kw) -> torch.Tensor:
        """The stack's lower bound with the reverse-AIS estimate as its top term, float64 ``[B]``
        (``imdbn.utils.likelihood.dbn_conservative_bound``; no AIS estimate of log Z enters)."""
        self._no_gaussian("log_likelihood_bound_conservative")
        from imdbn.utils.likelihood import dbn_conservative_bound
        return dbn_conservative_bound(self, v, **kw)

    @torch.no_grad()
    def gaussian_log_likelihood_bound(self, v: torch.Tensor, log_z_top, n_samples: int = 8, importance: bool = False,
                                      seed: Optional[int] = None) -> torch.Tensor:
        """Variational lower bound on the log-density log p(v) of a stack built with ``GAUSSIAN_VISIBLE`` per row, float64 ``[B]``
        (``imdbn.utils.likelihood.gaussian_dbn_lower_bound``; ``importance``: ``gaussian_dbn_log_likelihood_is``; ``log_z_top`` =
        log Z of the top RBM)."""
        from imdbn.utils.likelihood import gaussian_dbn_log_likelihood_is, gaussian_dbn_lower_bound
        return (gaussian_dbn_log_likelihood_is if importance else gaussian_dbn_lower_bound)(self, v, log_z_top, n_samples, seed)

    def gaussian_log_likelihood_bound_conservative(self, v: torch.Tensor, **kw) -> torch.Tensor:
        """The lower bound of a stack built with ``GAUSSIAN_VISIBLE`` with the reverse-AIS estimate as its top term, float64 ``[B]``
        (``imdbn.utils.likelihood.gaussian_dbn_conservative_bound``; no AIS estimate of log Z enters)."""
        from imdbn.utils.likelihood import gaussian_dbn_conservative_bound
        return gaussian_dbn_conservative_bound(self, v, **kw)

    def unit_tuning(self, upto_layer: Optional[int] = None, **kw) -> dict:
        """Per-unit tuning curves and feature regressions of layer ``upto_layer`` (default: the top) over the validation split
        (``imdbn.utils.unit_tuning.evaluate_unit_tuning``)."""
        from imdbn.utils.unit_tuning import evaluate_unit_tuning
        return evaluate_unit_tuning(self, upto_layer=upto_layer, **kw)

    def to_dbm(self, **kw):
        """This stack as a deep Boltzmann machine (``imdbn.models.dbm.DBM.from_idbn``): deep copies, this model is untouched."""
        from imdbn.models.dbm import DBM
        return DBM.from_idbn(self, **kw)

    def save_model(self, path: str):
        """idbn.py:370-372: pickle of {"layers", "params"} (live RBM modules)."""
        model_copy = {"layers": self.layers, "params": self.params}
        if self.is_untied():
            model_copy["gen_layers"] = self.gen_layers      # RBM.__getstate__: contiguous, no native descriptor
        with open(path, "wb") as f:
            pickle.dump(model_copy, f)
        print(f"[iDBN] Model saved to {path}")

    def load_model(self, path: str):
        """Read back what ``save_model`` wrote into this model (same architecture): the layers, and the generative twins when the
        saved model was untied (a tied file leaves this model tied)."""
        with open(path, "rb") as f:
            saved = pickle.load(f)
        self.layers = [rbm.to(self.device) for rbm in saved["layers"]]
        self.params = saved.get("params", self.params)
        self.__dict__.pop("gen_layers", None)
        if saved.get("gen_layers") is not None:
            self.gen_layers = [rbm.to(self.device) for rbm in saved["gen_layers"]]
        return self
