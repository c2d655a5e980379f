"""MultimodalDBM: the whole iMDBN -- image stack, joint RBM and label layer -- as one deep Boltzmann machine (extension; Srivastava &
Salakhutdinov 2012).

The image stack is the DBM of ``imdbn.models.dbm``; on top of it the joint hidden layer ``J`` hears from the top image layer
``z_img`` and from the label layer ``Y``, whose ``K`` units are one categorical per row.  The engine's ``dbm_group_layer`` is the
half-step of that layer; ``mdbm_infer``, ``mdbm_gibbs`` and ``mdbm_step`` are built from it and from ``dbm_layer``.  Explicit only:
nothing in ``iMDBN.train_joint`` turns it on; the way in is ``iMDBN.to_dbm().finetune(...)``.
"""
from __future__ import annotations

import copy
import pickle
from typing import List, Optional, Sequence

import torch

from imdbn.models.grbm import GaussianRBM
from imdbn.models.rbm import RBM
from imdbn.utils import batches, rows_on_device


class MultimodalDBM:
    """Layers ``0 .. L`` of Bernoulli units joined by the RBM copies ``layers[0 .. L-1]`` (the image stack, ``N_L = Dz``), the joint
    hidden layer ``J`` and the label layer ``Y`` (``K`` units, one softmax group), joined by the joint RBM copy ``joint`` whose
    visible side is ``[z_img | y]``:

        -E = sum_l b_l.s_l + sum_{l<L} s_l W_l s_{l+1} + [s_L | y] W_J s_J + b_J.s_J + b_Y.y

    Biases: ONE per layer.  ``b_0 = layers[0].vis_bias``, ``b_l = layers[l-1].hid_bias``, ``b_J = joint.hid_bias``, ``b_Y =
    joint.vis_bias[Dz:]``.  ``layers[l].vis_bias`` for l >= 1 and ``joint.vis_bias[:Dz]`` are NO parameters of the model: the
    conversion zeroes them, what the reused weight update writes there is never read and never saved.

    The state of ``z_img`` and ``y`` lives in one ``[M, Dz + K]`` tensor, the joint RBM's visible row, so ``self.particles`` is the
    ``L + 2`` tensors ``[s_0 .. s_{L-1}, zy, s_J]``."""

    # ---- conversion ---------------------------------------------------------------------------------------------------------------
    @classmethod
    @torch.no_grad()
    def from_imdbn(cls, imdbn, weight_scale: Optional[Sequence[float]] = None) -> "MultimodalDBM":
        """The multimodal DBM whose weights are those of a greedily trained ``iMDBN`` (deep copies: the iMDBN is untouched).
        ``weight_scale``: an optional multiplier per RBM, the image RBMs bottom first and the joint RBM last, as ``DBM.from_idbn``
        takes it.  A ``GaussianRBM`` layer or softmax groups inside the image stack are refused."""
        stack = imdbn.image_idbn
        for l, r in enumerate(stack.layers):
            if isinstance(r, GaussianRBM):
                raise ValueError(f"MultimodalDBM.from_imdbn: image layer {l} is a GaussianRBM; the image stack of a multimodal DBM has "
                                 "Bernoulli units only (DESIGN section 42)")
            if getattr(r, "softmax_groups", None):
                raise ValueError(f"MultimodalDBM.from_imdbn: image layer {l} has softmax groups; the image stack of a multimodal DBM has "
                                 "Bernoulli units only (DESIGN section 42)")
        L = len(stack.layers)
        Dz, K = int(stack.layers[-1].num_hidden), int(imdbn.num_labels)
        jr = imdbn.joint_rbm
        if int(jr.num_visible) != Dz + K or [tuple(map(int, g)) for g in jr.softmax_groups] != [(Dz, Dz + K)]:
            raise ValueError(f"MultimodalDBM.from_imdbn: the joint RBM's visible side must be [z_img ({Dz}) | y ({K})] with y its one "
                             "softmax group")
        scale = [1.0] * (L + 1) if weight_scale is None else [float(s) for s in weight_scale]
        if len(scale) != L + 1:
            raise ValueError(f"MultimodalDBM.from_imdbn: weight_scale needs {L + 1} entries, got {len(scale)}")
        self = cls.__new__(cls)
        self.params = copy.deepcopy(imdbn.params)
        self.dataloader = imdbn.dataloader
        self.device = torch.device(imdbn.device)
        self.num_labels, self.Dz = K, Dz
        rbms: List[RBM] = []
        for l, r in enumerate(list(stack.layers) + [jr]):
            g = copy.deepcopy(r)                      # every attribute of the RBM (RBM.__getstate__: no chains, no native descriptor)
            g.sparsity = False
            if l < L:
                g.softmax_groups = []
            if scale[l] != 1.0:
                g.W.data.mul_(scale[l])
            if 0 < l < L:
                g.vis_bias.data.zero_()               # no parameter of the model
            elif l == L:
                g.vis_bias.data[:Dz].zero_()          # the z_img part: no parameter either; [Dz:] is b_Y
            g.W_m = torch.zeros_like(g.W.data)
            g.hb_m, g.vb_m = torch.zeros_like(g.hid_bias.data), torch.zeros_like(g.vis_bias.data)
            rbms.append(g)
        self.layers, self.joint = rbms[:L], rbms[L]
        self.particles = None
        self.history = []
        return self

    # ---- the model's view of its parameters ---------------------------------------------------------------------------------------
    @property
    def sizes(self) -> List[int]:
        """``[N_0 .. N_L, J, K]``."""
        return [self.layers[0].num_visible] + [r.num_hidden for r in self.layers] + [self.joint.num_hidden, self.num_labels]

    def biases(self) -> List[torch.Tensor]:
        """The ``L + 3`` layer biases ``b_0 .. b_L, b_J, b_Y`` (see the class docstring)."""
        return ([self.layers[0].vis_bias.data] + [r.hid_bias.data for r in self.layers]
                + [self.joint.hid_bias.data, self.joint.vis_bias.data[self.Dz:]])

    def bias_momenta(self) -> List[torch.Tensor]:
        return [self.layers[0].vb_m] + [r.hb_m for r in self.layers] + [self.joint.hb_m, self.joint.vb_m[self.Dz:]]

    def _rbms(self) -> List[RBM]:
        return self.layers + [self.joint]

    def _eng(self):
        return self.layers[0]._eng()

    def _onehot(self, y: torch.Tensor) -> torch.Tensor:
        """Labels as one-hot ``[B, K]`` fp32 rows on the device: class indices ``[B]`` or rows that are one-hot already."""
        y = y.to(self.device)
        if y.dim() == 1:
            return torch.nn.functional.one_hot(y.long(), self.num_labels).float()
        return y.float()

    # ---- inference ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def infer(self, img: torch.Tensor, y: Optional[torch.Tensor] = None, n_mf: int = 10, damp: float = 0.0):
        """``([mu_1 .. mu_L, mu_J, mu_Y], res)``: the mean-field posterior given the image and, with ``y``, the label (clamped;
        ``mu_Y`` is then ``y``); without one the labels are free (the engine's ``mdbm_infer``)."""
        x = rows_on_device(img, self.device)
        return self._eng().mdbm_infer(self.layers, self.joint, self.biases(), x, None if y is None else self._onehot(y), int(n_mf),
                                      damp=float(damp))

    @torch.no_grad()
    def predict_labels(self, img: torch.Tensor, n_mf: int = 10, damp: float = 0.0):
        """Free-label mean field: ``(mu_Y [B, K], argmax [B])``."""
        mu, _ = self.infer(img, None, n_mf, damp)
        return mu[-1], mu[-1].argmax(1)

    @torch.no_grad()
    def generate(self, y: torch.Tensor, n_sweeps: int = 100, init: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Images for the labels ``y``: block Gibbs with the labels clamped on fresh particles (started from ``init`` ``[B, N_0]``,
        default zeros), then ``sigmoid`` of layer 0's input given layer 1."""
        yh = self._onehot(y)
        B = yh.size(0)
        x0 = torch.zeros(B, self.layers[0].num_visible, device=self.device) if init is None else rows_on_device(init, self.device)
        keep, self.particles = self.particles, None
        try:
            parts = self.init_particles(x0, yh)
            self._eng().mdbm_gibbs(self.layers, self.joint, self.biases(), parts, int(n_sweeps), self.layers[0]._rng(B), clamp_labels=yh)
        finally:
            self.particles = keep
        return self._eng().prop_down(self.layers[0], parts[1][:, :self.Dz] if len(self.layers) == 1 else parts[1])

    # ---- particles ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def init_particles(self, data: torch.Tensor, labels: torch.Tensor) -> List[torch.Tensor]:
        """Persistent particles from the rows of ``(data, labels)``: layer 0 and the label are copies, every layer above is sampled
        bottom-up (``("u", N_l)`` per layer, in order; ``J`` from ``[s_L | y]``)."""
        x, yh = rows_on_device(data, self.device), self._onehot(labels)
        eng, rng = self._eng(), self.layers[0]._rng(x.size(0))
        L = len(self.layers)
        parts = [x.clone()]
        for r in self.layers:
            parts.append(eng.prop_up(r, parts[-1], sample=True, rng=rng)[1])
        parts[L] = torch.cat([parts[L], yh], 1)
        parts.append(eng.prop_up(self.joint, parts[L], sample=True, rng=rng)[1])
        self.particles = parts
        return parts

    @torch.no_grad()
    def gibbs(self, n_sweeps: int, clamp_bottom: Optional[torch.Tensor] = None, clamp_labels: Optional[torch.Tensor] = None):
        """``n_sweeps`` block-Gibbs sweeps on the particles, in place; ``clamp_bottom`` / ``clamp_labels`` hold that layer."""
        if self.particles is None:
            raise ValueError("MultimodalDBM.gibbs: no particles yet (init_particles, or a train_step)")
        M = self.particles[0].size(0)
        cb = None if clamp_bottom is None else rows_on_device(clamp_bottom, self.device)
        cl = None if clamp_labels is None else self._onehot(clamp_labels)
        return self._eng().mdbm_gibbs(self.layers, self.joint, self.biases(), self.particles, int(n_sweeps), self.layers[0]._rng(M),
                                      clamp_bottom=cb, clamp_labels=cl)

    # ---- training -----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def train_step(self, data: torch.Tensor, labels: torch.Tensor, epoch: int, max_epochs: int, n_mf: int = 10, damp: float = 0.0,
                   gibbs_k: int = 5, lr_scale: float = 1.0, monitor: bool = True):
        """One update on one mini-batch of ``(data, labels)`` (the engine's ``mdbm_step``): mean-field positive phase with the label
        clamped, ``gibbs_k`` sweeps of the persistent particles (created from the first batch; a shorter batch advances their first
        rows), one weight update per RBM with that RBM's own learning rate (times ``lr_scale``) / momentum schedule and weight decay.
        Returns ``{"recon_loss", "res"}`` (device tensors) or None with ``monitor=False``.  No host sync."""
        from imdbn import engine as _E
        if _E.dp.active():
            raise NotImplementedError("MultimodalDBM.train_step has no data-parallel split")
        x, yh = rows_on_device(data, self.device), self._onehot(labels)
        B = x.size(0)
        if self.particles is None or self.particles[0].size(0) < B:
            self.init_particles(x, yh)
        parts = self.particles if self.particles[0].size(0) == B else [p[:B] for p in self.particles]
        scalars = []
        for r in self._rbms():
            lr, mom = r._lr_mom(epoch)
            scalars.append((lr * float(lr_scale), mom))
        out = self._eng().mdbm_step(self.layers, self.joint, x, yh, parts, scalars, int(n_mf), float(damp), int(gibbs_k),
                                    self.layers[0]._rng(B), monitor=monitor)
        return {"recon_loss": out["recon_loss"], "res": out["res"]} if monitor else None

    def finetune(self, epochs: int, n_mf: int = 10, damp: float = 0.0, gibbs_k: int = 5, lr_scale: float = 1.0, log_every: int = 0):
        """``epochs`` passes of ``train_step`` over ``self.dataloader`` (batches of ``(images, labels)``).  ``log_every`` > 0: the
        monitors of every ``log_every``-th epoch are evaluated, fetched in ONE host read after the epoch's last batch and appended to
        ``self.history`` as ``(epoch, recon_loss, res)``; otherwise nothing is evaluated and the host never reads."""
        if self.dataloader is None:
            raise ValueError("MultimodalDBM.finetune: the model has no dataloader")
        for epoch in range(int(epochs)):
            watch = int(log_every) > 0 and epoch % int(log_every) == 0
            mons = []
            for item in batches(self.dataloader):
                m = self.train_step(rows_on_device(item[0], self.device), item[1], epoch, epochs, n_mf=n_mf, damp=damp, gibbs_k=gibbs_k,
                                    lr_scale=lr_scale, monitor=watch)
                if watch:
                    mons.append(torch.stack([m["recon_loss"].double(), m["res"].max().double()]))
            if mons:
                t = torch.stack(mons)
                loss, res = torch.stack([t[:, 0].mean(), t[:, 1].max()]).cpu().tolist()
                self.history.append((epoch, loss, res))
        return self

    # ---- persistence --------------------------------------------------------------------------------------------------------------
    def save_model(self, path: str):
        """Plain state only: the sizes, ``W`` and its momentum per RBM (the joint RBM last), the ``L + 3`` layer biases and their
        momenta, the particles (None before the first step).  The non-model ``vis_bias`` entries are not written."""
        cpu = lambda t: t.detach().to("cpu").contiguous().clone()
        state = {"sizes": self.sizes, "W": [cpu(r.W.data) for r in self._rbms()], "W_m": [cpu(r.W_m) for r in self._rbms()],
                 "biases": [cpu(b) for b in self.biases()], "bias_momenta": [cpu(b) for b in self.bias_momenta()],
                 "particles": None if self.particles is None else [cpu(p) for p in self.particles]}
        with open(path, "wb") as f:
            pickle.dump(state, f)

    @torch.no_grad()
    def load_model(self, path: str) -> "MultimodalDBM":
        """Read back what ``save_model`` wrote into this model (same sizes); the non-model ``vis_bias`` entries are zeroed."""
        with open(path, "rb") as f:
            state = pickle.load(f)
        if list(state["sizes"]) != self.sizes:
            raise ValueError(f"MultimodalDBM.load_model: the file holds layers {state['sizes']}, this model {self.sizes}")
        L = len(self.layers)
        for l, r in enumerate(self._rbms()):
            r.W.data.copy_(state["W"][l])
            r.W_m.copy_(state["W_m"][l])
            r.hid_bias.data.copy_(state["biases"][l + 1])
            r.hb_m.copy_(state["bias_momenta"][l + 1])
            r.vis_bias.data.zero_()
            r.vb_m.zero_()
        self.layers[0].vis_bias.data.copy_(state["biases"][0])
        self.layers[0].vb_m.copy_(state["bias_momenta"][0])
        self.joint.vis_bias.data[self.Dz:].copy_(state["biases"][L + 2])
        self.joint.vb_m[self.Dz:].copy_(state["bias_momenta"][L + 2])
        self.particles = None if state["particles"] is None else [p.to(self.device).clone() for p in state["particles"]]
        return self
