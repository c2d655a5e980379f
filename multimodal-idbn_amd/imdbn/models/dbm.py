"""DBM: a deep Boltzmann machine over a stack of engine-backed RBMs (extension; Salakhutdinov & Hinton 2009).

Every pair of neighbouring layers is joined by undirected weights, so a layer in the middle of the stack hears from below and from
above at once.  The engine's ``dbm_layer`` is that half-step; ``dbm_infer`` (mean field), ``dbm_gibbs`` (block Gibbs on persistent
particles) and ``dbm_step`` (one update) are built from it.  Explicit only: nothing in ``iDBN.train`` turns it on; the way in is
``iDBN.to_dbm().finetune(...)``.
"""
from __future__ import annotations

import copy
import pickle
from typing import List, Optional, Sequence

import torch

from imdbn.models.grbm import GaussianRBM
from imdbn.models.rbm import RBM
from imdbn.utils import batches, rows_on_device


class DBM:
    """Layers ``0 .. L`` of Bernoulli units, joined by the weights of the RBM copies ``layers[0 .. L-1]`` (``layers[l].W`` between
    layer l and layer l + 1).

    Biases: there is ONE bias per layer.  The bias of layer 0 is ``layers[0].vis_bias``; the bias of layer l >= 1 is
    ``layers[l-1].hid_bias``.  ``layers[l].vis_bias`` for l >= 1 is NOT a parameter of the model: the conversion zeroes it, what the
    reused weight update writes there is never read and never saved.

    Training keeps persistent particles (``self.particles``: ``L + 1`` 0/1 tensors) for the negative phase and uses every RBM's own
    learning-rate / momentum schedule and weight decay; there is no sparsity term."""

    def __init__(self, layer_sizes: Sequence[int], params: dict, dataloader=None, device=None):
        """A fresh model with the initialisation law of the iDBN constructor (``W ~ N(0, 1 / V)``, zero biases)."""
        sizes = [int(n) for n in layer_sizes]
        if len(sizes) < 2:
            raise ValueError("DBM: needs at least two layers")
        self.params = params
        self.dataloader = dataloader
        self.device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.layers: List[RBM] = []
        for i in range(len(sizes) - 1):
            self.layers.append(RBM(num_visible=sizes[i], num_hidden=sizes[i + 1], learning_rate=params["LEARNING_RATE"],
                                   weight_decay=params["WEIGHT_PENALTY"], momentum=params["INIT_MOMENTUM"],
                                   dynamic_lr=params["LEARNING_RATE_DYNAMIC"], final_momentum=params["FINAL_MOMENTUM"]).to(self.device))
        self.particles: Optional[List[torch.Tensor]] = None
        self.history: list = []

    # ---- conversion ---------------------------------------------------------------------------------------------------------------
    @classmethod
    @torch.no_grad()
    def from_idbn(cls, idbn, weight_scale: Optional[Sequence[float]] = None) -> "DBM":
        """The DBM whose weights are those of a greedily trained ``iDBN`` (deep copies: the iDBN is untouched).  ``weight_scale``:
        an optional multiplier per RBM applied to the copied weights -- Salakhutdinov & Hinton (2009, section 3.1) halve the weights
        of the RBMs that were pretrained with doubled input (``[1, 0.5, ..., 0.5, 1]`` for their recipe); the default leaves the
        weights as they are.  A stack with softmax groups or a ``GaussianRBM`` layer is refused: the model is Bernoulli."""
        for l, r in enumerate(idbn.layers):
            if isinstance(r, GaussianRBM):
                raise ValueError(f"DBM.from_idbn: layer {l} is a GaussianRBM; a DBM has Bernoulli units only (DESIGN section 40)")
            if getattr(r, "softmax_groups", None):
                raise ValueError(f"DBM.from_idbn: layer {l} has softmax groups; a DBM has Bernoulli units only (DESIGN section 40)")
        L = len(idbn.layers)
        scale = [1.0] * L if weight_scale is None else [float(s) for s in weight_scale]
        if len(scale) != L:
            raise ValueError(f"DBM.from_idbn: weight_scale needs {L} entries, got {len(scale)}")
        self = cls.__new__(cls)
        self.params = copy.deepcopy(idbn.params)
        self.dataloader = idbn.dataloader
        self.device = torch.device(idbn.device)
        self.layers = []
        for l, r in enumerate(idbn.layers):
            g = copy.deepcopy(r)                      # every attribute of the RBM, whatever it grows later (RBM.__getstate__: no chains,
            g.sparsity, g.softmax_groups = False, []  # no native descriptor); then the fields a DBM layer sets itself
            if scale[l] != 1.0:
                g.W.data.mul_(scale[l])
            if l > 0:
                g.vis_bias.data.zero_()               # l >= 1: no parameter of the model
            g.W_m = torch.zeros_like(g.W.data)
            g.hb_m, g.vb_m = torch.zeros_like(g.hid_bias.data), torch.zeros_like(g.vis_bias.data)
            self.layers.append(g)
        self.particles = None
        self.history = []
        return self

    # ---- the model's view of its parameters ---------------------------------------------------------------------------------------
    @property
    def sizes(self) -> List[int]:
        return [self.layers[0].num_visible] + [r.num_hidden for r in self.layers]

    def biases(self) -> List[torch.Tensor]:
        """The ``L + 1`` layer biases, bottom first (see the class docstring)."""
        return [self.layers[0].vis_bias.data] + [r.hid_bias.data for r in self.layers]

    def bias_momenta(self) -> List[torch.Tensor]:
        return [self.layers[0].vb_m] + [r.hb_m for r in self.layers]

    def _eng(self):
        return self.layers[0]._eng()

    # ---- inference ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def infer(self, v: torch.Tensor, n_mf: int = 10, damp: float = 0.0):
        """``([mu_1 .. mu_L], res)``: the mean-field posterior of the layers above ``v`` after the doubled-weights bottom-up pass
        and ``n_mf`` sweeps, and the residual of the last sweep per row (the engine's ``dbm_infer``)."""
        x = rows_on_device(v, self.device)
        return self._eng().dbm_infer(self.layers, self.biases(), x, int(n_mf), damp=float(damp))

    @torch.no_grad()
    def represent(self, v: torch.Tensor, upto_layer: Optional[int] = None, n_mf: int = 10, damp: float = 0.0) -> torch.Tensor:
        """The mean-field magnetisations of layer ``upto_layer`` (default: the top layer; 0: the input itself)."""
        L = len(self.layers)
        l = L if upto_layer is None else max(0, min(L, int(upto_layer)))
        if l == 0:
            return rows_on_device(v, self.device)
        return self.infer(v, n_mf, damp)[0][l - 1]

    @torch.no_grad()
    def reconstruct(self, v: torch.Tensor, n_mf: int = 10, damp: float = 0.0) -> torch.Tensor:
        """``sigmoid(mu_1 W_0^T + b_0)`` of the mean-field posterior of ``v``."""
        mu, _ = self.infer(v, n_mf, damp)
        return self._eng().prop_down(self.layers[0], mu[0])

    # ---- the density model (imdbn.utils.likelihood) ------------------------------------------------------------
    def log_partition(self, **ais_kwargs) -> dict:
        """``imdbn.utils.likelihood.estimate_dbm_log_partition(self, **ais_kwargs)``: AIS over the odd layers."""
        from imdbn.utils.likelihood import estimate_dbm_log_partition
        return estimate_dbm_log_partition(self, **ais_kwargs)

    def log_likelihood_bound(self, v: torch.Tensor, log_z, n_mf: int = 10, damp: float = 0.0) -> torch.Tensor:
        """``imdbn.utils.likelihood.dbm_variational_bound``: the mean-field lower bound on log p(v) per row, float64 ``[B]``."""
        from imdbn.utils.likelihood import dbm_variational_bound
        return dbm_variational_bound(self, v, log_z, n_mf=n_mf, damp=damp)

    # ---- particles ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def init_particles(self, data: torch.Tensor) -> List[torch.Tensor]:
        """Persistent particles from the rows of ``data``: layer 0 is a copy of them, every layer above is sampled bottom-up
        (``("u", N_l)`` per layer, in order)."""
        x = rows_on_device(data, self.device)
        eng, rng = self._eng(), self.layers[0]._rng(x.size(0))
        parts = [x.clone()]
        for r in self.layers:
            parts.append(eng.prop_up(r, parts[-1], sample=True, rng=rng)[1])
        self.particles = parts
        return parts

    @torch.no_grad()
    def gibbs(self, n_sweeps: int, clamp_bottom: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """``n_sweeps`` block-Gibbs sweeps on the particles, in place; with ``clamp_bottom`` layer 0 is held at that tensor."""
        if self.particles is None:
            raise ValueError("DBM.gibbs: no particles yet (init_particles, or a train_step)")
        M = self.particles[0].size(0)
        cb = None if clamp_bottom is None else rows_on_device(clamp_bottom, self.device)
        return self._eng().dbm_gibbs(self.layers, self.biases(), self.particles, int(n_sweeps), self.layers[0]._rng(M), clamp_bottom=cb)

    # ---- training -----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def train_step(self, data: torch.Tensor, epoch: int, max_epochs: int, n_mf: int = 10, damp: float = 0.0, gibbs_k: int = 5,
                   lr_scale: float = 1.0, monitor: bool = True):
        """One DBM update on one mini-batch (the engine's ``dbm_step``): mean-field positive phase, ``gibbs_k`` sweeps of the
        persistent particles (created from the first batch; a shorter batch advances their first rows), one weight update per RBM
        with that RBM's own learning rate (times ``lr_scale``) / momentum schedule and weight decay.  Returns ``{"recon_loss",
        "res"}`` (device tensors) or None with ``monitor=False`` (the reconstruction is then not launched).  No host sync."""
        from imdbn import engine as _E
        if _E.dp.active():
            raise NotImplementedError("DBM.train_step has no data-parallel split")
        x = rows_on_device(data, self.device)
        B = x.size(0)
        if self.particles is None or self.particles[0].size(0) < B:
            self.init_particles(x)
        parts = self.particles if self.particles[0].size(0) == B else [p[:B] for p in self.particles]
        scalars = []
        for r in self.layers:
            lr, mom = r._lr_mom(epoch)
            scalars.append((lr * float(lr_scale), mom))
        out = self._eng().dbm_step(self.layers, x, parts, scalars, int(n_mf), float(damp), int(gibbs_k), self.layers[0]._rng(B),
                                   monitor=monitor)
        return {"recon_loss": out["recon_loss"], "res": out["res"]} if monitor else None

    def finetune(self, epochs: int, n_mf: int = 10, damp: float = 0.0, gibbs_k: int = 5, lr_scale: float = 1.0, log_every: int = 0):
        """``epochs`` passes of ``train_step`` over ``self.dataloader``.  ``log_every`` > 0: the monitors of every ``log_every``-th
        epoch are evaluated, fetched in ONE host read after the epoch's last batch and appended to ``self.history`` as ``(epoch,
        recon_loss, res)`` (batch mean, largest residual); otherwise nothing is evaluated and the host never reads."""
        if self.dataloader is None:
            raise ValueError("DBM.finetune: the model has no dataloader")
        for epoch in range(int(epochs)):
            watch = int(log_every) > 0 and epoch % int(log_every) == 0
            mons = []
            for item in batches(self.dataloader):
                m = self.train_step(rows_on_device(item[0], self.device), epoch, epochs, n_mf=n_mf, damp=damp, gibbs_k=gibbs_k,
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
        """Plain state only: the sizes, ``W`` and its momentum per RBM, the ``L + 1`` layer biases and their momenta, the particles
        (None before the first step).  The non-model ``vis_bias`` vectors are not written."""
        cpu = lambda t: t.detach().to("cpu").contiguous().clone()
        state = {"sizes": self.sizes, "W": [cpu(r.W.data) for r in self.layers], "W_m": [cpu(r.W_m) for r in self.layers],
                 "biases": [cpu(b) for b in self.biases()], "bias_momenta": [cpu(b) for b in self.bias_momenta()],
                 "particles": None if self.particles is None else [cpu(p) for p in self.particles]}
        with open(path, "wb") as f:
            pickle.dump(state, f)

    @torch.no_grad()
    def load_model(self, path: str) -> "DBM":
        """Read back what ``save_model`` wrote into this model (same sizes); the non-model ``vis_bias`` vectors are zeroed."""
        with open(path, "rb") as f:
            state = pickle.load(f)
        if list(state["sizes"]) != self.sizes:
            raise ValueError(f"DBM.load_model: the file holds layers {state['sizes']}, this model {self.sizes}")
        for l, r in enumerate(self.layers):
            r.W.data.copy_(state["W"][l])
            r.W_m.copy_(state["W_m"][l])
            r.hid_bias.data.copy_(state["biases"][l + 1])
            r.hb_m.copy_(state["bias_momenta"][l + 1])
            r.vis_bias.data.zero_()
            r.vb_m.zero_()
        self.layers[0].vis_bias.data.copy_(state["biases"][0])
        self.layers[0].vb_m.copy_(state["bias_momenta"][0])
        self.particles = None if state["particles"] is None else [p.to(self.device).clone() for p in state["particles"]]
        return self
