"""GaussianRBM: an RBM whose visible units are Gaussian with learned variances (extension).

The parameterisation of Cho, Ilin & Raiko (2011, "Improved learning of Gaussian-Bernoulli RBMs"): next to ``W``, ``vis_bias`` (b) and
``hid_bias`` (c) of ``RBM`` a log-variance ``logvar`` (z, ``sigma_i^2 = exp(z_i)``), and

    E(v, h)  = sum_i (v_i - b_i)^2 / (2 sigma_i^2) - sum_ij (v_i / sigma_i^2) W_ij h_j - sum_j c_j h_j
    p(h | v) = sigmoid(c + (v / sigma^2) W),      p(v | h) = N(b + h W^T, sigma^2)

Every method body is host-side scalar logic plus calls into the native engine (``HipEngine.gauss_*``), as in ``rbm.py``.  The hidden
layer is Bernoulli, so ``forward`` feeds a Bernoulli RBM above it (``iDBN`` with ``params["GAUSSIAN_VISIBLE"]``).  The inherited
methods that assume Bernoulli visibles -- AIS, the pseudo-log-likelihood, the persistent / centered / label / clamped trainers and
the chains -- raise ``ValueError``: none of them may return a number computed for the wrong model.  The density of THIS model has
methods of its own, ``gaussian_log_partition`` (AIS over Gaussian visibles, ``HipEngine.gauss_ais``) and ``gaussian_log_likelihood``
(-F(v) - log Z), over ``imdbn.utils.likelihood``, and ``gaussian_log_likelihood_conservative``, the reverse-AIS
side that needs no log Z (``HipEngine.gauss_reverse_ais``).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from imdbn import engine as _E
from imdbn.models.rbm import RBM


def _refuse(name: str):
    def method(self, *args, **kw):
        raise ValueError(f"GaussianRBM.{name}: needs Bernoulli visible units; this layer's visibles are Gaussian (DESIGN section 29)")
    method.__name__ = name
    method.__doc__ = f"Refused: ``RBM.{name}`` assumes Bernoulli visibles."
    return method


class GaussianRBM(RBM):
    """Gaussian visible units, Bernoulli hidden units, learned per-unit variances."""

    gaussian_visible = True

    def __init__(self, num_visible: int, num_hidden: int, learning_rate: float, weight_decay: float, momentum: float,
                 dynamic_lr: bool = False, final_momentum: float = 0.97, sparsity: bool = False, sparsity_factor: float = 0.05,
                 lr_sigma_mult: float = 1.0, logvar_min: float = -math.inf, logvar_max: float = math.inf):
        super().__init__(num_visible, num_hidden, learning_rate, weight_decay, momentum, dynamic_lr=dynamic_lr,
                         final_momentum=final_momentum, sparsity=sparsity, sparsity_factor=sparsity_factor, softmax_groups=None)
        if not float(logvar_min) <= float(logvar_max):
            raise ValueError(f"GaussianRBM: logvar_min = {logvar_min} above logvar_max = {logvar_max}")
        self.lr_sigma_mult = float(lr_sigma_mult)         # learning rate of logvar = lr_sigma_mult * lr; 0 fixes the variances
        self.logvar_min, self.logvar_max = float(logvar_min), float(logvar_max)
        self.logvar = nn.Parameter(torch.zeros(self.num_visible, device=self.W.device), requires_grad=False)
        self.logvar_m = torch.zeros_like(self.logvar.data)      # a plain attribute, as the other momentum buffers

    # ---- helpers ------------------------------------------------------------------------------
    def _z(self) -> torch.Tensor:
        return self.logvar.data

    def _zm(self) -> torch.Tensor:
        """The momentum of logvar on the device of logvar (``.to()`` does not move plain attributes)."""
        m = self.__dict__.get("logvar_m")
        if not isinstance(m, torch.Tensor) or m.shape != self.logvar.shape:
            m = self.logvar_m = torch.zeros_like(self.logvar.data)
        elif m.device != self.logvar.device or m.dtype != torch.float32 or not m.is_contiguous():
            m = self.logvar_m = m.to(device=self.logvar.device, dtype=torch.float32).contiguous()
        return m

    def variances(self) -> torch.Tensor:
        """sigma^2 = exp(logvar), ``[V]``."""
        return torch.exp(self.logvar.data)

    @torch.no_grad()
    def init_from_data(self, data: torch.Tensor):
        """``vis_bias`` := the column means of ``data``, ``logvar`` := the log of its column variances (1/n; a zero variance is
        floored at the smallest positive variance of the batch, or 1 when every column is constant).  Returns self."""
        x = self._in(data).double()
        mean, var = x.mean(0), x.var(0, unbiased=False)
        pos = var[var > 0]
        var = torch.where(var > 0, var, torch.full_like(var, float(pos.min()) if pos.numel() else 1.0))
        self.vis_bias.data.copy_(mean.float())
        self.logvar.data.copy_(torch.log(var).float().clamp_(self.logvar_min, self.logvar_max))
        return self

    # ---- propagations ---------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, v: torch.Tensor, T: float = 1.0) -> torch.Tensor:
        """p(h | v) = sigmoid(((v exp(-logvar)) W + c) / max(1e-6, T))."""
        out = self._eng().gauss_forward(self, self._z(), self._in(v), T=T)
        out._imdbn_binary = False
        return out

    @torch.no_grad()
    def _visible_logits(self, h: torch.Tensor, T: float = 1.0) -> torch.Tensor:
        return self.visible_probs(h, T)

    @torch.no_grad()
    def visible_probs(self, h: torch.Tensor, T: float = 1.0) -> torch.Tensor:
        """The mean of p(v | h): b + h W^T.  (The name is the base class's: a Gaussian layer has a mean, not probabilities.)"""
        if T != 1.0:
            raise ValueError(f"GaussianRBM.visible_probs: T = {T}; the mean of a Gaussian layer has no temperature")
        return self._eng().gauss_backward(self, self._z(), self._in(h))

    @torch.no_grad()
    def backward(self, h: torch.Tensor, return_logits: bool = False) -> torch.Tensor:
        """The mean b + h W^T (with or without ``return_logits``: the reconstruction is linear)."""
        return self.visible_probs(h)

    @torch.no_grad()
    def sample_visible(self, mean: torch.Tensor) -> torch.Tensor:
        """v ~ N(mean, sigma^2): mean + exp(logvar / 2) n, one ("n", V) draw."""
        return self._eng().gauss_sample_visible(self, self._z(), self._in(mean), self._rng(mean.size(0)))

    @torch.no_grad()
    def backward_sample(self, h: torch.Tensor) -> torch.Tensor:
        return self._eng().gauss_backward(self, self._z(), self._in(h), sample=True, rng=self._rng(h.size(0)))[1]

    @torch.no_grad()
    def free_energy(self, v: torch.Tensor) -> torch.Tensor:
        """F(v) = sum_i (v_i - b_i)^2 / (2 sigma_i^2) - sum_j softplus(c_j + ((v / sigma^2) W)_j), shape [B]."""
        return self._eng().gauss_free_energy(self, self._z(), self._in(v))

    @torch.no_grad()
    def gibbs_step(self, v: torch.Tensor, sample_h: bool = True, sample_v: bool = True):
        """One v -> h -> v' step; returns (v_next, v_mean, h, h_prob).  Without ``sample_h`` the mean is taken from h_prob, without
        ``sample_v`` v_next is the mean."""
        eng, rng = self._eng(), self._rng(v.size(0))
        if sample_h:
            h_prob, h = eng.gauss_forward(self, self._z(), self._in(v), sample=True, rng=rng)
        else:
            h_prob = h = eng.gauss_forward(self, self._z(), self._in(v))
        if sample_v:
            mean, v_next = eng.gauss_backward(self, self._z(), h, sample=True, rng=rng)
        else:
            mean = v_next = eng.gauss_backward(self, self._z(), h)
        return v_next, mean, h, h_prob

    # ---- CD-k update ----------------------------------------------------------------------------
    @torch.no_grad()
    def train_epoch(self, data: torch.Tensor, epoch: int, max_epochs: int, CD: int = 1, sample_v: bool = True, monitor: bool = True):
        """One CD-``CD`` update on one mini-batch with the gradient of Cho, Ilin & Raiko for W, b, c and logvar (one engine call,
        ``HipEngine.gauss_cd_step``); learning rate and momentum follow ``RBM.train_epoch``'s schedule, logvar learns with
        ``lr_sigma_mult`` times that rate and stays inside ``[logvar_min, logvar_max]``.  ``sample_v``: the negative visible state
        is drawn from N(mean, sigma^2), else it is the mean.  Returns the 0-d loss ``mean((data - mean_last)^2)``, or None with
        ``monitor=False``.  No data-parallel split."""
        if _E.dp.active():
            raise NotImplementedError("GaussianRBM.train_epoch has no data-parallel split")
        lr, mom = self._lr_mom(epoch)
        x = self._in(data)
        return self._eng().gauss_cd_step(self, self._z(), self._zm(), x, lr, mom, int(CD), self._rng(x.size(0)), self.lr_sigma_mult * lr,
                                         z_lo=self.logvar_min, z_hi=self.logvar_max, sample_v=bool(sample_v), monitor=monitor)

    # ---- the density of this model -------------------------------------------------
    def gaussian_log_partition(self, n_chains: int = 256, n_betas: int = 1000, betas=None, base_vis_bias=None, seed=None) -> dict:
        """AIS estimate of log Z (``imdbn.utils.likelihood.estimate_gaussian_log_partition``): ``log_z``, ``log_z_base``, ``logw``,
        ``ess``, ``se``."""
        from imdbn.utils.likelihood import estimate_gaussian_log_partition
        return estimate_gaussian_log_partition(self, n_chains=n_chains, n_betas=n_betas, betas=betas, base_vis_bias=base_vis_bias, seed=seed)

    def gaussian_log_likelihood(self, v: torch.Tensor, log_z) -> torch.Tensor:
        """log p(v) = -F(v) - log Z per row, float64 ``[B]`` (``imdbn.utils.likelihood.gaussian_log_likelihood``)."""
        from imdbn.utils.likelihood import gaussian_log_likelihood
        return gaussian_log_likelihood(self, self._in(v), log_z)

    def gaussian_log_likelihood_conservative(self, v: torch.Tensor, n_chains: int = 16, n_betas: int = 1000, betas=None,
                                             base_vis_bias=None, seed=None, max_rows: int = 4096) -> dict:
        """Reverse-AIS estimate of the log-density of the annealing model per row: ``{"ll", "ess", "logw"}``
        (``imdbn.utils.likelihood.gaussian_reverse_ais_log_likelihood``; no AIS estimate of log Z enters)."""
        from imdbn.utils.likelihood import gaussian_reverse_ais_log_likelihood
        return gaussian_reverse_ais_log_likelihood(self, self._in(v), n_chains=n_chains, n_betas=n_betas, betas=betas,
                                                   base_vis_bias=base_vis_bias, seed=seed, max_rows=max_rows)

    def gaussian_log_partition_exact(self, **kw) -> dict:
        """Exact log Z by on-device enumeration of the hidden side (``imdbn.utils.likelihood.exact_gaussian_log_partition``; at most
        ``max_bits`` = 24 hidden units); with ``marginals=True`` also E[v_i] and p(h_j = 1)."""
        from imdbn.utils.likelihood import exact_gaussian_log_partition
        return exact_gaussian_log_partition(self, **kw)

    # ---- what assumes Bernoulli visibles --------------------------------------------------------
    log_partition_exact = _refuse("log_partition_exact")      # (the two exact names are not in REFUSED: they take no rows)
    exact_marginals = _refuse("exact_marginals")
    log_partition = _refuse("log_partition")
    pseudo_log_likelihood = _refuse("pseudo_log_likelihood")
    log_likelihood = _refuse("log_likelihood")
    log_likelihood_conservative = _refuse("log_likelihood_conservative")
    train_epoch_persistent = _refuse("train_epoch_persistent")
    train_epoch_centered = _refuse("train_epoch_centered")
    train_epoch_labels = _refuse("train_epoch_labels")
    label_backprop = _refuse("label_backprop")
    train_epoch_clamped = _refuse("train_epoch_clamped")
    conditional_gibbs_annealed = _refuse("conditional_gibbs_annealed")
    noisy_meanfield_annealed = _refuse("noisy_meanfield_annealed")
    conditional_gibbs = _refuse("conditional_gibbs")
    _chain_pair = _refuse("_chain_pair")


REFUSED = ("log_partition", "pseudo_log_likelihood", "log_likelihood", "log_likelihood_conservative", "train_epoch_persistent",
           "train_epoch_centered", "train_epoch_labels", "label_backprop", "train_epoch_clamped", "conditional_gibbs_annealed",
           "noisy_meanfield_annealed", "conditional_gibbs", "_chain_pair")
