"""Extended mean-field (TAP) training and log Z (extension).

Gabrie, Tramel & Krzakala 2015, "Training Restricted Boltzmann Machines via the Thouless-Anderson-Palmer free energy"; Tramel et
al. 2018.  The deterministic members of the two families this package has: a negative phase without draws -- persistent
*magnetisations* relaxed by a few fixed-point iterations (``train_epoch_tap``, ``HipEngine.tap_step``) -- and a closed-form
approximation ``-Gamma*`` of log Z at any layer size in a handful of weight passes (``tap_log_partition``,
``HipEngine.tap_iterate``).  Order 2 is the TAP free energy, order 1 naive mean field.  Bernoulli units on both sides only: softmax
groups and ``GaussianRBM`` are refused.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from imdbn import engine as _E
from imdbn.utils.batches import batches, rows_on_device

__all__ = ["train_epoch_tap", "tap_log_partition", "evaluate_log_likelihood_tap", "tap_calibration", "tap_params"]


def _check(rbm, who: str):
    if getattr(rbm, "gaussian_visible", False):
        raise ValueError(f"{who}: needs Bernoulli units on both sides; this RBM's visible layer is Gaussian (DESIGN section 29)")
    if getattr(rbm, "softmax_groups", None):
        raise ValueError(f"{who}: needs Bernoulli units on both sides; this RBM has softmax groups")


def _settings(n_iters, damp, order, who: str):
    n_iters, damp, order = int(n_iters), float(damp), int(order)
    if n_iters < 0 or order not in (1, 2) or not (0.0 <= damp < 1.0):
        raise ValueError(f"{who}: n_iters = {n_iters} (>= 0), order = {order} (1 or 2), damp = {damp} (in [0, 1))")
    return n_iters, damp, order


def tap_params(params: dict):
    """``params["TAP"]`` of ``iDBN.train`` -> None (absent / False) or ``(n_iters, order, damp)``: True means 3 iterations, order 2,
    damp 0.5; a dict sets ``n_iters`` / ``order`` / ``damp``.  Together with ``PERSISTENT`` or ``CENTERED``: ValueError."""
    tap = params.get("TAP", False)
    if tap is None or tap is False:
        return None
    if params.get("PERSISTENT", False) or params.get("CENTERED", False) not in (None, False):
        raise ValueError("iDBN.train: params['TAP'] cannot be combined with params['PERSISTENT'] or params['CENTERED']")
    cfg = {} if tap is True else dict(tap)
    unknown = set(cfg) - {"n_iters", "order", "damp"}
    if unknown:
        raise ValueError(f"iDBN.train: params['TAP'] has unknown keys {sorted(unknown)}")
    n_iters, damp, order = _settings(cfg.get("n_iters", 3), cfg.get("damp", 0.5), cfg.get("order", 2), "iDBN.train: params['TAP']")
    return n_iters, order, damp


def tap_layer_ok(rbm) -> bool:
    """Whether ``iDBN.train`` with ``params["TAP"]`` may route this layer through ``train_epoch_tap`` (else it keeps CD-k)."""
    return not getattr(rbm, "gaussian_visible", False) and not getattr(rbm, "softmax_groups", None)


@torch.no_grad()
def train_epoch_tap(rbm, data: torch.Tensor, epoch: int, max_epochs: int, n_iters: int = 3, damp: float = 0.5, order: int = 2,
                    monitor: bool = True):
    """One TAP update on one mini-batch: ``train_epoch`` with the negative phase replaced by ``n_iters`` damped fixed-point
    iterations on persistent magnetisations and the gradient of the TAP free energy (order 2) or of naive mean field (order 1).
    Learning rate and momentum follow ``train_epoch``'s schedule.

    The magnetisations are ``rbm._tap_mv`` ``[B, V]`` / ``rbm._tap_mh`` ``[B, H]``: created on the first call as the batch and
    ``forward(batch)``, created again when the batch size (or the device) changes, never pickled.

    Returns the 0-d mean-field reconstruction error of the data, or None with ``monitor=False``.  No draws; no data-parallel split."""
    _check(rbm, "train_epoch_tap")
    if _E.dp.active():
        raise NotImplementedError("train_epoch_tap has no data-parallel split")
    n_iters, damp, order = _settings(n_iters, damp, order, "train_epoch_tap")
    lr, mom = rbm._lr_mom(epoch)
    eng, x = rbm._eng(), rbm._in(data)
    mv, mh = rbm.__dict__.get("_tap_mv"), rbm.__dict__.get("_tap_mh")
    if mv is None or mh is None or mv.device != x.device or mv.size(0) != x.size(0) or mh.size(0) != x.size(0):
        mv = rbm._tap_mv = x.clone().contiguous()
        mh = rbm._tap_mh = eng.forward(rbm, x, data_binary=eng.binary_hint(data)).clone().contiguous()
    return eng.tap_step(rbm, x, mv, mh, lr, mom, n_iters, damp=damp, order=order, data_binary=eng.binary_hint(data), monitor=monitor)


@torch.no_grad()
def tap_log_partition(rbm, n_starts: int = 16, max_iters: int = 1000, check_every: int = 25, tol: float = 1e-6, damp: float = 0.5,
                      order: int = 2, seed: int = 0) -> dict:
    """``-Gamma*``, the TAP (order 2) or naive mean-field (order 1) approximation of log Z, from ``n_starts`` starts: visible
    magnetisations uniform in [0.05, 0.95] from a CPU generator seeded with ``seed``, ``mh = forward(mv)``.  The starts are relaxed
    ``check_every`` iterations per engine call, with ONE host read of the residuals after each call, until every residual is
    below ``tol`` or ``max_iters`` iterations have run.

    Returns ``{"log_z": the largest -Gamma over the starts (float), "per_start": float64 [n_starts] on the device, "residual": fp32
    [n_starts] on the device, "converged": bool, "iters": iterations run}``."""
    _check(rbm, "tap_log_partition")
    n_starts, max_iters, check_every = int(n_starts), int(max_iters), int(check_every)
    if n_starts < 1 or max_iters < 0 or check_every < 1:
        raise ValueError(f"tap_log_partition: n_starts = {n_starts} (>= 1), max_iters = {max_iters} (>= 0), check_every = {check_every} (>= 1)")
    _, damp, order = _settings(0, damp, order, "tap_log_partition")
    eng, dev = rbm._eng(), rbm.W.device
    V = rbm.W.shape[0]
    g = np.random.default_rng(int(seed))
    mv = torch.from_numpy((0.05 + 0.9 * g.random((n_starts, V))).astype(np.float32)).to(dev)
    mh = eng.forward(rbm, mv, data_binary=False).clone().contiguous()
    iters, converged = 0, False
    while True:
        n = min(check_every, max_iters - iters)
        gamma, res = eng.tap_iterate(rbm, mv, mh, n, damp=damp, order=order, want_gamma=True, want_res=True)
        iters += n
        converged = n > 0 and float(res.max()) < tol          # the one host read of this round
        if converged or iters >= max_iters:
            break
    per_start = -gamma
    return {"log_z": float(per_start.max()), "per_start": per_start, "residual": res, "converged": converged, "iters": iters}


@torch.no_grad()
def evaluate_log_likelihood_tap(model, loader=None, max_batches: Optional[int] = None, **kw) -> Optional[dict]:
    """Mean ``-F(v) - log_z`` of an ``RBM`` -- or of the BOTTOM layer of an ``iDBN`` -- over ``loader`` (default
    ``model.val_loader``; None without one) with ``log_z`` from ``tap_log_partition(**kw)``: ``mean_ll``, ``sum_ll``, ``n``,
    ``log_z``, ``converged``, ``iters``.  An approximation, not a bound: ``-Gamma*`` may fall on either side of log Z."""
    layers = getattr(model, "layers", None)
    rbm = layers[0] if layers is not None and len(layers) > 0 else model
    _check(rbm, "evaluate_log_likelihood_tap")
    loader = loader if loader is not None else getattr(model, "val_loader", None)
    if loader is None:
        return None
    est = tap_log_partition(rbm, **kw)
    tot, n = None, 0
    for b, batch in enumerate(batches(loader)):
        if max_batches is not None and b >= int(max_batches):
            break
        x = rows_on_device(batch[0] if isinstance(batch, (tuple, list)) else batch, rbm.W.device)
        t = (-rbm.free_energy(x).double() - est["log_z"]).sum()
        tot = t if tot is None else tot + t
        n += x.size(0)
    s = 0.0 if tot is None else float(tot)
    return {"mean_ll": s / max(1, n), "sum_ll": s, "n": n, "log_z": est["log_z"], "converged": est["converged"], "iters": est["iters"]}


@torch.no_grad()
def tap_calibration(rbm, max_bits: int = 24, **kw) -> dict:
    """How far the mean-field values are from the truth on ``rbm``'s own parameters: ``tap_log_partition(order=1)`` and
    ``(order=2)`` against ``exact_log_partition`` (a side of at most ``max_bits`` units): ``{"log_z_exact", "log_z_tap",
    "log_z_nmf", "gap_tap", "gap_nmf", "converged"}``; a gap is exact minus approximation."""
    from imdbn.utils.likelihood import exact_log_partition
    _check(rbm, "tap_calibration")
    kw.pop("order", None)
    exact = float(exact_log_partition(rbm, max_bits=max_bits)["log_z"])
    nmf, tap = tap_log_partition(rbm, order=1, **kw), tap_log_partition(rbm, order=2, **kw)
    return {"log_z_exact": exact, "log_z_tap": tap["log_z"], "log_z_nmf": nmf["log_z"], "gap_tap": exact - tap["log_z"],
            "gap_nmf": exact - nmf["log_z"], "converged": bool(tap["converged"] and nmf["converged"])}
