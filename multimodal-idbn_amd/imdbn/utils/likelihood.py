"""Partition function and held-out log-likelihood of a binary RBM by annealed importance sampling, on the engine.

Reconstruction error and free energy do not say whether an RBM improves as a density model: log p(v) = -F(v) - log Z needs the
partition function.  ``estimate_log_partition`` estimates log Z with AIS (Salakhutdinov & Murray 2008, "On the quantitative
analysis of deep belief networks"): ``n_chains`` chains are annealed from the base-rate model A (no weights, visible biases
``base_vis_bias``, whose partition function is known: log Z_A = H log 2 + sum_i softplus(b_A,i)) to the RBM through the
temperatures ``betas``, and log Z ~= log Z_A + logmeanexp(logw).  The whole loop is ONE ``HipEngine.ais`` call
(imdbn_rbm_ais).

Binary visibles without softmax groups only (``ValueError`` otherwise: a softmax group is not a product of Bernoulli units and
the estimator above does not describe it).

Random draws: ``seed=None`` consumes the ambient draw source; ``seed=int`` runs under a ``PhiloxRng(seed)`` of its own and leaves the
caller's draw counter where it was, so estimating between epochs does not change training (the rule of ``evaluate_cross_modal``).
The draw schedules are those of ``imdbn.engine.rng`` (``sched_ais``, ``sched_ais_groups``, ``sched_reverse_ais``, ``sched_bound``).

Stacks: what the project trains is an ``iDBN``, and the RBM likelihood above only speaks about its bottom layer.  The DBN's
generative model is the top RBM over (h_{L-1}, h_L) with directed layers p(h_{l-1} | h_l) = Bernoulli(sigmoid(b_l + h_l W_l^T))
below it; with h_l ~ q(h_l | h_{l-1}) = Bernoulli(sigmoid(c_l + h_{l-1} W_l)) drawn bottom-up, one sample's value is

    w = sum_{l < L} [ log p(h_{l-1} | h_l) + E_l ] - F_top(h_{L-1}) - log Z_top

``E_l`` = the entropy of q(h_l | h_{l-1}) (mode ``entropy``: the mean of w is an unbiased estimate of the variational lower bound
on log p_DBN(v), ``dbn_lower_bound``) or -log q of the drawn h_l (mode ``logq``: E_q[exp w] = p_DBN(v), and the logmeanexp over
samples approaches log p(v) from below, ``dbn_log_likelihood_is``).  Each directed layer is ONE ``HipEngine.bound_step`` call
(imdbn_rbm_bound_step); the top layer is ``free_energy``.

The multimodal model: an ``iMDBN`` is an image stack under a joint RBM whose visible layer is ``[z | one-hot label]``, the label a
softmax group.  Its generative model, in the DBN reading, is that joint RBM over (z, y, h) with ALL L image layers directed below
it, and z -- the top image layer's hidden state -- is BINARY.  (``train_joint`` feeds the joint RBM real-valued probabilities
instead; the numbers below are those of the binary-z model, not of that training input.)  One sample's value is

    w_joint = sum_{l <= L} [ log p(h_{l-1} | h_l) + E_l ] - F_joint([z, e_y]) - log Z_joint,      z = h_L ~ q
    w_image = the same with log sum_y' exp(-F_joint([z, e_y'])) in place of -F_joint([z, e_y]): the label summed out

(``imdbn_sample_values``; ``imdbn_lower_bound`` / ``imdbn_log_likelihood_is`` as for the DBN; ``evaluate_imdbn_bound``).  One
``bound_step`` per image layer, then ONE ``HipEngine.label_loglik`` call (imdbn_rbm_label_loglik) for both label-side
values.  ``log Z_joint`` comes from ``estimate_joint_log_partition``: AIS over Bernoulli columns plus softmax groups
(``HipEngine.ais_groups``, imdbn_rbm_ais_groups), whose base-rate model treats the columns of ``base_vis_bias`` inside a group as the
logits of a categorical (``base_rate_bias_joint``).  The functions of the first two paragraphs keep refusing softmax groups.
``iMDBN_BiModal`` is not covered.

The other side of the sandwich: every number above rests on ONE AIS estimate of log Z, and AIS under-estimates Z in expectation, so
they are optimistic.  Reverse AIS ("RAISE", Burda, Grosse & Salakhutdinov 2015) reads the forward annealing chain as a generative model
p_ann (v_1 ~ p_A, then one AIS transition per temperature, the one at beta = 1 included), runs it backwards from each held-out row and
averages importance weights that only need log Z_A: ``reverse_ais_log_likelihood`` is a stochastic LOWER bound on log p_ann(v) -- of
the annealing model, which approaches the RBM as the ladder grows, not of the RBM itself.  ONE ``HipEngine.reverse_ais`` call per
chunk of rows (imdbn_rbm_reverse_ais) and one ``HipEngine.rows_logmeanexp``.
``evaluate_log_likelihood_sandwich`` reports both sides and their gap;
``dbn_conservative_bound`` puts the reverse estimate in place of the top term of ``dbn_lower_bound``.  The iMDBN is not composed.

The cheap monitor: everything above costs hundreds to thousands of annealing steps per estimate.  The pseudo-log-likelihood
PLL(v) = sum_sites log p(v_site | v_rest) needs no partition function, no chain and no draw, and the engine computes the EXACT sum over
all sites -- every visible column outside the softmax groups, every group as one site -- in about the time of one propagation
(``pseudo_log_likelihood``, ONE ``HipEngine.pseudo_loglik`` call, imdbn_rbm_pseudo_loglik; the toolkits' estimate from one
random bit per row is not offered).  Softmax groups are accepted; rows must be 0/1 with one-hot groups (NaN otherwise, that row only).
``evaluate_pseudo_likelihood`` is the per-epoch monitor over a loader; ``imdbn_pseudo_log_likelihood`` evaluates the joint RBM of an
``iMDBN`` on ``[z | one-hot y]`` with z drawn as the bounds above draw it, and its group term is log p(y | z), the classification
log-loss, without a chain.  It is a training monitor, not a likelihood: PLL is not comparable with the numbers above.

Gaussian visibles: a ``GaussianRBM`` is refused by everything above -- those estimators describe Bernoulli visibles --
and has functions of its own.  ``estimate_gaussian_log_partition`` anneals from the base-rate model A with the RBM's
variances, no weights and visible bias ``base_vis_bias`` (log Z_A = H log 2 + (V / 2) log 2 pi + sum(logvar) / 2) through
p*_beta(v) = exp(-(1 - beta) q_A(v) - beta q_B(v)) prod_j (1 + exp(beta x_j)), q_X(v) = sum_i (v_i - b_X,i)^2 / (2 sigma_i^2): ONE
``HipEngine.gauss_ais`` call (imdbn_rbm_gauss_ais).  No ``base_vis_bias`` means the RBM's own visible bias, not zeros: a Gaussian
centred on 0 is a useless start for data far from 0 (``gaussian_base_rate_bias``: the column means of the data).
``gaussian_log_likelihood`` is the log-DENSITY -F(v) - log Z; ``evaluate_gaussian_log_likelihood`` its mean over a loader.

Stacks with a Gaussian bottom layer (``iDBN`` with ``params["GAUSSIAN_VISIBLE"]``): the generative model is that of the
stacks paragraph with p(v | h_1) = N(b_1 + h_1 W_1^T, sigma^2) at the bottom and q(h_1 | v) = Bernoulli(sigmoid(c_1 + u W_1)),
u = v exp(-logvar), as its recognition model; the bottom bracket of ``w`` is log N(v; b_1 + h_1 W_1^T, sigma^2) + E_1, ONE
``HipEngine.gauss_bound_step`` call (imdbn_rbm_gauss_bound_step), and the Bernoulli layers above go through ``bound_step`` on the same
accumulator and draw source.  ``gaussian_dbn_sample_values`` / ``gaussian_dbn_lower_bound`` / ``gaussian_dbn_log_likelihood_is`` /
``evaluate_gaussian_dbn_bound`` are log-DENSITIES; the ``dbn_*`` functions go on refusing a Gaussian layer and these refuse a stack
whose bottom layer is not Gaussian.

The conservative side under Gaussian visibles: AIS over continuous visibles with learned variances under-estimates
log Z when a chain misses a narrow mode, so ``gaussian_log_likelihood`` with an AIS log Z is the number to trust least.
``gaussian_reverse_ais_log_likelihood`` runs the chain of ``estimate_gaussian_log_partition`` backwards from each held-out row (ONE
``HipEngine.gauss_reverse_ais`` call per chunk of rows, imdbn_rbm_gauss_reverse_ais): a stochastic LOWER bound on the log-density
log p_ann(v).  ``evaluate_gaussian_log_likelihood_sandwich`` reports both sides and their gap; ``gaussian_dbn_conservative_bound`` /
``evaluate_gaussian_dbn_bound_conservative`` put a reverse estimate in place of the top term of ``gaussian_dbn_lower_bound`` -- the
Bernoulli one on the sampled top states for two layers and more, the Gaussian one for a stack of one.  These are the functions of the
Bernoulli paragraph above on another engine call and another log Z_A; each family refuses the other's layers.

The ground truth: everything above is an estimate.  When the smaller side of the RBM has at most 30 units the engine
enumerates it on the device and sums the other side out in closed form: ``exact_log_partition`` (Bernoulli visibles, softmax groups
accepted) and ``exact_gaussian_log_partition`` are ONE ``HipEngine.exact_log_z`` call (imdbn_rbm_exact_logz) and return the exact
log Z and, on request, the exact model marginals p(v_i = 1) / E[v_i] and p(h_j = 1).  ``evaluate_log_likelihood_exact`` /
``evaluate_gaussian_log_likelihood_exact`` are ``evaluate_log_likelihood`` with that log Z; ``ais_calibration`` /
``gaussian_ais_calibration`` run the AIS estimator unchanged and report its distance from the truth on the caller's own parameters;
``chain_marginal_gap`` compares the column means of a PCD or tempering particle cloud with the exact visible marginals.  ``max_bits``
(24) guards the cost of 2^n states times the other side's width.

The deep Boltzmann machine (``imdbn.models.DBM``): its layers are joined by undirected weights, so none of the stack
figures above describes it.  ``estimate_dbm_log_partition`` is the AIS of Salakhutdinov & Hinton (2009, section 4.1): the chains live
on the odd layers, the even layers are summed out analytically, ONE ``HipEngine.dbm_ais`` call (imdbn_dbm_ais);
``dbm_variational_bound`` is the mean-field lower bound on log p(v) (``HipEngine.dbm_infer``, then ``HipEngine.dbm_bound``) and
``evaluate_dbm_log_likelihood`` its mean over a loader.  Bernoulli layers only.

Data parallelism: the chains are NOT sharded over ranks -- every rank that calls runs all ``n_chains`` chains and gets the same
estimate (same seed) or an independent one; sharding the chains is a follow-up.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from imdbn import engine as _E
from imdbn.utils.batches import batches, rows_on_device

__all__ = ["base_rate_bias", "linear_betas", "estimate_log_partition", "log_likelihood", "evaluate_log_likelihood",
           "dbn_sample_values", "dbn_lower_bound", "dbn_log_likelihood_is", "evaluate_dbn_bound",
           "base_rate_bias_joint", "estimate_joint_log_partition", "imdbn_sample_values", "imdbn_lower_bound",
           "imdbn_log_likelihood_is", "evaluate_imdbn_bound",
           "reverse_ais_log_likelihood", "evaluate_log_likelihood_sandwich", "dbn_conservative_bound", "evaluate_dbn_bound_conservative",
           "pseudo_log_likelihood", "evaluate_pseudo_likelihood", "imdbn_pseudo_log_likelihood",
           "gaussian_base_rate_bias", "estimate_gaussian_log_partition", "gaussian_log_likelihood", "evaluate_gaussian_log_likelihood",
           "gaussian_dbn_sample_values", "gaussian_dbn_lower_bound", "gaussian_dbn_log_likelihood_is", "evaluate_gaussian_dbn_bound",
           "gaussian_reverse_ais_log_likelihood", "evaluate_gaussian_log_likelihood_sandwich", "gaussian_dbn_conservative_bound",
           "evaluate_gaussian_dbn_bound_conservative",
           "exact_log_partition", "exact_gaussian_log_partition", "evaluate_log_likelihood_exact",
           "evaluate_gaussian_log_likelihood_exact", "ais_calibration", "gaussian_ais_calibration", "chain_marginal_gap",
           "estimate_dbm_log_partition", "dbm_variational_bound", "evaluate_dbm_log_likelihood"]


def _bottom(model):
    """The RBM whose likelihood is meant: `model` itself, or the bottom layer of an iDBN."""
    layers = getattr(model, "layers", None)
    return layers[0] if layers is not None and len(layers) > 0 else model


def _check_binary(rbm, groups_ok: bool = False):
    if getattr(rbm, "gaussian_visible", False):
        raise ValueError("the likelihood estimators need Bernoulli visibles: this RBM's visible layer is Gaussian (DESIGN section 29)")
    if getattr(rbm, "softmax_groups", None) and not groups_ok:
        raise ValueError("AIS likelihood needs an RBM with binary visibles and no softmax groups")


def _first(batch):
    return batch[0] if isinstance(batch, (tuple, list)) else batch


def _draws(seed):
    """The draw source of `seed` (module docstring): the ambient one, or a private PhiloxRng on the caller's row offset."""
    return _E.get_rng() if seed is None else _E.PhiloxRng(int(seed), row0=int(getattr(_E.get_rng(), "row0", 0)))


def _log_z_base(rbm, base_vis_bias, dev) -> torch.Tensor:
    """log Z_A of the base-rate model of ``rbm`` (float64 scalar on ``dev``): H log 2 + sum_{i outside groups} softplus(b_A,i) +
    sum_g logsumexp(b_A[g]); no ``base_vis_bias`` = zeros."""
    V, H = rbm.W.shape
    bA = torch.zeros(V, dtype=torch.float64, device=dev) if base_vis_bias is None else base_vis_bias.to(dev).double().reshape(-1)
    if bA.numel() != V:
        raise ValueError(f"base_vis_bias must have {V} elements")
    free = torch.ones(V, dtype=torch.bool, device=dev)
    lzb = torch.full((), H * math.log(2.0), dtype=torch.float64, device=dev)
    for s, e in (getattr(rbm, "softmax_groups", None) or []):
        free[int(s):int(e)] = False
        lzb = lzb + torch.logsumexp(bA[int(s):int(e)], 0)
    return lzb + torch.nn.functional.softplus(bA[free]).sum()


def _weight_stats_device(logw: torch.Tensor, lzb: torch.Tensor) -> torch.Tensor:
    """``[log_z, log_z_base, ess, se]`` of the AIS weights ``logw`` (``estimate_log_partition``) as one float64 device vector."""
    M = logw.numel()
    mx = logw.max()
    w = torch.exp(logw - mx)
    mean = w.mean()
    log_z = lzb + mx + torch.log(mean)
    ess = w.sum() ** 2 / (w * w).sum()
    se = (w.std(unbiased=True) if M > 1 else w.new_zeros(())) / (mean * math.sqrt(M))
    return torch.stack([log_z.reshape(()), lzb.reshape(()), ess.reshape(()), se.reshape(())])


def _weight_stats(logw: torch.Tensor, lzb: torch.Tensor) -> dict:
    """The result dict of ``estimate_log_partition``, with its one device-to-host copy."""
    host = _weight_stats_device(logw, lzb).cpu().tolist()
    return {"log_z": host[0], "log_z_base": host[1], "logw": logw, "ess": host[2], "se": host[3]}


def _known_or_estimated(log_z, estimate, rbm, ais_kwargs):
    """``(log_z, se, ess)``: the caller's ``log_z`` (se and ess None), or those of ``estimate(rbm, **ais_kwargs)``."""
    if log_z is not None:
        return log_z, None, None
    est = estimate(rbm, **ais_kwargs)
    return est["log_z"], est["se"], est["ess"]


def _sum_batches(loader, max_batches, batch_sums, width: int, extra: Optional[torch.Tensor] = None):
    """``(sums, n)`` over the batches of ``loader``, at most ``max_batches`` of them: ``batch_sums(batch)`` gives a float64 device
    vector of ``width`` sums over the batch's rows, they are added up on the device and come to the host in ONE copy after the last
    batch, as a list; ``n`` counts the rows.  ``extra``: a device vector that rides along with that copy, appended to the list."""
    tot, n = None, 0
    for b, batch in enumerate(batches(loader)):
        if max_batches is not None and b >= int(max_batches):
            break
        t = batch_sums(batch)
        tot = t if tot is None else tot + t
        n += _first(batch).size(0)
    parts = [t for t in (tot, extra) if t is not None]
    host = torch.cat(parts).cpu().tolist() if parts else []
    return ([0.0] * width if tot is None else []) + host, n


def _log_scalars(model, prefix: str, res: dict, keys):
    run = getattr(model, "wandb_run", None)
    if run:
        run.log({prefix + k: res[k] for k in keys if res[k] is not None})


def _gen(model):
    """The generative twins of an untied iDBN (``iDBN.untie``), else None: the model is tied and runs the tied lines."""
    return getattr(model, "__dict__", {}).get("gen_layers")


def _directed_untied(layers, gen, cur, mode, rng):
    """``_directed``'s layer loop for recognition weights ``layers`` and generative twins ``gen``: per layer the wake sample
    ``h ~ q_R(. | v)`` on the tied path's draw (``("u", H)``), then three evaluate-only ``delta_step``s at most:
    ``acc += log p_G(v | h)`` (down on the twin) and ``acc -= log q_R(h | v)`` (mode ``logq``: up with the sample as target) or
    ``acc += `` the entropy of ``q_R(. | v)`` (mode ``entropy``: up with the probabilities as target gives minus the entropy)."""
    acc = None
    for rbm, g in zip(layers, gen):
        eng = _E.get_engine(rbm.W.data)
        p, h = eng.prop_up(rbm, cur, sample=True, rng=rng)
        lp = eng.delta_step(g, "down", h, cur, apply=False) - eng.delta_step(rbm, "up", cur, h if mode == "logq" else p, apply=False)
        acc = lp if acc is None else acc + lp
        cur = h
    return acc, cur


def _directed(layers, v, dev, n_samples, mode, rng, gen=None):
    """The directed layers ``layers`` (binary, bottom first) above the rows ``v``: every row ``n_samples`` times (row b's samples are
    the engine rows b S .. b S + S - 1), one ``bound_step`` per layer -- ``gauss_bound_step`` for a Gaussian one, which only
    ``_gaussian_stack`` lets through (the other callers take their layers from ``_stack``).  ``(acc, top state, B, S)``; ``acc`` None
    without layers.  ``gen``: the generative twins of an untied model (``_directed_untied``)."""
    if mode not in ("entropy", "logq"):
        raise ValueError("mode must be 'entropy' or 'logq'")
    S = int(n_samples)
    if S < 1:
        raise ValueError("n_samples must be >= 1")
    cur = rows_on_device(v, dev)
    B = cur.size(0)
    if S > 1:
        cur = cur.repeat_interleave(S, 0)
    if gen is not None:
        return _directed_untied(layers, gen, cur, mode, rng) + (B, S)
    acc = None
    for rbm in layers:
        eng = _E.get_engine(rbm.W.data)
        if getattr(rbm, "gaussian_visible", False):
            acc, cur = eng.gauss_bound_step(rbm, rbm.logvar.data, cur, rng, acc=acc, mode=mode)
        else:
            acc, cur = eng.bound_step(rbm, cur, rng, acc=acc, mode=mode)
    return acc, cur, B, S


def _column_means(who: str, data, device) -> torch.Tensor:
    """The float64 column means of a tensor ``[N, ...]`` or of a loader of such batches, summed on the device."""
    tot, n = None, 0
    for b in ([data] if isinstance(data, torch.Tensor) else batches(data)):
        x = _first(b)
        x = rows_on_device(x, device if device is not None else x.device).double()
        tot = x.sum(0) if tot is None else tot + x.sum(0)
        n += x.size(0)
    if tot is None or n == 0:
        raise ValueError(f"{who}: no rows")
    return tot / n


@torch.no_grad()
def base_rate_bias(loader_or_tensor, smoothing: float = 0.05, device=None) -> torch.Tensor:
    """Visible biases of the base-rate model: the log-odds of the smoothed pixel means, log(p / (1 - p)) with
    p = (mean + smoothing) / (1 + 2 smoothing) (the "base-rate" start of the AIS paper: the closer A is to the data, the lower
    the variance of the estimate).  A tensor ``[N, ...]`` or a loader of such batches; sums are accumulated on the device."""
    p = (_column_means("base_rate_bias", loader_or_tensor, device) + smoothing) / (1.0 + 2.0 * smoothing)
    return (torch.log(p) - torch.log1p(-p)).float()


def linear_betas(n_betas: int) -> torch.Tensor:
    """``n_betas`` temperature steps: K + 1 = n_betas + 1 float32 values from 0 to 1, evenly spaced."""
    K = int(n_betas)
    if K < 1:
        raise ValueError("n_betas must be >= 1")
    b = torch.arange(K + 1, dtype=torch.float64) / K
    return b.float()


@torch.no_grad()
def estimate_log_partition(rbm, n_chains: int = 256, n_betas: int = 1000, betas=None, base_vis_bias: Optional[torch.Tensor] = None,
                           seed: Optional[int] = None) -> dict:
    """AIS estimate of log Z of ``rbm``: ``log_z``, ``log_z_base`` (log Z_A), ``logw`` (float64 device tensor ``[n_chains]``),
    ``ess`` = (sum w)^2 / sum w^2 (effective sample size) and ``se`` = std(w) / (mean(w) sqrt(M)), the relative standard error of
    the mean weight = the standard error of log Z to first order; both on weights shifted by their maximum.  ``betas`` overrides
    the ``n_betas`` evenly spaced temperatures.  One device-to-host copy.  See the module docstring for ``seed``."""
    return _weight_stats(*_ais_weights(rbm, n_chains, n_betas, betas, base_vis_bias, seed))


def _ais_weights(rbm, n_chains=256, n_betas=1000, betas=None, base_vis_bias=None, seed=None):
    """``(logw, log Z_A)`` of ``estimate_log_partition``, both on the device."""
    _check_binary(rbm)
    betas = linear_betas(n_betas) if betas is None else betas
    logw = _E.get_engine(rbm.W.data).ais(rbm, betas, int(n_chains), _draws(seed), base_vis_bias=base_vis_bias)
    return logw, _log_z_base(rbm, base_vis_bias, logw.device)


@torch.no_grad()
def log_likelihood(rbm, v: torch.Tensor, log_z) -> torch.Tensor:
    """log p(v) = -F(v) - log Z per row, a float64 tensor ``[B]`` on the device of ``v`` (``rbm.free_energy``; no host sync)."""
    _check_binary(rbm)
    return -rbm.free_energy(v).double() - log_z


@torch.no_grad()
def evaluate_log_likelihood(model, loader=None, log_z: Optional[float] = None, max_batches: Optional[int] = None, **ais_kwargs) -> Optional[dict]:
    """Mean held-out log-likelihood of an ``RBM`` -- or of the BOTTOM layer of an ``iDBN`` -- over ``loader`` (default
    ``model.val_loader``; None without one): ``mean_ll``, ``sum_ll``, ``n``, ``log_z``, ``se``, ``ess`` (the last two None when
    ``log_z`` was passed in instead of estimated with ``estimate_log_partition(**ais_kwargs)``).  The sum is accumulated on the
    device; the host synchronises once, after the last batch.  A ragged last batch is fine; ``max_batches`` stops early.  With a
    ``wandb_run`` on the model the scalars are logged as ``ll/...``."""
    return _evaluate_ll(model, loader, log_z, max_batches, ais_kwargs, _check_binary, estimate_log_partition)


def _evaluate_ll(model, loader, log_z, max_batches, ais_kwargs, check, estimate):
    """``evaluate_log_likelihood`` / ``evaluate_gaussian_log_likelihood``: ``check`` admits the bottom RBM, ``estimate`` is its AIS."""
    rbm = _bottom(model)
    check(rbm)
    loader = loader if loader is not None else getattr(model, "val_loader", None)
    if loader is None:
        return None
    log_z, se, ess = _known_or_estimated(log_z, estimate, rbm, ais_kwargs)
    (s,), n = _sum_batches(loader, max_batches, lambda batch: (-rbm.free_energy(rows_on_device(_first(batch), rbm.W.device)).double()
                                                               - log_z).sum().reshape(1), 1)
    res = {"mean_ll": s / max(1, n), "sum_ll": s, "n": n, "log_z": float(log_z), "se": se, "ess": ess}
    _log_scalars(model, "ll/", res, ("mean_ll", "log_z", "se", "ess"))
    return res


# ---- the whole stack: variational lower bound and importance-sampled likelihood of the DBN ---------------------------------------
def _layers(model):
    layers = getattr(model, "layers", None)
    return list(layers) if layers is not None and len(layers) > 0 else [model]


def _stack(model):
    """The RBMs of the stack, bottom first: the layers of an iDBN, or `model` itself as a stack of one.  All Bernoulli."""
    layers = _layers(model)
    for rbm in layers:
        _check_binary(rbm)
    return layers


def _sample_values(layers, v, log_z_top, n_samples, mode, rng, gen=None) -> torch.Tensor:
    top = layers[-1]
    acc, cur, B, S = _directed(layers[:-1], v, top.W.device, n_samples, mode, rng, gen)
    w = -top.free_energy(cur).double() - log_z_top
    if acc is not None:
        w = acc + w
    return w.view(B, S)


@torch.no_grad()
def dbn_sample_values(model, v: torch.Tensor, log_z_top, n_samples: int = 1, mode: str = "entropy", seed: Optional[int] = None) -> torch.Tensor:
    """``w`` of the module docstring for ``n_samples`` draws of the hidden states per row of ``v``: float64 ``[B, n_samples]`` on
    the device (row b's samples are the engine rows b S .. b S + S - 1 of the replicated batch).  One ``bound_step`` per directed
    layer, ``free_energy`` on the top RBM, no host sync.  ``model``: an ``iDBN`` or an ``RBM`` (a stack of one: no draw, and the
    value is ``log_likelihood``).  ``log_z_top``: log Z of the TOP RBM (``estimate_log_partition(model.layers[-1])``)."""
    return _sample_values(_stack(model), v, log_z_top, n_samples, mode, _draws(seed), _gen(model))


@torch.no_grad()
def dbn_lower_bound(model, v: torch.Tensor, log_z_top, n_samples: int = 8, seed: Optional[int] = None) -> torch.Tensor:
    """Monte-Carlo estimate of the variational lower bound on log p_DBN(v) per row: the mean of ``n_samples`` values in mode
    ``entropy``; float64 ``[B]``."""
    return dbn_sample_values(model, v, log_z_top, n_samples, "entropy", seed).mean(1)


def _logmeanexp_rows(w: torch.Tensor) -> torch.Tensor:
    m = w.max(1, keepdim=True).values
    return (m + torch.log(torch.exp(w - m).mean(1, keepdim=True))).squeeze(1)


@torch.no_grad()
def dbn_log_likelihood_is(model, v: torch.Tensor, log_z_top, n_samples: int = 64, seed: Optional[int] = None) -> torch.Tensor:
    """Importance-sampled estimate of log p_DBN(v) per row with q as the proposal: the logmeanexp of ``n_samples`` values in mode
    ``logq`` (in expectation a lower bound that tightens with ``n_samples``); float64 ``[B]``."""
    return _logmeanexp_rows(dbn_sample_values(model, v, log_z_top, n_samples, "logq", seed))


@torch.no_grad()
def evaluate_dbn_bound(model, loader=None, log_z_top: Optional[float] = None, n_samples: int = 8, max_batches: Optional[int] = None,
                       importance: bool = False, **ais_kwargs) -> Optional[dict]:
    """Mean held-out ``dbn_lower_bound`` (``importance=True``: ``dbn_log_likelihood_is``) of the stack over ``loader`` (default
    ``model.val_loader``; None without one): ``mean_bound``, ``sum_bound``, ``n``, ``log_z_top``, ``se``, ``ess`` (of the AIS
    estimate; None when ``log_z_top`` was passed in instead of estimated with ``estimate_log_partition(top_rbm, **ais_kwargs)``)
    and ``n_samples``.  A ``seed`` among ``ais_kwargs`` also puts the hidden samples of all batches under ONE private draw source,
    so evaluating between epochs does not change training.  The sum is accumulated on the device; the host synchronises once,
    after the last batch.  A ragged last batch is fine; ``max_batches`` stops early.  With a ``wandb_run`` on the model the
    scalars are logged as ``ll/dbn_...``."""
    return _evaluate_bound(model, _stack(model), estimate_log_partition, "ll/dbn_", _gen(model), loader, log_z_top, n_samples,
                           max_batches, importance, ais_kwargs)


def _evaluate_bound(model, layers, estimate, prefix, gen, loader, log_z_top, n_samples, max_batches, importance, ais_kwargs):
    """``evaluate_dbn_bound`` / ``evaluate_gaussian_dbn_bound`` over the checked ``layers``: ``estimate`` is the AIS of the top RBM,
    ``prefix`` that of the logged scalars, ``gen`` the generative twins of an untied model."""
    loader = loader if loader is not None else getattr(model, "val_loader", None)
    if loader is None:
        return None
    log_z_top, se, ess = _known_or_estimated(log_z_top, estimate, layers[-1], ais_kwargs)
    rng = _draws(ais_kwargs.get("seed"))

    def sums(batch):
        w = _sample_values(layers, _first(batch), log_z_top, n_samples, "logq" if importance else "entropy", rng, gen)
        return (_logmeanexp_rows(w) if importance else w.mean(1)).sum().reshape(1)

    (s,), n = _sum_batches(loader, max_batches, sums, 1)
    res = {"mean_bound": s / max(1, n), "sum_bound": s, "n": n, "log_z_top": float(log_z_top), "se": se, "ess": ess, "n_samples": int(n_samples)}
    _log_scalars(model, prefix, res, ("mean_bound", "log_z_top", "se", "ess", "n_samples"))
    return res


# ---- the multimodal model: joint RBM with a softmax group above a directed image stack -------------------------------------------
def _label_index(y: torch.Tensor) -> torch.Tensor:
    """Class indices ``[B]`` from a one-hot / score tensor ``[B, K]`` (argmax) or from indices."""
    return y.argmax(dim=1) if y.dim() == 2 else y


@torch.no_grad()
def base_rate_bias_joint(model, loader=None, smoothing: float = 0.05) -> torch.Tensor:
    """Visible biases ``[Dz + K]`` of the base-rate model of ``model.joint_rbm``, from the ``(img, y)`` batches of ``loader``
    (default ``model.dataloader``).  Code columns: the log-odds of the smoothed mean code, as ``base_rate_bias`` gives them for
    ``model.image_idbn.represent(img)``.  Label columns: the log of the smoothed class frequencies
    ``(count_k + smoothing n) / (n + K smoothing n)`` -- the logits of the base model's categorical.  Sums on the device."""
    loader = loader if loader is not None else getattr(model, "dataloader", None)
    if loader is None:
        raise ValueError("base_rate_bias_joint: no loader")
    dev = model.joint_rbm.W.device
    K = int(model.num_labels)
    tot, cnt, n = None, torch.zeros(K, dtype=torch.float64, device=dev), 0
    for img, y in batches(loader):
        z = model.image_idbn.represent(rows_on_device(img, dev)).double()
        tot = z.sum(0) if tot is None else tot + z.sum(0)
        cnt += torch.bincount(_label_index(y.to(dev)).long(), minlength=K)[:K].double()
        n += z.size(0)
    if tot is None or n == 0:
        raise ValueError("base_rate_bias_joint: no rows")
    p = (tot / n + smoothing) / (1.0 + 2.0 * smoothing)
    f = (cnt / n + smoothing) / (1.0 + K * smoothing)
    return torch.cat([torch.log(p) - torch.log1p(-p), torch.log(f)]).float()


@torch.no_grad()
def estimate_joint_log_partition(rbm, n_chains: int = 256, n_betas: int = 1000, betas=None, base_vis_bias: Optional[torch.Tensor] = None,
                                 seed: Optional[int] = None) -> dict:
    """``estimate_log_partition`` for an RBM with softmax groups (the joint RBM of an ``iMDBN``): the same dict, from
    ``HipEngine.ais_groups``, with ``log_z_base`` = H log 2 + sum_{i outside groups} softplus(b_A,i) + sum_g logsumexp(b_A[g])
    (no ``base_vis_bias``: zeros, i.e. log 2 per Bernoulli column and log(width) per group).  One device-to-host copy."""
    return _weight_stats(*_joint_ais_weights(rbm, n_chains, n_betas, betas, base_vis_bias, seed))


def _joint_ais_weights(rbm, n_chains=256, n_betas=1000, betas=None, base_vis_bias=None, seed=None):
    """``(logw, log Z_A)`` of ``estimate_joint_log_partition``, both on the device."""
    betas = linear_betas(n_betas) if betas is None else betas
    logw = _E.get_engine(rbm.W.data).ais_groups(rbm, betas, int(n_chains), _draws(seed), base_vis_bias=base_vis_bias)
    return logw, _log_z_base(rbm, base_vis_bias, logw.device)


def _imdbn_values(model, img, y, log_z_joint, n_samples, mode, rng):
    jr = model.joint_rbm
    dev = jr.W.device
    # ALL image layers are directed: the joint RBM sits above the top one
    acc, cur, B, S = _directed(_stack(model.image_idbn), img, dev, n_samples, mode, rng)
    gt = _label_index(y.to(dev)).to(torch.int32)
    if S > 1:
        gt = gt.repeat_interleave(S, 0)
    joint, marg = _E.get_engine(jr.W.data).label_loglik(jr, cur, int(model.num_labels), gt)
    return (acc + joint - log_z_joint).view(B, S), (acc + marg - log_z_joint).view(B, S)


@torch.no_grad()
def imdbn_sample_values(model, img: torch.Tensor, y: torch.Tensor, log_z_joint, n_samples: int = 1, mode: str = "entropy",
                        seed: Optional[int] = None):
    """``(joint, marginal)``: ``w_joint`` and ``w_image`` of the module docstring for ``n_samples`` draws of the hidden states per
    row, float64 ``[B, n_samples]`` on the device (row b's samples are the engine rows b S .. b S + S - 1 of the replicated batch).
    ``y``: one-hot ``[B, K]`` or class indices ``[B]``; a label outside ``[0, K)`` makes that row's ``joint`` NaN.  One
    ``bound_step`` per image layer, one ``label_loglik``, no host sync.  The model meant has a BINARY code z (module docstring).
    ``log_z_joint``: log Z of the joint RBM (``estimate_joint_log_partition(model.joint_rbm)``)."""
    return _imdbn_values(model, img, y, log_z_joint, n_samples, mode, _draws(seed))


@torch.no_grad()
def imdbn_lower_bound(model, img: torch.Tensor, y: torch.Tensor, log_z_joint, n_samples: int = 8, seed: Optional[int] = None):
    """Monte-Carlo estimates of the variational lower bounds on log p(img, y) and on log p(img) per row (binary-z model): the means
    of ``n_samples`` values in mode ``entropy``; ``(joint, image)``, float64 ``[B]`` each."""
    j, m = imdbn_sample_values(model, img, y, log_z_joint, n_samples, "entropy", seed)
    return j.mean(1), m.mean(1)


@torch.no_grad()
def imdbn_log_likelihood_is(model, img: torch.Tensor, y: torch.Tensor, log_z_joint, n_samples: int = 64, seed: Optional[int] = None):
    """Importance-sampled estimates of log p(img, y) and log p(img) per row (binary-z model) with q as the proposal: the logmeanexp
    of ``n_samples`` values in mode ``logq``; ``(joint, image)``, float64 ``[B]`` each."""
    j, m = imdbn_sample_values(model, img, y, log_z_joint, n_samples, "logq", seed)
    return _logmeanexp_rows(j), _logmeanexp_rows(m)


@torch.no_grad()
def evaluate_imdbn_bound(model, loader=None, log_z_joint: Optional[float] = None, n_samples: int = 8, max_batches: Optional[int] = None,
                         **ais_kwargs) -> Optional[dict]:
    """Mean held-out ``imdbn_lower_bound`` of an ``iMDBN`` over the ``(img, y)`` batches of ``loader`` (default
    ``model.val_loader``; None without one): ``mean_joint_bound`` (bound on log p(img, y)), ``mean_image_bound`` (bound on
    log p(img), the label summed out), ``mean_label_logprob``, ``n``, ``log_z_joint``, ``se``, ``ess`` (of the AIS estimate; None
    when ``log_z_joint`` was passed in instead of estimated with ``estimate_joint_log_partition(model.joint_rbm, **ais_kwargs)``)
    and ``n_samples``.  ``mean_label_logprob`` is the mean over rows and samples of ``joint - marginal`` = the exact
    log p(y | z) of the SAMPLED code z under the joint RBM: a diagnostic, NOT a bound on log p(y | img).  All numbers are those of
    the binary-z model (module docstring).  A ``seed`` among ``ais_kwargs`` also puts the hidden samples of all batches under ONE
    private draw source.  Sums are accumulated on the device; the host synchronises once, after the last batch.  A ragged last
    batch is fine; ``max_batches`` stops early.  With a ``wandb_run`` on the model the scalars are logged as ``ll/imdbn_...``."""
    loader = loader if loader is not None else getattr(model, "val_loader", None)
    if loader is None:
        return None
    log_z_joint, se, ess = _known_or_estimated(log_z_joint, estimate_joint_log_partition, model.joint_rbm, ais_kwargs)
    rng = _draws(ais_kwargs.get("seed"))

    def sums(batch):
        j, m = _imdbn_values(model, batch[0], batch[1], log_z_joint, n_samples, "entropy", rng)
        return torch.stack([j.mean(1).sum(), m.mean(1).sum(), (j - m).mean(1).sum()])

    t, n = _sum_batches(loader, max_batches, sums, 3)
    d = max(1, n)
    res = {"mean_joint_bound": t[0] / d, "mean_image_bound": t[1] / d, "mean_label_logprob": t[2] / d, "n": n,
           "log_z_joint": float(log_z_joint), "se": se, "ess": ess, "n_samples": int(n_samples)}
    _log_scalars(model, "ll/imdbn_", res, ("mean_joint_bound", "mean_image_bound", "mean_label_logprob", "log_z_joint", "se", "ess",
                                            "n_samples"))
    return res


# ---- the conservative side: reverse annealed importance sampling ------------------------------------------------------------------
def _bernoulli_reverse(eng, rbm, rows, betas, rng, base_vis_bias):
    return eng.reverse_ais(rbm, rows, betas, rng, base_vis_bias=base_vis_bias)


# A side of the reverse estimate: (the name its errors carry, the engine call over one chunk of rows, log Z_A of the base-rate model)
_REVERSE_BERNOULLI = ("reverse_ais_log_likelihood", _bernoulli_reverse, _log_z_base)


def _reverse_rows(rbm, v, n_chains, betas, base_vis_bias, rng, max_rows, side=_REVERSE_BERNOULLI):
    """``(ll [B], ess [B], logw [B, M])`` of ``reverse_ais_log_likelihood`` -- ``side=_REVERSE_GAUSSIAN``: of
    ``gaussian_reverse_ais_log_likelihood`` -- under the draw source ``rng``, which advances by ONE schedule however many chunks ran:
    every chunk draws from the same draw numbers, keyed on its global rows."""
    who, run, log_z_base = side
    M = int(n_chains)
    if M < 1:
        raise ValueError("n_chains must be >= 1")
    if int(max_rows) < 1:
        raise ValueError("max_rows must be >= 1")
    dev = rbm.W.device
    if v.size(0) < 1:
        raise ValueError(f"{who}: no rows")
    v = rows_on_device(v, dev)
    B = v.size(0)
    if v.size(1) != rbm.W.shape[0]:
        raise ValueError(f"{who}: rows of {v.size(1)} elements, the RBM has {rbm.W.shape[0]} visible units")
    if base_vis_bias is not None and base_vis_bias.numel() != rbm.W.shape[0]:
        raise ValueError(f"base_vis_bias must have {rbm.W.shape[0]} elements")
    eng = _E.get_engine(rbm.W.data)
    per = max(1, int(max_rows) // M)
    philox = isinstance(rng, _E.PhiloxRng)
    if not philox and B > per:
        raise ValueError(f"{who}: more than one chunk of rows needs a PhiloxRng (draws keyed on the global row)")
    parts, used = [], 0
    for s in range(0, B, per):
        rows = v[s:s + per].repeat_interleave(M, 0) if M > 1 else v[s:s + per]
        r = rng
        if philox:
            r = _E.PhiloxRng(rng.seed, row0=rng.row0 + s * M)
            r.offset, r.device_counter = rng.offset, rng.device_counter
        parts.append(run(eng, rbm, rows, betas, r, base_vis_bias))
        if philox:
            used = r.offset - rng.offset
    if philox:
        rng.advance(used)
    logw = parts[0] if len(parts) == 1 else torch.cat(parts)
    lme, ess = eng.rows_logmeanexp(logw, M)
    return lme - log_z_base(rbm, base_vis_bias, logw.device), ess, logw.view(B, M)


@torch.no_grad()
def reverse_ais_log_likelihood(rbm, v: torch.Tensor, n_chains: int = 16, n_betas: int = 1000, betas=None,
                               base_vis_bias: Optional[torch.Tensor] = None, seed: Optional[int] = None, max_rows: int = 4096) -> dict:
    """Reverse-AIS estimate of log p_ann(v) per row of ``v`` (0/1): ``{"ll": float64 [B], "ess": float64 [B], "logw": float64
    [B, n_chains]}`` on the device.  ``ll = -log Z_A + logmeanexp(logw)``: exp(ll) is an unbiased estimate of p_ann(v), so ``ll`` is a
    stochastic LOWER bound on log p_ann(v), the likelihood under the annealing model of the module docstring -- conservative where
    ``log_likelihood`` with an AIS log Z is optimistic.  ``ess`` = (sum w)^2 / sum w^2 over the row's chains.  RBMs with softmax groups
    are accepted (``base_vis_bias`` inside a group: the logits of a categorical, as in ``estimate_joint_log_partition``).  A row
    that is not 0/1 (or a group without exactly one 1) gives NaN in that row.  Rows are processed in chunks of at most
    ``max_rows // n_chains`` (engine rows = rows x chains); a chunk's draws are keyed on ``first_row * n_chains``, so a row's chains
    see the same draws whatever the chunking (the same bits while the chunks stay within the same multiple of 64 engine rows, the
    engine's rule for batch sizes).  ``K (2 + G)`` draw tensors for K temperatures and G groups.  No host sync."""
    if getattr(rbm, "gaussian_visible", False):
        raise ValueError("reverse_ais_log_likelihood needs Bernoulli visibles: this RBM's visible layer is Gaussian (DESIGN section 29)")
    betas = linear_betas(n_betas) if betas is None else betas
    ll, ess, logw = _reverse_rows(rbm, v, n_chains, betas, base_vis_bias, _draws(seed), max_rows)
    return {"ll": ll, "ess": ess, "logw": logw}


@torch.no_grad()
def evaluate_log_likelihood_sandwich(model, loader=None, max_batches: Optional[int] = None, **kwargs) -> Optional[dict]:
    """Both sides of the held-out log-likelihood of an ``RBM`` -- or of the BOTTOM layer of an ``iDBN`` -- over ``loader`` (default
    ``model.val_loader``; None without one): ``mean_ll_ais`` (``log_likelihood`` with the AIS log Z: optimistic),
    ``mean_ll_reverse`` (``reverse_ais_log_likelihood``: conservative), ``gap`` = their difference (a long enough ladder closes it),
    ``n``, ``log_z``, ``se``, ``ess`` (of the AIS estimate) and ``ess_reverse`` (mean over rows).  ``kwargs``: ``n_chains``,
    ``n_betas``, ``betas``, ``base_vis_bias``, ``seed`` as ``estimate_log_partition`` takes them, and ``n_chains_reverse`` (16),
    ``max_rows`` for the reverse side, which shares the ladder and the base-rate bias; one draw source carries the AIS run and then
    every batch.  Binary visibles only (the AIS side).  Everything is accumulated on the device; the host synchronises ONCE, after
    the last batch.  With a ``wandb_run`` on the model the scalars are logged as ``ll/...``."""
    return _evaluate_sandwich("evaluate_log_likelihood_sandwich", model, loader, max_batches, kwargs, _check_binary,
                              lambda eng, rbm, betas, M, rng, bA: eng.ais(rbm, betas, M, rng, base_vis_bias=bA), _REVERSE_BERNOULLI, "ll/")


def _evaluate_sandwich(who, model, loader, max_batches, kwargs, check, ais, side, prefix):
    """``evaluate_log_likelihood_sandwich`` / ``evaluate_gaussian_log_likelihood_sandwich``: ``check`` admits the bottom RBM, ``ais`` is
    its forward engine call, ``side`` its reverse side (whose log Z_A is the forward one's), ``prefix`` that of the logged scalars."""
    rbm = _bottom(model)
    check(rbm)
    loader = loader if loader is not None else getattr(model, "val_loader", None)
    if loader is None:
        return None
    M = int(kwargs.pop("n_chains", 256))
    Mr = int(kwargs.pop("n_chains_reverse", 16))
    betas = kwargs.pop("betas", None)
    betas = linear_betas(kwargs.pop("n_betas", 1000)) if betas is None else betas
    bA, seed, max_rows = kwargs.pop("base_vis_bias", None), kwargs.pop("seed", None), kwargs.pop("max_rows", 4096)
    if kwargs:
        raise TypeError(f"{who}: unexpected arguments {sorted(kwargs)}")
    rng = _draws(seed)
    logw = ais(_E.get_engine(rbm.W.data), rbm, betas, M, rng, bA)
    stats = _weight_stats_device(logw, side[2](rbm, bA, logw.device))          # log_z, log_z_base, ess, se
    log_z = stats[0]

    def sums(batch):
        v = rows_on_device(_first(batch), rbm.W.device)
        ll_r, ess_r, _ = _reverse_rows(rbm, v, Mr, betas, bA, rng, max_rows, side)
        ll_a = -rbm.free_energy(v).double().to(log_z.device) - log_z
        return torch.stack([ll_a.sum(), ll_r.sum(), ess_r.sum()])

    host, n = _sum_batches(loader, max_batches, sums, 3, extra=stats)
    d = max(1, n)
    res = {"mean_ll_ais": host[0] / d, "mean_ll_reverse": host[1] / d, "gap": (host[0] - host[1]) / d, "n": n,
           "log_z": host[3], "se": host[6], "ess": host[5], "ess_reverse": host[2] / d}
    _log_scalars(model, prefix, res, ("mean_ll_ais", "mean_ll_reverse", "gap", "log_z", "se", "ess", "ess_reverse"))
    return res


def _conservative_values(layers, v, n_samples, n_chains, betas, base_vis_bias, rng, max_rows, gen=None, side=_REVERSE_BERNOULLI):
    """``(w [B, S], ess [B, S])``: the directed layers as ``_sample_values`` in mode ``entropy``, the top term from reverse AIS
    (``side``: the top RBM's) on the sampled top-layer states."""
    top = layers[-1]
    acc, cur, B, S = _directed(layers[:-1], v, top.W.device, n_samples, "entropy", rng, gen)
    w, ess, _ = _reverse_rows(top, cur, n_chains, betas, base_vis_bias, rng, max_rows, side)
    if acc is not None:
        w = acc.to(w.device) + w
    return w.view(B, S), ess.view(B, S)


@torch.no_grad()
def dbn_conservative_bound(model, v: torch.Tensor, n_samples: int = 8, n_chains: int = 16, n_betas: int = 1000, betas=None,
                           base_vis_bias: Optional[torch.Tensor] = None, seed: Optional[int] = None, max_rows: int = 4096) -> torch.Tensor:
    """``dbn_lower_bound`` without an AIS estimate in it: the directed layers through ``bound_step`` in mode ``entropy``
    (``n_samples`` draws of the hidden states per row), and in place of ``-F_top - log Z_top`` the reverse-AIS estimate of
    log p_ann of the top RBM at the sampled top-layer state (``n_chains`` chains each; ``base_vis_bias``: the TOP RBM's base-rate
    model).  In expectation a lower bound on the variational bound of the stack whose top is the annealing model; float64 ``[B]``
    on the device, no host sync.  ``model``: an ``iDBN`` or an ``RBM`` (a stack of one: ``reverse_ais_log_likelihood``)."""
    betas = linear_betas(n_betas) if betas is None else betas
    return _conservative_values(_stack(model), v, n_samples, n_chains, betas, base_vis_bias, _draws(seed), max_rows, _gen(model))[0].mean(1)


@torch.no_grad()
def evaluate_dbn_bound_conservative(model, loader=None, n_samples: int = 8, n_chains: int = 16, max_batches: Optional[int] = None,
                                    n_betas: int = 1000, betas=None, base_vis_bias: Optional[torch.Tensor] = None,
                                    seed: Optional[int] = None, max_rows: int = 4096) -> Optional[dict]:
    """Mean held-out ``dbn_conservative_bound`` of the stack over ``loader`` (default ``model.val_loader``; None without one):
    ``mean_bound``, ``sum_bound``, ``n``, ``ess_reverse`` (mean over rows and samples), ``n_samples``, ``n_chains``.  One draw source
    carries every batch (``seed``: a private one).  Sums on the device, one host sync after the last batch.  With a ``wandb_run`` on
    the model the scalars are logged as ``ll/dbn_conservative_...``."""
    return _evaluate_conservative(model, _stack(model), _REVERSE_BERNOULLI, "ll/dbn_conservative_", _gen(model), loader, n_samples,
                                  n_chains, max_batches, n_betas, betas, base_vis_bias, seed, max_rows)


def _evaluate_conservative(model, layers, side, prefix, gen, loader, n_samples, n_chains, max_batches, n_betas, betas, base_vis_bias, seed,
                           max_rows):
    """``evaluate_dbn_bound_conservative`` / ``evaluate_gaussian_dbn_bound_conservative`` over the checked ``layers``: ``side`` is the
    reverse side of the top RBM, ``prefix`` that of the logged scalars, ``gen`` the generative twins of an untied model."""
    loader = loader if loader is not None else getattr(model, "val_loader", None)
    if loader is None:
        return None
    betas = linear_betas(n_betas) if betas is None else betas
    rng = _draws(seed)

    def sums(batch):
        w, ess = _conservative_values(layers, _first(batch), n_samples, n_chains, betas, base_vis_bias, rng, max_rows, gen, side)
        return torch.stack([w.mean(1).sum(), ess.mean(1).sum()])

    t, n = _sum_batches(loader, max_batches, sums, 2)
    d = max(1, n)
    res = {"mean_bound": t[0] / d, "sum_bound": t[0], "n": n, "ess_reverse": t[1] / d, "n_samples": int(n_samples), "n_chains": int(n_chains)}
    _log_scalars(model, prefix, res, ("mean_bound", "ess_reverse", "n_samples", "n_chains"))
    return res


# ---- the cheap monitor: exact pseudo-log-likelihood --------------------------------------------------------------------------------
def _n_sites(rbm) -> int:
    """Sites of a row: the visible columns outside the softmax groups, plus one per group."""
    groups = getattr(rbm, "softmax_groups", None) or []
    return int(rbm.W.shape[0]) - sum(int(e) - int(s) for s, e in groups) + len(groups)


@torch.no_grad()
def pseudo_log_likelihood(model, v: torch.Tensor, return_sites: bool = False):
    """Exact PLL(v) = sum_sites log p(v_site | v_rest) per row of ``v`` (0/1, one-hot softmax groups) under an ``RBM`` -- or the BOTTOM
    layer of an ``iDBN``: float64 ``[B]`` on the device; with ``return_sites`` also the per-column terms, fp32 ``[B, V]`` (a group's
    term at its observed column, 0 in the group's other columns; a row sums to its PLL).  A row that is not 0/1, or a group without
    exactly one 1, is NaN.  One ``HipEngine.pseudo_loglik`` call; no draws, no host sync."""
    rbm = _bottom(model)
    if getattr(rbm, "gaussian_visible", False):
        raise ValueError("pseudo_log_likelihood needs Bernoulli visibles: this RBM's visible layer is Gaussian (DESIGN section 29)")
    return _E.get_engine(rbm.W.data).pseudo_loglik(rbm, rows_on_device(v, rbm.W.device), return_sites=return_sites)


@torch.no_grad()
def evaluate_pseudo_likelihood(model, loader=None, max_batches: Optional[int] = None) -> Optional[dict]:
    """Mean held-out ``pseudo_log_likelihood`` of an ``RBM`` -- or of the BOTTOM layer of an ``iDBN`` -- over ``loader`` (default
    ``model.val_loader``; None without one): ``mean_pll``, ``sum_pll``, ``n`` (the valid rows), ``mean_site`` = mean_pll / number of
    sites (the mean log-probability of one site given the rest) and ``n_invalid``: the NaN rows, which are counted and left out of
    the sums.  Sums on the device, ONE host copy after the last batch.  A ragged last batch is fine; ``max_batches`` stops early.
    With a ``wandb_run`` on the model the scalars are logged as ``ll/pll_...``."""
    rbm = _bottom(model)
    loader = loader if loader is not None else getattr(model, "val_loader", None)
    if loader is None:
        return None

    def sums(batch):
        pll = pseudo_log_likelihood(rbm, _first(batch))
        bad = torch.isnan(pll)
        return torch.stack([torch.where(bad, torch.zeros_like(pll), pll).sum(), bad.sum().double()])

    (s, bad), rows = _sum_batches(loader, max_batches, sums, 2)
    n = rows - int(bad)
    mean = s / max(1, n)
    res = {"mean_pll": mean, "sum_pll": s, "n": n, "mean_site": mean / _n_sites(rbm), "n_invalid": int(bad)}
    _log_scalars(model, "ll/pll_", res, ("mean_pll", "mean_site", "n", "n_invalid"))
    return res


@torch.no_grad()
def imdbn_pseudo_log_likelihood(model, img: torch.Tensor, y: torch.Tensor, seed: Optional[int] = None):
    """``(pll_joint [B], log_p_y_given_z [B])``, float64 on the device: the pseudo-log-likelihood of ``model.joint_rbm`` at the rows
    ``[z | one-hot y]``, z the binary code drawn from the image layers as ``imdbn_sample_values`` draws it (one sample per row, one
    ``bound_step`` per image layer), and the label group's site term, which is the exact log p(y | z) of the joint RBM -- the
    classification log-loss, without a chain.  ``y``: one-hot ``[B, K]`` or class indices ``[B]``; a label outside ``[0, K)`` leaves
    the group empty and makes both outputs of that row NaN.  See the module docstring for ``seed``.  No host sync."""
    jr = model.joint_rbm
    dev = jr.W.device
    _, z, B, _ = _directed(_stack(model.image_idbn), img, dev, 1, "entropy", _draws(seed))
    K = int(model.num_labels)
    Dz = z.size(1)
    gt = _label_index(y.to(dev)).long()
    rows = torch.zeros(B, Dz + K, device=dev)
    rows[:, :Dz] = z
    ok = (gt >= 0) & (gt < K)
    rows[:, Dz:] = torch.nn.functional.one_hot(torch.where(ok, gt, torch.zeros_like(gt)), K).float() * ok.unsqueeze(1).float()
    pll, sites = _E.get_engine(jr.W.data).pseudo_loglik(jr, rows, return_sites=True)
    return pll, sites[:, Dz:].double().sum(1)


# ---- Gaussian visible units (imdbn/models/grbm.py) -------------------------------------------------------------------
def _check_gaussian(rbm):
    if not getattr(rbm, "gaussian_visible", False):
        raise ValueError("the Gaussian likelihood functions need a GaussianRBM (Gaussian visible units, DESIGN section 29); "
                         "Bernoulli layers have estimate_log_partition / log_likelihood")


@torch.no_grad()
def gaussian_base_rate_bias(data, device=None) -> torch.Tensor:
    """Visible bias of the Gaussian base-rate model: the column means of the data.  A tensor ``[N, ...]`` or a loader of such batches;
    sums are accumulated on the device in float64."""
    return _column_means("gaussian_base_rate_bias", data, device).float()


def _gaussian_log_z_base(rbm, dev) -> torch.Tensor:
    """log Z_A of the Gaussian base-rate model (float64 scalar on ``dev``): H log 2 + (V / 2) log 2 pi + sum(logvar) / 2 -- whatever b_A."""
    V, H = rbm.W.shape
    return rbm.logvar.data.to(dev).double().sum() * 0.5 + (H * math.log(2.0) + 0.5 * V * math.log(2.0 * math.pi))


@torch.no_grad()
def estimate_gaussian_log_partition(rbm, n_chains: int = 256, n_betas: int = 1000, betas=None, base_vis_bias: Optional[torch.Tensor] = None,
                                    seed: Optional[int] = None) -> dict:
    """AIS estimate of log Z of a ``GaussianRBM``: the keys of ``estimate_log_partition`` (``log_z``, ``log_z_base``, ``logw``,
    ``ess``, ``se``).  ``base_vis_bias`` None: the RBM's own visible bias (module docstring).  One device-to-host copy; ``seed`` as
    in ``estimate_log_partition``."""
    return _weight_stats(*_gaussian_ais_weights(rbm, n_chains, n_betas, betas, base_vis_bias, seed))


def _gaussian_ais_weights(rbm, n_chains=256, n_betas=1000, betas=None, base_vis_bias=None, seed=None):
    """``(logw, log Z_A)`` of ``estimate_gaussian_log_partition``, both on the device."""
    _check_gaussian(rbm)
    if base_vis_bias is not None and base_vis_bias.numel() != rbm.W.shape[0]:
        raise ValueError(f"base_vis_bias must have {rbm.W.shape[0]} elements")
    betas = linear_betas(n_betas) if betas is None else betas
    logw = _E.get_engine(rbm.W.data).gauss_ais(rbm, rbm.logvar.data, betas, int(n_chains), _draws(seed), base_vis_bias=base_vis_bias)
    return logw, _gaussian_log_z_base(rbm, logw.device)


@torch.no_grad()
def gaussian_log_likelihood(rbm, v: torch.Tensor, log_z) -> torch.Tensor:
    """log p(v) = -F(v) - log Z per row, the log-density of a ``GaussianRBM``: a float64 tensor ``[B]`` on the device of ``v``
    (``rbm.free_energy``; no host sync)."""
    _check_gaussian(rbm)
    return -rbm.free_energy(v).double() - log_z


@torch.no_grad()
def evaluate_gaussian_log_likelihood(model, loader=None, log_z: Optional[float] = None, max_batches: Optional[int] = None,
                                     **ais_kwargs) -> Optional[dict]:
    """Mean held-out log-density of a ``GaussianRBM`` -- or of the BOTTOM layer of an ``iDBN`` built with ``GAUSSIAN_VISIBLE`` -- over
    ``loader`` (default ``model.val_loader``; None without one): the keys of ``evaluate_log_likelihood``.  ``log_z`` None: estimated
    with ``estimate_gaussian_log_partition(**ais_kwargs)``.  Sums on the device, one host sync after the last batch; with a
    ``wandb_run`` on the model the scalars are logged as ``ll/...``."""
    return _evaluate_ll(model, loader, log_z, max_batches, ais_kwargs, _check_gaussian, estimate_gaussian_log_partition)


# ---- the whole stack above a Gaussian bottom layer -------------------------------------------------------------
def _gaussian_stack(model):
    """The RBMs of a stack with a Gaussian bottom layer, bottom first: the layers of an ``iDBN`` built with ``GAUSSIAN_VISIBLE``, or
    a ``GaussianRBM`` as a stack of one.  Every layer above the bottom one is Bernoulli without softmax groups."""
    layers = _layers(model)
    if not getattr(layers[0], "gaussian_visible", False):
        raise ValueError("the Gaussian stack bounds need a GaussianRBM as the bottom layer (an iDBN built with GAUSSIAN_VISIBLE, or a "
                         "GaussianRBM; DESIGN section 31); Bernoulli stacks have dbn_lower_bound / dbn_log_likelihood_is")
    if _gen(model) is not None:
        raise NotImplementedError("the Gaussian stack bounds have no untied form (gen_layers present)")
    for rbm in layers[1:]:
        _check_binary(rbm)
    return layers


@torch.no_grad()
def gaussian_dbn_sample_values(model, v: torch.Tensor, log_z_top, n_samples: int = 1, mode: str = "entropy",
                               seed: Optional[int] = None) -> torch.Tensor:
    """``dbn_sample_values`` for a stack with a Gaussian bottom layer (module docstring): float64 ``[B, n_samples]`` on the device
    (row b's samples are the engine rows b S .. b S + S - 1 of the replicated batch).  One ``gauss_bound_step`` on layer 0, one
    ``bound_step`` per directed Bernoulli layer on the same accumulator, ``free_energy`` on the top RBM, no host sync.  ``model``: an
    ``iDBN`` built with ``GAUSSIAN_VISIBLE`` or a ``GaussianRBM`` (a stack of one: no draw, the value is ``gaussian_log_likelihood``
    and ``log_z_top`` is the Gaussian log Z).  ``log_z_top``: log Z of the TOP RBM."""
    return _sample_values(_gaussian_stack(model), v, log_z_top, n_samples, mode, _draws(seed))


@torch.no_grad()
def gaussian_dbn_lower_bound(model, v: torch.Tensor, log_z_top, n_samples: int = 8, seed: Optional[int] = None) -> torch.Tensor:
    """Monte-Carlo estimate of the variational lower bound on the log-density log p_DBN(v) per row: the mean of ``n_samples`` values in
    mode ``entropy``; float64 ``[B]``."""
    return gaussian_dbn_sample_values(model, v, log_z_top, n_samples, "entropy", seed).mean(1)


@torch.no_grad()
def gaussian_dbn_log_likelihood_is(model, v: torch.Tensor, log_z_top, n_samples: int = 64, seed: Optional[int] = None) -> torch.Tensor:
    """Importance-sampled estimate of the log-density log p_DBN(v) per row with q as the proposal: the logmeanexp of ``n_samples``
    values in mode ``logq`` (in expectation a lower bound that tightens with ``n_samples``); float64 ``[B]``."""
    return _logmeanexp_rows(gaussian_dbn_sample_values(model, v, log_z_top, n_samples, "logq", seed))


@torch.no_grad()
def evaluate_gaussian_dbn_bound(model, loader=None, log_z_top: Optional[float] = None, n_samples: int = 8, max_batches: Optional[int] = None,
                                importance: bool = False, **ais_kwargs) -> Optional[dict]:
    """``evaluate_dbn_bound`` for a stack with a Gaussian bottom layer: the mean held-out ``gaussian_dbn_lower_bound``
    (``importance=True``: ``gaussian_dbn_log_likelihood_is``) over ``loader`` (default ``model.val_loader``; None without one), the
    same keys.  ``log_z_top`` None: ``estimate_log_partition(top_rbm, **ais_kwargs)`` for two layers and more,
    ``estimate_gaussian_log_partition`` for a stack of one.  A ``seed`` among ``ais_kwargs`` also carries the hidden samples of all
    batches; the sum is accumulated on the device and the host synchronises once, after the last batch.  With a ``wandb_run`` on the
    model the scalars are logged as ``ll/gdbn_...``."""
    layers = _gaussian_stack(model)
    estimate = estimate_log_partition if len(layers) > 1 else estimate_gaussian_log_partition
    return _evaluate_bound(model, layers, estimate, "ll/gdbn_", None, loader, log_z_top, n_samples, max_batches, importance, ais_kwargs)


# ---- the conservative side under Gaussian visibles -------------------------------------------------------------
def _gaussian_reverse(eng, rbm, rows, betas, rng, base_vis_bias):
    return eng.gauss_reverse_ais(rbm, rbm.logvar.data, rows, betas, rng, base_vis_bias=base_vis_bias)


_REVERSE_GAUSSIAN = ("gaussian_reverse_ais_log_likelihood", _gaussian_reverse, lambda rbm, base_vis_bias, dev: _gaussian_log_z_base(rbm, dev))


@torch.no_grad()
def gaussian_reverse_ais_log_likelihood(rbm, v: torch.Tensor, n_chains: int = 16, n_betas: int = 1000, betas=None,
                                        base_vis_bias: Optional[torch.Tensor] = None, seed: Optional[int] = None, max_rows: int = 4096) -> dict:
    """Reverse-AIS estimate of the log-density log p_ann(v) per row of ``v`` (real) under a ``GaussianRBM``: the keys and shapes of
    ``reverse_ais_log_likelihood`` (``ll``, ``ess`` float64 ``[B]``, ``logw`` float64 ``[B, n_chains]``, on the device).
    ``ll = -log Z_A + logmeanexp(logw)`` with log Z_A = H log 2 + (V / 2) log 2 pi + sum(logvar) / 2: exp(ll) is an unbiased estimate
    of p_ann(v), the density of the annealing model of ``estimate_gaussian_log_partition`` on the same ladder, so ``ll`` is
    conservative where ``gaussian_log_likelihood`` with an AIS log Z is optimistic.  ``base_vis_bias`` None: the RBM's own visible
    bias.  A row with a non-finite element gives NaN in that row.  Chunks, draws (``2 K`` draw tensors) and ``seed`` as in
    ``reverse_ais_log_likelihood``.  No host sync."""
    _check_gaussian(rbm)
    betas = linear_betas(n_betas) if betas is None else betas
    ll, ess, logw = _reverse_rows(rbm, v, n_chains, betas, base_vis_bias, _draws(seed), max_rows, _REVERSE_GAUSSIAN)
    return {"ll": ll, "ess": ess, "logw": logw}


@torch.no_grad()
def evaluate_gaussian_log_likelihood_sandwich(model, loader=None, max_batches: Optional[int] = None, **kwargs) -> Optional[dict]:
    """``evaluate_log_likelihood_sandwich`` for a ``GaussianRBM`` -- or the BOTTOM layer of an ``iDBN`` built with
    ``GAUSSIAN_VISIBLE``: the same keys, ``mean_ll_ais`` from ``gaussian_log_likelihood`` with the ``gauss_ais`` log Z and
    ``mean_ll_reverse`` from ``gaussian_reverse_ais_log_likelihood``, log-densities both; the same ``kwargs``.  One draw source
    carries the AIS run and then every batch; the host synchronises ONCE, after the last batch.  With a ``wandb_run`` on the model
    the scalars are logged as ``ll/gaussian_...``."""
    return _evaluate_sandwich("evaluate_gaussian_log_likelihood_sandwich", model, loader, max_batches, kwargs, _check_gaussian,
                              lambda eng, rbm, betas, M, rng, bA: eng.gauss_ais(rbm, rbm.logvar.data, betas, M, rng, base_vis_bias=bA),
                              _REVERSE_GAUSSIAN, "ll/gaussian_")


def _top_side(layers):
    """The reverse side of the top RBM of a Gaussian stack: the Gaussian one for a stack of one, else the Bernoulli one."""
    return _REVERSE_GAUSSIAN if len(layers) == 1 else _REVERSE_BERNOULLI


@torch.no_grad()
def gaussian_dbn_conservative_bound(model, v: torch.Tensor, n_samples: int = 8, n_chains: int = 16, n_betas: int = 1000, betas=None,
                                    base_vis_bias: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                                    max_rows: int = 4096) -> torch.Tensor:
    """``dbn_conservative_bound`` for a stack with a Gaussian bottom layer: the bottom bracket through ``gauss_bound_step`` in mode
    ``entropy``, the Bernoulli layers above through ``bound_step``, and in place of ``-F_top - log Z_top`` the Bernoulli reverse-AIS
    estimate at the sampled top-layer states (``base_vis_bias``: the TOP RBM's base-rate model).  Float64 ``[B]`` on the device, a
    log-density, no host sync.  A ``GaussianRBM`` alone is a stack of one: ``gaussian_reverse_ais_log_likelihood``."""
    layers = _gaussian_stack(model)
    betas = linear_betas(n_betas) if betas is None else betas
    return _conservative_values(layers, v, n_samples, n_chains, betas, base_vis_bias, _draws(seed), max_rows, None, _top_side(layers))[0].mean(1)


@torch.no_grad()
def evaluate_gaussian_dbn_bound_conservative(model, loader=None, n_samples: int = 8, n_chains: int = 16, max_batches: Optional[int] = None,
                                             n_betas: int = 1000, betas=None, base_vis_bias: Optional[torch.Tensor] = None,
                                             seed: Optional[int] = None, max_rows: int = 4096) -> Optional[dict]:
    """Mean held-out ``gaussian_dbn_conservative_bound`` over ``loader`` (default ``model.val_loader``; None without one): the keys of
    ``evaluate_dbn_bound_conservative``.  One draw source carries every batch, sums on the device, one host sync after the last
    batch.  With a ``wandb_run`` on the model the scalars are logged as ``ll/gdbn_conservative_...``."""
    layers = _gaussian_stack(model)
    return _evaluate_conservative(model, layers, _top_side(layers), "ll/gdbn_conservative_", None, loader, n_samples, n_chains, max_batches,
                                  n_betas, betas, base_vis_bias, seed, max_rows)


# ---- the ground truth: exact log Z and marginals by on-device enumeration ----------------------------------------
def _exact(rbm, logvar, side, max_bits, marginals) -> dict:
    return _E.get_engine(rbm.W.data).exact_log_z(rbm, logvar=logvar, side=side, marginals=bool(marginals), max_bits=int(max_bits))


@torch.no_grad()
def exact_log_partition(rbm, side: str = "auto", max_bits: int = 24, marginals: bool = False) -> dict:
    """Exact log Z of a Bernoulli RBM, softmax groups accepted, by enumerating one side on the device (ONE ``HipEngine.exact_log_z``
    call): ``{"log_z": 0-d float64 device tensor, "log_w_max", "side": "hidden" | "visible", "bits": n, "vis_mean", "hid_mean"}``.
    ``side="auto"``: the smaller side, the hidden one when the visible layer has softmax groups (a one-hot group cannot be
    enumerated bit by bit).  The enumerated side may hold ``max_bits`` units at most (the library stops at 30).  ``marginals``: also
    the exact p(v_i = 1) (the category probabilities inside a group) and p(h_j = 1), fp32 ``[V]`` / ``[H]``.  No draws, no host sync."""
    _check_binary(rbm, groups_ok=True)
    return _exact(rbm, None, side, max_bits, marginals)


@torch.no_grad()
def exact_gaussian_log_partition(rbm, max_bits: int = 24, marginals: bool = False) -> dict:
    """Exact log Z of a ``GaussianRBM`` by enumerating its hidden side: the keys of ``exact_log_partition``; ``vis_mean`` is E[v_i]."""
    _check_gaussian(rbm)
    return _exact(rbm, rbm.logvar.data, "hidden", max_bits, marginals)


def _exact_estimate(exact):
    """``exact`` in the shape ``_known_or_estimated`` asks of an estimator: log Z on the host, no standard error, no sample size."""
    def estimate(rbm, max_bits=24):
        return {"log_z": float(exact(rbm, max_bits=max_bits)["log_z"]), "se": None, "ess": None}
    return estimate


@torch.no_grad()
def evaluate_log_likelihood_exact(model, loader=None, max_batches: Optional[int] = None, max_bits: int = 24) -> Optional[dict]:
    """``evaluate_log_likelihood`` with the exact log Z of ``exact_log_partition`` in place of an AIS estimate (``se`` and ``ess``
    None): the mean held-out log-likelihood of an ``RBM`` -- or of the BOTTOM layer of an ``iDBN`` -- itself, not an estimate of it.
    Softmax groups are accepted.  With a ``wandb_run`` on the model the scalars are logged as ``ll/...``."""
    return _evaluate_ll(model, loader, None, max_batches, {"max_bits": max_bits}, lambda r: _check_binary(r, groups_ok=True),
                        _exact_estimate(exact_log_partition))


@torch.no_grad()
def evaluate_gaussian_log_likelihood_exact(model, loader=None, max_batches: Optional[int] = None, max_bits: int = 24) -> Optional[dict]:
    """``evaluate_gaussian_log_likelihood`` with the exact log Z of ``exact_gaussian_log_partition``: the mean held-out log-density."""
    return _evaluate_ll(model, loader, None, max_batches, {"max_bits": max_bits}, _check_gaussian, _exact_estimate(exact_gaussian_log_partition))


def _calibration(rbm, weights, exact, max_bits, ais_kwargs) -> dict:
    """The AIS run of ``weights`` (what its ``estimate_*`` runs), then the exact call; every figure in ONE device-to-host copy."""
    logw, lzb = weights(rbm, **ais_kwargs)
    lz = exact(rbm, max_bits=max_bits)["log_z"]
    host = torch.cat([_weight_stats_device(logw, lzb), lz.reshape(1).to(logw.device)]).cpu().tolist()
    return {"log_z": host[0], "log_z_base": host[1], "logw": logw, "ess": host[2], "se": host[3], "log_z_exact": host[4],
            "log_z_gap": host[0] - host[4]}


@torch.no_grad()
def ais_calibration(rbm, max_bits: int = 24, **ais_kwargs) -> dict:
    """How far AIS is from the truth on ``rbm``'s own parameters: the dict of ``estimate_log_partition(rbm, **ais_kwargs)`` -- of
    ``estimate_joint_log_partition`` for an RBM with softmax groups -- plus ``log_z_exact`` and ``log_z_gap`` = AIS minus exact."""
    _check_binary(rbm, groups_ok=True)
    weights = _joint_ais_weights if getattr(rbm, "softmax_groups", None) else _ais_weights
    return _calibration(rbm, weights, exact_log_partition, max_bits, ais_kwargs)


@torch.no_grad()
def gaussian_ais_calibration(rbm, max_bits: int = 24, **ais_kwargs) -> dict:
    """``ais_calibration`` for a ``GaussianRBM``: ``estimate_gaussian_log_partition`` against ``exact_gaussian_log_partition``."""
    _check_gaussian(rbm)
    return _calibration(rbm, _gaussian_ais_weights, exact_gaussian_log_partition, max_bits, ais_kwargs)


@torch.no_grad()
def chain_marginal_gap(rbm, particles: torch.Tensor, max_bits: int = 24) -> dict:
    """The distance between a particle cloud and the model it should sample: ``{"max_gap", "rms_gap"}``, the largest and the
    root-mean-square difference between the column means of ``particles`` ``[M, V]`` (the chains of ``train_epoch_persistent``; of a
    tempering state ``[R M, V]`` pass the last replica's rows, ``state[-M:]``, the ones at beta = 1) and the exact ``vis_mean`` of
    ``exact_log_partition``; 0-d float64 device tensors, no host sync."""
    _check_binary(rbm, groups_ok=True)
    if particles.dim() != 2 or particles.size(1) != rbm.W.shape[0] or particles.size(0) < 1:
        raise ValueError(f"chain_marginal_gap: particles must be [M, {rbm.W.shape[0]}], got {tuple(particles.shape)}")
    want = exact_log_partition(rbm, max_bits=max_bits, marginals=True)["vis_mean"].double()
    gap = rows_on_device(particles, want.device).double().mean(0) - want
    return {"max_gap": gap.abs().max(), "rms_gap": gap.pow(2).mean().sqrt()}


# ---- the deep Boltzmann machine (imdbn.models.DBM) -----------------------------------------------------------------
def _check_dbm(who: str, dbm):
    """The refusals of ``DBM.from_idbn``, for a model that was changed after its conversion; no data-parallel split."""
    from imdbn.models.grbm import GaussianRBM
    for l, r in enumerate(dbm.layers):
        if isinstance(r, GaussianRBM):
            raise ValueError(f"{who}: layer {l} is a GaussianRBM; a DBM has Bernoulli units only (DESIGN section 40)")
        if getattr(r, "softmax_groups", None):
            raise ValueError(f"{who}: layer {l} has softmax groups; a DBM has Bernoulli units only (DESIGN section 40)")
    if _E.dp.active():
        raise NotImplementedError(f"{who} has no data-parallel split")


def _dbm_log_z_base(dbm, base_bias, dev) -> torch.Tensor:
    """log Z_A of the DBM's base model (float64 scalar on ``dev``): sum_{l >= 1} N_l log 2 + sum_i softplus(a_i)."""
    sizes = dbm.sizes
    a = torch.zeros(sizes[0], dtype=torch.float64, device=dev) if base_bias is None else base_bias.to(dev).double().reshape(-1)
    if a.numel() != sizes[0]:
        raise ValueError(f"base_bias must have {sizes[0]} elements")
    return torch.nn.functional.softplus(a).sum() + sum(sizes[1:]) * math.log(2.0)


@torch.no_grad()
def estimate_dbm_log_partition(dbm, n_chains: int = 256, n_betas: int = 1000, betas=None, base_bias: Optional[torch.Tensor] = None,
                               seed: Optional[int] = None) -> dict:
    """AIS estimate of log Z of a ``DBM`` (Salakhutdinov & Hinton 2009, section 4.1): the chains live on the odd layers, the even
    layers -- layer 0 included -- are summed out analytically, and the base model A has no weights, zero biases above layer 0 and
    ``base_bias`` on layer 0 (None = zeros; ``base_rate_bias`` of the data is the usual choice).  The whole run is ONE
    ``HipEngine.dbm_ais`` call (imdbn_dbm_ais).  The dict is ``estimate_log_partition``'s; one device-to-host
    copy; ``seed`` as in the module docstring."""
    _check_dbm("estimate_dbm_log_partition", dbm)
    betas = linear_betas(n_betas) if betas is None else betas
    lzb = _dbm_log_z_base(dbm, base_bias, dbm.layers[0].W.device)      # (first: it refuses a base_bias of the wrong length)
    logw = dbm._eng().dbm_ais(dbm.layers, dbm.biases(), betas, int(n_chains), _draws(seed), base_bias=base_bias)
    return _weight_stats(logw, lzb)


@torch.no_grad()
def dbm_variational_bound(dbm, v: torch.Tensor, log_z, n_mf: int = 10, damp: float = 0.0) -> torch.Tensor:
    """The mean-field lower bound on log p(v) of a ``DBM`` per row, a float64 device tensor ``[B]``: with ``mu`` the posterior of
    ``dbm.infer(v, n_mf, damp)`` and ``mu_0 = v``, ``b_0 v + sum_{l >= 1} sum_n mu_{l,n} (mu_{l-1} W_{l-1} + b_l)_n + h(mu_{l,n})
    - log Z`` (``HipEngine.dbm_bound``).  It holds for ANY ``mu``, so more sweeps only tighten it; with an AIS ``log_z`` the figure
    is as optimistic as that estimate.  No host sync."""
    _check_dbm("dbm_variational_bound", dbm)
    x = rows_on_device(v, dbm.device)
    eng = dbm._eng()
    mu, _ = eng.dbm_infer(dbm.layers, dbm.biases(), x, int(n_mf), damp=float(damp), want_res=False)
    return eng.dbm_bound(dbm.layers, dbm.biases(), x, mu) - log_z


@torch.no_grad()
def evaluate_dbm_log_likelihood(dbm, loader=None, log_z: Optional[float] = None, max_batches: Optional[int] = None, n_mf: int = 10,
                                damp: float = 0.0, **ais_kwargs) -> Optional[dict]:
    """Mean held-out variational bound of a ``DBM`` over ``loader`` (default ``dbm.val_loader``, then ``dbm.dataloader``; None
    without one): ``mean_bound``, ``sum_bound``, ``n``, ``log_z``, ``se``, ``ess`` (the last two None when ``log_z`` was passed in
    instead of estimated with ``estimate_dbm_log_partition(**ais_kwargs)``).  Summed on the device, ONE host sync after the last
    batch; with a ``wandb_run`` on the model the scalars are logged as ``ll/dbm_...``."""
    _check_dbm("evaluate_dbm_log_likelihood", dbm)
    loader = loader if loader is not None else (getattr(dbm, "val_loader", None) or getattr(dbm, "dataloader", None))
    if loader is None:
        return None
    log_z, se, ess = _known_or_estimated(log_z, estimate_dbm_log_partition, dbm, ais_kwargs)
    (s,), n = _sum_batches(loader, max_batches, lambda batch: dbm_variational_bound(dbm, _first(batch), log_z, n_mf, damp).sum().reshape(1), 1)
    res = {"mean_bound": s / max(1, n), "sum_bound": s, "n": n, "log_z": float(log_z), "se": se, "ess": ess}
    _log_scalars(dbm, "ll/dbm_", res, ("mean_bound", "log_z", "se", "ess"))
    return res
