"""Float64 numpy twin of imdbn_rbm_pseudo_loglik (include/imdbn_engine.h) and the engine's test double for it.

TEST INFRASTRUCTURE ONLY.  ``sites`` states the pseudo-log-likelihood by its DEFINITION: every conditional comes from free energies of
whole visible states, F(v) = -v.b - sum_j softplus(c_j + (v W)_j) in float64 on the explicitly changed row -- never from the
log1p(sigma expm1(.)) form the kernel uses, so the two are independent statements.
  Bernoulli column i:  log p(v_i | v_rest) = -log(1 + exp(F(v) - F(v with bit i flipped)))
  softmax group g:     log p(v_g | v_rest) = log-softmax over the group's categories k of -F(v with the group set to e_k), at the observed one
A row holding an element that is not exactly 0 or 1, or a group without exactly one 1, is NaN throughout."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from bound_oracle import LikelihoodOracleEngine
from oracle_engine import _np

F64 = np.float64


def free_energy(W, b, c, v):
    """F(v) per row in float64."""
    W, b, c, v = (np.asarray(a, F64) for a in (W, b, c, v))
    return -(v @ b) - np.logaddexp(0.0, v @ W + c).sum(1)


def valid_rows(v, groups):
    v = np.asarray(v, F64)
    ok = ((v == 0.0) | (v == 1.0)).all(1)
    for s, e in groups:
        ok &= (v[:, s:e] == 1.0).sum(1) == 1
    return ok


def sites(W, b, c, v, groups=()):
    """-> (site [N, V] float64, total [N] float64): the term of every column (a group's at its observed column, 0 in the group's
    other columns) and their sum per row."""
    v = np.asarray(v, F64)
    N, V = v.shape
    ok = valid_rows(v, groups)
    vc = np.where(ok[:, None], v, 0.0)                          # invalid rows: computed on zeros, overwritten below
    in_group = np.zeros(V, bool)
    for s, e in groups:
        in_group[s:e] = True
    out = np.zeros((N, V), F64)
    F0 = free_energy(W, b, c, vc)
    for i in np.nonzero(~in_group)[0]:
        vf = vc.copy()
        vf[:, i] = 1.0 - vf[:, i]
        out[:, i] = -np.logaddexp(0.0, F0 - free_energy(W, b, c, vf))
    for s, e in groups:
        a = np.empty((N, e - s), F64)
        for k in range(e - s):
            vk = vc.copy()
            vk[:, s:e] = 0.0
            vk[:, s + k] = 1.0
            a[:, k] = -free_energy(W, b, c, vk)
        mx = a.max(1)
        lse = mx + np.log(np.exp(a - mx[:, None]).sum(1))
        t = vc[:, s:e].argmax(1)
        out[np.arange(N), s + t] = a[np.arange(N), t] - lse
    out[~ok] = np.nan
    return out, out.sum(1)


class PllOracleEngine(LikelihoodOracleEngine):
    """The likelihood test double plus ``pseudo_loglik`` from the twin; ``calls`` records ("pseudo_loglik", rows)."""

    def pseudo_loglik(self, rbm, v, return_sites=False):
        self.calls.append(("pseudo_loglik", int(v.shape[0])))
        site, tot = sites(_np(rbm.W.data), _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), _np(v), self._groups(rbm))
        pll = torch.from_numpy(tot)
        return (pll, torch.from_numpy(site.astype(np.float32))) if return_sites else pll


@pytest.fixture()
def pll_double():
    """The test double installed as the engine for one test (a test module imports the fixture by name)."""
    from imdbn import engine as E
    eng = PllOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)
