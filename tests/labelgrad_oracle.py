"""Float64 numpy twin of imdbn_rbm_label_step (include/imdbn_engine.h) and the engine's test double for it.

TEST INFRASTRUCTURE ONLY.  Joint RBM over [z (Dz) | y (K)], U = W[Dz:], base = c + z W[:Dz], o_kj = base_j + U_kj:
  a_k = z . b_z + b_y,k + sum_j softplus(o_kj)        logp = a_t - logsumexp_k a_k        p_k = exp(a_k - logsumexp a)
  r_k = 1[k = t] - p_k        s = sigmoid(o)        hpos_j = s_tj        hneg_j = sum_k p_k s_kj
  G_W[:Dz] = z^T (hpos - hneg)    G_W[Dz + k][j] = sum_n r_nk s_nkj    G_c = sum_n (hpos - hneg)    G_b[Dz + k] = sum_n r_nk    G_b[:Dz] = 0
and the update  m = mom m + lr (G / N - wd W [weights only]);  parameter += m  on all six tensors.  A row whose label is outside
[0, K) has logp = NaN and enters no sum; the divisor stays N.  A state is a dict W [V, H], b [V], c [H], Wm, bm, cm."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from bound_oracle import LikelihoodOracleEngine
from oracle_engine import _np

F64 = np.float64


def rows(W, b, c, z, K, gt):
    """Everything per row, in float64: dict(logp [N], p [N, K], r [N, K], s [N, K, H], hpos [N, H], hneg [N, H], ok [N])."""
    W, b, c, z = (np.asarray(x, F64) for x in (W, b, c, z))
    N, Dz = z.shape
    assert Dz + K == W.shape[0]
    o = (z @ W[:Dz] + c)[:, None, :] + W[Dz:][None, :, :]
    a = (z @ b[:Dz])[:, None] + b[Dz:][None, :] + np.logaddexp(0.0, o).sum(2)
    mx = a.max(1)
    marg = mx + np.log(np.exp(a - mx[:, None]).sum(1))
    gt = np.asarray(gt).astype(np.int64)
    ok = (gt >= 0) & (gt < K)
    t = np.where(ok, gt, 0)
    n = np.arange(N)
    p = np.exp(a - marg[:, None])
    r = -p
    r[n, t] += 1.0
    s = 1.0 / (1.0 + np.exp(-o))
    hpos, hneg = s[n, t], np.einsum("nk,nkj->nj", p, s)
    r[~ok], hpos[~ok], hneg[~ok] = 0.0, 0.0, 0.0
    return dict(logp=np.where(ok, a[n, t] - marg, np.nan), p=p, r=r, s=s, hpos=hpos, hneg=hneg, ok=ok)


def gradients(W, b, c, z, K, gt):
    """-> (logp [N], G_W [V, H], G_b [V], G_c [H]): the gradient SUMS over the valid rows."""
    q = rows(W, b, c, z, K, gt)
    z = np.asarray(z, F64)
    delta = q["hpos"] - q["hneg"]
    G_W = np.concatenate([z.T @ delta, np.einsum("nk,nkj->kj", q["r"], q["s"])], 0)
    G_b = np.concatenate([np.zeros(z.shape[1]), q["r"].sum(0)])
    return q["logp"], G_W, G_b, delta.sum(0)


def step(st, z, K, gt, lr, mom, wd):
    """-> (logp [N], the state after one step); float64 throughout, the input state is left unchanged."""
    st = {k: np.asarray(v, F64) for k, v in st.items()}
    n = float(np.asarray(z).shape[0])
    logp, G_W, G_b, G_c = gradients(st["W"], st["b"], st["c"], z, K, gt)
    Wm = mom * st["Wm"] + lr * (G_W / n - wd * st["W"])
    cm = mom * st["cm"] + lr * G_c / n
    bm = mom * st["bm"] + lr * G_b / n
    return logp, dict(W=st["W"] + Wm, b=st["b"] + bm, c=st["c"] + cm, Wm=Wm, bm=bm, cm=cm)


class LabelGradOracleEngine(LikelihoodOracleEngine):
    """The likelihood test double plus ``label_step`` from the twin (the RBM's fp32 tensors updated in place).  ``calls`` records
    ("label_step", rows, lr, mom) and ("clamped_step",) next to the base double's ("cd_step", ...), in call order."""

    def label_step(self, rbm, z, K, gt, lr, mom):
        self.calls.append(("label_step", int(z.shape[0]), float(lr), float(mom)))
        x = self._state(rbm, True)
        st = dict(W=x.W, b=x.vis_bias, c=x.hid_bias, Wm=x.W_m, bm=x.vb_m, cm=x.hb_m)
        logp, new = step(st, _np(z), int(K), gt.cpu().numpy(), lr, mom, float(rbm.weight_decay))
        for k, arr in st.items():
            arr[...] = new[k].astype(np.float32)
        return torch.from_numpy(logp)

    def clamped_step(self, *a, **k):
        self.calls.append(("clamped_step",))
        return super().clamped_step(*a, **k)


@pytest.fixture()
def labelgrad_double():
    """The test double installed as the engine for one test (a test module imports the fixture by name)."""
    from imdbn import engine as E
    eng = LabelGradOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)
