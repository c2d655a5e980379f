"""Shapes, models and tolerances of the discriminative fine-tuning tests, shared by tests/test_discrim_cpu.py and
tests/test_discrim_gpu.py.

The engine call runs on the cases of the label-gradient tests (labelgrad_cases.CASES at both weight scales: they cross the edges of the
row kernel, and their (Dz, H, N) send the propagation of e through W[:Dz] over the fused, the split-K and the V > 1024 routes); the
end-to-end runs use one small stack: image layers [100, 40, 20], a joint RBM with 16 hidden units over [20 | 4 labels], 3 batches of 8
rows of separable toy data."""
from types import SimpleNamespace

import numpy as np
import torch

from labelgrad_cases import CASES, LR, MOM, SCALES, WD, case, eps, state, tol_delta, tol_logp  # noqa: F401  (re-exported)

F32, F64 = np.float32, np.float64
ALL = [(n, s) for n in CASES for s in SCALES]
PRED_LEFT_OUT = 0.10                 # share of a case's rows the argmax test may leave out as too close to call
TOY = dict(sizes=[100, 40, 20], joint=16, K=4, B=8, NB=3)
PARAMS = {"LEARNING_RATE": 0.1, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95, "LEARNING_RATE_DYNAMIC": True,
          "CD": 1, "JOINT_LEARNING_RATE": 0.04, "JOINT_CD": 1, "JOINT_AUX_COND_STEPS": 10, "CROSS_GIBBS_STEPS": 5,
          "JOINT_METRICS_OVERLAP": False}


def tol_err_z(H, want):
    """Element by element, from a twin result ``want`` (discrim_oracle.head):
         0.25 tol_delta(H) sum_j |W_ij|  +  (H + 16) 2^-23 z (1 - z) sum_j |e_j| |W_ij|
    The first term: every entry of the device's e is within tol_delta(H) of the twin's (the label side's convention), it enters
    column i through |W_ij|, and z (1 - z) <= 1/4.  The second: the product bound of the backprop tests, a sum of H fp32 products.
    Both are derived, neither is measured."""
    return 0.25 * tol_delta(H) * want["wsum"][None, :] + (H + 16) * 2.0 ** -23 * want["mag"]


def pred_rows(H, want):
    """The rows whose argmax is decided: the float64 top-two gap above 2 eps(H), a class value being within eps(H) of float64."""
    return want["gap"] > 2 * eps(H)


def toy_data():
    """(X [24, 100] 0/1, labels [24]): four prototypes, 10 % of the pixels flipped -- separable."""
    g = np.random.Generator(np.random.PCG64(11))
    K, n = TOY["K"], TOY["B"] * TOY["NB"]
    yi = g.integers(0, K, n)
    proto = (g.random((K, 100)) > 0.7).astype(F32)
    X = np.abs(proto[yi] - (g.random((n, 100)) > 0.9).astype(F32)).astype(F32)
    return X, yi


def toy_model(device, seed=5):
    """The small iMDBN on ``device`` over toy_data(), its loaders unshuffled."""
    from torch.utils.data import DataLoader, TensorDataset
    from imdbn.models import iMDBN
    X, yi = toy_data()
    K = TOY["K"]
    dl = DataLoader(TensorDataset(torch.from_numpy(X).to(device), torch.from_numpy(np.eye(K, dtype=F32)[yi]).to(device)),
                    batch_size=TOY["B"], shuffle=False)
    torch.manual_seed(seed)
    return iMDBN(list(TOY["sizes"]), TOY["joint"], params=dict(PARAMS), dataloader=dl, val_loader=dl, device=torch.device(device), num_labels=K)


def small_stack(seed=31, sizes=(12, 7, 5), K=3, Hj=6, B=6):
    """A 2-layer stack and a joint RBM in float64 for the finite-difference checks: (layers [backprop_oracle states], joint
    [labelgrad_oracle state], data [B, sizes[0]] in [0, 1], labels [B])."""
    g = np.random.Generator(np.random.PCG64(seed))
    layers = []
    for V, H in zip(sizes[:-1], sizes[1:]):
        layers.append(SimpleNamespace(W=g.standard_normal((V, H)) * 0.4, hid_bias=g.standard_normal(H) * 0.3, vis_bias=g.standard_normal(V) * 0.3,
                                      W_m=np.zeros((V, H)), hb_m=np.zeros(H), vb_m=np.zeros(V), weight_decay=0.0))
    Vj = sizes[-1] + K
    joint = dict(W=g.standard_normal((Vj, Hj)) * 0.5, b=g.standard_normal(Vj) * 0.3, c=g.standard_normal(Hj) * 0.3,
                 Wm=np.zeros((Vj, Hj)), bm=np.zeros(Vj), cm=np.zeros(Hj))
    return layers, joint, g.random((B, sizes[0])), g.integers(0, K, B)


def layer_state(r):
    """A float64 backprop_oracle state of a torch RBM (copies)."""
    f = lambda t: t.detach().cpu().numpy().astype(F64)
    return SimpleNamespace(W=f(r.W.data), hid_bias=f(r.hid_bias.data), vis_bias=f(r.vis_bias.data), W_m=f(r.W_m), hb_m=f(r.hb_m), vb_m=f(r.vb_m),
                           weight_decay=float(r.weight_decay))


def joint_state(r):
    """A float64 labelgrad_oracle state of a torch RBM (copies)."""
    f = lambda t: t.detach().cpu().numpy().astype(F64)
    return dict(W=f(r.W.data), b=f(r.vis_bias.data), c=f(r.hid_bias.data), Wm=f(r.W_m), bm=f(r.vb_m), cm=f(r.hb_m))
