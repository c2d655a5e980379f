"""Time one backprop step of an unrolled stack with a Gaussian bottom layer: [10000, 1500, 500], batch 64, standardised
real data.

  gaussian_autoencoder_step   HipEngine.gauss_autoencoder_step, monitors off;
  composed                    the same step with the two Gaussian calls hand-composed from calls that were there before
                              imdbn_rbm_gauss_backprop_step: gauss_backward for the mean, torch arithmetic for e_0 = (v - m) e^{-z},
                              u = v e^{-z} and the two logvar gradients, backprop_step with apply on the Gaussian layer's W (its
                              update is the same formula on (x_h, e_0) and (u, e_h)), and an explicit logits-only prop_down on a
                              zero-bias clone for e_h W^T in gz; logvar and its momentum move in torch.

HIP events around `reps` steps after a warm-up, microseconds per step, `runs` times each in one process.  Not a test, no threshold."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 1500, 500])
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import iDBN

    dev = "cuda:0"
    B = a.rows
    g = np.random.Generator(np.random.PCG64(1))
    net = iDBN(list(a.sizes), {"LEARNING_RATE": 0.01, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95,
                               "LEARNING_RATE_DYNAMIC": False, "CD": 1, "GAUSSIAN_VISIBLE": True, "GAUSSIAN_LR_SIGMA_MULT": 0.5,
                               "GAUSSIAN_LOGVAR_MIN": -4.0, "GAUSSIAN_LOGVAR_MAX": 4.0}, [], [], torch.device(dev))
    gen = net.gaussian_untie()
    rec = net.layers
    L = len(rec)
    X = g.standard_normal((B, a.sizes[0])) * (0.5 + g.random(a.sizes[0])) + g.standard_normal(a.sizes[0])
    data = torch.from_numpy(((X - X.mean(0)) / X.std(0)).astype(np.float32)).to(dev)
    eng = E.get_hip_engine()
    scalars = [(0.0005, 0.5)] * L

    def zero_bias(r):
        z = copy.copy(r)
        z._parameters = dict(r._parameters)
        z.__dict__.pop("_imdbn_desc", None)
        z.hid_bias = torch.nn.Parameter(torch.zeros_like(r.hid_bias.data), requires_grad=False)
        z.vis_bias = torch.nn.Parameter(torch.zeros_like(r.vis_bias.data), requires_grad=False)
        return z
    zeros = {id(r): zero_bias(r) for r in (rec[0], gen[0] if L > 1 else rec[0])}

    def composed_gauss(rbm, logvar, logvar_m, v, up=None, down=None, lr=0.0, mom=0.0, lr_z=0.0, z_lo=float("-inf"), z_hi=float("inf"),
                       apply=True, want_h=False, monitor=False):
        iv = torch.exp(-logvar)
        n = v.size(0)
        gz = torch.zeros_like(logvar)
        pairs = {}
        if down is not None:
            d = v - eng.gauss_backward(rbm, logvar, down)
            e0 = d * iv
            gz += iv * (d * d).sum(0) / (2 * n) - 0.5
            pairs["down"] = (down, e0)
        if up is not None:
            u = v * iv
            gz -= (u * eng.prop_down(zeros[id(rbm)], up, logits_only=True)).sum(0) / n
            pairs["up"] = (u, up)
        err_h = eng.backprop_step(rbm, lr=lr, mom=mom, apply=apply, want_h=want_h, **pairs)[1]
        if apply and lr_z != 0:
            logvar_m.mul_(mom).add_(gz, alpha=lr_z)
            logvar.add_(logvar_m).clamp_(z_lo, z_hi)
        return err_h, None, None

    class Composed:
        """The engine with gauss_backprop_step replaced: gauss_autoencoder_step is host logic over the engine's calls."""
        def __getattr__(self, k):
            return getattr(eng, k)
    comp = Composed()
    comp.gauss_backprop_step = composed_gauss
    step = type(eng).gauss_autoencoder_step

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return round(1000.0 * t0.elapsed_time(t1) / a.reps, 1)

    out = {"sizes": list(a.sizes), "rows": B}
    out["gaussian_autoencoder_step_us"] = [timed(lambda: eng.gauss_autoencoder_step(rec, gen, data, scalars, monitor=False)) for _ in range(a.runs)]
    out["composed_us"] = [timed(lambda: step(comp, rec, gen, data, scalars, monitor=False)) for _ in range(a.runs)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
