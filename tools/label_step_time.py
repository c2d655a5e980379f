"""Time the supervised label step of the joint RBM at the joint RBM of BASELINE's train_joint configuration:
532 <-> 256 (Dz = 500, K = 32 labels as one softmax group), batch 64.

  label_step   HipEngine.label_step: the up propagation, the two kernels of kernels_labelgrad.hpp and the update path;
  clamped      one label-clamped RBM.train_epoch_clamped call on the same model as train_joint's main phase issues it
               (CD-1, 30 noisy mean-field steps, reclamp_negative=False), for scale: the generative update the step rides behind;
  autograd     the same step restated in torch on the same GPU: fp32 log_softmax of the K free energies, backward, the momentum
               update of all three parameters.

HIP events around `reps` calls after a warm-up, microseconds per call.  Not a test, no threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Dz", type=int, default=500)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM

    dev = "cuda:0"
    Dz, K, H, B = a.Dz, a.K, a.H, a.rows
    V = Dz + K
    g = np.random.Generator(np.random.PCG64(1))
    r = RBM(V, H, 0.04, 1e-4, 0.5, dynamic_lr=True, final_momentum=0.95, softmax_groups=[(Dz, V)]).to(dev)
    r.vis_bias.data.copy_(torch.from_numpy((0.3 * g.standard_normal(V)).astype(np.float32)))
    z = torch.from_numpy(g.random((B, Dz)).astype(np.float32)).to(dev)
    gt = torch.from_numpy(g.integers(0, K, B)).to(dev)
    y = torch.eye(K, device=dev)[gt]
    eng = E.get_hip_engine()
    lr, mom = 0.5 * 0.04, 0.5

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            out = fn()
        t1.record()
        torch.cuda.synchronize()
        return 1000.0 * t0.elapsed_time(t1) / a.reps, out

    step_us, logp = timed(lambda: eng.label_step(r, z, K, gt, lr, mom))

    vk = torch.zeros(B, V, device=dev); km = torch.zeros_like(vk)
    vk[:, Dz:] = y; km[:, Dz:] = 1.0
    E.manual_seed(3)
    clamped_us, _ = timed(lambda: r.train_epoch_clamped(vk, km, 8, 20, CD=1, cond_init_steps=30, sample_h=False, sample_v=False,
                                                        reclamp_negative=False, aux_lr_mult=0.3, use_noisy_init=True))

    W = r.W.data.clone().contiguous().requires_grad_(True)
    b = r.vis_bias.data.clone().requires_grad_(True)
    c = r.hid_bias.data.clone().requires_grad_(True)
    moms = [torch.zeros_like(t) for t in (W, b, c)]
    wd = 1e-4

    def autograd_step():
        base = z @ W[:Dz] + c
        a_k = (z @ b[:Dz])[:, None] + b[Dz:][None, :] + torch.nn.functional.softplus(base[:, None, :] + W[Dz:][None]).sum(2)
        lp = torch.log_softmax(a_k, 1)[torch.arange(B, device=dev), gt]
        gW, gb, gc = torch.autograd.grad(lp.sum(), (W, b, c))
        with torch.no_grad():
            for p, m, gr, decay in ((W, moms[0], gW, wd), (b, moms[1], gb, 0.0), (c, moms[2], gc, 0.0)):
                m.mul_(mom).add_(lr * (gr / B - decay * p))
                p.add_(m)
        return lp

    auto_us, _ = timed(autograd_step)
    print(json.dumps({"Dz": Dz, "K": K, "H": H, "rows": B, "label_step_us": round(step_us, 1), "clamped_update_us": round(clamped_us, 1),
                      "torch_autograd_us": round(auto_us, 1), "mean_logp_last": float(torch.nanmean(logp))}))


if __name__ == "__main__":
    main()
