#!/usr/bin/env python3
"""Time of the IMG->TXT energy trace (HipEngine.energy_trace, csrc/kernels_energy.hpp) at the joint size: Dz = 500, K = 32, H = 256,
30 steps, N in {1, 128, 4096} clamped codes.

(a) ``entry``: one imdbn_energy_trace call (one K1 propagation + the label kernel), HIP events around it.
(b) ``composed``: the same numbers from the engine calls that existed before the entry: per step ``prop_up`` + ``prop_down``
    logits on a group-free descriptor + a torch sigmoid / softmax / top-2 / L1 tail on the label slice, then
    ``class_free_energies`` (the stacked free-energy call) with its min / top-2 / softmax tail.  No host sync inside either.

Each figure is the median of ``--reps`` timed runs after warm-up, with the min and max next to it (the spread).  Prints one JSON
line; ``--out FILE`` also writes it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multimodal-idbn_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    from imdbn.models import RBM
    from imdbn.utils import energy_utils as EU
    dev = torch.device("cuda")
    Dz, K, H, T = 500, 32, 256, 30
    g = np.random.Generator(np.random.PCG64(1))

    def rbm(groups):
        r = RBM(Dz + K, H, 0.1, 1e-4, 0.5, softmax_groups=groups).to(dev)
        return r

    joint = rbm([(Dz, Dz + K)])
    joint.W.data.copy_(torch.from_numpy((g.standard_normal((Dz + K, H)) * 0.15).astype(np.float32)))
    joint.hid_bias.data.copy_(torch.from_numpy((g.standard_normal(H) * 0.2).astype(np.float32)))
    joint.vis_bias.data.copy_(torch.from_numpy(np.concatenate([g.standard_normal(Dz) * 0.2, g.standard_normal(K) * 1.5]).astype(np.float32)))
    plain = rbm(None)                                        # the same parameters without the label softmax group
    plain.W.data, plain.hid_bias.data, plain.vis_bias.data = joint.W.data, joint.hid_bias.data, joint.vis_bias.data
    eng = E.get_hip_engine()

    def entry(z, gt):
        return eng.energy_trace(joint, z, K, T, gt=gt)

    def composed(z, gt):
        n = z.size(0)
        v = torch.cat([z, torch.full((n, K), 1.0 / K, device=dev)], 1)
        y_prev = v[:, Dz:].clone()
        rows = torch.arange(n, device=dev)
        curves = []
        for _ in range(T):
            h = eng.prop_up(plain, v)
            y = torch.softmax(torch.sigmoid(eng.prop_down(plain, h, logits_only=True)[:, Dz:]), dim=1)
            top = y.topk(2, dim=1)
            curves.append((top.values, top.indices[:, 0], y[rows, gt], (y - y_prev).abs().sum(1)))
            y_prev = y
            v[:, Dz:] = y
        F = EU.class_free_energies(joint, z, K, Dz)
        f2 = torch.topk(F, 2, dim=1, largest=False)
        fe = torch.softmax(-F, dim=1).topk(2, dim=1).values
        return curves, F, f2.values[:, 1] - f2.values[:, 0], fe[:, 0] - fe[:, 1]

    def gpu_ms(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return {"median_ms": round(float(np.median(out)), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4)}

    rows = []
    for n in (1, 128, 4096):
        z = torch.from_numpy(g.random((n, Dz), dtype=np.float32) * 0.98 + 0.01).to(dev)
        gt = torch.arange(n, device=dev) % K
        a = entry(z, gt)
        c = composed(z, gt)
        torch.cuda.synchronize()
        # the two compute the same thing (fp32 summation order apart)
        err = float((a["p_top1"][:, -1] - c[0][-1][0][:, 0]).abs().max())
        rows.append({"N": n, "entry": gpu_ms(lambda: entry(z, gt), args.reps), "composed": gpu_ms(lambda: composed(z, gt), args.reps),
                     "max_abs_diff_p_top1_last_step": err})
        rows[-1]["speedup"] = round(rows[-1]["composed"]["median_ms"] / rows[-1]["entry"]["median_ms"], 1)
    res = {"what": "energy_trace_time", "Dz": Dz, "K": K, "H": H, "steps": T, "reps": args.reps, "rows": rows,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
