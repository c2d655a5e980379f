#!/usr/bin/env python3
"""Time of a MOD2->MOD1 trajectory panel of iMDBN_BiModal at the paper's sizes: joint 1000 <-> 1000 (Dz1 = Dz2 = 500), MOD1 stack
[10000, 1500, 500], N = 16 samples, 50 sampled steps after the mean-field step; the result is ``traj_h`` [51, 16, 1000] and ``traj_z1``.

(a) ``hidden_trace``: one ``chain_traced_vh`` call with the hidden window [0, H) and the visible window [0, Dz1).
(b) ``recompute``: what the engine could do for the same result before the hidden trace existed: ``chain_traced`` with a full-width
    visible trace, the (steps + 1) * N states that entered the steps reassembled from it (re-clamped), and one ``forward`` over them.
    Possible here only because visibles are mean-field and there is no noise: a sampled or noisy chain cannot be recomputed.

Each figure is the median of ``--reps`` timed runs (HIP events, no host sync inside) after warm-up, with min and max.  Prints one
JSON line; ``--out FILE`` also writes it."""
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
    dev = torch.device("cuda")
    Dz1, Dz2, H, N, T = 500, 500, 1000, 16, 50
    V = Dz1 + Dz2
    g = np.random.Generator(np.random.PCG64(1))
    joint = RBM(V, H, 0.1, 1e-4, 0.5).to(dev)
    joint.W.data.copy_(torch.from_numpy((g.standard_normal((V, H)) * 0.05).astype(np.float32)))
    joint.hid_bias.data.copy_(torch.from_numpy((g.standard_normal(H) * 0.2).astype(np.float32)))
    joint.vis_bias.data.copy_(torch.from_numpy((g.standard_normal(V) * 0.2).astype(np.float32)))
    sizes = [10000, 1500, 500]
    stack = []
    for i in range(2):
        r = RBM(sizes[i], sizes[i + 1], 0.1, 1e-4, 0.5).to(dev)
        r.W.data.copy_(torch.from_numpy((g.standard_normal((sizes[i], sizes[i + 1])) / np.sqrt(sizes[i + 1])).astype(np.float32)))
        stack.append(r)
    eng = E.get_hip_engine()
    vk = torch.zeros(N, V, device=dev)
    km = torch.zeros(N, V, device=dev)
    vk[:, Dz1:] = torch.from_numpy(g.random((N, Dz2), dtype=np.float32)).to(dev)
    km[:, Dz1:] = 1.0
    step = {"T": 1.0, "sigma": 0.0, "eta": 0.0, "sample_h": False, "vmode": 0, "clamp": True}
    steps = [step] + [dict(step, sample_h=True)] * T
    sel = np.unique(np.linspace(0, T, 8, dtype=int)).tolist()

    def frames(traj_z1):
        cur = traj_z1[sel].reshape(len(sel) * N, Dz1)
        for r in reversed(stack):
            cur = r.backward(cur)
        return cur

    def hidden_trace():
        spec = {"v_known": vk, "mask": km, "init_uniform": False, "steps": steps, "trace": (0, Dz1, False), "trace_h": (0, H)}
        ((_, tz, th),) = eng.chain_traced_vh(joint, spec, None, E.PhiloxRng(seed=5))
        return th, tz, frames(tz)

    def recompute():
        spec = {"v_known": vk, "mask": km, "init_uniform": False, "steps": steps, "trace": (0, V, False)}
        ((_, tv),) = eng.chain_traced(joint, spec, None, E.PhiloxRng(seed=5))
        states = torch.cat([vk.unsqueeze(0), tv[:-1] * (1 - km) + vk * km], 0)          # what entered step t
        th = eng.forward(joint, states.reshape((T + 1) * N, V)).view(T + 1, N, H)
        tz = tv[:, :, :Dz1]
        return th, tz, frames(tz)

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

    a, c = hidden_trace(), recompute()
    torch.cuda.synchronize()
    res = {"what": "bimodal_traj_time", "joint": [V, H], "mod1_stack": sizes, "N": N, "steps": T, "reps": args.reps,
           "hidden_trace": gpu_ms(hidden_trace, args.reps), "recompute": gpu_ms(recompute, args.reps),
           "max_abs_diff_traj_h": float((a[0] - c[0]).abs().max()), "max_abs_diff_traj_z1": float((a[1] - c[1]).abs().max()),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
