"""Time the categorical DBM layer and the multimodal DBM update at the paper's shapes: image stack 10000 - 1500 - 500, joint
hidden layer 256, 32 labels, batch 64.

  group_layer_mf / group_layer_sample   HipEngine.dbm_group_layer at the label layer's own shape (K_hi = J, N = K): one mean-field
                                        half-step with its residual / one sampling half-step (Philox), through a row block of the joint W;
  composed                              what the call fuses, composed from what the engine offered before, on the same joint RBM:
                                        prop_down(logits_only=True) over the WHOLE visible side (it has no row-block form), an ATen
                                        softmax of the label columns and the engine's categorical draw (sample_visible);
  mdbm_step / dbm_step                  HipEngine.mdbm_step on the whole model against HipEngine.dbm_step on the image stack alone, both
                                        with n_mf = 10, gibbs_k = 5 and their monitor.

Every measurement runs in a child process of its own under a time limit (--limit seconds); the first one that fails or runs out of
time ends the tool, nothing more is started.  HIP events around `reps` calls after a warm-up, microseconds per call, `runs` runs.
Not a test, no threshold."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("group_layer_mf", "group_layer_sample", "composed", "mdbm_step", "dbm_step")


def measure(a):
    import __graft_entry__ as ge
    ge.build(compile_ok=False)
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM

    dev = "cuda:0"
    sizes, J, K, B = tuple(a.sizes), a.J, a.K, a.rows
    Dz = sizes[-1]
    g = np.random.Generator(np.random.PCG64(1))
    torch.manual_seed(1)
    layers = [RBM(sizes[l], sizes[l + 1], 0.1, 1e-4, 0.5).to(dev) for l in range(len(sizes) - 1)]
    joint = RBM(Dz + K, J, 0.1, 1e-4, 0.5, softmax_groups=[(Dz, Dz + K)]).to(dev)
    eng = E.get_hip_engine()
    rng = E.PhiloxRng(3)
    bits = lambda n, p: torch.from_numpy((g.random((B, n)) < p).astype(np.float32)).to(dev)
    onehot = lambda: torch.from_numpy(np.eye(K, dtype=np.float32)[g.integers(0, K, B)]).to(dev)
    h = bits(J, 0.5)
    zy = torch.cat([bits(Dz, 0.5), onehot()], 1)
    Wy, b_y = joint.W.data[Dz:], joint.vis_bias.data[Dz:]
    data, y = bits(sizes[0], 0.2), onehot()
    particles = [bits(n, 0.5) for n in sizes[:-1]] + [zy.clone(), bits(J, 0.5)]
    img_particles = [bits(n, 0.5) for n in sizes]
    scalars = [(0.001, 0.5)] * (len(layers) + 1)

    def composed():
        logits = eng.prop_down(joint, h, logits_only=True)
        p = torch.zeros_like(logits)
        p[:, Dz:] = torch.softmax(logits[:, Dz:], 1)
        eng.sample_visible(joint, p, rng)

    calls = {
        "group_layer_mf": lambda: eng.dbm_group_layer(None, Wy, None, h, b_y, [(0, K)], m=zy[:, Dz:], damp=0.5, want_res=True),
        "group_layer_sample": lambda: eng.dbm_group_layer(None, Wy, None, h, b_y, [(0, K)], sample=True, rng=rng, s_out=zy[:, Dz:]),
        "composed": composed,
        "mdbm_step": lambda: eng.mdbm_step(layers, joint, data, y, particles, scalars, 10, 0.0, 5, rng),
        "dbm_step": lambda: eng.dbm_step(layers, data, img_particles, scalars[:-1], 10, 0.0, 5, rng),
    }
    fn = calls[a.only]

    def timed():
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

    us = [timed() for _ in range(a.runs)]
    finite = bool(all(torch.isfinite(r.W.data).all() for r in layers + [joint]) and torch.isfinite(zy).all())
    print(json.dumps({a.only + "_us": us, "finite": finite, "cus": eng.device_info()[0]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 1500, 500], help="the image stack, bottom first")
    ap.add_argument("--J", type=int, default=256)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds every measurement may take")
    ap.add_argument("--only", default=None, choices=NAMES, help="run this measurement in this process")
    a = ap.parse_args()
    if a.only:
        return measure(a)
    import __graft_entry__ as ge
    ge.build()                               # in this process, which never touches the GPU
    out = {"sizes": a.sizes, "J": a.J, "K": a.K, "rows": a.rows}
    for name in NAMES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--only", name, "--sizes", *map(str, a.sizes)]
        for k in ("J", "K", "rows", "reps", "warmup", "runs"):
            cmd += [f"--{k}", str(getattr(a, k))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            out["failed"] = {"name": name, "status": p.returncode}
            print(json.dumps(out))
            sys.exit(1)                      # nothing more is started on the GPU
        out.update(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
