"""Time the DBM layer half-step and the DBM update at the paper stack's middle layer: 10000 - 1500 - 500, batch 64.

  dbm_layer_mf / dbm_layer_sample   HipEngine.dbm_layer at (K_lo 10000, N 1500, K_hi 500, B 64): one mean-field half-step with its
                                    residual / one sampling half-step (Philox);
  pair                              what the kernel fuses, composed from what the engine offered before, on the same two RBMs:
                                    prop_up of the lower RBM + prop_down(logits_only=True) of the upper one (the element-wise rest
                                    -- logit, add, sigmoid, damping -- is not even counted);
  dbm_step                          HipEngine.dbm_step on the three-layer stack with n_mf = 10, gibbs_k = 5, with its monitor.

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

NAMES = ("dbm_layer_mf", "dbm_layer_sample", "pair", "dbm_step")


def measure(a):
    import __graft_entry__ as ge
    ge.build(compile_ok=False)
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM

    dev = "cuda:0"
    sizes, B = (a.K_lo, a.N, a.K_hi), a.rows
    g = np.random.Generator(np.random.PCG64(1))
    torch.manual_seed(1)
    layers = [RBM(sizes[l], sizes[l + 1], 0.1, 1e-4, 0.5).to(dev) for l in range(2)]
    eng = E.get_hip_engine()
    rng = E.PhiloxRng(3)
    bits = lambda n, p: torch.from_numpy((g.random((B, n)) < p).astype(np.float32)).to(dev)
    x_lo, x_hi = bits(sizes[0], 0.2), bits(sizes[2], 0.5)
    m = torch.from_numpy((0.05 + 0.9 * g.random((B, sizes[1]))).astype(np.float32)).to(dev)
    bias = layers[0].hid_bias.data
    data, particles = bits(sizes[0], 0.2), [bits(n, 0.5) for n in sizes]
    scalars = [(0.001, 0.5), (0.001, 0.5)]

    def pair():
        eng.prop_up(layers[0], x_lo)
        eng.prop_down(layers[1], x_hi, logits_only=True)

    calls = {
        "dbm_layer_mf": lambda: eng.dbm_layer(layers[0], layers[1], x_lo, x_hi, bias, m=m, damp=0.5, want_res=True),
        "dbm_layer_sample": lambda: eng.dbm_layer(layers[0], layers[1], x_lo, x_hi, bias, sample=True, rng=rng),
        "pair": pair,
        "dbm_step": lambda: eng.dbm_step(layers, data, particles, scalars, 10, 0.0, 5, rng),
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
    finite = bool(all(torch.isfinite(r.W.data).all() for r in layers) and torch.isfinite(m).all())
    print(json.dumps({a.only + "_us": us, "finite": finite, "cus": eng.device_info()[0]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K_lo", type=int, default=10000)
    ap.add_argument("--N", type=int, default=1500)
    ap.add_argument("--K_hi", type=int, default=500)
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
    out = {"K_lo": a.K_lo, "N": a.N, "K_hi": a.K_hi, "rows": a.rows}
    for name in NAMES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--only", name]
        for k in ("K_lo", "N", "K_hi", "rows", "reps", "warmup", "runs"):
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
