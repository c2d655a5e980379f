"""Time the centered update next to the plain updates on the benchmarked RBM: 10000 <-> 1500, batch 64, binary data.

  cd_step / pcd_step            HipEngine.cd_step (CD-1, no next-batch prefetch) / HipEngine.pcd_step (cd_k = 1, with its loss);
  centered_cd / centered_pcd    HipEngine.centered_step on the same phases: the statistics pass of the update kernel into the
                                scratch, centered_apply, centered_finish instead of the fused update.

HIP events around `reps` calls after a warm-up, microseconds per call, `runs` times each.  The per-kernel times of the three
launches come from a kernel trace of this script in a run of its own (rocprofv3 --kernel-trace --stats -- python
tools/centered_step_time.py --no-build --only centered_cd).  Not a test, no threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=10000)
    ap.add_argument("--H", type=int, default=1500)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default=None, help="time this call alone (for a kernel trace)")
    ap.add_argument("--no-build", action="store_true", help="the library is built: only load it (a process under a profiler)")
    a = ap.parse_args()

    import __graft_entry__ as ge
    ge.build(compile_ok=not a.no_build)
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM

    dev = "cuda:0"
    V, H, B = a.V, a.H, a.rows
    g = np.random.Generator(np.random.PCG64(1))
    r = RBM(V, H, 0.1, 1e-4, 0.5, dynamic_lr=True, final_momentum=0.95).to(dev)
    data = torch.from_numpy((g.random((B, V)) > 0.8).astype(np.float32)).to(dev)
    data._imdbn_binary = True
    particles = torch.from_numpy((g.random((B, V)) > 0.8).astype(np.float32)).to(dev)
    mu, lam = torch.full((V,), 0.2, device=dev), torch.full((H,), 0.5, device=dev)
    eng = E.get_hip_engine()
    rng = E.PhiloxRng(3)
    lr, mom = 0.01, 0.5

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

    calls = {
        "cd_step": lambda: eng.cd_step(r, data, lr, mom, 1, rng),
        "centered_cd": lambda: eng.centered_step(r, data, None, lr, mom, 1, rng, mu, lam, 0.01, 0),
        "pcd_step": lambda: eng.pcd_step(r, data, particles, lr, mom, 1, rng),
        "centered_pcd": lambda: eng.centered_step(r, data, particles, lr, mom, 1, rng, mu, lam, 0.01, 0),
    }
    out = {"V": V, "H": H, "rows": B, "cus": eng.device_info()[0]}
    for name, fn in calls.items():
        if a.only in (None, name):
            out[name + "_us"] = [timed(fn) for _ in range(a.runs)]
    out["finite"] = bool(torch.isfinite(r.W.data).all() and torch.isfinite(mu).all() and torch.isfinite(lam).all())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
