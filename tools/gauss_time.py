"""Time the Gaussian-visible update next to the centered update on the benchmarked shape: 10000 <-> 1500, batch 64.

  centered_cd     HipEngine.centered_step with CD-1 phases on binary data (tools/centered_step_time.py's call): the yardstick, the same
                  statistics-pass-plus-apply structure;
  gauss_cd        HipEngine.gauss_cd_step, CD-1 with sample_v, on real data (offset + scale N(0, 1));
  gauss_cd_mean   ... with sample_v off (no normals drawn).

HIP events around `reps` calls after a warm-up, microseconds per call, `runs` times each; the median and the spread (max - min) of
the runs are reported next to them.  The per-kernel times come from a kernel trace of this script in a run of its own (rocprofv3
--kernel-trace --stats -- python tools/gauss_time.py --no-build --only gauss_cd).  Not a test, no threshold."""
import argparse
import json
import os
import statistics
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
    ap.add_argument("--runs", type=int, default=5)
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
    binary = torch.from_numpy((g.random((B, V)) > 0.8).astype(np.float32)).to(dev)
    binary._imdbn_binary = True
    real = torch.from_numpy((g.standard_normal(V) + (0.3 + 2.7 * g.random(V)) * g.standard_normal((B, V))).astype(np.float32)).to(dev)
    mu, lam = torch.full((V,), 0.2, device=dev), torch.full((H,), 0.5, device=dev)
    z, zm = torch.zeros(V, device=dev), torch.zeros(V, device=dev)
    eng = E.get_hip_engine()
    rng = E.PhiloxRng(3)
    lr, mom = 1e-4, 0.5

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
        "centered_cd": lambda: eng.centered_step(r, binary, None, lr, mom, 1, rng, mu, lam, 0.01, 0),
        "gauss_cd": lambda: eng.gauss_cd_step(r, z, zm, real, lr, mom, 1, rng, 0.5 * lr, z_lo=-4.0, z_hi=4.0, sample_v=True),
        "gauss_cd_mean": lambda: eng.gauss_cd_step(r, z, zm, real, lr, mom, 1, rng, 0.5 * lr, z_lo=-4.0, z_hi=4.0, sample_v=False),
    }
    out = {"V": V, "H": H, "rows": B, "cus": eng.device_info()[0]}
    for name, fn in calls.items():
        if a.only in (None, name):
            t = [timed(fn) for _ in range(a.runs)]
            out[name + "_us"] = t
            out[name + "_median_us"] = statistics.median(t)
            out[name + "_spread_us"] = round(max(t) - min(t), 1)
    out["finite"] = bool(torch.isfinite(r.W.data).all() and torch.isfinite(z).all() and torch.isfinite(mu).all())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
