"""Time the persistent-chain calls next to the CD-1 update on the benchmarked RBM: 10000 <-> 1500, batch 64, binary data.

  cd_step          HipEngine.cd_step, CD-1 (no next-batch prefetch: the persistent calls have none either);
  pcd_step         HipEngine.pcd_step, cd_k = 1, with the mean-field reconstruction error;
  pcd_step_noloss  the same with monitor=False (no reconstruction launch);
  pt_sweep         HipEngine.pt_sweep, R replicas of `rows` chains, one sweep (a Gibbs step per replica, one exchange).

By launch count PCD-1 is CD-1 plus one up propagation plus the particles' operand preparation (and the reconstruction's down
propagation when monitored).  HIP events around `reps` calls after a warm-up, microseconds per call, `runs` times each.  Not a test,
no threshold."""
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
    ap.add_argument("--replicas", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM

    dev = "cuda:0"
    V, H, B, Rn = a.V, a.H, a.rows, a.replicas
    g = np.random.Generator(np.random.PCG64(1))
    r = RBM(V, H, 0.1, 1e-4, 0.5, dynamic_lr=True, final_momentum=0.95).to(dev)
    data = torch.from_numpy((g.random((B, V)) > 0.8).astype(np.float32)).to(dev)
    data._imdbn_binary = True
    particles = torch.from_numpy((g.random((B, V)) > 0.8).astype(np.float32)).to(dev)
    state = torch.from_numpy((g.random((Rn * B, V)) > 0.8).astype(np.float32)).to(dev)
    betas = [float(x) for x in np.linspace(1.0 / Rn, 1.0, Rn)]
    eng = E.get_hip_engine()
    rng = E.PhiloxRng(3)
    lr, mom = 0.01, 0.5
    tries = torch.zeros(max(Rn - 1, 1), dtype=torch.int64, device=dev)
    accs = torch.zeros_like(tries)

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
        "cd_step_us": lambda: eng.cd_step(r, data, lr, mom, 1, rng),
        "pcd_step_us": lambda: eng.pcd_step(r, data, particles, lr, mom, 1, rng),
        "pcd_step_noloss_us": lambda: eng.pcd_step(r, data, particles, lr, mom, 1, rng, monitor=False),
        "pt_sweep_us": lambda: eng.pt_sweep(r, state, betas, 1, rng, tries, accs),
    }
    out = {"V": V, "H": H, "rows": B, "replicas": Rn}
    for name, fn in calls.items():
        out[name] = [timed(fn) for _ in range(a.runs)]
    out["swap_rates"] = (accs.double() / tries.double().clamp(min=1.0)).cpu().tolist()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
