"""Time HipEngine.exact_log_z: one call between the event pair of imdbn_profile_enable / imdbn_profile_read, warm, best of
`reps`, at the shapes of the section's table.  Prints one JSON line per shape.  Not a test, no threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (n, D, side, marginals)
SHAPES = [(20, 784, "hidden", False), (20, 784, "hidden", True), (24, 784, "hidden", False), (24, 10000, "hidden", False),
          (20, 1500, "visible", False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-n", type=int, default=24)
    a = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM

    dev = "cuda:0"
    eng = E.get_hip_engine()
    g = np.random.Generator(np.random.PCG64(1))
    for n, D, side, marg in SHAPES:
        if n > a.max_n:
            continue
        V, H = (D, n) if side == "hidden" else (n, D)
        r = RBM(V, H, 0.1, 0.0, 0.5).to(dev)
        r.W.data.copy_(torch.from_numpy((0.05 * g.standard_normal((V, H))).astype(np.float32)))
        r.vis_bias.data.copy_(torch.from_numpy((0.1 * g.standard_normal(V)).astype(np.float32)))
        r.hid_bias.data.copy_(torch.from_numpy((0.1 * g.standard_normal(H)).astype(np.float32)))
        res = eng.exact_log_z(r, side=side, marginals=marg, max_bits=n)          # warm
        torch.cuda.synchronize()
        best = None
        for _ in range(a.reps):
            eng.profile(True)
            res = eng.exact_log_z(r, side=side, marginals=marg, max_bits=n)
            ms, pairs = eng.profile_read()
            eng.profile(False)
            assert pairs == 1
            best = ms if best is None else min(best, ms)
        print(json.dumps({"n": n, "D": D, "side": side, "marginals": marg, "best_ms": round(best, 3), "log_z": float(res["log_z"]),
                          "softplus_per_s": round((2.0 ** n) * D * (2 if marg else 1) / (best * 1e-3), 0)}), flush=True)


if __name__ == "__main__":
    main()
