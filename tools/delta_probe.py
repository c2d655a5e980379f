"""Time one delta-rule step of a directed layer next to the same update composed from the calls that existed before it,
at 10000 <-> 1500 and 1500 <-> 500, batch 64, 0/1 operands, in both directions.

  delta_step   HipEngine.delta_step with apply and rowlp on: operand preparation, logits propagation, delta_rows, delta_finish, the
               update kernel.
  composed     the logits propagation of the predicting side with its sigmoid (prop_up; prop_down(logits_only) + torch.sigmoid) and
               HipEngine.assoc_update with the pairs (in, target) / (in, p): four operand preparations, the update kernel with its
               bias rows.  It computes no row log-probability and also moves the other bias's momentum.  These calls are unchanged
               by the feature, so the figure is the parent commit's.

HIP events around `reps` calls after a warm-up, microseconds per call; the two forms alternate `runs` times in one process.  Not a
test, no threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000x1500,1500x500")
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-build", action="store_true", help="the library is built: only load it (a process under a profiler)")
    a = ap.parse_args()

    import __graft_entry__ as ge
    ge.build(compile_ok=not a.no_build)
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM

    dev = "cuda:0"
    eng = E.get_hip_engine()
    g = np.random.Generator(np.random.PCG64(1))
    lr, mom, B = 0.01, 0.5, a.rows

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

    out = {"rows": B, "cus": eng.device_info()[0], "reps": a.reps}
    for shape in a.shapes.split(","):
        V, H = (int(x) for x in shape.split("x"))
        r = RBM(V, H, 0.1, 1e-4, 0.5, dynamic_lr=True, final_momentum=0.95).to(dev)
        lo = torch.from_numpy((g.random((B, V)) > 0.8).astype(np.float32)).to(dev)
        hi = torch.from_numpy((g.random((B, H)) > 0.5).astype(np.float32)).to(dev)
        calls = {
            "up_delta_step": lambda: eng.delta_step(r, "up", lo, hi, lr, mom),
            "up_composed": lambda: eng.assoc_update(r, lo, hi, lo, eng.prop_up(r, lo), lr, mom),
            "down_delta_step": lambda: eng.delta_step(r, "down", hi, lo, lr, mom),
            "down_composed": lambda: eng.assoc_update(r, lo, hi, torch.sigmoid(eng.prop_down(r, hi, logits_only=True)), hi, lr, mom),
            "up_evaluate_only": lambda: eng.delta_step(r, "up", lo, hi, apply=False),
            "down_evaluate_only": lambda: eng.delta_step(r, "down", hi, lo, apply=False),
        }
        res = {k: [] for k in calls}
        for _ in range(a.runs):
            for k, fn in calls.items():
                res[k].append(timed(fn))
        res["finite"] = bool(torch.isfinite(r.W.data).all() and torch.isfinite(r.W_m).all())
        out[shape] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
