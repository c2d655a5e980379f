"""Time HipEngine.unit_moments on one validation split -- N = 10 000 rows, H = 1500, K = 32, R = 2 -- against the same
statistics composed in torch on the device (``index_add_`` into float64 [K, H] for the class sums and sums of squares, a float64
matmul for xa) and against the copy of the [N, H] activations to the host that a numpy analysis starts with.  HIP events around
`reps` calls after `warm`, the whole measurement twice in one process.  Prints one JSON line per run.  Not a test, no threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--units", type=int, default=1500)
    ap.add_argument("--classes", type=int, default=32)
    ap.add_argument("--regressors", type=int, default=2)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    import torch
    from imdbn import engine as E

    dev = "cuda:0"
    eng = E.get_hip_engine()
    N, H, K, R = a.rows, a.units, a.classes, a.regressors
    g = torch.Generator(device=dev).manual_seed(1)
    act = torch.rand(N, H, device=dev, generator=g)
    cls = torch.randint(0, K, (N,), device=dev, generator=g, dtype=torch.int32)
    x = torch.randn(N, R, device=dev, generator=g)
    cls64 = cls.long()
    z = torch.cat([torch.ones(N, 1, device=dev), x], 1).double()

    def kernel():
        return eng.unit_moments(act, cls, K, x)

    def composed():
        a64 = act.double()
        s1 = torch.zeros(K, H, dtype=torch.float64, device=dev).index_add_(0, cls64, a64)
        s2 = torch.zeros(K, H, dtype=torch.float64, device=dev).index_add_(0, cls64, a64 * a64)
        return s1, s2, z.T @ a64

    def to_host():
        return act.cpu()

    def timed(fn):
        for _ in range(a.warm):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.reps

    moved = 4 * N * H + 4 * N * (R + 1)                                # bytes the kernel must read: act, x and cls once
    for run in range(a.runs):
        ms = {"unit_moments_ms": timed(kernel), "torch_composed_ms": timed(composed), "copy_to_host_ms": timed(to_host)}
        print(json.dumps({"run": run, "N": N, "H": H, "K": K, "R": R, **{k: round(v, 4) for k, v in ms.items()},
                          "input_bytes": moved, "input_GBps": round(moved / (ms["unit_moments_ms"] * 1e-3) / 1e9, 1),
                          "workspace_bytes": int(eng._lib.imdbn_unit_moments_ws_bytes(N, H, K, R))}), flush=True)


if __name__ == "__main__":
    main()
