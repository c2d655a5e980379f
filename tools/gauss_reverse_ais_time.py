"""Time per temperature of the Gaussian reverse-AIS call next to the forward call on the same rows.

  reverse   HipEngine.gauss_reverse_ais with K linear temperatures from R rows: gauss_rais_load_v, then per temperature prep_operand,
            the up propagation's logits (one launch, or split-K GEMM + finish), gauss_ais_weight_sample_h, the down propagation's mean
            and gauss_ais_visible -- the launches of the forward call, K transitions where the forward call makes K - 1;
  forward   HipEngine.gauss_ais with the same ladder and R chains.

Shapes: 784 <-> 500 and the bench layer 10000 <-> 1500, each with R = 64 and R = 4096.  Warm-up calls of both, then `runs` pairs,
the two calls alternating, each between two stream events: the median and the spread (max - min), divided by K.  Prints one JSON
line per shape and R.  `--only V,H,R --which reverse|forward` runs one call at one point, for a kernel trace of its own.  Not a test,
no threshold."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--no-build", action="store_true", help="the library is built: only load it (a process under a profiler)")
    ap.add_argument("--only", default=None, help="V,H,R: time this one configuration")
    ap.add_argument("--which", default="both", choices=["both", "reverse", "forward"], help="run one of the two calls only (a kernel trace)")
    a = ap.parse_args()

    import __graft_entry__ as ge
    ge.build(compile_ok=not a.no_build)
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import GaussianRBM
    from imdbn.utils.likelihood import linear_betas

    dev = "cuda:0"
    eng = E.get_hip_engine()
    betas = linear_betas(a.K)

    def once(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return 1000.0 * t0.elapsed_time(t1) / a.K

    def stats(t):
        return round(statistics.median(t), 1), round(max(t) - min(t), 1)

    shapes = [(784, 500, 64), (784, 500, 4096), (10000, 1500, 64), (10000, 1500, 4096)]
    if a.only:
        shapes = [tuple(int(x) for x in a.only.split(","))]
    for V, H, Rn in shapes:
        g = np.random.Generator(np.random.PCG64(1))
        r = GaussianRBM(V, H, 0.01, 1e-4, 0.5).to(dev)
        r.W.data.copy_(torch.from_numpy((g.standard_normal((V, H)) / np.sqrt(V)).astype(np.float32)).to(dev))
        r.vis_bias.data.copy_(torch.from_numpy((0.5 * g.standard_normal(V)).astype(np.float32)).to(dev))
        r.logvar.data.copy_(torch.from_numpy((0.4 * g.standard_normal(V)).astype(np.float32)).to(dev))
        bA = (r.vis_bias.data + 0.3 * torch.randn(V, device=dev)).contiguous()
        rows = (r.vis_bias.data + torch.exp(0.5 * r.logvar.data) * torch.randn(Rn, V, device=dev)).contiguous()
        rng = E.PhiloxRng(3)
        rev = lambda: eng.gauss_reverse_ais(r, r.logvar.data, rows, betas, rng, base_vis_bias=bA)
        fwd = lambda: eng.gauss_ais(r, r.logvar.data, betas, Rn, rng, base_vis_bias=bA)
        calls = [(n, f) for n, f in (("reverse", rev), ("forward", fwd)) if a.which in ("both", n)]
        for _ in range(a.warmup):
            for _, f in calls:
                f()
        torch.cuda.synchronize()
        t = {n: [] for n, _ in calls}
        for _ in range(a.runs):
            for n, f in calls:
                t[n].append(once(f))
        out = {"V": V, "H": H, "R": Rn, "K": a.K, "cus": eng.device_info()[0]}
        for n, _ in calls:
            out[n + "_us_per_temperature"], out[n + "_spread_us"] = stats(t[n])
        lw = calls[0][1]()
        out["up_route"], out["down_route"] = eng.last_route()["up"], eng.last_route()["down"]
        out["finite"] = bool(torch.isfinite(lw).all())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
