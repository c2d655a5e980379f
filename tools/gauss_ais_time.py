"""Time per temperature of the Gaussian AIS call next to the same loop written in PyTorch on the same device.

  engine    HipEngine.gauss_ais with K = 20 linear temperatures: the start kernel, then per temperature prep_operand, the up
            propagation's logits (one launch, or split-K GEMM + finish), gauss_ais_weight_sample_h, the down propagation's mean and
            gauss_ais_visible -- 5 launches (6 with split-K up; 2 or 3 at the last temperature);
  torch     the same estimator in eager PyTorch: fp32 matmuls and state, float64 weight sums, torch's own generator.

Shapes: 784 <-> 256 with 256 chains, 10000 <-> 1500 with 64.  Two warm-up calls, then 7 calls each between two stream events: the
median, divided by K.  Prints one JSON line per shape.  Not a test, no threshold."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_ais(W, b, c, z, bA, betas, M):
    import torch
    V, H = W.shape
    sd, iv = torch.exp(0.5 * z), torch.exp(-z)
    coef, mid = ((b - bA) * iv).double(), (0.5 * (b + bA)).double()
    v = bA + sd * torch.randn(M, V, device=W.device)
    logw = torch.zeros(M, dtype=torch.float64, device=W.device)
    sp = torch.nn.functional.softplus
    for k in range(1, len(betas)):
        x = ((v * iv) @ W + c).double()
        logw += (betas[k] - betas[k - 1]) * ((v.double() - mid) * coef).sum(1) + (sp(betas[k] * x) - sp(betas[k - 1] * x)).sum(1)
        if k == len(betas) - 1:
            break
        h = (torch.sigmoid(betas[k] * x.float()) > torch.rand(M, H, device=W.device)).float()
        v = ((1.0 - betas[k]) * bA + betas[k] * (h @ W.t() + b)) + sd * torch.randn(M, V, device=W.device)
    return logw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-build", action="store_true", help="the library is built: only load it (a process under a profiler)")
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
    bl = [float(x) for x in betas.tolist()]

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            t.append(1000.0 * t0.elapsed_time(t1) / a.K)
        return round(statistics.median(t), 1), round(max(t) - min(t), 1)

    for V, H, M in ((784, 256, 256), (10000, 1500, 64)):
        g = np.random.Generator(np.random.PCG64(1))
        r = GaussianRBM(V, H, 0.01, 1e-4, 0.5).to(dev)
        r.W.data.copy_(torch.from_numpy((g.standard_normal((V, H)) / np.sqrt(V)).astype(np.float32)).to(dev))
        r.vis_bias.data.copy_(torch.from_numpy((0.5 * g.standard_normal(V)).astype(np.float32)).to(dev))
        r.logvar.data.copy_(torch.from_numpy((0.4 * g.standard_normal(V)).astype(np.float32)).to(dev))
        bA = (r.vis_bias.data + 0.3 * torch.randn(V, device=dev)).contiguous()
        rng = E.PhiloxRng(3)
        Wc = r.W.data.contiguous()
        out = {"V": V, "H": H, "chains": M, "K": a.K, "cus": eng.device_info()[0]}
        out["engine_us_per_temperature"], out["engine_spread_us"] = timed(
            lambda: eng.gauss_ais(r, r.logvar.data, betas, M, rng, base_vis_bias=bA))
        out["torch_us_per_temperature"], out["torch_spread_us"] = timed(
            lambda: torch_ais(Wc, r.vis_bias.data, r.hid_bias.data, r.logvar.data, bA, bl, M))
        lw = eng.gauss_ais(r, r.logvar.data, betas, M, rng, base_vis_bias=bA)
        out["up_route"], out["down_route"] = eng.last_route()["up"], eng.last_route()["down"]
        out["finite"] = bool(torch.isfinite(lw).all())
        print(json.dumps(out))


if __name__ == "__main__":
    main()
