"""Time one bracket of the Gaussian stack bound next to the same bracket written in PyTorch on the same tensors.

  engine    HipEngine.gauss_bound_step: the scale launch, prep_operand, the up propagation's logits (one launch, or split-K GEMM +
            finish), bound_entropy_sample_h, the down propagation's mean and gauss_bound_loglik_rows -- 6 launches (7 with split-K up);
  torch     the same bracket in eager PyTorch: fp32 matmuls, float64 sums, torch's own generator.

Shapes: 784 <-> 256 and 10000 <-> 1500, M = 1024 rows, mode entropy.  A warm-up, then 7 calls each between two stream events: the
median and the spread, microseconds per call.  Prints one JSON line per shape.  Not a test, no threshold."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_bracket(W, b, c, z, v, acc):
    import torch
    sp = torch.nn.functional.softplus
    x = ((v * torch.exp(-z)) @ W + c)
    h = (torch.sigmoid(x) > torch.rand_like(x)).float()
    xd = x.double()
    e = (sp(xd) - xd * torch.sigmoid(xd)).sum(1)
    d = v.double() - (h @ W.t() + b).double()
    zd = z.double()
    acc += e - (d * d * torch.exp(-zd) / 2 + zd / 2).sum(1) - 0.5 * W.shape[0] * 1.8378770664093453
    return acc, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
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

    dev = "cuda:0"
    eng = E.get_hip_engine()

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
            t.append(1000.0 * t0.elapsed_time(t1))
        return round(statistics.median(t), 1), round(max(t) - min(t), 1)

    for V, H in ((784, 256), (10000, 1500)):
        M = a.rows
        g = np.random.Generator(np.random.PCG64(1))
        r = GaussianRBM(V, H, 0.01, 1e-4, 0.5).to(dev)
        r.W.data.copy_(torch.from_numpy((g.standard_normal((V, H)) / np.sqrt(V)).astype(np.float32)).to(dev))
        r.vis_bias.data.copy_(torch.from_numpy((0.5 * g.standard_normal(V)).astype(np.float32)).to(dev))
        r.logvar.data.copy_(torch.from_numpy((0.4 * g.standard_normal(V)).astype(np.float32)).to(dev))
        v = (r.vis_bias.data + torch.exp(0.5 * r.logvar.data) * torch.randn(M, V, device=dev)).contiguous()
        rng = E.PhiloxRng(3)
        Wc = r.W.data.contiguous()
        acc_e = torch.zeros(M, dtype=torch.float64, device=dev)
        acc_t = torch.zeros(M, dtype=torch.float64, device=dev)
        out = {"V": V, "H": H, "rows": M, "cus": eng.device_info()[0]}
        out["engine_us"], out["engine_spread_us"] = timed(lambda: eng.gauss_bound_step(r, r.logvar.data, v, rng, acc=acc_e))
        out["torch_us"], out["torch_spread_us"] = timed(lambda: torch_bracket(Wc, r.vis_bias.data, r.hid_bias.data, r.logvar.data, v, acc_t))
        a1, _ = eng.gauss_bound_step(r, r.logvar.data, v, E.PhiloxRng(2))
        out["up_route"], out["down_route"] = eng.last_route()["up"], eng.last_route()["down"]
        a2, _ = torch_bracket(Wc, r.vis_bias.data, r.hid_bias.data, r.logvar.data, v, torch.zeros(M, dtype=torch.float64, device=dev))
        out["finite"] = bool(torch.isfinite(a1).all())
        out["mean_engine"], out["mean_torch"] = round(float(a1.mean()), 3), round(float(a2.mean()), 3)      # different draws: close, not equal
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
