"""Time one HipEngine.bound_step call against the same layer step written in torch, on the GPU.

Both forms run on the same tensors in the same process, alternating in rounds; each round times `--calls` calls between two device
events.  Prints the median time per call of either form and their ratio per shape.  No GPU: an error, never a CPU number."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-idbn_amd")]


def torch_step(W, b, c, v, acc):
    import torch
    import torch.nn.functional as Fn
    x = v @ W + c
    p = torch.sigmoid(x)
    h = (p > torch.rand_like(p)).float()
    e = (Fn.softplus(x) - x * p).sum(1)
    a = h @ W.t() + b
    acc += ((v * a - Fn.softplus(a)).sum(1) + e).double()
    return acc, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="10000x1500,1500x500")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM
    if not torch.cuda.is_available():
        raise SystemExit("bound_step_time needs a GPU")
    dev = "cuda:0"
    eng = E.get_hip_engine()
    for shape in args.shapes.split(","):
        V, H = (int(t) for t in shape.split("x"))
        r = RBM(V, H, 0.1, 0.0, 0.5).to(dev)
        r.hid_bias.data.normal_(0, 0.5); r.vis_bias.data.normal_(0, 0.5)
        Wc, b, c = r.W.data.contiguous(), r.vis_bias.data, r.hid_bias.data
        v = (torch.rand(args.rows, V, device=dev) > 0.5).float()
        rng = E.PhiloxRng(1)
        acc_e = torch.zeros(args.rows, dtype=torch.float64, device=dev)
        acc_t = torch.zeros_like(acc_e)
        forms = {"engine": lambda: eng.bound_step(r, v, rng, acc=acc_e), "torch": lambda: torch_step(Wc, b, c, v, acc_t)}
        for fn in forms.values():                      # warm-up: code objects, workspaces, GEMM algorithm choice
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        a1, _ = eng.bound_step(r, v, E.PhiloxRng(2))
        a2, _ = torch_step(Wc, b, c, v, torch.zeros_like(acc_e))
        print(f"{V}x{H} rows {args.rows}: mean acc engine {float(a1.mean()):.3f}, torch {float(a2.mean()):.3f} (other draws)", flush=True)
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.calls):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                ms[k].append(t0.elapsed_time(t1) / args.calls)
        me, mt = statistics.median(ms["engine"]), statistics.median(ms["torch"])
        print(f"{V}x{H} rows {args.rows}: bound_step {me:.3f} ms (min {min(ms['engine']):.3f}, max {max(ms['engine']):.3f}); "
              f"torch {mt:.3f} ms (min {min(ms['torch']):.3f}, max {max(ms['torch']):.3f}); torch / bound_step {mt / me:.2f}", flush=True)


if __name__ == "__main__":
    main()
