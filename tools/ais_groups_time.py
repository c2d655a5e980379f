"""Time per temperature of HipEngine.ais_groups against the same AIS step written in torch, on the GPU.

Both forms run on the same parameters in the same process, alternating in rounds; each round times one whole chain of `--temps`
temperatures between two device events and divides by the number of temperatures.  Prints the median time per temperature of either
form and their ratio.  ``--reverse`` times HipEngine.reverse_ais instead, one chain per start state and `--chains` of
them at the same shape; the engine form only.  No GPU: an error, never a CPU number."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-idbn_amd")]


def torch_chain(W, b, c, bA, s, e, betas, M):
    """The chain of imdbn_rbm_ais_groups for ONE trailing softmax group [s, e) in torch ops: fp32 logits, weights in double."""
    import torch
    import torch.nn.functional as Fn
    V = W.size(0)

    def sample(logits):
        v = (torch.sigmoid(logits) > torch.rand_like(logits)).float()
        idx = torch.multinomial(torch.softmax(logits[:, s:e], 1).clamp(1e-8, 1.0), 1)
        v[:, s:e] = 0
        v.scatter_(1, s + idx, 1.0)
        return v

    v = sample(bA.expand(M, V))
    logw = torch.zeros(M, dtype=torch.float64, device=W.device)
    db = (b - bA).double()
    for k in range(1, len(betas)):
        x = (v @ W + c).double()
        logw += (betas[k] - betas[k - 1]) * (v.double() @ db) + (Fn.softplus(betas[k] * x) - Fn.softplus(betas[k - 1] * x)).sum(1)
        if k < len(betas) - 1:
            h = (torch.sigmoid(betas[k] * x.float()) > torch.rand(M, W.size(1), device=W.device)).float()
            v = sample(betas[k] * (h @ W.t() + b) + (1.0 - betas[k]) * bA)
    return logw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--temps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shape", default="532x256")
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--reverse", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM
    from imdbn.utils.likelihood import linear_betas
    if not torch.cuda.is_available():
        raise SystemExit("ais_groups_time needs a GPU")
    dev = "cuda:0"
    eng = E.get_hip_engine()
    V, H = (int(t) for t in args.shape.split("x"))
    s, e = V - args.labels, V
    r = RBM(V, H, 0.1, 0.0, 0.5, softmax_groups=[(s, e)]).to(dev)
    r.hid_bias.data.normal_(0, 0.5); r.vis_bias.data.normal_(0, 0.5)
    Wc, b, c = r.W.data.contiguous(), r.vis_bias.data, r.hid_bias.data
    bA = torch.randn(V, device=dev) * 0.5
    betas = linear_betas(args.temps)
    bl = betas.tolist()
    rng = E.PhiloxRng(1)
    forms = {"engine": lambda: eng.ais_groups(r, betas, args.chains, rng, base_vis_bias=bA),
             "torch": lambda: torch_chain(Wc, b, c, bA, s, e, bl, args.chains)}
    if args.reverse:
        x = (torch.rand(args.chains, V, device=dev) < 0.5).float()
        x[:, s:e] = 0
        x[torch.arange(args.chains), s + torch.randint(0, e - s, (args.chains,), device=dev)] = 1
        forms = {"engine": lambda: eng.reverse_ais(r, x, betas, rng, base_vis_bias=bA)}
    out = {}
    for k, fn in forms.items():                        # warm-up: code objects, workspaces, GEMM algorithm choice
        out[k] = fn()
    torch.cuda.synchronize()
    lme = {k: float(torch.logsumexp(w, 0)) - float(torch.log(torch.tensor(float(args.chains)))) for k, w in out.items()}
    print(f"{V}x{H} group ({s},{e}) chains {args.chains} temps {args.temps}: logmeanexp(logw) "
          + ", ".join(f"{k} {v:.3f}" for k, v in lme.items()) + " (other draws)", flush=True)
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms[k].append(1e3 * t0.elapsed_time(t1) / args.temps)
    me = statistics.median(ms["engine"])
    if args.reverse:
        print(f"{V}x{H} chains {args.chains}: reverse_ais {me:.1f} us per temperature (min {min(ms['engine']):.1f}, max {max(ms['engine']):.1f})",
              flush=True)
        return
    mt = statistics.median(ms["torch"])
    print(f"{V}x{H} chains {args.chains}: ais_groups {me:.1f} us per temperature (min {min(ms['engine']):.1f}, max {max(ms['engine']):.1f}); "
          f"torch {mt:.1f} us (min {min(ms['torch']):.1f}, max {max(ms['torch']):.1f}); torch / ais_groups {mt / me:.2f}", flush=True)


if __name__ == "__main__":
    main()
