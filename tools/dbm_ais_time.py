"""Time one temperature of the DBM's annealed importance sampling on the paper stack: 10000 - 1500 - 500, 64 chains.

  dbm_ais    HipEngine.dbm_ais over `temps` temperatures in one call, divided by `temps`: per temperature one WEIGH pass (with its
             draw) per even layer and one SAMPLE pass per odd layer, each with its one-thread-per-row finish;
  composed   the same step from what the engine offered before, on the same RBMs and in the same layer order: the pre-activation of
             an even layer by prop_down(logits_only=True) (layer 0) / prop_up and a logit (the top layer), the softplus difference
             and its float64 row sums in ATen, the draw by dbm_layer in sample mode (its scales standing in for the temperature); the
             odd layer by dbm_layer in sample mode and an ATen bias dot.

Every measurement runs in a child process of its own under a time limit (--limit seconds); the first one that fails or runs out of
time ends the tool, nothing more is started.  HIP events around `reps` calls after a warm-up, microseconds per temperature, `runs`
runs.  Not a test, no threshold."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("dbm_ais", "composed")


def measure(a):
    import __graft_entry__ as ge
    ge.build(compile_ok=False)
    import torch
    import torch.nn.functional as F
    from imdbn import engine as E
    from imdbn.models import RBM

    dev = "cuda:0"
    sizes, M, K = (a.N0, a.N1, a.N2), a.chains, a.temps
    torch.manual_seed(1)
    layers = [RBM(sizes[l], sizes[l + 1], 0.1, 1e-4, 0.5).to(dev) for l in range(2)]
    for r in layers:
        r.hid_bias.data.normal_(0, 0.3)
    layers[0].vis_bias.data.normal_(-1, 0.3)
    biases = [layers[0].vis_bias.data] + [r.hid_bias.data for r in layers]
    base = (layers[0].vis_bias.data * 0.8).contiguous()
    eng = E.get_hip_engine()
    rng = E.PhiloxRng(3)
    betas = (torch.arange(K + 1, dtype=torch.float64) / K).float()
    s = [(torch.rand(M, n, device=dev) < 0.5).float() for n in sizes]
    logw = torch.zeros(M, dtype=torch.float64, device=dev)

    def composed():
        for k in range(1, K):
            b1, b0 = float(betas[k]), float(betas[k - 1])
            pre0 = eng.prop_down(layers[0], s[1], logits_only=True)
            logw.add_((F.softplus(b1 * pre0 + (1 - b1) * base) - F.softplus(b0 * pre0 + (1 - b0) * base)).double().sum(1))
            eng._dbm_layer(None, layers[0], None, s[1], biases[0], None, 0.0, 1.0, b1, True, rng, False, False, s_out=s[0])
            pre2 = torch.logit(eng.prop_up(layers[1], s[1]), eps=1e-6)
            logw.add_((F.softplus(b1 * pre2) - F.softplus(b0 * pre2)).double().sum(1))
            eng._dbm_layer(layers[1], None, s[1], None, biases[2], None, 0.0, b1, 1.0, True, rng, False, False, s_out=s[2])
            eng._dbm_layer(layers[0], layers[1], s[0], s[2], biases[1], None, 0.0, b1, b1, True, rng, False, False, s_out=s[1])
            logw.add_((float(betas[k + 1]) - b1) * (s[1].double() @ biases[1].double()))

    calls = {"dbm_ais": lambda: eng.dbm_ais(layers, biases, betas, M, rng, base_bias=base), "composed": composed}
    fn = calls[a.only]
    steps = K if a.only == "dbm_ais" else K - 1           # the last temperature of the call only weighs

    def timed():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            out = fn()
        t1.record()
        torch.cuda.synchronize()
        return round(1000.0 * t0.elapsed_time(t1) / (a.reps * steps), 1), out

    runs = [timed() for _ in range(a.runs)]
    last = runs[-1][1] if a.only == "dbm_ais" else logw
    print(json.dumps({a.only + "_us_per_temperature": [r[0] for r in runs], "finite": bool(torch.isfinite(last).all()),
                      "cus": eng.device_info()[0]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N0", type=int, default=10000)
    ap.add_argument("--N1", type=int, default=1500)
    ap.add_argument("--N2", type=int, default=500)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--temps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds every measurement may take")
    ap.add_argument("--only", default=None, choices=NAMES, help="run this measurement in this process")
    a = ap.parse_args()
    if a.only:
        return measure(a)
    import __graft_entry__ as ge
    ge.build()                               # in this process, which never touches the GPU
    out = {"sizes": [a.N0, a.N1, a.N2], "chains": a.chains, "temps": a.temps}
    for name in NAMES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--only", name]
        for k in ("N0", "N1", "N2", "chains", "temps", "reps", "warmup", "runs"):
            cmd += [f"--{k}", str(getattr(a, k))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            out["failed"] = {"name": name, "status": p.returncode}
            print(json.dumps(out))
            sys.exit(1)                      # nothing more is started on the GPU
        out.update(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
