"""Time the TAP update and iteration on the benchmarked RBM: 10000 <-> 1500, batch 64, 0/1 data.

  tap_step_o2 / tap_step_o1     HipEngine.tap_step at n_iters = 3, order 2 / order 1, with its loss;
  pcd_step_k3                   HipEngine.pcd_step at cd_k = 3 with its loss, on this build: the stochastic sibling;
  tap_iterate_o2 / _o1          HipEngine.tap_iterate, n_iters = 10 without outputs, per iteration (two tap_half launches);
  composed_o2                   the same order-2 iteration composed from what the engine offered before: prop_up / prop_down with
                                logits on W and on a W o W copy (two propagations per half-step) and the element-wise rest in torch;
  square_copy                   the torch copy W o W that composition needs, re-made after every update.

HIP events around `reps` calls after a warm-up, microseconds per call, `runs` runs in one process.  Not a test, no threshold."""
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--only", default=None, help="time this call alone (for a kernel trace)")
    ap.add_argument("--no-build", action="store_true", help="the library is built: only load it (a process under a profiler)")
    a = ap.parse_args()

    import __graft_entry__ as ge
    ge.build(compile_ok=not a.no_build)
    import copy
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM

    dev = "cuda:0"
    V, H, B = a.V, a.H, a.rows
    g = np.random.Generator(np.random.PCG64(1))
    r = RBM(V, H, 0.1, 1e-4, 0.5, dynamic_lr=True, final_momentum=0.95).to(dev)
    data = torch.from_numpy((g.random((B, V)) > 0.8).astype(np.float32)).to(dev)
    data._imdbn_binary = True
    particles = torch.from_numpy((g.random((B, V)) > 0.8).astype(np.float32)).to(dev)
    eng = E.get_hip_engine()
    rng = E.PhiloxRng(3)
    lr, mom = 0.01, 0.5
    mv = torch.from_numpy((0.05 + 0.9 * g.random((B, V))).astype(np.float32)).to(dev)
    mh = eng.forward(r, mv).clone()
    # the composition: a second RBM object whose weights are the squares
    r2 = copy.copy(r)
    r2.__dict__.pop("_imdbn_desc", None)
    r2._parameters = dict(r._parameters)
    sq = torch.nn.Parameter(torch.empty_like(torch.as_strided(r.W.data, (V, r.W.stride(0)), (r.W.stride(0), 1)))[:, :H], requires_grad=False)
    r2._parameters["W"] = sq

    def square():
        torch.mul(r.W.data, r.W.data, out=sq.data)

    def composed():
        nonlocal mv, mh
        x = eng.prop_up(r, mv, T=1.0)            # sigmoid(c + mv W): inverted below, the engine has no up-logits entry
        a2 = eng.prop_up(r2, mv - mv * mv, T=1.0)
        x = torch.logit(x) - (mh - 0.5) * (torch.logit(a2) - r.hid_bias.data)
        mh = 0.5 * mh + 0.5 * torch.sigmoid(x)
        y = eng.prop_down(r, mh, logits_only=True)
        b2 = eng.prop_down(r2, mh - mh * mh, logits_only=True) - r.vis_bias.data
        mv = 0.5 * mv + 0.5 * torch.sigmoid(y - (mv - 0.5) * b2)

    def timed(fn, per=1):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return round(1000.0 * t0.elapsed_time(t1) / (a.reps * per), 1)

    square()
    calls = {
        "tap_step_o2": (lambda: eng.tap_step(r, data, mv, mh, lr, mom, 3, order=2), 1),
        "tap_step_o1": (lambda: eng.tap_step(r, data, mv, mh, lr, mom, 3, order=1), 1),
        "pcd_step_k3": (lambda: eng.pcd_step(r, data, particles, lr, mom, 3, rng), 1),
        "tap_iterate_o2": (lambda: eng.tap_iterate(r, mv, mh, 10, order=2, want_gamma=False, want_res=False), 10),
        "tap_iterate_o1": (lambda: eng.tap_iterate(r, mv, mh, 10, order=1, want_gamma=False, want_res=False), 10),
        "composed_o2": (composed, 1),
        "square_copy": (square, 1),
    }
    out = {"V": V, "H": H, "rows": B, "cus": eng.device_info()[0]}
    for name, (fn, per) in calls.items():
        if a.only in (None, name):
            out[name + "_us"] = [timed(fn, per) for _ in range(a.runs)]
    out["finite"] = bool(torch.isfinite(r.W.data).all() and torch.isfinite(mv).all() and torch.isfinite(mh).all())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
