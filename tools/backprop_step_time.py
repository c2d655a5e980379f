"""Time one backprop step of the unrolled stack: [10000, 1500, 500], batch 64, binary data.

  autoencoder_step   HipEngine.autoencoder_step, monitors off: the forward pass up the encoder and down the decoder, then one
                     backprop_step per decoder layer, two on the tied top RBM and one per encoder layer below it;
  composed           the same sequence hand-composed from older calls: each back-propagated error as prop_down / prop_up on a
                     zero-bias clone of the layer (prop_up has no logits-only form: its sigmoid is undone with torch.logit, which is
                     good enough for a timing and not for a result) times a torch x (1 - x), each update as assoc_update with a zero
                     second pair -- two of them on the tied top RBM, one per pair.

Next to the times the tool prints the engine calls per step and the kernel launches of the backprop calls per step, counted from the
launch list of host_backprop.hpp (a propagation is counted as one launch; a split-K route adds its epilogue launch).  HIP events
around `reps` steps after a warm-up, microseconds per step, `runs` times each.  Not a test, no threshold."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 1500, 500])
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import iDBN

    dev = "cuda:0"
    B = a.rows
    g = np.random.Generator(np.random.PCG64(1))
    net = iDBN(list(a.sizes), {"LEARNING_RATE": 0.01, "WEIGHT_PENALTY": 1e-4, "INIT_MOMENTUM": 0.5, "FINAL_MOMENTUM": 0.95,
                               "LEARNING_RATE_DYNAMIC": False, "CD": 1}, [], [], torch.device(dev))
    gen = net.untie()
    rec = net.layers
    L = len(rec)
    data = torch.from_numpy((g.random((B, a.sizes[0])) > 0.8).astype(np.float32)).to(dev)
    data._imdbn_binary = True
    eng = E.get_hip_engine()
    scalars = [(0.001, 0.5)] * L

    def zero_bias(r):
        z = copy.copy(r)
        z._parameters = dict(r._parameters)
        z.__dict__.pop("_imdbn_desc", None)
        z.hid_bias = torch.nn.Parameter(torch.zeros_like(r.hid_bias.data), requires_grad=False)
        z.vis_bias = torch.nn.Parameter(torch.zeros_like(r.vis_bias.data), requires_grad=False)
        return z
    zeros = {id(r): zero_bias(r) for r in rec + gen}
    launches = [0]

    def composed_backprop(r, up=None, down=None, lr=0.0, mom=0.0, apply=True, want_v=False, want_h=False):
        z = zeros[id(r)]
        ev = eh = None
        if want_v:
            ev = eng.prop_down(z, up[1], logits_only=True) * (up[0] * (1 - up[0]))
        if want_h:
            eh = torch.logit(eng.prop_up(z, down[1])) * (down[0] * (1 - down[0]))
        if apply and up is not None:
            eng.assoc_update(r, up[0], up[1], up[0], torch.zeros_like(up[1]), lr, mom)
        if apply and down is not None:
            eng.assoc_update(r, down[1], down[0], torch.zeros_like(down[1]), down[0], lr, mom)
        return ev, eh

    def counted_backprop(r, up=None, down=None, lr=0.0, mom=0.0, apply=True, want_v=False, want_h=False):
        rows = -(-B // 64)
        launches[0] += 4 * (int(want_v) + int(want_h))                      # preparation, memset node, propagation, backprop_apply
        if apply:
            launches[0] += 2 * ((up is not None) + (down is not None)) + 1 + rows      # preparation + backprop_rows per pair, finish, update
        return eng.backprop_step(r, up, down, lr, mom, apply, want_v, want_h)

    class Composed:
        """The engine with backprop_step replaced: autoencoder_step is host logic over the engine's calls."""
        def __getattr__(self, k):
            return getattr(eng, k)
    comp, cnt = Composed(), Composed()
    comp.backprop_step, cnt.backprop_step = composed_backprop, counted_backprop
    step = type(eng).autoencoder_step
    step(cnt, rec, gen, data, scalars, monitor=False)
    calls_per_step = 2 * L + (L - 1) + 2 + (L - 1)      # forward, backward, then the backprop calls

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

    out = {"sizes": list(a.sizes), "rows": B, "engine_calls_per_step": calls_per_step, "backprop_launches_per_step": launches[0]}
    out["autoencoder_step_us"] = [timed(lambda: eng.autoencoder_step(rec, gen, data, scalars, monitor=False)) for _ in range(a.runs)]
    out["composed_us"] = [timed(lambda: step(comp, rec, gen, data, scalars, monitor=False)) for _ in range(a.runs)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
