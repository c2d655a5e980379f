"""Time the exact pseudo-log-likelihood call against its composition from free energies.

At 10000 x 1500 with 64 binary rows:
  fused      HipEngine.pseudo_loglik: the up propagation and the three kernels of imdbn_rbm_pseudo_loglik, HIP events around `reps`
             calls after a warm-up;
  composed   the same quantity from HipEngine.free_energy on flipped copies: -softplus(F(v) - F(v with bit i flipped)) for a SUBSET
             of `cols` columns (64 rows x cols flipped rows in one call), HIP events likewise, SCALED to V columns by V / cols.

Prints both times, the ratio, and the largest difference between the two on the subset.  Not a test, no threshold."""
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
    ap.add_argument("--cols", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM

    dev = "cuda:0"
    g = np.random.Generator(np.random.PCG64(1))
    r = RBM(a.V, a.H, 0.1, 0.0, 0.5).to(dev)
    r.W.data.copy_(torch.from_numpy((g.standard_normal((a.V, a.H)) / np.sqrt(a.V)).astype(np.float32)))
    r.vis_bias.data.copy_(torch.from_numpy((0.1 * g.standard_normal(a.V)).astype(np.float32)))
    r.hid_bias.data.copy_(torch.from_numpy((0.1 * g.standard_normal(a.H)).astype(np.float32)))
    v = torch.from_numpy((g.random((a.rows, a.V)) > 0.8).astype(np.float32)).to(dev)
    eng = E.get_hip_engine()

    def timed(fn, reps):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps, out

    fused_ms, (pll, site) = timed(lambda: eng.pseudo_loglik(r, v, return_sites=True), a.reps)

    cols = np.linspace(0, a.V - 1, a.cols).astype(np.int64)
    flipped = v.repeat_interleave(a.cols, 0)                            # row n's flips: the rows cols n .. cols n + cols - 1
    idx = torch.arange(a.rows * a.cols, device=dev)
    ci = torch.from_numpy(cols).to(dev).repeat(a.rows)
    flipped[idx, ci] = 1.0 - flipped[idx, ci]

    def composed():
        F0 = eng.free_energy(r, v).double()
        F1 = eng.free_energy(r, flipped).double().view(a.rows, a.cols)
        return -torch.nn.functional.softplus(F0[:, None] - F1)

    sub_ms, want = timed(composed, max(1, a.reps // 4))
    scaled_ms = sub_ms * a.V / a.cols
    diff = float((site[:, torch.from_numpy(cols).to(dev)].double() - want).abs().max())
    print(json.dumps({"V": a.V, "H": a.H, "rows": a.rows, "fused_ms": round(fused_ms, 4),
                      "composed_subset_ms": round(sub_ms, 4), "subset_cols": a.cols,
                      "composed_scaled_to_V_ms": round(scaled_ms, 2), "scaled": True,
                      "ratio_scaled_composed_over_fused": round(scaled_ms / fused_ms, 1),
                      "max_abs_diff_on_subset": diff, "mean_pll": float(pll.mean())}))


if __name__ == "__main__":
    main()
