#!/usr/bin/env python3
"""Time of the latent top-k search (HipEngine.latent_topk, csrc/kernels_knn.hpp) at user sizes: a bank of N in {4096, 16384}
codes of D = 500 against Q in {1, 256, 13056} queries (13056 = 256 samples x 51 trajectory steps), k = 8 and k = 64, cosine,
with and without the image-key dedup -- against torch matmul + topk on the device (no dedup) and, for a few queries, the
reference's path (CPU scores, full sort, Python dedup walk).  Prints one JSON line; the floor is 2 Q N D FLOP at the fp32
MFMA peak (157 TF).  ``--out PATH`` also writes the JSON to PATH."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multimodal-idbn_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK = 157.3e12


def gpu_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best = []
    for _ in range(3):
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        best.append(ev[0].elapsed_time(ev[1]) / reps)
    return min(best)


def ref_walk_ms(Z, H, q, k):
    """The reference's per-query path (imdbn_logging.py:782-818) on the CPU, ms per query."""
    Zn = torch.nn.functional.normalize(Z, dim=1)
    t0 = time.perf_counter()
    for r in range(q.size(0)):
        s = (torch.nn.functional.normalize(q[r:r + 1], dim=1) @ Zn.T).squeeze(0)
        vals, idx = torch.sort(s, descending=True)
        picked, seen = [], set()
        for i, v in zip(idx.tolist(), vals.tolist()):
            key = (float(H[i, 0].item()), float(H[i, 1].item()))
            if key in seen:
                continue
            seen.add(key)
            picked.append(i)
            if len(picked) >= k:
                break
    return (time.perf_counter() - t0) * 1e3 / q.size(0)


def main():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    eng = E.get_hip_engine()
    dev = torch.device("cuda")
    torch.set_num_threads(16)
    g = torch.Generator(device="cpu").manual_seed(5)
    D = 500
    rows = []
    for N in (4096, 16384):
        bank = torch.rand(N, D, generator=g).to(dev)
        X = (torch.rand(N, 100, generator=g) < 0.3).float().to(dev)
        key = eng.row_stats(X)
        bss = eng.row_stats(bank)[:, 1].contiguous()
        for Q in (1, 256, 13056):
            q = torch.rand(Q, D, generator=g).to(dev)
            reps = 20 if Q < 13056 else 5
            for k in (8, 64):
                r = {"N": N, "D": D, "Q": Q, "k": k, "floor_ms": 2.0 * Q * N * D / PEAK * 1e3}
                r["topk_ms"] = gpu_ms(lambda: eng.latent_topk(bank, q, 0, k, bank_sumsq=bss), reps)
                r["topk_dedup_ms"] = gpu_ms(lambda: eng.latent_topk(bank, q, 0, k, key=key, bank_sumsq=bss), reps)
                bn = torch.nn.functional.normalize(bank, dim=1)
                r["torch_mm_topk_ms"] = gpu_ms(lambda: torch.topk(torch.nn.functional.normalize(q, dim=1) @ bn.T, k, dim=1), reps)
                r["tflops"] = 2.0 * Q * N * D / (r["topk_ms"] * 1e-3) / 1e12
                rows.append(r)
        nq = 4
        rows.append({"N": N, "D": D, "Q": nq, "k": 8, "reference_cpu_ms_per_query": ref_walk_ms(bank.cpu(), key.cpu(), torch.rand(nq, D, generator=g), 8)})
    out = {"what": "latent_topk (cosine; dedup = image-key dedup) vs torch matmul + topk (no dedup) vs the reference's CPU walk",
           "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(out))
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
