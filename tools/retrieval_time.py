"""Time the pairwise free-energy sweep against a chunked PyTorch computation of the same ranks and against the bare softplus loop
(DESIGN §28).

At Q = N = 4096, D1 = D2 = 512 and each H of --H (default 256, 1024):
  engine    HipEngine.pair_scores(gt_q = gt_n = arange): both propagations and the five kernels of imdbn_rbm_pair_scores, HIP events
            around `reps` calls after a warm-up (mean and minimum of per-call times);
  torch     the same two rank vectors in PyTorch: a and b by two GEMMs, then per chunk of `--chunk` queries the [chunk, N, H] temporary,
            softplus, the sum over H and the comparisons (hundreds of launches); HIP events likewise;
  ceiling   a kernel of this tool (compiled before the GPU is initialised): 16 accumulators per thread, the sweep's own pair_term on
            operands that stay in registers, no LDS and no memory traffic -- the rate at which this part issues the softplus body.
Prints one JSON line per H: the three times, the engine's pair terms per second and its share of the ceiling.  Not a test, no threshold."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "multimodal-idbn_amd")

CEILING_SRC = r'''
#include <hip/hip_runtime.h>
#include "kernels_pair.hpp"
using namespace imdbn;
// every thread: 4 x 4 pairs, `iters` hidden units; the operands drift by an exact step so nothing hoists out of the loop
__global__ __launch_bounds__(256) void pair_ceiling(float* out, int iters, float step) {
    float av[4], bv[4];
    for (int i = 0; i < 4; ++i) { av[i] = 0.01f * (threadIdx.x & 15) + i - 2.f; bv[i] = 0.02f * (threadIdx.x >> 4) - i; }
    double acc[4][4];
    for (int i = 0; i < 4; ++i) for (int m = 0; m < 4; ++m) acc[i][m] = 0.0;
    for (int j = 0; j < iters; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int m = 0; m < 4; ++m) pair_term(acc[i][m], av[i], bv[m]);
#pragma unroll
        for (int i = 0; i < 4; ++i) { av[i] += step; bv[i] -= step; }
    }
    double s = 0.0;
    for (int i = 0; i < 4; ++i) for (int m = 0; m < 4; ++m) s += acc[i][m];
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = (float)s;
}
extern "C" int pair_ceiling_run(float* out, int blocks, int iters, void* stream) {
    hipLaunchKernelGGL(pair_ceiling, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, iters, 1e-3f);
    return (int)hipGetLastError();
}
'''


def build_ceiling():
    """Compile the ceiling kernel next to the engine library (before this process touches the GPU); reuse an up-to-date one."""
    out = os.path.join(PKG, "lib", "libpair_ceiling.so")
    src = os.path.join(PKG, "lib", "pair_ceiling.hip")
    hdr = os.path.join(PKG, "csrc", "kernels_pair.hpp")
    if os.path.exists(out) and os.path.exists(src) and open(src).read() == CEILING_SRC and os.path.getmtime(out) >= os.path.getmtime(hdr):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(src, "w") as f:
        f.write(CEILING_SRC)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-shared", "-fPIC", "-I", os.path.join(PKG, "csrc"), src, "-o", out])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=4096)
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--D", type=int, default=512)
    ap.add_argument("--H", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()

    ceiling_lib = build_ceiling()
    import __graft_entry__ as ge
    ge.build()
    if a.build_only:
        return
    import numpy as np
    import torch
    from imdbn import engine as E
    from imdbn.models import RBM

    dev = "cuda:0"
    eng = E.get_hip_engine()
    lib = C.CDLL(ceiling_lib)
    lib.pair_ceiling_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]

    def timed(fn, reps):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        return float(np.mean(ms)), float(np.min(ms)), out

    # the ceiling: 8 blocks per CU, 4096 hidden units per pair
    cus = eng.device_info()[0]
    blocks, iters = 8 * int(cus), 4096
    sink = torch.empty(blocks * 256, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    c_mean, c_min, _ = timed(lambda: lib.pair_ceiling_run(sink.data_ptr(), blocks, iters, stream), a.reps)
    ceiling_rate = blocks * 256 * 16 * iters / (c_min * 1e-3)

    g = np.random.Generator(np.random.PCG64(1))
    for H in a.H:
        V = 2 * a.D
        r = RBM(V, H, 0.1, 0.0, 0.5).to(dev)
        r.W.data.copy_(torch.from_numpy((4 * g.standard_normal((V, H)) / np.sqrt(V)).astype(np.float32)))
        r.vis_bias.data.copy_(torch.from_numpy((0.1 * g.standard_normal(V)).astype(np.float32)))
        r.hid_bias.data.copy_(torch.from_numpy((0.1 * g.standard_normal(H)).astype(np.float32)))
        z1 = torch.from_numpy(g.random((a.Q, a.D)).astype(np.float32)).to(dev)
        z2 = torch.from_numpy(g.random((a.N, a.D)).astype(np.float32)).to(dev)
        gt = torch.arange(a.Q, dtype=torch.int32, device=dev)
        gtn = torch.arange(a.N, dtype=torch.int32, device=dev) % a.Q

        e_mean, e_min, o = timed(lambda: eng.pair_scores(r, z1, z2, gt_q=gt % a.N, gt_n=gtn), a.reps)

        def baseline():
            W, b = r.W.data, r.vis_bias.data
            A = r.hid_bias.data + z1 @ W[:a.D]
            B = z2 @ W[a.D:]
            sa, sb = z1 @ b[:a.D], z2 @ b[a.D:]
            gq, gn = (gt % a.N).long(), gtn.long()
            sp = torch.nn.functional.softplus
            ref_q = sa + sb[gq] + sp(A + B[gq]).sum(1)
            ref_n = sa[gn] + sb + sp(A[gn] + B).sum(1)
            rank_q = torch.empty(a.Q, dtype=torch.int64, device=dev)
            rank_n = torch.zeros(a.N, dtype=torch.int64, device=dev)
            cols = torch.arange(a.N, device=dev)
            for q0 in range(0, a.Q, a.chunk):
                q1 = min(a.Q, q0 + a.chunk)
                S = sa[q0:q1, None] + sb[None, :] + sp(A[q0:q1, None, :] + B[None, :, :]).sum(2)
                rq = ref_q[q0:q1, None]
                rank_q[q0:q1] = ((S > rq) | ((S == rq) & (cols[None, :] < gq[q0:q1, None]))).sum(1)
                rows = torch.arange(q0, q1, device=dev)
                rank_n += ((S > ref_n[None, :]) | ((S == ref_n[None, :]) & (rows[:, None] < gn[None, :]))).sum(0)
            return rank_q, rank_n

        t_mean, t_min, (bq, bn) = timed(baseline, max(2, a.reps // 3))
        agree_q = float((bq == o["rank_q"].long()).double().mean())
        agree_n = float((bn == o["rank_n"].long()).double().mean())
        rate = a.Q * a.N * H / (e_min * 1e-3)
        print(json.dumps({"Q": a.Q, "N": a.N, "D1": a.D, "D2": a.D, "H": H, "engine_ms_mean": round(e_mean, 3), "engine_ms_min": round(e_min, 3),
                          "torch_chunked_ms_mean": round(t_mean, 2), "torch_chunked_ms_min": round(t_min, 2), "torch_chunk_rows": a.chunk,
                          "torch_over_engine": round(t_min / e_min, 1), "engine_pair_terms_per_s": rate,
                          "ceiling_pair_terms_per_s": ceiling_rate, "ceiling_ms_min": round(c_min, 3),
                          "engine_share_of_ceiling": round(rate / ceiling_rate, 3),
                          "ranks_equal_to_torch_q": agree_q, "ranks_equal_to_torch_n": agree_n, "reps": a.reps, "warmup": a.warmup}))


if __name__ == "__main__":
    main()
