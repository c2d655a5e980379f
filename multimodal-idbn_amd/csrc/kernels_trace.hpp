// Convergence tracing of conditional chains (imdbn/utils/conditional_steps.py).
//
// A traced chain (imdbn_rbm_chain_traced) records, per step, the visible probabilities of a column window.  The kernels here
// turn such a trace into the per-step curves and the per-row convergence decision of the reference's B = 1 Python loops
// (reference conditional_steps.py:40-130 IMG->TXT, :133-241 TXT->IMG), for a whole batch, without a host round trip:
//   * trace_label_scan   -- IMG->TXT: top-2 of the label probabilities, p(gt), L1 change, argmax streak, stop rule;
//   * trace_code_scan    -- TXT->IMG, first half: EMA of the code (z_new) and its L2 change dz;
//   * trace_patience_scan-- TXT->IMG, second half: best-MSE tracker with a no-improvement counter;
//   * row_sqerr          -- mean squared error of decoded rows against reference rows (fixed-order, no atomics).
// The scans are sequential over steps per row: one wave per row (lanes over the columns), one thread per row for the
// patience rule (two scalars per step).  Decisions compare in double, as the reference does with Python floats.
#pragma once
#include "kernels_rows.hpp"

namespace imdbn {

__global__ __launch_bounds__(64 * ROW_WAVES) void trace_label_scan(const float* __restrict__ tr, int64_t ss, int64_t ld, int T, int B,
                                                                  int K, const int32_t* __restrict__ gt, double eps_l1, int stable_steps,
                                                                  double gap_thresh, float* __restrict__ p1o, float* __restrict__ p2o,
                                                                  int32_t* __restrict__ k1o, int32_t* __restrict__ k2o,
                                                                  float* __restrict__ pgo, float* __restrict__ l1o,
                                                                  int32_t* __restrict__ steps_o, int32_t* __restrict__ pred_o) {
    const int l = wave_lane(), b = wave_row();
    if (b >= B) return;                                                    // wave-uniform
    const int g = gt ? gt[b] : -1;
    // slot 0 = baseline p(v | p(h | v0)): its argmax starts the streak, its values are y_prev of step 1
    float prev[4], y[4];
    slots_load(prev, tr + (int64_t)b * ld, l, K);
    int pred = slots_argmax(prev, l, K), streak = 0, conv = T + 1;
    for (int t = 1; t <= T; ++t) {
        slots_load(y, tr + (int64_t)t * ss + (int64_t)b * ld, l, K);
        float l1 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            l1 += fabsf(y[q] - prev[q]);                                   // slots past K hold 0 on both sides
            prev[q] = y[q];
        }
        l1 = wave_sum_all(l1);
        const Top2 ty = slots_top2(y, l, K);
        const float v1 = ty.v1, v2 = ty.v2;
        const int i1 = ty.i1, i2 = ty.i2;
        const float pg = g >= 0 && g < K ? slots_pick(y, g) : 0.f;         // wave-uniform: every lane shuffles
        if (l == 0) {
            const int64_t o = (int64_t)b * T + (t - 1);
            p1o[o] = v1; p2o[o] = v2; k1o[o] = i1; k2o[o] = i2; l1o[o] = l1;
            if (pgo) pgo[o] = pg;
        }
        streak = (i1 == pred) ? streak + 1 : 1;
        pred = i1;
        if (conv > T && (double)l1 < eps_l1 && streak >= stable_steps && (double)v1 - (double)v2 >= gap_thresh) {
            conv = t;
            if (l == 0) pred_o[b] = pred;                                  // predT: the argmax at the stopping step
        }
    }
    if (l == 0) {
        steps_o[b] = conv;
        if (conv > T) pred_o[b] = pred;
    }
}

// z trace [T][B] rows of Dz (slot t at tr + t*ss + b*ld) -> z_new [T][B][Dz] (EMA when beta > 0), dz [B][T] = ||z_new_t - z_new_{t-1}||_2
__global__ __launch_bounds__(64 * ROW_WAVES) void trace_code_scan(const float* __restrict__ tr, int64_t ss, int64_t ld, int T, int B,
                                                                 int Dz, const float* __restrict__ z0, int64_t ldz0, float beta,
                                                                 float* __restrict__ zn, float* __restrict__ dzo) {
    const int l = wave_lane(), b = wave_row();
    if (b >= B) return;
    const float* zp = z0 + (int64_t)b * ldz0;
    for (int t = 0; t < T; ++t) {
        const float* zs = tr + (int64_t)t * ss + (int64_t)b * ld;
        float* zo = zn + ((int64_t)t * B + b) * Dz;
        float acc = 0.f;
        for (int c = l; c < Dz; c += 64) {                                // each lane re-reads only what it wrote itself
            const float p = zp[c];
            const float z = beta > 0.f ? (1.0f - beta) * p + beta * zs[c] : zs[c];
            const float d = z - p;
            acc += d * d;
            zo[c] = z;
        }
        acc = wave_sum_all(acc);
        if (l == 0) dzo[(int64_t)b * T + t] = sqrtf(acc);
        zp = zo;
    }
}

// reference conditional_steps.py:217-234, literally (best_mse starts at +inf; the +1e-12 included)
__global__ __launch_bounds__(64) void trace_patience_scan(const float* __restrict__ dz, const float* __restrict__ mse, int T, int B,
                                                          double eps_z, double mse_tol, int patience,
                                                          int32_t* __restrict__ steps_o, float* __restrict__ best_o) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double best = INFINITY;
    int no_improve = 0, conv = T + 1;
    for (int t = 1; t <= T; ++t) {
        const double m = (double)mse[(int64_t)b * T + t - 1];
        if ((double)dz[(int64_t)b * T + t - 1] < eps_z) {
            if (m + 1e-12 < best - mse_tol) { best = m; no_improve = 0; }
            else ++no_improve;
            if (no_improve >= patience) { conv = t; break; }
        } else {
            if (m + 1e-12 < best - mse_tol) best = m;
            no_improve = 0;
        }
    }
    steps_o[b] = conv;
    best_o[b] = (float)best;
}

// out[i] = mean_c (x[i][c] - ref[ref_row[i]][c])^2: one block per row, a fixed column subset per thread, a fixed-order tree
__global__ __launch_bounds__(256) void row_sqerr(const float* __restrict__ x, int64_t ldx, int B, int N, const float* __restrict__ ref,
                                                 int64_t ldr, const int32_t* __restrict__ ref_row, float* __restrict__ out) {
    __shared__ float red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i >= B) return;                                                    // block-uniform
    const float* xr = x + (int64_t)i * ldx;
    const float* rr = ref + (int64_t)(ref_row ? ref_row[i] : i) * ldr;
    float s = 0.f;
    for (int c = tid; c < N; c += 256) { const float d = xr[c] - rr[c]; s += d * d; }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[i] = red[0] / (float)N;
}

// dst[b][c - c0] = src[b][c], c in [c0, c1)  (the per-launch chain's trace: the window of its fp32 v_prob)
__global__ __launch_bounds__(256) void trace_copy(const float* __restrict__ src, int64_t lds, int B, int c0, int c1,
                                                  float* __restrict__ dst, int64_t ldd) {
    const int w = c1 - c0;
    const int64_t n = (int64_t)B * w;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
        const int b = (int)(k / w), c = (int)(k - (int64_t)b * w);
        dst[(int64_t)b * ldd + c] = src[(int64_t)b * lds + c0 + c];
    }
}

}  // namespace imdbn
