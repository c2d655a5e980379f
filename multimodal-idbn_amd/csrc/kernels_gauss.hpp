// kernels_gauss.hpp -- Gaussian visible units with learned variances (imdbn_rbm_gauss_*).
//
// Cho, Ilin & Raiko 2011: with the log-variance z (sigma_i^2 = e^{z_i}) and u = v e^{-z},
//     p(h | v) = sigmoid(c + u W),      p(v | h) = N(b + h W^T, sigma^2),      F(v) = sum (v - b)^2 / (2 sigma^2) - sum softplus(c + u W)
// so the hidden side of every call is the Bernoulli engine applied to u, and the mean of the visible side is its logits path.  What is
// new sits around those: the visible epilogue, and the update with the variance gradient.  With n batch rows, S = u0^T P0 - u1^T P1
// (the statistics pass of the update kernel), q0_i = sum_b (data_bi - b_i)^2, q1_i = sum_b (v_bi - b_i)^2 and r_i = sum_j W_ij S_ij:
//     gW = S / n,   gb = colsum(u0 - u1) / n,   gc = colsum(P0 - P1) / n,   gz_i = e^{-z_i} (q0_i - q1_i) / (2 n) - r_i / n
//
//   gauss_rows          grid (ceil(V / 256), ceil(B / 8)), 256 threads: a thread owns one column of 8 batch rows of a [B][V] tensor
//                       of means (or of data): v = mean (+ e^{z/2} n with `sample`), u = v e^{-z}; writes v and u where asked, the
//                       8-row partials of sum u and sum (v - b)^2 into [P][V], and the block's sum of (ref - mean)^2.
//   gauss_apply<VEC4>   grid (column tiles, row stripes), 256 threads, the tiling of centered_apply: every wave takes the rows w, w + 4, ...
//                       of the stripe, streams S, W and W_m of the row once, does the momentum / decay update, writes W and W_m once
//                       and sums W_ij S_ij of the W it has just read over its lanes (shuffles) into row_part[tile][row].
//   gauss_finish        one small launch: sums all partials in index order, updates the three bias vectors and logvar (clamped),
//                       reduces the loss partials.
//   gauss_free_energy_rows   one block per batch row: the quadratic term and the softplus sum, fixed-order tree.
//
// No floating-point atomics; every sum has an order fixed by (V, H, B) and the grid, which depends on (V, H) and the CU count only.
// The row padding of W / W_m (pitch > H) is neither read nor written.
#pragma once
#include "kernels_centered.hpp"

namespace imdbn {

constexpr int GAUSS_RPT = 8;                     // batch rows of a gauss_rows thread

struct GaussRowsArgs {
    const float* in; int64_t ldi;                // means, or data: [B][V]
    const float* ref; int64_t ldr;               // nullable: the data the loss compares the means with
    const float* bias; const float* logvar; int B, V;
    int sample; DrawSrc nz;                      // v = in + e^{z/2} n
    float* out_v; int64_t ldv;                   // nullable
    float* out_u; int64_t ldu;                   // nullable
    float* su_part; float* q_part;               // nullable: [ceil(B / 8)][V]
    float* loss_part;                            // nullable: [gridDim.y][gridDim.x]
};

__global__ __launch_bounds__(256) void gauss_rows(const GaussRowsArgs a) {
    __shared__ float sh[256];
    const int tid = threadIdx.x, col = blockIdx.x * 256 + tid, b0 = blockIdx.y * GAUSS_RPT;
    const bool cok = col < a.V;
    const int cc = min(col, a.V - 1);
    const float z = a.logvar[cc], bias = a.bias[cc];
    const float sd = expf(0.5f * z), iv = expf(-z);
    float m[GAUSS_RPT], ref[GAUSS_RPT], nz[GAUSS_RPT];
#pragma unroll
    for (int i = 0; i < GAUSS_RPT; ++i) {        // all loads first, from clamped addresses
        const int bc = min(b0 + i, a.B - 1);
        m[i] = a.in[(int64_t)bc * a.ldi + cc];
        ref[i] = a.ref ? a.ref[(int64_t)bc * a.ldr + cc] : m[i];
        nz[i] = 0.f;
    }
    if (a.sample) {
#pragma unroll
        for (int j = 0; j < GAUSS_RPT / 2; ++j) {
            float t[2];
            draw_normal_rows2(a.nz, b0 + 2 * j, a.B - 1, cc, t);
            nz[2 * j] = t[0]; nz[2 * j + 1] = t[1];
        }
    }
    float su = 0.f, q = 0.f, ls = 0.f;
#pragma unroll
    for (int i = 0; i < GAUSS_RPT; ++i) {
        const int b = b0 + i;
        if (!cok || b >= a.B) continue;
        const float v = a.sample ? m[i] + sd * nz[i] : m[i];
        const float u = v * iv;
        if (a.out_v) a.out_v[(int64_t)b * a.ldv + col] = v;
        if (a.out_u) a.out_u[(int64_t)b * a.ldu + col] = u;
        su += u;
        const float dq = v - bias;
        q += dq * dq;
        const float dl = ref[i] - m[i];
        ls += dl * dl;
    }
    if (cok && a.su_part) a.su_part[(int64_t)blockIdx.y * a.V + col] = su;
    if (cok && a.q_part) a.q_part[(int64_t)blockIdx.y * a.V + col] = q;
    if (a.loss_part) {                           // block-uniform
        sh[tid] = ls;
        __syncthreads();
        for (int s2 = 128; s2 > 0; s2 >>= 1) {
            if (tid < s2) sh[tid] += sh[tid + s2];
            __syncthreads();
        }
        if (tid == 0) a.loss_part[blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
    }
}

struct GaussArgs {
    float* W; float* Wm; int64_t ldw; int V, H;
    const float* S;                              // [V][H], pitch H: un-normalised statistics
    float lr, mom, wd, n;
    int rps, tw, nstripes, ctiles;               // rows per stripe, columns per tile, grid
    float* row_part;                             // [ctiles][V]: sum over the tile's columns of W_ij S_ij
    const float* hpos; const float* hneg; int P; // column-sum partials [P][H] of P0 / P1
    const float* su0; const float* su1; const float* q0; const float* q1; int RP;      // gauss_rows partials [RP][V]
    float* hid_bias; float* hb_m; float* vis_bias; float* vb_m; float* logvar; float* logvar_m;
    float lr_z, z_lo, z_hi;
    int sparsity; float target;
    const float* loss_part; int n_loss; float loss_den; float* loss_out;
};

template <bool VEC4>
__global__ __launch_bounds__(256) void gauss_apply(const GaussArgs a) {
    constexpr int E = VEC4 ? 4 : 1;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col0 = blockIdx.x * a.tw, ncols = min(a.tw, a.H - col0);
    const int row0 = blockIdx.y * a.rps, nrows = min(a.rps, a.V - row0);
    for (int r = w; r < nrows; r += 4) {         // wave-uniform
        const int row = row0 + r;
        const float* dp = a.S + (int64_t)row * a.H + col0;
        float* wp = a.W + (int64_t)row * a.ldw + col0;
        float* mp = a.Wm + (int64_t)row * a.ldw + col0;
        float d[CTR_CS][E], w0[CTR_CS][E], m[CTR_CS][E];
#pragma unroll
        for (int s = 0; s < CTR_CS; ++s) {       // the whole row's loads first
            const int j = (s * 64 + lane) * E;   // (VEC4: ncols is a multiple of 4, a float4 is inside or outside as a whole)
            if (j < ncols) {
                if constexpr (VEC4) {
                    const float4 x = *reinterpret_cast<const float4*>(dp + j);
                    const float4 y = *reinterpret_cast<const float4*>(wp + j);
                    const float4 z = *reinterpret_cast<const float4*>(mp + j);
                    d[s][0] = x.x; d[s][1] = x.y; d[s][2] = x.z; d[s][3] = x.w;
                    w0[s][0] = y.x; w0[s][1] = y.y; w0[s][2] = y.z; w0[s][3] = y.w;
                    m[s][0] = z.x; m[s][1] = z.y; m[s][2] = z.z; m[s][3] = z.w;
                } else {
                    d[s][0] = dp[j]; w0[s][0] = wp[j]; m[s][0] = mp[j];
                }
            }
        }
        float dot = 0.f;
#pragma unroll
        for (int s = 0; s < CTR_CS; ++s) {
            const int j = (s * 64 + lane) * E;
            if (j < ncols) {
                float wn[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    dot += w0[s][e] * d[s][e];
                    const float g = d[s][e] / a.n;
                    float t = m[s][e] * a.mom;
                    t = t + a.lr * (g - a.wd * w0[s][e]);
                    m[s][e] = t;
                    wn[e] = w0[s][e] + t;
                }
                if constexpr (VEC4) {
                    *reinterpret_cast<float4*>(mp + j) = make_float4(m[s][0], m[s][1], m[s][2], m[s][3]);
                    *reinterpret_cast<float4*>(wp + j) = make_float4(wn[0], wn[1], wn[2], wn[3]);
                } else {
                    mp[j] = m[s][0]; wp[j] = wn[0];
                }
            }
        }
        dot = wave_sum_all(dot);
        if (lane == 0) a.row_part[(int64_t)blockIdx.x * a.V + row] = dot;
    }
}

// grid = ceil(max(V, H) / 256) + 1: the last block reduces the loss partials, the others take one hidden and one visible unit per thread
__global__ __launch_bounds__(256) void gauss_finish(const GaussArgs a) {
    __shared__ double sh[256];
    if (blockIdx.x == gridDim.x - 1) {
        if (a.loss_out) {
            const double t = loss_total_256(a.loss_part, a.n_loss, sh);
            if (threadIdx.x == 0) a.loss_out[0] = (float)(t / (double)a.loss_den);
        }
        return;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.H) {
        const float sp = sum_parts(a.hpos, a.P, a.H, i), sn = sum_parts(a.hneg, a.P, a.H, i);
        float m = a.hb_m[i] * a.mom;
        m = m + (a.lr * (sp - sn)) / a.n;
        if (a.sparsity) m = m + (-a.lr) * (sp / a.n - a.target);
        a.hb_m[i] = m;
        a.hid_bias[i] += m;
    }
    if (i < a.V) {
        const float sp = sum_parts(a.su0, a.RP, a.V, i), sn = sum_parts(a.su1, a.RP, a.V, i);
        float m = a.vb_m[i] * a.mom;
        m = m + (a.lr * (sp - sn)) / a.n;
        a.vb_m[i] = m;
        a.vis_bias[i] += m;
        if (a.lr_z != 0.0f) {
            const float q0 = sum_parts(a.q0, a.RP, a.V, i), q1 = sum_parts(a.q1, a.RP, a.V, i);
            const float r = ctr_sum_parts(a.row_part, a.ctiles, a.V, i);
            const float z = a.logvar[i];
            const float gz = (expf(-z) * (q0 - q1)) / (2.0f * a.n) - r / a.n;
            float mz = a.logvar_m[i] * a.mom;
            mz = mz + a.lr_z * gz;
            a.logvar_m[i] = mz;
            a.logvar[i] = fminf(fmaxf(z + mz, a.z_lo), a.z_hi);
        }
    }
}

// F(v) = sum_i (v_i - b_i)^2 / (2 sigma_i^2) - sum_j softplus(x_j), x = c + u W from the K1 path (logits_only), softplus as
// free_energy_rows; one block per batch row, fixed-order tree sums
__global__ __launch_bounds__(256) void gauss_free_energy_rows(const float* __restrict__ v, int64_t ldv, const float* __restrict__ vis_bias,
                                                              const float* __restrict__ logvar, int V, const float* __restrict__ x,
                                                              int64_t ldx, int H, float* __restrict__ out) {
    __shared__ float sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    float acc = 0.f;
    for (int i = tid; i < V; i += 256) {
        const float dv = v[(int64_t)b * ldv + i] - vis_bias[i];
        acc += 0.5f * (dv * dv) * expf(-logvar[i]);
    }
    for (int j = tid; j < H; j += 256) {
        const float t = x[(int64_t)b * ldx + j];
        acc -= t > 20.0f ? t : log1pf(expf(t));
    }
    sh[tid] = acc;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if (tid < s2) sh[tid] += sh[tid + s2];
        __syncthreads();
    }
    if (tid == 0) out[b] = sh[0];
}

}  // namespace imdbn
