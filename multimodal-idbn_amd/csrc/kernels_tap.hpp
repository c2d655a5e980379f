// kernels_tap.hpp -- extended mean-field (TAP) training and log Z (imdbn_rbm_tap_iterate, imdbn_rbm_tap_step).
//
// Magnetisations mv [B][V], mh [B][H] in [0, 1]; cv = mv - mv^2, ch = mh - mh^2; W2 = fl32(W W), made in registers, never in memory.
//     hidden half-step    x = c + mv W - (mh - 1/2) (cv W2),      mh <- damp mh + (1 - damp) sigmoid(x)
//     visible half-step   y = a + mh W^T - (mv - 1/2) (ch W2^T),  mv <- damp mv + (1 - damp) sigmoid(y)
// Order 1 (naive mean field) drops every W2 term.
//
//   tap_half<ORDER2, UP>   grid (output tiles of 64 units, K slices, chunks of 64 batch rows), 256 threads.  A block streams its
//                          K slice of the tile's weights once, TAP_KC reduction steps at a time, through LDS (the visible form
//                          transposes there); the input magnetisations and their cv / ch (formed while staging: two operations
//                          per staged element, against a [B][K] buffer written and read back) sit beside them.  Wave w owns the
//                          batch rows 16 w .. 16 w + 15 of the chunk, a lane one output unit: 16 (order 1) or 32 fp32 accumulators,
//                          fused multiply-adds in k order.  With more than one K slice the partial tiles meet in the workspace and
//                          the block that arrives last (an integer counter, left at zero again) sums them in slice order -- the
//                          same sum whoever is last.  Epilogue, fused: bias, correction, sigmoid, |sigmoid - m_old| as a per-row
//                          maximum per tile, damping, the store of the new magnetisation.  `gamma` epilogue (UP form only): the
//                          final mv, mh are only read, A1 = mv W and A2 = cv W2 come from the same stream, and the hidden part of
//                          the row's free energy leaves per tile, summed over the wave in double.
//   tap_rows_finish        one block per batch row: the row's residual (maximum over the tiles of both half-steps of the last
//                          iteration) and Gamma = visible part (double, fixed tree) + the tile partials in tile order.
//   tap_outer              C = cv^T ch, [V][H] fp32: a thread owns one column and keeps ch of 32 batch rows in registers, cv of
//                          the block's 32 weight rows comes from LDS; batch chunks are added in order.
//   tap_apply<VEC4>        streams dW, C, W, W_m once: gW = (dW - W o C) / n, the momentum / decay rule of rbm.py:212-213.
//
// No floating-point atomics; every sum has an order fixed by (V, H, B) and the CU count.  The row padding of W / W_m (pitch > H)
// and of strided magnetisation rows is neither read nor written.
#pragma once
#include "kernels_ew.hpp"
#include "kernels_rows.hpp"
#include "kernels_centered.hpp"

namespace imdbn {

constexpr int TAP_TN = 64;                       // output units of a tile (one per lane)
constexpr int TAP_BM = 64;                       // batch rows of a chunk (16 per wave)
constexpr int TAP_KC = 32;                       // reduction steps staged at a time
constexpr int TAP_LDW = TAP_TN + 1;              // LDS pitch of the weight tile [k][n]: the transposing stores spread over the banks

struct TapHalfArgs {
    const float* W; int64_t ldw; int K, N;       // K: reduction length (V when UP), N: output units
    const float* m_in; int64_t ld_in;            // [B][K]
    float* m_out; int64_t ld_out;                // [B][N]: the old value is read, the new one written (gamma: read only)
    const float* bias;                           // [N]
    int B; float damp;
    int ks, kchunk, ntiles;                      // K slices of kchunk (a multiple of TAP_KC) steps
    float* slabs;                                // [chunk][slice][tile][2][TAP_BM][TAP_TN] partial tiles (ks > 1)
    int* counters;                               // [chunk][tile], zero at launch, zero again at exit
    float* res_part;                             // [tile][B]: max over the tile's units of |sigmoid - m_old|
    int gamma; double* gam_part;                 // [tile][B]: the hidden part of Gamma over the tile's units
};

__device__ __forceinline__ double tap_entropy(float m) {
    const double p = (double)m, q = 1.0 - (double)m;
    return (p > 0.0 ? p * log(p) : 0.0) + (q > 0.0 ? q * log(q) : 0.0);
}
__device__ __forceinline__ float tap_var(float m) { return m - m * m; }

template <bool ORDER2, bool UP>
__global__ __launch_bounds__(256) void tap_half(const TapHalfArgs a) {
    __shared__ float s_w[TAP_KC * TAP_LDW];
    __shared__ __attribute__((aligned(16))) float s_m[TAP_BM * TAP_KC];
    __shared__ __attribute__((aligned(16))) float s_c[ORDER2 ? TAP_BM * TAP_KC : 4];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tile = blockIdx.x, sl = blockIdx.y, z = blockIdx.z;
    const int n0 = tile * TAP_TN, b0 = z * TAP_BM;
    const int k_begin = sl * a.kchunk, k_end = min(a.K, k_begin + a.kchunk);
    float acc1[16], acc2[ORDER2 ? 16 : 1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[r] = 0.f;
#pragma unroll
    for (int r = 0; r < (ORDER2 ? 16 : 1); ++r) acc2[r] = 0.f;

    // eight weights and eight magnetisations per thread and stage; everything outside W [K][N] and m [B][K] is zero
    float gw[8], gm[8];
    auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int k, n;
            if (UP) { n = tid & 63; k = (tid >> 6) + 4 * i; }
            else    { k = tid & 31; n = (tid >> 5) + 8 * i; }
            const int gk = k0 + k, gn = n0 + n;
            const bool in = gk < k_end && gn < a.N;
            const int64_t off = UP ? (int64_t)gk * a.ldw + gn : (int64_t)gn * a.ldw + gk;
            gw[i] = in ? a.W[off] : 0.f;
            const int mk = tid & 31, mr = (tid >> 5) + 8 * i;
            const bool min_ = k0 + mk < k_end && b0 + mr < a.B;
            gm[i] = min_ ? a.m_in[(int64_t)(b0 + mr) * a.ld_in + k0 + mk] : 0.f;
        }
    };
    auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int k, n;
            if (UP) { n = tid & 63; k = (tid >> 6) + 4 * i; }
            else    { k = tid & 31; n = (tid >> 5) + 8 * i; }
            s_w[k * TAP_LDW + n] = gw[i];
            const int mk = tid & 31, mr = (tid >> 5) + 8 * i;
            s_m[mr * TAP_KC + mk] = gm[i];
            if constexpr (ORDER2) s_c[mr * TAP_KC + mk] = tap_var(gm[i]);
        }
    };
    if (k_begin < k_end) fetch(k_begin);
    for (int k0 = k_begin; k0 < k_end; k0 += TAP_KC) {
        __syncthreads();                         // the previous stage has been read
        stage();
        __syncthreads();
        if (k0 + TAP_KC < k_end) fetch(k0 + TAP_KC);      // in flight under the arithmetic below
#pragma unroll 2
        for (int k4 = 0; k4 < TAP_KC / 4; ++k4) {
            float w1[4], w2[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                w1[e] = s_w[(4 * k4 + e) * TAP_LDW + lane];
                w2[e] = w1[e] * w1[e];           // fl32(W W): rounded once, as the numpy twin states it
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float4 m4 = *reinterpret_cast<const float4*>(&s_m[(16 * w + r) * TAP_KC + 4 * k4]);
                acc1[r] = __builtin_fmaf(m4.x, w1[0], acc1[r]);
                acc1[r] = __builtin_fmaf(m4.y, w1[1], acc1[r]);
                acc1[r] = __builtin_fmaf(m4.z, w1[2], acc1[r]);
                acc1[r] = __builtin_fmaf(m4.w, w1[3], acc1[r]);
                if constexpr (ORDER2) {
                    const float4 c4 = *reinterpret_cast<const float4*>(&s_c[(16 * w + r) * TAP_KC + 4 * k4]);
                    acc2[r] = __builtin_fmaf(c4.x, w2[0], acc2[r]);
                    acc2[r] = __builtin_fmaf(c4.y, w2[1], acc2[r]);
                    acc2[r] = __builtin_fmaf(c4.z, w2[2], acc2[r]);
                    acc2[r] = __builtin_fmaf(c4.w, w2[3], acc2[r]);
                }
            }
        }
    }

    if (a.ks > 1) {
        // publish the partial tile, count the arrival; the block whose add comes last sums all slices in slice order
        typedef __attribute__((address_space(1))) uint32_t gu32;
        constexpr int TILE = TAP_BM * TAP_TN;
        const int64_t zt = (int64_t)z * a.ks * a.ntiles;
        gu32* mine = (gu32*)(a.slabs + ((zt + (int64_t)sl * a.ntiles + tile) * 2) * TILE) + (16 * w) * TAP_TN + lane;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            __hip_atomic_store(mine + r * TAP_TN, __float_as_uint(acc1[r]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if constexpr (ORDER2) __hip_atomic_store(mine + TILE + r * TAP_TN, __float_as_uint(acc2[r]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");      // every storing wave drains before the counter add
        int* cnt = a.counters + z * a.ntiles + tile;
        if (tid == 0) s_last = (__hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.ks - 1) ? 1 : 0;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (!s_last) return;
        if (tid == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // zero again for the next launch
        const gu32* p0 = (const gu32*)(a.slabs + ((zt + tile) * 2) * TILE) + (16 * w) * TAP_TN + lane;
        for (int q = 0; q < a.ks; ++q) {
            const gu32* p = p0 + (int64_t)q * a.ntiles * 2 * TILE;
            float t1[16], t2[ORDER2 ? 16 : 1];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                t1[r] = __uint_as_float(__hip_atomic_load(p + r * TAP_TN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if constexpr (ORDER2) t2[r] = __uint_as_float(__hip_atomic_load(p + TILE + r * TAP_TN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc1[r] = q == 0 ? t1[r] : acc1[r] + t1[r];
                if constexpr (ORDER2) acc2[r] = q == 0 ? t2[r] : acc2[r] + t2[r];
            }
        }
    }

    // ---- epilogue: lane = output unit n, rows 16 w .. 16 w + 15 of the chunk
    const int n = n0 + lane;
    const bool n_ok = n < a.N;
    const float bias = n_ok ? a.bias[n] : 0.f;
    for (int r = 0; r < 16; ++r) {               // wave-uniform bounds
        const int b = b0 + 16 * w + r;
        if (b >= a.B) break;
        const float mo = n_ok ? a.m_out[(int64_t)b * a.ld_out + n] : 0.f;
        if (a.gamma) {
            double t = 0.0;
            if (n_ok) {
                t = tap_entropy(mo) - (double)bias * (double)mo - (double)mo * (double)acc1[r];
                if constexpr (ORDER2) t -= 0.5 * (double)tap_var(mo) * (double)acc2[r];
            }
            t = wave_sum_all(t);
            if (lane == 0) a.gam_part[(int64_t)tile * a.B + b] = t;
            continue;
        }
        float x = bias + acc1[r];
        if constexpr (ORDER2) x = x - (mo - 0.5f) * acc2[r];
        const float s = sigmoidf_ref(x);
        const float res = wave_max_all(n_ok ? fabsf(s - mo) : 0.f);
        if (n_ok) a.m_out[(int64_t)b * a.ld_out + n] = a.damp * mo + (1.0f - a.damp) * s;
        if (lane == 0) a.res_part[(int64_t)tile * a.B + b] = res;
    }
}

struct TapRowsArgs {
    int B, V;
    const float* mv; int64_t ldmv; const float* vis_bias;
    const float* res_up; int nt_up; const float* res_dn; int nt_dn; float* out_res;        // out_res: nullable; nt == 0: no iteration ran
    const double* gam_part; int nt_gam; double* out_gamma;                                  // out_gamma: nullable
};

// grid = B, 256 threads
__global__ __launch_bounds__(256) void tap_rows_finish(const TapRowsArgs a) {
    __shared__ double sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.out_res && tid == 0) {
        float r = 0.f;
        for (int t = 0; t < a.nt_up; ++t) r = fmaxf(r, a.res_up[(int64_t)t * a.B + b]);
        for (int t = 0; t < a.nt_dn; ++t) r = fmaxf(r, a.res_dn[(int64_t)t * a.B + b]);
        a.out_res[b] = r;
    }
    if (!a.out_gamma) return;
    double t = 0.0;
    for (int i = tid; i < a.V; i += 256) {
        const float m = a.mv[(int64_t)b * a.ldmv + i];
        t += tap_entropy(m) - (double)a.vis_bias[i] * (double)m;
    }
    sh[tid] = t;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if (tid < s2) sh[tid] += sh[tid + s2];
        __syncthreads();
    }
    if (tid == 0) {
        double g = sh[0];
        for (int q = 0; q < a.nt_gam; ++q) g += a.gam_part[(int64_t)q * a.B + b];
        a.out_gamma[b] = g;
    }
}

// C[i][j] = sum_b cv[b][i] ch[b][j], pitch H.  grid (ceil(H / 256), ceil(V / 32)), 256 threads
struct TapOuterArgs { const float* mv; int64_t ldmv; const float* mh; int64_t ldmh; int B, V, H; float* C; };

__global__ __launch_bounds__(256) void tap_outer(const TapOuterArgs a) {
    __shared__ float s_cv[32][33];
    const int tid = threadIdx.x, j = blockIdx.x * 256 + tid, i0 = blockIdx.y * 32;
    const int nrows = min(32, a.V - i0);
    for (int c0 = 0; c0 < a.B; c0 += 32) {
        float ch[32];
#pragma unroll
        for (int q = 0; q < 32; ++q) ch[q] = (c0 + q < a.B && j < a.H) ? tap_var(a.mh[(int64_t)(c0 + q) * a.ldmh + j]) : 0.f;
        __syncthreads();
        for (int e = tid; e < 32 * 32; e += 256) {
            const int q = e >> 5, i = e & 31;
            s_cv[q][i] = (c0 + q < a.B && i < nrows) ? tap_var(a.mv[(int64_t)(c0 + q) * a.ldmv + i0 + i]) : 0.f;
        }
        __syncthreads();
        if (j < a.H) {
            for (int i = 0; i < nrows; ++i) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < 32; ++q) s = __builtin_fmaf(s_cv[q][i], ch[q], s);
                float* out = a.C + (int64_t)(i0 + i) * a.H + j;
                *out = c0 == 0 ? s : *out + s;
            }
        }
    }
}

struct TapApplyArgs {
    float* W; float* Wm; int64_t ldw; int V, H;
    const float* dW; const float* C;             // [V][H], pitch H; C: order 2 only (else null)
    float lr, mom, wd, n;
    int rps, tw;                                 // rows per stripe, columns per tile (the grid of centered_apply)
};

template <bool VEC4>
__global__ __launch_bounds__(256) void tap_apply(const TapApplyArgs a) {
    constexpr int E = VEC4 ? 4 : 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col0 = blockIdx.x * a.tw, ncols = min(a.tw, a.H - col0);
    const int row0 = blockIdx.y * a.rps, nrows = min(a.rps, a.V - row0);
    for (int r = w; r < nrows; r += 4) {         // wave-uniform
        const int row = row0 + r;
        const float* dp = a.dW + (int64_t)row * a.H + col0;
        const float* cp = a.C ? a.C + (int64_t)row * a.H + col0 : nullptr;
        float* wp = a.W + (int64_t)row * a.ldw + col0;
        float* mp = a.Wm + (int64_t)row * a.ldw + col0;
        float d[CTR_CS][E], c[CTR_CS][E], w0[CTR_CS][E], m[CTR_CS][E];
#pragma unroll
        for (int s = 0; s < CTR_CS; ++s) {       // the whole row's loads first
            const int j = (s * 64 + lane) * E;
            if (j < ncols) {                     // (VEC4: ncols is a multiple of 4, a float4 is inside or outside as a whole)
                if constexpr (VEC4) {
                    const float4 x = *reinterpret_cast<const float4*>(dp + j);
                    const float4 u = cp ? *reinterpret_cast<const float4*>(cp + j) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 y = *reinterpret_cast<const float4*>(wp + j);
                    const float4 q = *reinterpret_cast<const float4*>(mp + j);
                    d[s][0] = x.x; d[s][1] = x.y; d[s][2] = x.z; d[s][3] = x.w;
                    c[s][0] = u.x; c[s][1] = u.y; c[s][2] = u.z; c[s][3] = u.w;
                    w0[s][0] = y.x; w0[s][1] = y.y; w0[s][2] = y.z; w0[s][3] = y.w;
                    m[s][0] = q.x; m[s][1] = q.y; m[s][2] = q.z; m[s][3] = q.w;
                } else {
                    d[s][0] = dp[j]; c[s][0] = cp ? cp[j] : 0.f; w0[s][0] = wp[j]; m[s][0] = mp[j];
                }
            }
        }
#pragma unroll
        for (int s = 0; s < CTR_CS; ++s) {
            const int j = (s * 64 + lane) * E;
            if (j < ncols) {
                float wn[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float g = (cp ? d[s][e] - w0[s][e] * c[s][e] : d[s][e]) / a.n;
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
    }
}

}  // namespace imdbn
