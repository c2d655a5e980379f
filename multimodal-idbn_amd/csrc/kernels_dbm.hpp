// kernels_dbm.hpp -- the two-sided layer half-step of a deep Boltzmann machine (imdbn_dbm_layer).
//
// A layer in the middle of the stack hears from below and from above in one pre-activation:
//     pre[b][n] = s_lo sum_k x_lo[b][k] W_lo[k][n] + s_hi sum_j x_hi[b][j] W_hi[n][j] + bias[n]
// W_lo [K_lo][ldw_lo] is the lower RBM's W (the layer is its columns), W_hi [N][ldw_hi] the upper RBM's W (the layer is its rows).
//
//   dbm_layer<SAMPLE>      grid (output tiles of 64 units, K slices, chunks of 64 batch rows), 256 threads: the block shape of
//                          tap_half (kernels_tap.hpp), run over the concatenated reduction axis [0, K_lo) ++ [0, K_hi).  A block
//                          owns the slice [g0, g1) of that axis; it streams the lo part of the slice (units are columns), then the
//                          hi part (units are rows, transposed through LDS), DBM_KC steps at a time.  Wave w owns the batch rows
//                          16 w .. 16 w + 15 of the chunk, a lane one output unit.
//   dbm_pre_tile           everything of that kernel up to its epilogue, as one device function: dbm_rowsum_layer
//                          (kernels_dbm_ais.hpp) runs the same block, split and summation order under another epilogue.
//   dbm_rows_finish        one thread per batch row: the row's residual, the maximum over the tiles.
//
// Arithmetic: fp32 vector FMAs (not the bf16x3 MFMA split), one fused multiply-add per product.  Summation order of one output:
//     slice q:  lo_q = fma chain over the slice's k in [0, K_lo), ascending, from 0;  hi_q likewise over its j in [0, K_hi);
//               t_q = fl(fl(s_lo lo_q) + fl(s_hi hi_q))          -- the scales meet the finished side sums, never a product
//     pre = fl(fl(t_0 + t_1 + ... + t_{ks-1}) + bias)            -- slices in slice order, by the block that arrives last
// At most one slice holds both sides (the seam); every other t_q is one scaled side sum.  The last arriver is found with an integer
// counter that is left at zero; no floating-point atomics: the same call gives the same bits, whoever is last.
// Epilogue, fused: p = sigmoid(pre), then
//     mean field   |p - m_old| as a per-row maximum per tile, m = damp m_old + (1 - damp) p in place;
//     sample       s = 1[p > U], U the call's one ("u", N) draw (Philox keyed on the global row, or the replay tape), p optional.
// Everything outside W_lo [K_lo][N], W_hi [N][K_hi], x [B][K] and the outputs' [B][N] is neither read nor written.
#pragma once
#include "kernels_ew.hpp"
#include "kernels_rows.hpp"

namespace imdbn {

constexpr int DBM_TN = 64;                       // output units of a tile (one per lane)
constexpr int DBM_BM = 64;                       // batch rows of a chunk (16 per wave)
constexpr int DBM_KC = 32;                       // reduction steps staged at a time
constexpr int DBM_LDW = DBM_TN + 1;              // LDS pitch of the weight tile [k][n]: the transposing stores spread over the banks

struct DbmLayerArgs {
    const float* W_lo; int64_t ldw_lo; int K_lo; const float* x_lo; int64_t ldx_lo; float s_lo;
    const float* W_hi; int64_t ldw_hi; int K_hi; const float* x_hi; int64_t ldx_hi; float s_hi;
    const float* bias; int N, B;
    float* m; int64_t ldm; float damp;           // mean field: read and written in place
    float* res_part;                             // [tile][B]: max over the tile's units of |p - m_old| (mean field)
    DrawSrc uni; float* s; int64_t lds; float* p; int64_t ldp;      // sample: s written, p too when non-null
    int ks, kchunk, ntiles;                      // K slices of kchunk (a multiple of DBM_KC) steps of the concatenated axis
    float* slabs;                                // [chunk][slice][tile][DBM_BM][DBM_TN] partial tiles (ks > 1)
    int* counters;                               // [chunk][tile], zero at launch, zero again at exit
};

// acc += x[.][k_begin, k_end) W: UP reads W [k][n] (pitch ldw), !UP reads W [n][k] and transposes it on the way into LDS
template <bool UP>
__device__ __forceinline__ void dbm_side(float (&acc)[16], float* s_w, float* s_x, const float* W, int64_t ldw, const float* x, int64_t ldx,
                                         int k_begin, int k_end, int n0, int N, int b0, int B) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // eight weights and eight inputs per thread and stage; everything outside W and x is zero
    float gw[8], gx[8];
    auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int k, n;
            if (UP) { n = tid & 63; k = (tid >> 6) + 4 * i; }
            else    { k = tid & 31; n = (tid >> 5) + 8 * i; }
            const int gk = k0 + k, gn = n0 + n;
            const bool in = gk < k_end && gn < N;
            const int64_t off = UP ? (int64_t)gk * ldw + gn : (int64_t)gn * ldw + gk;
            gw[i] = in ? W[off] : 0.f;
            const int xk = tid & 31, xr = (tid >> 5) + 8 * i;
            const bool xin = k0 + xk < k_end && b0 + xr < B;
            gx[i] = xin ? x[(int64_t)(b0 + xr) * ldx + k0 + xk] : 0.f;
        }
    };
    if (k_begin < k_end) fetch(k_begin);
    for (int k0 = k_begin; k0 < k_end; k0 += DBM_KC) {
        __syncthreads();                         // the previous stage (of either side) has been read
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int k, n;
            if (UP) { n = tid & 63; k = (tid >> 6) + 4 * i; }
            else    { k = tid & 31; n = (tid >> 5) + 8 * i; }
            s_w[k * DBM_LDW + n] = gw[i];
            s_x[((tid >> 5) + 8 * i) * DBM_KC + (tid & 31)] = gx[i];
        }
        __syncthreads();
        if (k0 + DBM_KC < k_end) fetch(k0 + DBM_KC);      // in flight under the arithmetic below
#pragma unroll 2
        for (int k4 = 0; k4 < DBM_KC / 4; ++k4) {
            float w1[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) w1[e] = s_w[(4 * k4 + e) * DBM_LDW + lane];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float4 x4 = *reinterpret_cast<const float4*>(&s_x[(16 * w + r) * DBM_KC + 4 * k4]);
                acc[r] = __builtin_fmaf(x4.x, w1[0], acc[r]);
                acc[r] = __builtin_fmaf(x4.y, w1[1], acc[r]);
                acc[r] = __builtin_fmaf(x4.z, w1[2], acc[r]);
                acc[r] = __builtin_fmaf(x4.w, w1[3], acc[r]);
            }
        }
    }
}

// The pre-activation sums of the block's tile, without the bias: acc[r] = sum over the slices of t_q (header) for the unit n0 + lane and
// the rows b0 + 16 w + r.  `A` carries the operand and split-K fields of DbmLayerArgs under the same names.  False: another block is
// the last arriver of this tile and this one is done (ks > 1); every thread of the block gets the same answer.
template <class A>
__device__ __forceinline__ bool dbm_pre_tile(const A& a, float (&acc)[16], float* s_w, float* s_x, int* s_last) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tile = blockIdx.x, sl = blockIdx.y, z = blockIdx.z;
    const int n0 = tile * DBM_TN, b0 = z * DBM_BM;
    // the slice [g0, g1) of the concatenated axis, cut at the seam
    const int K = a.K_lo + a.K_hi;
    const int g0 = min(K, sl * a.kchunk), g1 = min(K, g0 + a.kchunk);
    const int lo_b = min(g0, a.K_lo), lo_e = min(g1, a.K_lo);
    const int hi_b = max(g0, a.K_lo) - a.K_lo, hi_e = max(g1, a.K_lo) - a.K_lo;

    float t[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    dbm_side<true>(acc, s_w, s_x, a.W_lo, a.ldw_lo, a.x_lo, a.ldx_lo, lo_b, lo_e, n0, a.N, b0, a.B);
#pragma unroll
    for (int r = 0; r < 16; ++r) { t[r] = a.s_lo * acc[r]; acc[r] = 0.f; }
    dbm_side<false>(acc, s_w, s_x, a.W_hi, a.ldw_hi, a.x_hi, a.ldx_hi, hi_b, hi_e, n0, a.N, b0, a.B);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = t[r] + a.s_hi * acc[r];

    if (a.ks > 1) {
        // publish the partial tile, count the arrival; the block whose add comes last sums all slices in slice order
        typedef __attribute__((address_space(1))) uint32_t gu32;
        constexpr int TILE = DBM_BM * DBM_TN;
        const int64_t zt = (int64_t)z * a.ks * a.ntiles;
        gu32* mine = (gu32*)(a.slabs + (zt + (int64_t)sl * a.ntiles + tile) * TILE) + (16 * w) * DBM_TN + lane;
#pragma unroll
        for (int r = 0; r < 16; ++r) __hip_atomic_store(mine + r * DBM_TN, __float_as_uint(acc[r]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");      // every storing wave drains before the counter add
        int* cnt = a.counters + z * a.ntiles + tile;
        if (tid == 0) *s_last = (__hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.ks - 1) ? 1 : 0;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (!*s_last) return false;
        if (tid == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // zero again for the next launch
        const gu32* p0 = (const gu32*)(a.slabs + (zt + tile) * TILE) + (16 * w) * DBM_TN + lane;
        for (int q = 0; q < a.ks; ++q) {
            const gu32* pq = p0 + (int64_t)q * a.ntiles * TILE;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = __uint_as_float(__hip_atomic_load(pq + r * DBM_TN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = q == 0 ? t[r] : acc[r] + t[r];
        }
    }
    return true;
}

template <bool SAMPLE>
__global__ __launch_bounds__(256) void dbm_layer(const DbmLayerArgs a) {
    __shared__ float s_w[DBM_KC * DBM_LDW];
    __shared__ __attribute__((aligned(16))) float s_x[DBM_BM * DBM_KC];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tile = blockIdx.x, z = blockIdx.z;
    const int n0 = tile * DBM_TN, b0 = z * DBM_BM;
    float acc[16];
    if (!dbm_pre_tile(a, acc, s_w, s_x, &s_last)) return;

    // ---- epilogue: lane = output unit n, rows 16 w .. 16 w + 15 of the chunk
    const int n = n0 + lane;
    const bool n_ok = n < a.N;
    const float bias = n_ok ? a.bias[n] : 0.f;
    uint4 blk = make_uint4(0u, 0u, 0u, 0u);
    for (int r = 0; r < 16; ++r) {               // wave-uniform bounds
        const int b = b0 + 16 * w + r;
        if (b >= a.B) break;
        const float pr = sigmoidf_ref(acc[r] + bias);
        if constexpr (SAMPLE) {
            float u;
            if (a.uni.tape) {
                u = n_ok ? a.uni.tape[(int64_t)b * a.uni.N + n] : 0.f;
            } else {                             // the four rows of a global 4-row group share one Philox block (common.hpp)
                const uint64_t g = (uint64_t)(a.uni.row0 + b);
                if (r == 0 || (g & 3) == 0) blk = draw_block4(a.uni, g, n_ok ? n : 0);
                u = u24(pick4(blk, (int)(g & 3)));
            }
            if (n_ok) {
                a.s[(int64_t)b * a.lds + n] = pr > u ? 1.f : 0.f;
                if (a.p) a.p[(int64_t)b * a.ldp + n] = pr;
            }
        } else {
            const float mo = n_ok ? a.m[(int64_t)b * a.ldm + n] : 0.f;
            const float res = wave_max_all(n_ok ? fabsf(pr - mo) : 0.f);
            if (n_ok) a.m[(int64_t)b * a.ldm + n] = a.damp * mo + (1.0f - a.damp) * pr;
            if (lane == 0) a.res_part[(int64_t)tile * a.B + b] = res;
        }
    }
}

// out_res[b] = max over the tiles.  grid = ceil(B / 256), 256 threads
__global__ __launch_bounds__(256) void dbm_rows_finish(const float* res_part, int ntiles, int B, float* out_res) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float r = 0.f;
    for (int t = 0; t < ntiles; ++t) r = fmaxf(r, res_part[(int64_t)t * B + b]);
    out_res[b] = r;
}

}  // namespace imdbn
