// kernels_dbm_ais.hpp -- row sums over a layer of a deep Boltzmann machine: the per-temperature step of its annealed importance
// sampling and the layer term of its variational bound (imdbn_dbm_rowsum_layer, imdbn_dbm_ais).
//
//   dbm_rowsum_layer<MODE>  the block, the concatenated-axis split-K, the last-arriver combine and the summation order of
//                           pre = x_lo W_lo + x_hi W_hi^T + bias are dbm_layer's (dbm_pre_tile, kernels_dbm.hpp; s_lo = s_hi = 1).
//                           The epilogue leaves, per batch row and tile of 64 units, ONE double: the sum over the tile's units of
//       WEIGH    sp(e(beta)) - sp(e(beta_prev)),  e(t) = t pre + (1 - t) base in double from the fp32 pre,
//                sp(t) = max(t, 0) + log1p(exp(-|t|)) (ais_softplus);  with s set it also draws the unit at beta as SAMPLE does
//       SAMPLE   bias_n s_n, where p = sigmoidf_ref(fl(fl(beta pre) + fl(fl(1 - beta) base))) (no base: fl(beta pre)), s = 1[p > U],
//                U the call's one ("u", N) draw as in dbm_layer; at beta = 1 without a base p and s are dbm_layer's bits
//       BOUND    mu_n pre_n + h(mu_n),  h(m) = -m log m - (1 - m) log(1 - m) with h(0) = h(1) = 0, in double
//                           The 64 lane terms of a row meet in the xor butterfly (wave_sum_all); lane 0 writes part[tile][row].
//   dbm_rowsum_finish       one thread per row: acc[row] += scale * (part[0][row] + part[1][row] + ...), tiles in order.
//   dbm_rows_bias_dot<DRAW> one wave per row: acc[row] (= or +=) scale * sum_n bias_n x_n in double, lane l taking n = l, l + 64, ...
//                           in ascending order, then the butterfly.  DRAW: x_n = 1[0.5 > U] is drawn here and written to s (the
//                           start state of an odd layer); else x is read (the b_0 v term of the bound).
// No floating-point atomics anywhere: the same call gives the same bits.  Nothing outside [B][N] of an output is written.
#pragma once
#include "kernels_ais.hpp"
#include "kernels_dbm.hpp"

namespace imdbn {

enum { DBM_WEIGH = 0, DBM_SAMPLE = 1, DBM_BOUND = 2 };

struct DbmRowsumArgs {
    // the operand and split-K fields of DbmLayerArgs, by name (dbm_pre_tile)
    const float* W_lo; int64_t ldw_lo; int K_lo; const float* x_lo; int64_t ldx_lo; float s_lo;
    const float* W_hi; int64_t ldw_hi; int K_hi; const float* x_hi; int64_t ldx_hi; float s_hi;
    const float* bias; int N, B;
    int ks, kchunk, ntiles;
    float* slabs;
    int* counters;
    // the epilogue
    float beta, beta_prev;
    const float* base;                           // [N], nullable: the base-rate bias of this layer
    const float* mu; int64_t ldmu;               // BOUND: the magnetisations of this layer
    DrawSrc uni; float* s; int64_t lds; float* p; int64_t ldp;      // the draw: s written (WEIGH: when non-null), p too when non-null
    double* part;                                // [tile][B]
};

// fp32 effective input of a unit at temperature beta
__device__ __forceinline__ float dbm_eff(float beta, float pre, const float* base, float bs) {
    const float t = __fmul_rn(beta, pre);
    return base ? __fadd_rn(t, __fmul_rn(__fsub_rn(1.0f, beta), bs)) : t;
}

__device__ __forceinline__ double dbm_entropy(double m) {
    return (m > 0.0 ? -m * log(m) : 0.0) + (m < 1.0 ? -(1.0 - m) * log1p(-m) : 0.0);
}

template <int MODE>
__global__ __launch_bounds__(256) void dbm_rowsum_layer(const DbmRowsumArgs a) {
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
    const float bs = (n_ok && a.base) ? a.base[n] : 0.f;
    const bool draw = MODE == DBM_SAMPLE || (MODE == DBM_WEIGH && a.s != nullptr);
    uint4 blk = make_uint4(0u, 0u, 0u, 0u);
    for (int r = 0; r < 16; ++r) {               // wave-uniform bounds
        const int b = b0 + 16 * w + r;
        if (b >= a.B) break;
        const float pre = acc[r] + bias;
        double term = 0.0;
        if constexpr (MODE == DBM_WEIGH) {
            const double e1 = (double)a.beta * (double)pre + (1.0 - (double)a.beta) * (double)bs;
            const double e0 = (double)a.beta_prev * (double)pre + (1.0 - (double)a.beta_prev) * (double)bs;
            if (n_ok) term = ais_softplus(e1) - ais_softplus(e0);
        }
        if constexpr (MODE == DBM_BOUND) {
            const double m = n_ok ? (double)a.mu[(int64_t)b * a.ldmu + n] : 0.0;
            if (n_ok) term = m * (double)pre + dbm_entropy(m);
        }
        if constexpr (MODE != DBM_BOUND) {
            if (draw) {                          // kernel-uniform
                const float pr = sigmoidf_ref(dbm_eff(a.beta, pre, a.base, bs));
                float u;
                if (a.uni.tape) {
                    u = n_ok ? a.uni.tape[(int64_t)b * a.uni.N + n] : 0.f;
                } else {                         // the four rows of a global 4-row group share one Philox block (common.hpp)
                    const uint64_t g = (uint64_t)(a.uni.row0 + b);
                    if (r == 0 || (g & 3) == 0) blk = draw_block4(a.uni, g, n_ok ? n : 0);
                    u = u24(pick4(blk, (int)(g & 3)));
                }
                const bool one = pr > u;
                if (n_ok) {
                    a.s[(int64_t)b * a.lds + n] = one ? 1.f : 0.f;
                    if (a.p) a.p[(int64_t)b * a.ldp + n] = pr;
                }
                if (MODE == DBM_SAMPLE && n_ok && one) term = (double)bias;
            }
        }
        term = wave_sum_all(term);
        if (lane == 0) a.part[(int64_t)tile * a.B + b] = term;
    }
}

// acc[b] += scale * (the tiles' partials, in tile order).  grid = ceil(B / 256), 256 threads
__global__ __launch_bounds__(256) void dbm_rowsum_finish(const double* part, int ntiles, int B, double scale, double* acc) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    double t = 0.0;
    for (int q = 0; q < ntiles; ++q) t += part[(int64_t)q * B + b];
    acc[b] += scale * t;
}

struct DbmBiasDotArgs {
    const float* bias; int N, B;
    const float* x; int64_t ldx;                 // !DRAW: the rows
    DrawSrc uni; float* s; int64_t lds;          // DRAW: the ("u", N) draw and the state it gives
    double scale; int first;                     // acc[row] = scale t (first) or += scale t
    double* acc;
};

// grid = ceil(B / ROW_WAVES), 64 ROW_WAVES threads
template <bool DRAW>
__global__ __launch_bounds__(64 * ROW_WAVES) void dbm_rows_bias_dot(const DbmBiasDotArgs a) {
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.B) return;                      // wave-uniform
    double t = 0.0;
    for (int n = lane; n < a.N; n += 64) {
        float x;
        if constexpr (DRAW) {
            x = 0.5f > draw_uniform(a.uni, row, n) ? 1.f : 0.f;
            a.s[(int64_t)row * a.lds + n] = x;
        } else {
            x = a.x[(int64_t)row * a.ldx + n];
        }
        t += (double)a.bias[n] * (double)x;
    }
    t = wave_sum_all(t);
    if (lane == 0) a.acc[row] = (a.first ? 0.0 : a.acc[row]) + a.scale * t;
}

}  // namespace imdbn
