// kernels_dbm_group.hpp -- the half-step of a DBM layer whose units are categorical (imdbn_dbm_group_layer): the label
// layer of the multimodal DBM, which hears from the joint hidden layer through a row block of the joint RBM's W.
//
// The N units are tiled exactly by G <= IMDBN_MAX_GROUPS consecutive softmax groups of 2 .. GROUP_WMAX units; group g is the columns
// [end[g-1], end[g]) (end[-1] = 0).  A group up to 256 wide spans up to four 64-unit tiles of the layer block, so the softmax cannot
// live in the tile epilogue: the call is two launches.
//
//   dbm_group_logits        the block, the concatenated-axis split-K, the last-arriver combine and the summation order of pre are
//                           dbm_layer's (dbm_pre_tile, kernels_dbm.hpp).  Its epilogue leaves x = fl(pre + bias) in the workspace,
//                           [B][N] fp32 with pitch N.
//   dbm_group_finish<SAMPLE>   grid = ceil(B / ROW_WAVES), 64 ROW_WAVES threads: one wave per batch row, the groups of the row one
//                           after the other.  Column j of a group sits in lane j & 63, slot j >> 6 (four slots).  Per group:
//       mx   = the maximum of the group's x (exact whatever the order)
//       e_j  = expf(x_j - mx)
//       sum  = lane partials ((e[slot 0] + e[slot 1]) + e[slot 2]) + e[slot 3] (absent columns add +0), then the xor butterfly
//              32, 16, .. 1 over the lanes (wave_sum_all): one order whatever the batch, the group's position or the other groups
//       p_j  = e_j / sum
//     mean field   res[b] = max over all units of |p - m_old|, m = damp m_old + (1 - damp) p in place (dbm_layer's damping)
//     sample       one index per row and group from the call's categorical source: REPLAY reads cat_tape[g][b]; PHILOX walks the
//                  inverse CDF over c_j = clamp(p_j, 1e-8, 1) in column order, fp32 left to right: tot = c_0 + c_1 + ..., the first j
//                  with c_0 + .. + c_j > U tot, else the last -- U the ("c", width) draw of group g, element (row, 0) of draw number
//                  draw0 + g (categorical_rows / finish_groups_body, kernels_ew.hpp; oracle/draws.py).  s = the one-hot row, p too
//                  when non-null.
// No floating-point atomics: the same call gives the same bits.  Nothing outside [B][N] of m, s, p and res [B] is written.
#pragma once
#include "kernels_dbm.hpp"

namespace imdbn {

constexpr int DBM_GROUP_SLOTS = GROUP_WMAX / 64;

struct DbmGroupArgs {
    // the operand and split-K fields of DbmLayerArgs, by name (dbm_pre_tile)
    const float* W_lo; int64_t ldw_lo; int K_lo; const float* x_lo; int64_t ldx_lo; float s_lo;
    const float* W_hi; int64_t ldw_hi; int K_hi; const float* x_hi; int64_t ldx_hi; float s_hi;
    const float* bias; int N, B;
    int ks, kchunk, ntiles;
    float* slabs;
    int* counters;
    // the epilogue
    float* logits;                               // [B][N]
};

__global__ __launch_bounds__(256) void dbm_group_logits(const DbmGroupArgs a) {
    __shared__ float s_w[DBM_KC * DBM_LDW];
    __shared__ __attribute__((aligned(16))) float s_x[DBM_BM * DBM_KC];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n0 = blockIdx.x * DBM_TN, b0 = blockIdx.z * DBM_BM;
    float acc[16];
    if (!dbm_pre_tile(a, acc, s_w, s_x, &s_last)) return;

    // ---- epilogue: lane = output unit n, rows 16 w .. 16 w + 15 of the chunk
    const int n = n0 + lane;
    if (n >= a.N) return;
    const float bias = a.bias[n];
    for (int r = 0; r < 16; ++r) {
        const int b = b0 + 16 * w + r;
        if (b >= a.B) break;
        a.logits[(int64_t)b * a.N + n] = acc[r] + bias;
    }
}

struct DbmGroupFinishArgs {
    const float* logits; int N, B;
    int n_groups, end[IMDBN_MAX_GROUPS];
    float* m; int64_t ldm; float damp; float* res;              // mean field: m read and written in place, res nullable
    const int32_t* cat_tape; DrawSrc cat_uni;                     // sample: the call's categorical source
    float* s; int64_t lds; float* p; int64_t ldp;                 // s written, p too when non-null
};

template <bool SAMPLE>
__global__ __launch_bounds__(64 * ROW_WAVES) void dbm_group_finish(const DbmGroupFinishArgs a) {
    __shared__ float s_c[SAMPLE ? ROW_WAVES : 1][GROUP_WMAX];    // the clipped probabilities of the wave's row, in column order
    const int lane = wave_lane(), w = threadIdx.x >> 6;
    const bool live = wave_row() < a.B;           // wave-uniform
    if (!SAMPLE && !live) return;
    const int b = min(wave_row(), a.B - 1);       // SAMPLE: a wave past the batch meets the barriers on row B - 1 and stores nothing
    const float* x = a.logits + (int64_t)b * a.N;
    float res = 0.f;
    int g0 = 0;
    for (int g = 0; g < a.n_groups; ++g) {       // kernel-uniform
        const int wd = a.end[g] - g0;
        float v[DBM_GROUP_SLOTS], mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < DBM_GROUP_SLOTS; ++q) {
            const int j = lane + 64 * q;
            v[q] = j < wd ? x[g0 + j] : -INFINITY;
            mx = fmaxf(mx, v[q]);
        }
        mx = wave_max_all(mx);
        float part = 0.f;
#pragma unroll
        for (int q = 0; q < DBM_GROUP_SLOTS; ++q) {
            v[q] = lane + 64 * q < wd ? expf(v[q] - mx) : 0.f;
            part = q == 0 ? v[0] : part + v[q];
        }
        const float sum = wave_sum_all(part);
#pragma unroll
        for (int q = 0; q < DBM_GROUP_SLOTS; ++q) v[q] = v[q] / sum;

        if constexpr (SAMPLE) {
            int idx;
            if (a.cat_tape) {
                idx = a.cat_tape[(int64_t)g * a.B + b];
            } else {
#pragma unroll
                for (int q = 0; q < DBM_GROUP_SLOTS; ++q)
                    if (lane + 64 * q < wd) s_c[w][lane + 64 * q] = fminf(fmaxf(v[q], 1e-8f), 1.0f);
                __syncthreads();
                // every lane walks the row (one LDS address per step: a broadcast), so every lane ends with the index
                DrawSrc cs = a.cat_uni; cs.draw += g; cs.N = 1;
                float tot = 0.f;
                for (int j = 0; j < wd; ++j) tot += s_c[w][j];
                const float target = draw_uniform(cs, b, 0) * tot;
                float acc = 0.f;
                idx = wd - 1;
                for (int j = 0; j < wd; ++j) {
                    acc += s_c[w][j];
                    if (acc > target) { idx = j; break; }
                }
                __syncthreads();                 // the row has been read before the next group overwrites it
            }
#pragma unroll
            for (int q = 0; q < DBM_GROUP_SLOTS; ++q) {
                const int j = lane + 64 * q;
                if (live && j < wd) {
                    a.s[(int64_t)b * a.lds + g0 + j] = j == idx ? 1.f : 0.f;
                    if (a.p) a.p[(int64_t)b * a.ldp + g0 + j] = v[q];
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < DBM_GROUP_SLOTS; ++q) {
                const int j = lane + 64 * q;
                if (j < wd) {
                    float* mp = a.m + (int64_t)b * a.ldm + g0 + j;
                    const float mo = *mp;
                    res = fmaxf(res, fabsf(v[q] - mo));
                    if (live) *mp = a.damp * mo + (1.0f - a.damp) * v[q];
                }
            }
        }
        g0 = a.end[g];
    }
    if constexpr (!SAMPLE) {
        res = wave_max_all(res);
        if (live && a.res && lane == 0) a.res[b] = res;
    }
}

}  // namespace imdbn
