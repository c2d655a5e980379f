// IMG->TXT energy tracing (imdbn/utils/energy_utils.py; reference energy_utils.py:60-195) for a whole panel in one launch.
//
// The code z is re-clamped after every step, so the hidden pre-activation splits into a constant and a label part:
//   base = z W[:Dz] + c      (one K1 propagation for the panel, done by the caller of this kernel)
//   h    = sigmoid(base + y Wy),            Wy = W[Dz:Dz+K]
//   y'   = softmax(sigmoid(h Wy^T + by))    -- the reference's quirk: a softmax over the SIGMOID outputs of the label slice
// and the class free energies come from the same base:  F_k = -(z.bz + by_k) - sum_j softplus(base_j + Wy[k][j]).
// energy_trace_rows does, per row and without a host round trip: z.bz, F (all k), Fmin / kstar / F(2) - F(1), softmax(-F) top-1 and
// gap, then `steps` label steps with the top-2 of y_t, p(gt), |y_t - y_{t-1}|_1, the argmax streak, F[pred] - Fmin and the stop rule
// of reference :164.  Decisions compare in double, as the reference does with Python floats.
//
// One wave per row, 4 rows per block.  Lanes run over the hidden columns (j = lane + 64 q) in BOTH phases, so Wy is only ever read
// row-wise -- consecutive lanes, consecutive dwords: no LDS bank conflict and coalesced when Wy stays in global memory -- and the
// y phase ends each k with a wave butterfly.  Every sum has a fixed order that depends on (Dz, K, H) alone: per lane ascending in q (or k),
// then the xor butterfly 32, 16, .. 1; a row gives the same bits alone or inside any panel.
//   WLDS: Wy [K][H] staged once per block in LDS (K H 4 <= ENERGY_WY_LDS bytes), else read from global (L2-resident).
//   HLDS: base and h of the wave's row live in LDS (H <= ENERGY_H_LDS), else base is re-read from global and h goes through a
//         global scratch row; each lane only reads back what it wrote itself.
// Label values sit in registers, label k in lane k & 63, slot k >> 6 (kernels_rows.hpp; K <= LABEL_KMAX = 256).
#pragma once
#include <type_traits>

#include "common.hpp"
#include "kernels_rows.hpp"

namespace imdbn {

constexpr int ENERGY_WY_LDS = 32 * 1024;         // bytes of Wy staged in LDS (32 x 256 fp32 fits exactly)
constexpr int ENERGY_H_LDS = 1024;               // widest H whose base / h rows are kept in LDS (2 x ROW_WAVES rows x 4 KB)

struct EnergyArgs {
    const float* base; int64_t ldb;              // [N][H] hidden pre-activations of the clamped code
    const float* z; int64_t ldz;                 // [N][Dz]
    const float* bz; const float* by;            // visible biases of the code / label columns
    const float* Wy; int64_t ldw;                // [K] rows of pitch ldw
    int N, Dz, K, H, steps;
    const int32_t* gt;                           // [N] nullable
    const float* y0; int64_t ldy0;               // [N][K] start distribution, nullable = uniform
    double eps_l1; int stable_steps; double gap_thresh;
    float* hscr;                                 // [N][H] (HLDS = false only)
    float *p1, *p2, *pgt, *dF, *l1;              // [N][steps]; pgt nullable
    int32_t* k1;                                 // [N][steps]
    int32_t *conv, *kstar, *predT;               // [N]
    float *margin, *fe_top1, *fe_gap;            // [N]
    float* F;                                    // [N][K]
    float* y_out;                                // [N][K] nullable: y after the last step
};

__device__ __forceinline__ float en_lane(float v, int lane) {      // lane is wave-uniform
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ float en_softplus(float t) { return t > 20.0f ? t : log1pf(expf(t)); }      // as torch

// The value of label k out of the label slots, in every lane, as the owner's value plus 63 zeros (exact; 0 for a k no lane owns).  Not
// slots_pick: its shuffle costs this kernel two to four VGPRs, and <true, false> sits at 64 of them, the last step of 8 waves per SIMD.
// For the same reason the kernel spells out its row and its two slot loads below: with wave_row() and slots_load the compiler allots
// its registers otherwise and a row's chain of steps measured 2 to 3 % slower.
__device__ __forceinline__ float en_pick(const float (&y)[4], int l, int k) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (l + 64 * q == k) v = y[q];
    return wave_sum_all(v);
}

// body(q) for the four label slots with q a compile-time constant (the slots are registers: no dynamic index)
template <class Fn>
__device__ __forceinline__ void en_slots(Fn&& body) {
    body(std::integral_constant<int, 0>{}); body(std::integral_constant<int, 1>{});
    body(std::integral_constant<int, 2>{}); body(std::integral_constant<int, 3>{});
}

template <bool WLDS, bool HLDS>
__global__ __launch_bounds__(64 * ROW_WAVES) void energy_trace_rows(const EnergyArgs a) {
    extern __shared__ float en_lds[];
    const int l = wave_lane(), wv = threadIdx.x >> 6, b = blockIdx.x * ROW_WAVES + wv;      // = wave_row()
    const int K = a.K, H = a.H;
    const float* W = a.Wy;
    int64_t ldw = a.ldw;
    if (WLDS) {
        for (int i = threadIdx.x; i < K * H; i += 64 * ROW_WAVES) {
            const int k = i / H, j = i - k * H;
            en_lds[i] = a.Wy[(int64_t)k * a.ldw + j];
        }
        __syncthreads();                                                   // before any wave leaves
        W = en_lds; ldw = H;
    }
    if (b >= a.N) return;                                                  // wave-uniform
    const float* bs;
    float* hs;
    if (HLDS) {
        float* mine = en_lds + (WLDS ? K * H : 0) + wv * 2 * H;
        for (int j = l; j < H; j += 64) mine[j] = a.base[(int64_t)b * a.ldb + j];
        bs = mine; hs = mine + H;
    } else {
        bs = a.base + (int64_t)b * a.ldb;
        hs = a.hscr + (int64_t)b * H;
    }
    // ---- z . bz
    float zb = 0.f;
    for (int c = l; c < a.Dz; c += 64) zb = fmaf(a.z[(int64_t)b * a.ldz + c], a.bz[c], zb);
    zb = wave_sum_all(zb);
    // ---- class free energies; nF = -F in the label slots
    float nF[4] = {0.f, 0.f, 0.f, 0.f}, by[4], y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                                          // slots_load of by and of y0, or the uniform start
        const int c = l + 64 * q;
        by[q] = c < K ? a.by[c] : 0.f;
        y[q] = c < K ? (a.y0 ? a.y0[(int64_t)b * a.ldy0 + c] : 1.0f / (float)K) : 0.f;
    }
    en_slots([&](auto qc) __attribute__((always_inline)) {
        constexpr int q = decltype(qc)::value;
        const int nk = min(64, K - 64 * q);
        for (int kk = 0; kk < nk; ++kk) {
            const float* wr = W + (int64_t)(64 * q + kk) * ldw;
            float s = 0.f;
            for (int j = l; j < H; j += 64) s += en_softplus(bs[j] + wr[j]);
            s = wave_sum_all(s);
            if (l == kk) nF[q] = (zb + by[q]) + s;                         // F_k = -(z.bz + by_k) - sum softplus
        }
    });
    const Top2 tf = slots_top2(nF, l, K);                                   // largest -F first, the lower index on ties (torch.min)
    const float f1 = tf.v1, f2 = tf.v2, Fmin = -tf.v1;
    const int kstar = tf.i1;
    {
        float e = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = l + 64 * q;
            if (c < K) { e += expf(nF[q] - f1); a.F[(int64_t)b * K + c] = -nF[q]; }
        }
        e = wave_sum_all(e);
        if (l == 0) {
            a.kstar[b] = kstar;
            a.margin[b] = K > 1 ? (-f2) - (-f1) : 0.f;                     // F(2) - F(1)
            a.fe_top1[b] = 1.0f / e;                                       // exp(0) / sum
            a.fe_gap[b] = K > 1 ? 1.0f / e - expf(f2 - f1) / e : 0.f;
        }
    }
    // ---- the label chain
    const int g = a.gt ? a.gt[b] : -1;
    int pred = slots_top2(y, l, K).i1, streak = 0, conv = a.steps + 1;      // argmax of the start (0 for the uniform start)
    for (int t = 1; t <= a.steps; ++t) {
        // h = sigmoid(base + y Wy): per column base first, then k ascending
        for (int j = l; j < H; j += 64) {
            float acc = bs[j];
            en_slots([&](auto qc) __attribute__((always_inline)) {
                constexpr int q = decltype(qc)::value;
                const int nk = min(64, K - 64 * q);
                for (int kk = 0; kk < nk; ++kk) acc = fmaf(en_lane(y[q], kk), W[(int64_t)(64 * q + kk) * ldw + j], acc);
            });
            hs[j] = sigmoidf_ref(acc);
        }
        // y' = softmax(sigmoid(h Wy^T + by))
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        en_slots([&](auto qc) __attribute__((always_inline)) {
            constexpr int q = decltype(qc)::value;
            const int nk = min(64, K - 64 * q);
            for (int kk = 0; kk < nk; ++kk) {
                const float* wr = W + (int64_t)(64 * q + kk) * ldw;
                float s = 0.f;
                for (int j = l; j < H; j += 64) s = fmaf(hs[j], wr[j], s);
                s = wave_sum_all(s);
                if (l == kk) x[q] = s;
            }
        });
        float mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            x[q] = sigmoidf_ref(x[q] + by[q]);
            if (l + 64 * q < K) mx = fmaxf(mx, x[q]);
        }
        mx = wave_max_all(mx);
        float den = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            x[q] = l + 64 * q < K ? expf(x[q] - mx) : 0.f;
            den += x[q];
        }
        den = wave_sum_all(den);
        float l1 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float yn = x[q] / den;
            l1 += fabsf(yn - y[q]);                                        // slots past K hold 0 on both sides
            y[q] = yn;
        }
        l1 = wave_sum_all(l1);
        const Top2 ty = slots_top2(y, l, K);
        const float v1 = ty.v1, v2 = ty.v2;
        const int i1 = ty.i1;
        streak = (i1 == pred) ? streak + 1 : 1;
        pred = i1;
        const float dF = (-en_pick(nF, l, pred)) - Fmin;
        if (l == 0) {
            const int64_t o = (int64_t)b * a.steps + (t - 1);
            a.p1[o] = v1; a.p2[o] = v2; a.k1[o] = i1; a.l1[o] = l1; a.dF[o] = dF;
        }
        if (a.pgt) {
            const float pg = g >= 0 && g < K ? en_pick(y, l, g) : 0.f;
            if (l == 0) a.pgt[(int64_t)b * a.steps + (t - 1)] = pg;
        }
        if (conv > a.steps && (double)l1 < a.eps_l1 && streak >= a.stable_steps &&
            (pred == kstar || (double)v1 - (double)v2 >= a.gap_thresh)) {
            conv = t;
            if (l == 0) a.predT[b] = pred;                                 // the argmax at the stopping step
        }
    }
    if (l == 0) {
        a.conv[b] = conv;
        if (conv > a.steps) a.predT[b] = pred;
    }
    if (a.y_out) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (l + 64 * q < K) a.y_out[(int64_t)b * K + l + 64 * q] = y[q];
    }
}

}  // namespace imdbn
