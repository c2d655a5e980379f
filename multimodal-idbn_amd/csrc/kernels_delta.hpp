// kernels_delta.hpp -- the element-wise half of one delta-rule step of a directed layer (imdbn_rbm_delta_step).
//
//   delta_rows     one pass over the fp32 logits a[B][N] of the predicting propagation and the caller's target rows:
//                  p = sigmoid(a), r = target - p.  It leaves, in that one pass,
//                    - the operands of the weight pass: the transposed three-term planes of `target` and of -p ([t][N][Bp], the form
//                      prep_operand writes; the update kernel adds in^T target and in^T (-p) in one accumulator, so in^T r never
//                      needs a rounded r) -- rows >= B are written as zeros, the update kernel reads whole 64-row chunks;
//                    - the column sums of r over each group of 8 rows, colsum_part[Bp / 8][N] (the bias gradient);
//                    - the row log-probability sum_j (target_j a_j - softplus(a_j)) in double, as one partial per 64-column tile,
//                      lp_part[ceil(N / 64)][Bp].
//   delta_finish   the predicting bias and its momentum from the column partials (summed in index order), and out_rowlp[b] = the
//                  row's tile partials added in ascending tile order: every sum has an order fixed by N.
//
// The mapping of prep_operand / finish (kernels_ew.hpp): a thread owns one column and 8 consecutive rows, so a plane leaves as one
// 16-B store per thread and term, and a column sum needs no cross-thread step.  A wave owns 64 consecutive columns; the 64 lane
// values of a row meet in the fixed butterfly (wave_sum_all).  No atomics, no LDS.
#pragma once
#include "kernels_ais.hpp"

namespace imdbn {

struct DeltaArgs {
    int B, Bp, N;
    const float* a; int64_t lda;              // logits [B][N] fp32
    const float* t; int64_t ldt;              // target [B][N] fp32
    bf16_t* tr_t; bf16_t* tr_p; int terms;    // planes of target / of -p, term stride N Bp (both null: evaluate only)
    float* colsum_part;                       // [Bp / 8][N] (nullable)
    double* lp_part;                          // [ceil(N / 64)][Bp] (nullable)
    // delta_finish
    float* bias; float* bias_m;               // the predicting bias [N] and its momentum (null: evaluate only)
    float lr, mom, n;
    double* out_rowlp;                        // [B] (nullable)
};

// grid = (ceil(N / 256), Bp / 8), block = 256: wave w of block x owns the 64-column tile 4 x + w
__global__ __launch_bounds__(256) void delta_rows(const DeltaArgs a) {
    const int lane = threadIdx.x & 63, tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile * 64 >= a.N) return;             // wave-uniform
    const int col = tile * 64 + lane, b0 = blockIdx.y * 8;
    const int cc = min(col, a.N - 1);
    float lg[8], tg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {             // all loads unconditional (clamped) and issued before any use
        const int bc = min(b0 + i, a.B - 1);
        lg[i] = a.a[(int64_t)bc * a.lda + cc];
        tg[i] = a.t[(int64_t)bc * a.ldt + cc];
    }
    float xt[8], xp[8], cs = 0.f;
    double lp[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool live = col < a.N && b0 + i < a.B;
        const float p = sigmoidf_ref(lg[i]);
        xt[i] = live ? tg[i] : 0.f;
        xp[i] = live ? p : 0.f;
        cs += xt[i] - xp[i];
        lp[i] = 0.0;
        if (a.lp_part && live) {
            const double x = (double)lg[i];
            lp[i] = (double)tg[i] * x - ais_softplus(x);
        }
    }
    if (a.tr_t) {
        OperandOut o{};
        o.Bp = a.Bp; o.tr_ts = (int64_t)a.N * a.Bp; o.tr_terms = a.terms;
        o.tr = a.tr_t; o.tr_negate = 0;
        store_forms<8>(o, xt, false, true, b0, col, a.N, a.Bp);
        o.tr = a.tr_p; o.tr_negate = 1;
        store_forms<8>(o, xp, false, true, b0, col, a.N, a.Bp);
    }
    if (a.colsum_part && col < a.N) a.colsum_part[(int64_t)blockIdx.y * a.N + col] = cs;
    if (a.lp_part) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double s = wave_sum_all(lp[i]);
            if (lane == 0) a.lp_part[(int64_t)tile * a.Bp + b0 + i] = s;
        }
    }
}

// grid = ceil(max(N, B) / 256), block = 256
__global__ __launch_bounds__(256) void delta_finish(const DeltaArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (a.bias && i < a.N) {
        const float s = sum_parts(a.colsum_part, a.Bp / 8, a.N, i);
        float m = a.bias_m[i] * a.mom;
        m = m + (a.lr * s) / a.n;
        a.bias_m[i] = m;
        a.bias[i] += m;
    }
    if (a.out_rowlp && i < a.B) {
        const int nt = (a.N + 63) / 64;
        double s = 0.0;
        for (int k = 0; k < nt; ++k) s += a.lp_part[(int64_t)k * a.Bp + i];
        a.out_rowlp[i] = s;
    }
}

}  // namespace imdbn
