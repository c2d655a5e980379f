// kernels_backprop.hpp -- the element-wise half of one back-propagation step through a sigmoid layer (imdbn_rbm_backprop_step,
// DESIGN §26).
//
//   backprop_rows    one pass over an error matrix e[B][N] (the error at a layer's pre-activation): it leaves the transposed
//                    three-term planes of e the weight pass reads ([t][N][Bp], the form prep_operand writes; rows >= B are written
//                    as zeros, the update kernel reads whole 64-row chunks), the column sums of e over each group of 8 rows,
//                    colsum_part[Bp / 8][N] (the bias gradient), and -- when the call has one pair only -- the all-zero planes of
//                    the other pair's slot on the same side.
//   backprop_apply   one pass over the bias-free product q[B][N] = e W^T (or e W) and the layer's input x:
//                    err_out = q * (x * (1 - x)), fp32.  Loads are clamped, nothing is written outside [B][N].
//   backprop_finish  the one or two biases and their momenta from the column partials, summed in index order.
//
// The mapping of delta_rows (kernels_delta.hpp): a thread owns one column and 8 consecutive rows, a wave 64 consecutive columns;
// a plane leaves as one 16-B store per thread and term, a column sum needs no cross-thread step.  No atomics, no LDS.
#pragma once
#include "kernels_ew.hpp"

namespace imdbn {

struct BackpropRowsArgs {
    int B, Bp, N;
    const float* e; int64_t lde;              // error rows [B][N] fp32
    bf16_t* tr_e; bf16_t* tr_zero; int terms; // planes of e / all-zero planes (nullable), term stride N Bp
    float* colsum_part;                       // [Bp / 8][N]
};

// grid = (ceil(N / 256), Bp / 8), block = 256: wave w of block x owns the 64-column tile 4 x + w
__global__ __launch_bounds__(256) void backprop_rows(const BackpropRowsArgs a) {
    const int lane = threadIdx.x & 63, tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile * 64 >= a.N) return;             // wave-uniform
    const int col = tile * 64 + lane, b0 = blockIdx.y * 8;
    const int cc = min(col, a.N - 1);
    float ev[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)               // all loads unconditional (clamped) and issued before any use
        ev[i] = a.e[(int64_t)min(b0 + i, a.B - 1) * a.lde + cc];
    float xe[8], cs = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        xe[i] = (col < a.N && b0 + i < a.B) ? ev[i] : 0.f;
        cs += xe[i];
    }
    OperandOut o{};
    o.Bp = a.Bp; o.tr_ts = (int64_t)a.N * a.Bp; o.tr_terms = a.terms; o.tr_negate = 0;
    o.tr = a.tr_e;
    store_forms<8>(o, xe, false, true, b0, col, a.N, a.Bp);
    if (a.tr_zero) {
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        o.tr = a.tr_zero;
        store_forms<8>(o, z, false, true, b0, col, a.N, a.Bp);
    }
    if (col < a.N) a.colsum_part[(int64_t)blockIdx.y * a.N + col] = cs;
}

struct BackpropApplyArgs {
    int B, N;
    const float* q; int64_t ldq;              // bias-free product [B][N] fp32
    const float* x; int64_t ldx;              // the layer's input [B][N] fp32 (a sigmoid output)
    float* out; int64_t ldo;                  // err_out [B][N]
};

// grid = (ceil(N / 256), ceil(B / 8)), block = 256
__global__ __launch_bounds__(256) void backprop_apply(const BackpropApplyArgs a) {
    const int col = blockIdx.x * 256 + threadIdx.x, b0 = blockIdx.y * 8;
    const int cc = min(col, a.N - 1);
    float qv[8], xv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {             // clamped, issued before any use
        const int bc = min(b0 + i, a.B - 1);
        qv[i] = a.q[(int64_t)bc * a.ldq + cc];
        xv[i] = a.x[(int64_t)bc * a.ldx + cc];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float d = xv[i] * (1.0f - xv[i]);
        if (col < a.N && b0 + i < a.B) a.out[(int64_t)(b0 + i) * a.ldo + col] = qv[i] * d;
    }
}

struct BackpropFinishArgs {
    int P;                                    // Bp / 8 partials per column
    const float* part_h; float* hid_bias; float* hb_m; int H;      // up pair: colsum(e_h) (hid_bias null: no up pair)
    const float* part_v; float* vis_bias; float* vb_m; int V;      // down pair: colsum(e_v) (vis_bias null: no down pair)
    float lr, mom, n;
};

__device__ __forceinline__ void backprop_bias(const float* part, int P, int N, int i, float* bias, float* bias_m, float lr, float mom, float n) {
    const float s = sum_parts(part, P, N, i);
    float m = bias_m[i] * mom;
    m = m + (lr * s) / n;
    bias_m[i] = m;
    bias[i] += m;
}

// grid = ceil(max(H, V) / 256), block = 256
__global__ __launch_bounds__(256) void backprop_finish(const BackpropFinishArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (a.hid_bias && i < a.H) backprop_bias(a.part_h, a.P, a.H, i, a.hid_bias, a.hb_m, a.lr, a.mom, a.n);
    if (a.vis_bias && i < a.V) backprop_bias(a.part_v, a.P, a.V, i, a.vis_bias, a.vb_m, a.lr, a.mom, a.n);
}

}  // namespace imdbn
