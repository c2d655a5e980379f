// kernels_bound.hpp -- the element-wise half of one directed layer of the DBN lower bound (imdbn_rbm_bound_step).
//
//   bound_entropy_sample_h   one pass over the fp32 logits x[M][H] of q(h | v): h = 1[sigmoid(x) > U] -- the fp32 decision of the
//                            sampling up propagation -- as fp32 0/1 for the caller AND as the bf16 form and the bit plane the down
//                            propagation reads; acc[row] += the entropy of q (IMDBN_BOUND_ENTROPY) or -log q(h) of the drawn h
//                            (IMDBN_BOUND_LOGQ), summed in double.
//   bound_loglik_rows        one pass over the fp32 logits a[M][V] of p(v | h) and the caller's rows:
//                            acc[row] += sum_i v_i a_i - softplus(a_i) = log p(v | h), summed in double.
//
// The mapping of kernels_ais.hpp: one wave per row, four rows per block, rows dealt up to Bp (the padded rows write zeros into
// the operand forms and touch nothing else), lane l takes the elements l, l + 64, ... in ascending order, the 64 lane sums meet in
// the fixed butterfly, lane 0 owns acc[row]; no atomics, no LDS, no scratch.
#pragma once
#include "kernels_ais.hpp"

namespace imdbn {

struct BoundArgs {
    int M, Bp, V, H, Hpad;
    int mode;                                           // IMDBN_BOUND_ENTROPY (0) / IMDBN_BOUND_LOGQ (1)
    const float* x; int64_t ldx;                        // logits c + v W    [M][H] fp32
    const float* a; int64_t lda;                        // logits b + h W^T  [M][V] fp32
    const float* v; int64_t ldv;                        // the caller's rows [M][V] fp32
    DrawSrc uni;                                        // the ("u", H) draw
    float* out_h; int64_t ldh;                          // h as fp32 0/1 [M][H]
    bf16_t* rm;                                         // hid_rm (ld Hpad), K16-blocked, one term
    uint8_t* bits;                                      // hidden bit plane, byte-major [rup(H, 64) / 8][Bp]
    double* acc;
};

__global__ __launch_bounds__(64 * ROW_WAVES) void bound_entropy_sample_h(const BoundArgs a) {
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.Bp) return;
    const bool live = row < a.M;      // wave-uniform
    double e = 0.0;
    const int Hb = (a.H + 63) & ~63;      // whole ballots: the bit plane covers [0, rup(H, 64))
    for (int j = lane; j < Hb; j += 64) {
        bool one = false;
        if (live && j < a.H) {
            const float x = a.x[(int64_t)row * a.ldx + j];
            one = sigmoidf_ref(x) > draw_uniform(a.uni, row, j);
            const double xd = (double)x, sp = ais_softplus(xd);
            if (a.mode == 0) e += sp - xd / (1.0 + exp(-xd));      // softplus(x) - x sigmoid(x)
            else e += sp - (one ? xd : 0.0);                       // -(h x - softplus(x))
            a.out_h[(int64_t)row * a.ldh + j] = one ? 1.f : 0.f;
        }
        ais_store_hidden(a.rm, a.bits, a.Bp, a.Hpad, row, j, one);
    }
    if (!live) return;
    e = wave_sum_all(e);
    if (lane == 0) a.acc[row] += e;
}

__global__ __launch_bounds__(64 * ROW_WAVES) void bound_loglik_rows(const BoundArgs a) {
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.M) return;           // wave-uniform
    const float* lg = a.a + (int64_t)row * a.lda;
    const float* v = a.v + (int64_t)row * a.ldv;
    double s = 0.0;
    for (int i = lane; i < a.V; i += 64) {
        const double t = (double)lg[i];
        s += (double)v[i] * t - ais_softplus(t);
    }
    s = wave_sum_all(s);
    if (lane == 0) a.acc[row] += s;
}

}  // namespace imdbn
