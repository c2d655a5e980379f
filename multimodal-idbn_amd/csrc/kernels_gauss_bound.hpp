// kernels_gauss_bound.hpp -- the Gaussian half of the bottom layer's bracket of the DBN lower bound with a Gaussian visible layer
// (imdbn_rbm_gauss_bound_step).  The hidden half -- h ~ q(h | v) and the entropy of q / -log q(h) -- is
// bound_entropy_sample_h of kernels_bound.hpp as it is: it sees logits and a draw and knows nothing of the visible type.
//
//   gauss_bound_loglik_rows   one pass over the fp32 mean m[M][V] = b + h W^T the down propagation left (logits_only), the caller's
//                             fp32 rows v[M][V] and the log-variances z[V]:
//                             acc[row] += -sum_i ((v_i - m_i)^2 e^{-z_i} / 2 + z_i / 2) - (V / 2) log 2 pi = log N(v; m, e^z),
//                             every element formed in double from the widened fp32 values (the subtraction too).
//
// The mapping of bound_loglik_rows: one wave per row, ROW_WAVES rows per block, rows >= M return, lane l takes the elements
// l, l + 64, ... in ascending order, the 64 lane sums meet in the fixed butterfly (wave_sum_all), lane 0 owns acc[row] and adds the
// row sum first and the constant second; no atomics, no LDS, no scratch.  Everything but acc is only read.
#pragma once
#include "kernels_bound.hpp"

namespace imdbn {

struct GaussBoundArgs {
    int M, V;
    const float* mean; int64_t ldm;                     // m = b + h W^T     [M][V] fp32
    const float* v; int64_t ldv;                        // the caller's rows [M][V] fp32
    const float* logvar;                                // z [V]
    double* acc;
};

__global__ __launch_bounds__(64 * ROW_WAVES) void gauss_bound_loglik_rows(const GaussBoundArgs a) {
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.M) return;           // wave-uniform
    const float* m = a.mean + (int64_t)row * a.ldm;
    const float* v = a.v + (int64_t)row * a.ldv;
    double s = 0.0;
    for (int i = lane; i < a.V; i += 64) {
        const double z = (double)a.logvar[i], d = (double)v[i] - (double)m[i];
        s += -((d * d) * exp(-z) / 2.0 + z / 2.0);
    }
    s = wave_sum_all(s);
    if (lane == 0) {
        double t = a.acc[row];
        t += s;
        t += -((double)a.V / 2.0) * 1.8378770664093453;      // log 2 pi
        a.acc[row] = t;
    }
}

}  // namespace imdbn
