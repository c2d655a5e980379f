// kernels_reverse_ais.hpp -- the element-wise half of reverse annealed importance sampling (imdbn_rbm_reverse_ais) and
// the per-test-row reduction of its weights (imdbn_rows_logmeanexp).  The weight-and-draw kernel of the call is ais_weight_sample_h.
//
//   rais_load_v            the caller's start states: fp32 state, single-term K16-blocked operand form (padding rows: zeros),
//                          logw = sum_i b_i v_i in double.  A row holding an element that is not exactly 0 or 1, or a softmax group
//                          that does not hold exactly one 1, gets logw = NaN -- every later step only adds to it, so the row stays NaN.
//   rows_logmeanexp        one wave per test row over its M chains: max-shifted sums of w and w^2 in double -> log mean w, ess.
//
// Rows, lanes and sums as in kernels_ais.hpp: one wave per row, ROW_WAVES rows per block, rows dealt up to Bp, lane l takes the
// elements l, l + 64, ... in ascending order, the 64 lane sums meet in the fixed butterfly.  No atomics, no LDS, no scratch.
#pragma once
#include "kernels_ais.hpp"

namespace imdbn {

struct RaisLoadArgs {
    AisArgs a;                                     // M rows; state / lds; rm = vis_rm; vis_bias; logw
    const float* v; int64_t ldv;                   // the caller's start states [M][V]
    GroupSpans sp;
};

__global__ __launch_bounds__(64 * ROW_WAVES) void rais_load_v(const RaisLoadArgs g) {
    const AisArgs& a = g.a;
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.Bp) return;
    const bool live = row < a.M;      // wave-uniform
    double sb = 0.0;
    bool bad = false;
    for (int i = lane; i < a.Vpad; i += 64) {
        bool one = false;
        if (live && i < a.V) {
            const float x = g.v[(int64_t)row * g.ldv + i];
            one = x == 1.f;
            bad |= !(one || x == 0.f);
            a.state[(int64_t)row * a.lds + i] = one ? 1.f : 0.f;
            if (one) sb += (double)a.vis_bias[i];
        }
        ais_store_rm(a.rm, a.Bp, row, i, one);
    }
    if (!live) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < g.sp.n_groups) {
            int ones = 0;
            for (int i = g.sp.gs[q] + lane; i < g.sp.ge[q]; i += 64) ones += g.v[(int64_t)row * g.ldv + i] == 1.f ? 1 : 0;
            bad |= wave_sum_all(ones) != 1;
        }
    }
    const bool any_bad = __ballot(bad) != 0ull;
    const double s = wave_sum_all(sb);
    if (lane == 0) a.logw[row] = any_bad ? (double)NAN : s;
}

// Row n owns logw[n M .. n M + M - 1].  out_lme[n] = log((1 / M) sum_m exp(logw)), out_ess[n] = (sum w)^2 / sum w^2 on the weights
// shifted by the row's maximum.  A NaN anywhere in the row makes both outputs of that row NaN, and of that row only.
__global__ __launch_bounds__(64 * ROW_WAVES) void rows_logmeanexp(const double* __restrict__ logw, int N, int M,
                                                                 double* __restrict__ out_lme, double* __restrict__ out_ess) {
    const int lane = wave_lane(), row = wave_row();
    if (row >= N) return;
    const double* x = logw + (int64_t)row * M;
    double mx = -INFINITY;
    bool nan = false;
    for (int m = lane; m < M; m += 64) {
        const double t = x[m];
        nan |= t != t;
        mx = fmax(mx, t);
    }
    mx = wave_max_all(mx);
    const bool any_nan = __ballot(nan) != 0ull;
    const double shift = mx == -INFINITY ? 0.0 : mx;      // a row of zero weights: log mean = -inf, not NaN
    double s1 = 0.0, s2 = 0.0;
    for (int m = lane; m < M; m += 64) {
        const double w = exp(x[m] - shift);
        s1 += w;
        s2 += w * w;
    }
    s1 = wave_sum_all(s1);
    s2 = wave_sum_all(s2);
    if (lane == 0) {
        out_lme[row] = any_nan ? (double)NAN : shift + log(s1 / (double)M);
        out_ess[row] = any_nan ? (double)NAN : s1 * s1 / s2;
    }
}

}  // namespace imdbn
