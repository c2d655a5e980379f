// kernels_gauss_ais.hpp -- the element-wise half of annealed importance sampling over Gaussian visibles (imdbn_rbm_gauss_ais,
// DESIGN §30) and of its reverse direction (imdbn_rbm_gauss_reverse_ais).  With z the log-variance, u = v e^{-z}, x = c + u W and q_X(v) = sum_i (v_i - b_X,i)^2 / (2 sigma_i^2), the
// intermediate distribution is p*_beta(v) = exp(-(1 - beta) q_A(v) - beta q_B(v)) prod_j (1 + e^{beta x_j}): the base-rate model A
// has the RBM's variances, no weights and the visible bias b_A.
//
//   gauss_ais_visible            the visible half of a transition, fused: from the fp32 mean m = b + h W^T the down propagation left
//                                (logits_only) and the ("n", V) draw,  v = ((1 - beta) b_A + beta m) + e^{z/2} n  in fp32, in that
//                                order; writes the fp32 state v, u = v e^{-z} for the next up propagation, and the row's visible
//                                weight term  t_v = sum_i (b_i - b_A,i) e^{-z_i} (v_i - (b_i + b_A,i) / 2) = q_A(v) - q_B(v)  in double.
//                                With a null mean and beta = 0 it is the start: v_1 = b_A + e^{z/2} n, and logw = 0.
//   gauss_ais_weight_sample_h    one pass over the fp32 logits x[M][H] of the current state, for the forward call and the reverse one.
//                                With Delta_k = (beta_k - beta_{k-1}) t_v + sum_j [softplus(beta_k x_j) - softplus(beta_{k-1} x_j)]
//                                (both sums in double, one expression, as ais_weight_sample_h): logw[row] += Delta_k forward,
//                                -= Delta_k in reverse, += sum_j softplus(x_j) in reverse's `first` form (with gauss_rais_load_v that
//                                is -F of the start row).  With `sample`, h = 1[sigmoid(beta_draw x) > U] -- the hidden half of the
//                                transition that FOLLOWS: beta_k forward, beta_{k-1} in reverse, beta_K in the first form -- as the
//                                bf16 form AND the bit plane the down propagation reads.  `sample` = 0 is the last step: the weight
//                                only, no draw.
//   gauss_rais_load_v            the reverse call's start: from the caller's row v the fp32 state, u = v e^{-z}, t_v(v) and
//                                logw = -q_B(v) in double; a row holding a non-finite element gets logw = NaN instead (wave-uniform),
//                                and every later step only adds to it, so the row stays NaN.
//
// One wave per chain (row), ROW_WAVES rows per block, rows dealt up to Bp (the padded rows write zeros into the operand forms and
// touch nothing else), so M is free.  Lane l of a row's wave takes the elements l, l + 64, ... in ascending order and the 64 lane
// sums meet in the fixed butterfly (wave_sum_all): the order of every sum depends on (V, H) only.  Lane 0 owns logw[row] and
// t_v[row]; no atomics, no LDS, no scratch.  Every element's loads come before its stores, from addresses inside the row.
#pragma once
#include "kernels_ais.hpp"

namespace imdbn {

struct GaussAisArgs {
    int M, Bp, V, H, Hpad;
    const float* vis_bias; const float* base_bias;      // b [V]; b_A [V] (the host passes b itself for a null base_vis_bias)
    const float* logvar;                                // z [V]
    const float* mean; int64_t ldm;                     // visible half: m = b + h W^T [M][V] fp32 (nullable: the start, with beta = 0)
    DrawSrc nz;                                         // visible half: the ("n", V) draw
    float* state; int64_t lds;                          // visible state [M][V] fp32
    float* u; int64_t ldu;                              // u = v e^{-z} [M][V] fp32
    double* tv;                                         // the rows' visible weight terms [M]
    const float* x; int64_t ldx;                        // weight step: logits c + u W  [M][H] fp32
    float beta_prev, beta;                              // weight step: its k; visible half: beta of the transition
    int first, reverse;                                 // weight step: sum_j softplus(x_j) instead of Delta_k; -Delta_k instead of +
    float beta_draw;                                    // weight step: temperature of the draw (forward: beta)
    int sample; DrawSrc uni;                            // weight step: h is drawn
    bf16_t* rm; uint8_t* bits;                          // weight step: hid_rm (ld Hpad, K16-blocked, one term); hidden bit plane
    double* logw;
};

__global__ __launch_bounds__(64 * ROW_WAVES) void gauss_ais_visible(const GaussAisArgs a) {
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.M) return;               // wave-uniform; the operand forms of u are prep_operand's, padding rows included
    const float* m = a.mean ? a.mean + (int64_t)row * a.ldm : nullptr;
    float* vs = a.state + (int64_t)row * a.lds;
    float* us = a.u + (int64_t)row * a.ldu;
    const float one_minus = 1.0f - a.beta;
    double sv = 0.0;
    for (int i = lane; i < a.V; i += 64) {
        const float b = a.vis_bias[i], bA = a.base_bias[i], z = a.logvar[i];
        const float mi = m ? m[i] : 0.f;
        const float n = draw_normal(a.nz, row, i);
        const float v = (one_minus * bA + a.beta * mi) + expf(0.5f * z) * n;
        const double db = (double)b - (double)bA;
        sv += (db * exp(-(double)z)) * ((double)v - 0.5 * ((double)b + (double)bA));
        vs[i] = v;
        us[i] = v * expf(-z);
    }
    const double tv = wave_sum_all(sv);
    if (lane == 0) {
        a.tv[row] = tv;
        if (!m) a.logw[row] = 0.0;
    }
}

__global__ __launch_bounds__(64 * ROW_WAVES) void gauss_ais_weight_sample_h(const GaussAisArgs a) {
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.Bp) return;
    const bool live = row < a.M;          // wave-uniform
    // ---- hidden term: sum_j softplus(beta_k x_j) - softplus(beta_{k-1} x_j), or sum_j softplus(x_j); h_j = 1[sigmoid(beta_draw x_j) > U]
    double sh = 0.0;
    const int Hb = (a.H + 63) & ~63;      // whole ballots: the bit plane covers [0, rup(H, 64))
    for (int j = lane; j < Hb; j += 64) {
        const bool in = live && j < a.H;
        bool one = false;
        if (in) {
            const float x = a.x[(int64_t)row * a.ldx + j];
            sh += a.first ? ais_softplus((double)x)
                          : ais_softplus((double)a.beta * (double)x) - ais_softplus((double)a.beta_prev * (double)x);
            if (a.sample) one = sigmoidf_ref(a.beta_draw * x) > draw_uniform(a.uni, row, j);
        }
        if (a.sample) ais_store_hidden(a.rm, a.bits, a.Bp, a.Hpad, row, j, one);
    }
    if (!live) return;
    const double th = wave_sum_all(sh);
    if (lane == 0) {
        const double delta = ((double)a.beta - (double)a.beta_prev) * a.tv[row] + th;
        a.logw[row] += a.first ? th : (a.reverse ? -delta : delta);
    }
}

struct GaussRaisLoadArgs {
    GaussAisArgs a;                                     // M rows; the biases, logvar; state / lds; u / ldu; tv; logw
    const float* v; int64_t ldv;                        // the caller's start rows [M][V]
};

__global__ __launch_bounds__(64 * ROW_WAVES) void gauss_rais_load_v(const GaussRaisLoadArgs g) {
    const GaussAisArgs& a = g.a;
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.M) return;               // wave-uniform; the operand forms of u are prep_operand's, padding rows included
    const float* x = g.v + (int64_t)row * g.ldv;
    float* vs = a.state + (int64_t)row * a.lds;
    float* us = a.u + (int64_t)row * a.ldu;
    double sv = 0.0, sq = 0.0;
    bool bad = false;
    for (int i = lane; i < a.V; i += 64) {
        const float b = a.vis_bias[i], bA = a.base_bias[i], z = a.logvar[i];
        const float v = x[i];
        bad |= !(fabsf(v) < INFINITY);    // inf or NaN
        const double ez = exp(-(double)z), d = (double)v - (double)b;
        const double db = (double)b - (double)bA;
        sv += (db * ez) * ((double)v - 0.5 * ((double)b + (double)bA));
        sq += (d * d) * (0.5 * ez);
        vs[i] = v;
        us[i] = v * expf(-z);
    }
    const bool any_bad = __ballot(bad) != 0ull;
    const double tv = wave_sum_all(sv), q = wave_sum_all(sq);
    if (lane == 0) {
        a.tv[row] = tv;
        a.logw[row] = any_bad ? (double)NAN : -q;
    }
}

}  // namespace imdbn
