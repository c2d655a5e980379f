// kernels_pt.hpp -- the replica-exchange half of parallel tempering (imdbn_rbm_pt_sweep).
//
// R replicas of M chains share one state tensor [R M][V]: replica r owns the rows [r M, (r + 1) M) and samples the tempered marginal
// p_beta(v) ~ exp(beta b.v + S(beta, v)),  S(beta, v) = sum_j softplus(beta x_j(v)),  x(v) = c + v W,  at beta = betas[r].
// A sweep proposes, for every pair (r, r + 1) of one parity and every chain m, to exchange the states u (replica r) and u'
// (replica r + 1) of that chain, and accepts with the Metropolis ratio of the two marginals:
//     Delta = (beta_{r+1} - beta_r) (b.u - b.u') + S(beta_r, u') + S(beta_{r+1}, u) - S(beta_r, u) - S(beta_{r+1}, u'),
//     swap  iff  log(U) < Delta,        U: the ("u", 1) draw at the LOWER replica's row.
//
//   pt_exchange_rows   follows ONE logits-only up propagation over all R M rows (x does not depend on the temperature).  One wave per
//                      (pair, chain), ROW_WAVES per block.  Lane l takes the hidden units l, l + 64, ...: the four softplus sums run
//                      in fp32 over a chunk of PT_JC hidden units (two per lane) and in double across the chunks, as kernels_pll.hpp
//                      sums; b.u - b.u' runs in double over the columns l, l + 64, ...; the 64 lane values meet in the fixed
//                      butterfly (wave_sum_all).  Lane 0 reads the draw and decides, every lane learns the decision and the wave
//                      swaps the two V-float rows.  Lane 0 counts the proposal (and the acceptance) of its pair: integer atomics.
//
// Every sum has an order fixed by (V, H); no floating-point atomics, no LDS, no scratch.  A row outside every pair of the sweep's
// parity is neither read nor written.
#pragma once
#include "kernels_ais.hpp"

namespace imdbn {

constexpr int PT_JC = 128;                       // hidden units per fp32 chunk (kernels_pll.hpp: PLL_JC)
constexpr int PT_RMAX = 64;                      // replicas of one call: their temperatures travel in the kernel arguments

struct PtArgs {
    float* state; int64_t lds;                   // [R M][V] fp32 0/1, in place
    const float* x; int64_t ldx;                 // logits c + v W of every row, [R M][H]
    const float* vis_bias;
    int R, M, V, H;
    int parity, n_pairs;                         // pair p is (parity + 2 p, parity + 2 p + 1)
    DrawSrc uni;                                 // ("u", 1) over all R M rows
    unsigned long long* swap_try; unsigned long long* swap_acc;      // [R - 1], added to
    float beta[PT_RMAX];
};

// softplus in fp32, stable form
__device__ __forceinline__ float pt_softplus(float t) { return fmaxf(t, 0.f) + log1pf(expf(-fabsf(t))); }

__global__ __launch_bounds__(64 * ROW_WAVES) void pt_exchange_rows(const PtArgs a) {
    const int lane = wave_lane(), w = wave_row();
    if (w >= a.n_pairs * a.M) return;      // wave-uniform
    const int p = w / a.M, m = w - p * a.M;
    const int r = a.parity + 2 * p;        // r + 1 < R by the host's n_pairs
    const int64_t row_lo = (int64_t)r * a.M + m, row_hi = row_lo + a.M;
    const float b_lo = a.beta[r], b_hi = a.beta[r + 1];
    const float* x_lo = a.x + row_lo * a.ldx;
    const float* x_hi = a.x + row_hi * a.ldx;
    // S(beta_r, u), S(beta_{r+1}, u), S(beta_r, u'), S(beta_{r+1}, u')
    double s_ll = 0.0, s_hl = 0.0, s_lh = 0.0, s_hh = 0.0;
    for (int j0 = 0; j0 < a.H; j0 += PT_JC) {
        float c_ll = 0.f, c_hl = 0.f, c_lh = 0.f, c_hh = 0.f;
#pragma unroll
        for (int q = 0; q < PT_JC / 64; ++q) {
            const int j = j0 + 64 * q + lane;
            if (j < a.H) {
                const float xl = x_lo[j], xh = x_hi[j];
                c_ll += pt_softplus(b_lo * xl); c_hl += pt_softplus(b_hi * xl);
                c_lh += pt_softplus(b_lo * xh); c_hh += pt_softplus(b_hi * xh);
            }
        }
        s_ll += (double)c_ll; s_hl += (double)c_hl; s_lh += (double)c_lh; s_hh += (double)c_hh;
    }
    s_ll = wave_sum_all(s_ll); s_hl = wave_sum_all(s_hl); s_lh = wave_sum_all(s_lh); s_hh = wave_sum_all(s_hh);
    // b.u - b.u'
    float* u_lo = a.state + row_lo * a.lds;
    float* u_hi = a.state + row_hi * a.lds;
    double sb = 0.0;
    for (int i = lane; i < a.V; i += 64) sb += (double)a.vis_bias[i] * ((double)u_lo[i] - (double)u_hi[i]);
    sb = wave_sum_all(sb);
    const double delta = ((double)b_hi - (double)b_lo) * sb + s_lh + s_hl - s_ll - s_hh;
    int acc = 0;
    if (lane == 0) {
        DrawSrc us = a.uni; us.N = 1;
        acc = log((double)draw_uniform(us, (int)row_lo, 0)) < delta ? 1 : 0;
        atomicAdd(a.swap_try + r, 1ull);
        if (acc) atomicAdd(a.swap_acc + r, 1ull);
    }
    acc = __shfl(acc, 0, 64);
    if (!acc) return;                      // wave-uniform
    for (int i = lane; i < a.V; i += 64) {
        const float lo = u_lo[i], hi = u_hi[i];
        u_lo[i] = hi; u_hi[i] = lo;
    }
}

}  // namespace imdbn
