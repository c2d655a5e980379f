// kernels_ais.hpp -- the element-wise half of annealed importance sampling (imdbn_rbm_ais).
//
//   ais_init_v_groups     v_1 from the base-rate model: fp32 state, single-term K16-blocked operand form, logw = 0.  Bernoulli
//                         columns: 1[sigmoid(b_A) > U].  Softmax groups (imdbn_rbm_ais_groups; none: n_groups = 0): per
//                         row one category per group from softmax(b_A[group]) -- the arithmetic of finish_groups: fp32 softmax,
//                         clamp(p, 1e-8, 1), inverse CDF in column order -- or from the replay tape.
//   ais_weight_sample_h   one pass over the fp32 logits x[M][H] of the current state, for the forward call and the reverse one
//                         (imdbn_rbm_reverse_ais).  With Delta_k the step's importance-weight increment (both sums in
//                         double): logw[row] += Delta_k forward, -= Delta_k in reverse, += sum_j softplus(x_j) in reverse's `first`
//                         form (with rais_load_v that is -F of the start state).  With `sample`, h = 1[sigmoid(beta_draw x) > U] --
//                         the hidden half of the transition that FOLLOWS: beta_k forward, beta_{k-1} in reverse, beta_K in the
//                         first form -- as the bf16 form AND the bit plane the down propagation reads, and that transition's
//                         effective visible bias.  `sample` = 0 is the last step: the weight only, no draw.
//
// One wave per chain (row), four rows per block, rows dealt up to Bp (the padded rows write zeros into the operand forms and touch
// nothing else), so M is free.  Lane l of a row's wave takes the elements l, l + 64, ... in ascending order and the 64 lane sums
// meet in the fixed butterfly (wave_sum_all): the order of every sum depends on (V, H) only.  Lane 0 owns logw[row]; no atomics, no
// LDS, no scratch.
#pragma once
#include "kernels_ew.hpp"
#include "kernels_rows.hpp"

namespace imdbn {

// softplus in double, stable form
__device__ __forceinline__ double ais_softplus(double t) { return fmax(t, 0.0) + log1p(exp(-fabs(t))); }

struct AisArgs {
    int M, Bp, V, H, Vpad, Hpad;
    const float* vis_bias; const float* base_bias;      // b [V]; b_A [V] (nullable: zeros)
    float* eff_bias; float eff_scale;                   // eff_bias[i] = b_i + eff_scale * b_A,i, written when base_bias is set
    float* state; int64_t lds;                          // 0/1 visible state [M][V] fp32
    const float* x; int64_t ldx;                        // logits c + v W  [M][H] fp32
    float beta_prev, beta;                              // the step's k: Delta_k = log p*_k(v) - log p*_{k-1}(v)
    int first, reverse;                                 // weight step: sum_j softplus(x_j) instead of Delta_k; -Delta_k instead of +
    float beta_draw;                                    // temperature of the draw (forward: beta)
    int sample; DrawSrc uni;                            // weight step: h is drawn; init: the ("u", V) draw
    bf16_t* rm;                                         // init: vis_rm (ld Vpad); weight step: hid_rm (ld Hpad); K16-blocked, one term
    uint8_t* bits;                                      // weight step: hidden bit plane, byte-major [rup(H, 64) / 8][Bp]
    double* logw;
};

// element (b, k) of the single-term K16-blocked operand form (OperandOut::rm)
__device__ __forceinline__ void ais_store_rm(bf16_t* rm, int Bp, int b, int k, bool one) {
    rm[((int64_t)(k >> 4) * Bp + b) * 16 + (k & 15)] = one ? (bf16_t)0x3F80u : (bf16_t)0u;
}

// hidden unit k of row b in both forms the down propagation reads: the operand form (columns below Hpad) and the bit plane, whose
// bytes come from a ballot -- every lane of the wave calls, k running over whole groups of 64 columns
__device__ __forceinline__ void ais_store_hidden(bf16_t* rm, uint8_t* bits, int Bp, int Hpad, int b, int k, bool one) {
    if (k < Hpad) ais_store_rm(rm, Bp, b, k, one);
    const OperandOut ob{nullptr, 0, 0, 0, Bp, nullptr, 0, 0, 0, bits, 0, 0};
    store_bits_row(ob, one, k, b, true, 0, 0);
}

__device__ __forceinline__ void ais_eff_bias(const AisArgs& a) {
    if (!a.base_bias) return;
    const int n = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.V; i += n) a.eff_bias[i] = a.vis_bias[i] + a.eff_scale * a.base_bias[i];
}

// the softmax groups [gs[q], ge[q]) of a visible layer
struct GroupSpans {
    int n_groups; int gs[4]; int ge[4];            // only ever indexed with compile-time constants (see FinishArgs)
};

// The initial state with one categorical per softmax group.  Lane 0 of the row's wave walks a group's logits (the same for every
// row: b_A; a one-time cost of the call, <= 4 groups of <= 256 columns), every lane then learns the picks and writes its columns.
struct AisGroupsArgs {
    AisArgs a;
    GroupSpans sp;
    const int32_t* cat_tape; DrawSrc cat_uni;      // categorical source for group g: cat_tape + g*M / draw+g
};

__device__ __forceinline__ int ais_pick_category(const AisGroupsArgs& g, int q, int s, int e, int row) {
    const AisArgs& a = g.a;
    if (g.cat_tape) return g.cat_tape[(int64_t)q * a.M + row];
    const int wd = e - s;
    float mx = -INFINITY;
    for (int j = 0; j < wd; ++j) mx = fmaxf(mx, a.base_bias ? a.base_bias[s + j] : 0.f);
    float sum = 0.f;
    for (int j = 0; j < wd; ++j) sum += expf((a.base_bias ? a.base_bias[s + j] : 0.f) - mx);
    DrawSrc cs = g.cat_uni; cs.draw += q; cs.N = 1;
    const float thr = draw_uniform(cs, row, 0);
    float tot = 0.f;
    int idx = -1;
    for (int pass = 0; pass < 2; ++pass) {
        float acc = 0.f;
        const float target = thr * tot;
        for (int j = 0; j < wd; ++j) {
            const float t = expf((a.base_bias ? a.base_bias[s + j] : 0.f) - mx) / sum;
            acc += fminf(fmaxf(t, 1e-8f), 1.0f);
            if (pass == 1 && acc > target) { idx = j; break; }
        }
        if (pass == 0) tot = acc; else if (idx < 0) idx = wd - 1;
    }
    return idx;
}

__global__ __launch_bounds__(64 * ROW_WAVES) void ais_init_v_groups(const AisGroupsArgs g) {
    const AisArgs& a = g.a;
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.Bp) return;
    const bool live = row < a.M;      // wave-uniform
    int pick[4] = {-1, -1, -1, -1};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < g.sp.n_groups && live) {
            int p = 0;
            if (lane == 0) p = ais_pick_category(g, q, g.sp.gs[q], g.sp.ge[q], row);
            pick[q] = __shfl(p, 0, 64);
        }
    }
    for (int i = lane; i < a.Vpad; i += 64) {
        bool one = false;
        if (live && i < a.V) {
            bool grp = false;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < g.sp.n_groups && i >= g.sp.gs[q] && i < g.sp.ge[q]) { grp = true; one = (i - g.sp.gs[q]) == pick[q]; }
            if (!grp) {
                const float p = sigmoidf_ref(a.base_bias ? a.base_bias[i] : 0.f);
                one = p > draw_uniform(a.uni, row, i);
            }
            a.state[(int64_t)row * a.lds + i] = one ? 1.f : 0.f;
        }
        ais_store_rm(a.rm, a.Bp, row, i, one);
    }
    if (live && lane == 0) a.logw[row] = 0.0;
}

__global__ __launch_bounds__(64 * ROW_WAVES) void ais_weight_sample_h(const AisArgs a) {
    const int lane = wave_lane(), row = wave_row();
    if (a.sample) ais_eff_bias(a);
    if (row >= a.Bp) return;
    const bool live = row < a.M;      // wave-uniform
    // ---- visible term of Delta_k: (beta_k - beta_{k-1}) sum_i (b_i - b_A,i) v_i
    double sv = 0.0;
    if (live && !a.first) {
        const float* v = a.state + (int64_t)row * a.lds;
        for (int i = lane; i < a.V; i += 64) {
            const double db = (double)a.vis_bias[i] - (a.base_bias ? (double)a.base_bias[i] : 0.0);
            sv += db * (double)v[i];
        }
    }
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
    const double tv = wave_sum_all(sv), th = wave_sum_all(sh);
    const double delta = ((double)a.beta - (double)a.beta_prev) * tv + th;
    if (lane == 0) a.logw[row] += a.first ? th : (a.reverse ? -delta : delta);
}

}  // namespace imdbn
