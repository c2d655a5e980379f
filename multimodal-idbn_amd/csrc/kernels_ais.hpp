// kernels_ais.hpp -- the element-wise half of annealed importance sampling (imdbn_rbm_ais).
//
//   ais_init_v            v_1 = 1[sigmoid(b_A) > U]: fp32 state, single-term K16-blocked operand form, logw = 0
//   ais_weight_sample_h   one pass over the fp32 logits x[M][H] of a temperature: logw[row] += the step's importance-weight increment
//                         (both sums in double), h = 1[sigmoid(beta_k x) > U] as the bf16 form AND the bit plane the down propagation
//                         reads, and the effective visible bias of the transition that follows.  `sample` = 0 is the last
//                         temperature: the weight only, no draw.
//
// One wave per chain (row), four rows per block, rows dealt up to Bp (the padded rows write zeros into the operand forms and touch
// nothing else), so M is free.  Lane l of a row's wave takes the elements l, l + 64, ... in ascending order and the 64 lane sums
// meet in a fixed butterfly: the order of every sum depends on (V, H) only.  Lane 0 owns logw[row]; no atomics, no LDS, no scratch.
#pragma once
#include "kernels_ew.hpp"

namespace imdbn {

constexpr int AIS_ROWS = 4;      // rows (waves) per block

// softplus in double, stable form
__device__ __forceinline__ double ais_softplus(double t) { return fmax(t, 0.0) + log1p(exp(-fabs(t))); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // fixed butterfly order: deterministic, every lane ends with the sum
    return v;
}

struct AisArgs {
    int M, Bp, V, H, Vpad, Hpad;
    const float* vis_bias; const float* base_bias;      // b [V]; b_A [V] (nullable: zeros)
    float* eff_bias; float eff_scale;                   // eff_bias[i] = b_i + eff_scale * b_A,i, written when base_bias is set
    float* state; int64_t lds;                          // 0/1 visible state [M][V] fp32
    const float* x; int64_t ldx;                        // logits c + v W  [M][H] fp32
    float beta_prev, beta;
    int sample; DrawSrc uni;                            // weight step: h is drawn; init: the ("u", V) draw
    bf16_t* rm;                                         // init: vis_rm (ld Vpad); weight step: hid_rm (ld Hpad); K16-blocked, one term
    uint8_t* bits;                                      // weight step: hidden bit plane, byte-major [rup(H, 64) / 8][Bp]
    double* logw;
};

// element (b, k) of the single-term K16-blocked operand form (OperandOut::rm)
__device__ __forceinline__ void ais_store_rm(bf16_t* rm, int Bp, int b, int k, bool one) {
    rm[((int64_t)(k >> 4) * Bp + b) * 16 + (k & 15)] = one ? (bf16_t)0x3F80u : (bf16_t)0u;
}

__device__ __forceinline__ void ais_eff_bias(const AisArgs& a) {
    if (!a.base_bias) return;
    const int n = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.V; i += n) a.eff_bias[i] = a.vis_bias[i] + a.eff_scale * a.base_bias[i];
}

__global__ __launch_bounds__(64 * AIS_ROWS) void ais_init_v(const AisArgs a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * AIS_ROWS + (threadIdx.x >> 6);
    if (row >= a.Bp) return;
    const bool live = row < a.M;
    for (int i = lane; i < a.Vpad; i += 64) {
        bool one = false;
        if (live && i < a.V) {
            const float p = sigmoidf_ref(a.base_bias ? a.base_bias[i] : 0.f);
            one = p > draw_uniform(a.uni, row, i);
            a.state[(int64_t)row * a.lds + i] = one ? 1.f : 0.f;
        }
        ais_store_rm(a.rm, a.Bp, row, i, one);
    }
    if (live && lane == 0) a.logw[row] = 0.0;
}

__global__ __launch_bounds__(64 * AIS_ROWS) void ais_weight_sample_h(const AisArgs a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * AIS_ROWS + (threadIdx.x >> 6);
    if (a.sample) ais_eff_bias(a);
    if (row >= a.Bp) return;
    const bool live = row < a.M;      // wave-uniform
    // ---- visible term: (beta_k - beta_{k-1}) sum_i (b_i - b_A,i) v_i
    double sv = 0.0;
    if (live) {
        const float* v = a.state + (int64_t)row * a.lds;
        for (int i = lane; i < a.V; i += 64) {
            const double db = (double)a.vis_bias[i] - (a.base_bias ? (double)a.base_bias[i] : 0.0);
            sv += db * (double)v[i];
        }
    }
    // ---- hidden term: sum_j softplus(beta_k x_j) - softplus(beta_{k-1} x_j); h_j = 1[sigmoid(beta_k x_j) > U]
    double sh = 0.0;
    const int Hb = (a.H + 63) & ~63;      // whole ballots: the bit plane covers [0, rup(H, 64))
    const OperandOut ob{nullptr, 0, 0, 0, a.Bp, nullptr, 0, 0, 0, a.bits, 0, 0};
    for (int j = lane; j < Hb; j += 64) {
        const bool in = live && j < a.H;
        bool one = false;
        if (in) {
            const float x = a.x[(int64_t)row * a.ldx + j];
            sh += ais_softplus((double)a.beta * (double)x) - ais_softplus((double)a.beta_prev * (double)x);
            if (a.sample) one = sigmoidf_ref(a.beta * x) > draw_uniform(a.uni, row, j);
        }
        if (a.sample) {
            if (j < a.Hpad) ais_store_rm(a.rm, a.Bp, row, j, one);
            store_bits_row(ob, one, j, row, true, 0, 0);
        }
    }
    if (!live) return;
    const double d = ((double)a.beta - (double)a.beta_prev) * wave_sum_f64(sv) + wave_sum_f64(sh);
    if (lane == 0) a.logw[row] += d;
}

}  // namespace imdbn
