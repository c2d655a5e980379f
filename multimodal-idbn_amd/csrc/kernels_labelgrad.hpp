// kernels_labelgrad.hpp -- the exact gradient of log p(y | z) under the joint RBM (imdbn_rbm_label_step).
//
// With base = hid_bias + z W[:Dz], U = W[Dz:Dz+K], o_kj = base_j + U_kj, s_kj = sigmoid(o_kj) and the class values a_k of
// kernels_joint.hpp:  p_k = exp(a_k - logsumexp a),  r_k = 1[k = t] - p_k,  and
//   d logp / d U_kj = r_k s_kj      d logp / d b_y,k = r_k      d logp / d c_j = s_tj - sum_k p_k s_kj      d logp / d W_z = z^T (that)
//
//   label_grad_rows     one wave per row, ROW_WAVES rows per block, as joint_label_loglik and with its pass 1 (label_class_values,
//                       label_logsumexp: the same bits).  Pass 2 writes logp (double), r [N][K] (the double difference rounded to
//                       fp32) and, lanes over j, hpos_j = s_tj and hneg_j = sum_k p_k s_kj: fp32 logits and sigmoids, p_k rounded
//                       to fp32, one fp32 fma chain over k in index order.  A row whose label is outside [0, K) gets logp = NaN
//                       and zeros in r, hpos and hneg: it adds exact zeros to every sum below, and nothing is read through it.
//   label_grad_update   one thread per (k, j), and K more for the label biases.  Recomputes s_nkj from base and the OLD U_kj (the
//                       same fp32 expression, so the same bits as above), sums r_nk s_nkj over n in index order in one fp32 fma
//                       chain, and applies rbm.py:212-224 without the sparsity term to U, W_m[Dz:], b_y and vb_m[Dz:].  Each
//                       thread reads and writes its own parameter only.
//
//   label_backprop_rows label_grad_rows (one row function serves both: the same bits in logp, r, hpos and hneg) that also leaves
//                       e_j = hpos_j - hneg_j (one fp32 subtraction; an exact zero row for an invalid label) -- the error
//                       imdbn_rbm_label_backprop_step sends down through W[:Dz] -- and pred = argmax_k a_k over the
//                       double class values of pass 1 (the lowest k on a tie, whatever gt holds).
//
// The code side (W[:Dz], hid_bias, the momentum of b_z) is the update kernel's, from z, hpos and hneg (engine.hip).  No atomics,
// no LDS; every sum has an order fixed by (Dz, K, H, N).
#pragma once
#include "kernels_joint.hpp"

namespace imdbn {

struct LabelGradArgs {
    JointArgs j;                           // pass 1; j.joint / j.marg are unused
    double* logp;                          // [N]
    float* r;                              // [N][K]
    float* hpos; float* hneg;              // [N][H]
};

struct LabelBackpropArgs {
    LabelGradArgs g;
    int32_t* pred;                         // [N], nullable
    float* e;                              // [N][H]
};

// index of the first maximum of a row of K doubles in the label slots, the same in every lane: the larger value first, the lower
// index on ties, NaN never wins (-1 for a row in which nothing wins)
__device__ __forceinline__ int slots_argmax_f64(const double (&v)[4], int l, int K) {
    double best = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = l + 64 * q;
        if (c < K && (v[q] > best || (v[q] == best && c < bi))) { best = v[q]; bi = c; }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const double w = __shfl_xor(best, o); const int j = __shfl_xor(bi, o);
        if (w > best || (w == best && j < bi)) { best = w; bi = j; }
    }
    return bi < K ? bi : -1;
}

// One row of label_grad_rows / label_backprop_rows.  BP adds pred and e and changes nothing else: one source, the same bits.
template <bool BP>
__device__ __forceinline__ void label_grad_row(const LabelGradArgs& g, int32_t* pred, float* e_out) {
    const JointArgs& a = g.j;
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.N) return;      // wave-uniform
    double val[4];
    label_class_values(a, row, lane, val);
    const double marg = label_logsumexp(val, a.K);
    const int t = a.gt[row];
    const bool ok = t >= 0 && t < a.K;      // wave-uniform
    const double at = slots_pick(val, t);
    if (lane == 0) g.logp[row] = ok ? at - marg : (double)NAN;
    if (BP && pred) {
        const int best = slots_argmax_f64(val, lane, a.K);
        if (lane == 0) pred[row] = best;
    }
    float pf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int k = s * 64 + lane;
        const double p = exp(val[s] - marg);      // an empty slot holds -inf: 0
        pf[s] = (float)p;
        if (k < a.K) g.r[(int64_t)row * a.K + k] = ok ? (float)((k == t ? 1.0 : 0.0) - p) : 0.f;
    }
    const float* base = a.base + (int64_t)row * a.ldb;
    float* hp = g.hpos + (int64_t)row * a.H;
    float* hn = g.hneg + (int64_t)row * a.H;
    float* er = BP ? e_out + (int64_t)row * a.H : nullptr;
    if (!ok) {
        for (int j = lane; j < a.H; j += 64) {
            hp[j] = 0.f; hn[j] = 0.f;
            if (BP) er[j] = 0.f;
        }
        return;
    }
    for (int j0 = 0; j0 < a.H; j0 += 64) {      // every lane walks k: slots_pick is a wave-wide shuffle
        const int j = j0 + lane;
        const bool in = j < a.H;
        const float b = in ? base[j] : 0.f;
        float pos = 0.f, neg = 0.f;
        for (int k = 0; k < a.K; ++k) {
            const float pk = slots_pick(pf, k);
            const float s = sigmoidf_ref(b + (in ? a.Wy[(int64_t)k * a.ldw + j] : 0.f));
            neg = fmaf(pk, s, neg);
            if (k == t) pos = s;
        }
        if (in) {
            hp[j] = pos; hn[j] = neg;
            if (BP) er[j] = pos - neg;
        }
    }
}

__global__ __launch_bounds__(64 * ROW_WAVES) void label_grad_rows(const LabelGradArgs g) { label_grad_row<false>(g, nullptr, nullptr); }

__global__ __launch_bounds__(64 * ROW_WAVES) void label_backprop_rows(const LabelBackpropArgs b) { label_grad_row<true>(b.g, b.pred, b.e); }

struct LabelUpdateArgs {
    const float* base; int64_t ldb;        // [N][H], as pass 1 read it
    const float* r;                        // [N][K]
    float* U; float* Um; int64_t ldw;      // label rows of W and of W_m, [K][H]
    float* by; float* bym;                 // label entries of vis_bias and of vb_m, [K]
    int N, K, H;
    float lr, mom, wd, n;
};

__global__ __launch_bounds__(256) void label_grad_update(const LabelUpdateArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nw = (int64_t)a.K * a.H;
    if (idx < nw) {
        const int k = (int)(idx / a.H), j = (int)(idx % a.H);
        const int64_t at = (int64_t)k * a.ldw + j;
        const float w0 = a.U[at];
        float d = 0.f;
        for (int n = 0; n < a.N; ++n) d = fmaf(a.r[(int64_t)n * a.K + k], sigmoidf_ref(a.base[(int64_t)n * a.ldb + j] + w0), d);
        const float gr = d / a.n - a.wd * w0;                                  // rbm.py:212
        float m = a.Um[at] * a.mom;
        m = m + a.lr * gr;
        a.Um[at] = m;
        a.U[at] = w0 + m;
    } else if (idx < nw + a.K) {
        const int k = (int)(idx - nw);
        float d = 0.f;
        for (int n = 0; n < a.N; ++n) d = d + a.r[(int64_t)n * a.K + k];
        float m = a.bym[k] * a.mom;
        m = m + (a.lr * d) / a.n;                                              // rbm.py:223
        a.bym[k] = m;
        a.by[k] = a.by[k] + m;
    }
}

}  // namespace imdbn
