// kernels_joint.hpp -- the label side of the joint RBM's log-likelihood (imdbn_rbm_label_loglik).
//
//   joint_label_loglik    for every row, from base = hid_bias + z W[:Dz] (the logits of an up propagation on the first Dz weight rows):
//                           a_k   = z . b_z + b_k + sum_j softplus(base_j + W[Dz + k][j])      = -F([z, e_k]),  k = 0 .. K-1
//                           joint = a_gt                                                        (NaN when gt is outside [0, K))
//                           marg  = logsumexp_k a_k                                             = log sum_y exp(-F([z, y]))
//                         all in double, the fp32 operands widened.
//
// One wave per row, four rows per block.  Lane l takes j = l, l + 64, ... in ascending order and the 64 lane sums meet in the fixed
// butterfly of wave_sum_all, so every sum is a function of (Dz, K, H) only and a row gives the same bits alone and inside a batch.
// The K class values are computed in index order and parked in the label slots of kernels_rows.hpp (in double, an empty slot holds
// -inf); the logsumexp is shifted by their maximum and its K terms are added in index order.  No atomics, no LDS, no scratch.
// label_class_values / label_logsumexp are that row pass as device functions: label_grad_rows (kernels_labelgrad.hpp) calls the same two.
#pragma once
#include "kernels_ais.hpp"

namespace imdbn {

struct JointArgs {
    const float* base; int64_t ldb;        // [N][H] fp32
    const float* z; int64_t ldz;           // [N][Dz] fp32
    const float* bz; const float* by;      // visible biases of the code columns [Dz] and of the label columns [K]
    const float* Wy; int64_t ldw;          // label rows of the weights [K][H]
    const int32_t* gt;                     // [N]
    int N, Dz, K, H;
    double* joint; double* marg;           // [N]
};

// Pass 1 of a row, shared with label_grad_rows (kernels_labelgrad.hpp) so that both calls give the same bits: the K class values
// into the label slots `val`, and their logsumexp.
__device__ __forceinline__ void label_class_values(const JointArgs& a, int row, int lane, double (&val)[4]) {
    const float* z = a.z + (int64_t)row * a.ldz;
    const float* base = a.base + (int64_t)row * a.ldb;
    double zb = 0.0;
    for (int i = lane; i < a.Dz; i += 64) zb += (double)z[i] * (double)a.bz[i];
    zb = wave_sum_all(zb);
#pragma unroll
    for (int s = 0; s < 4; ++s) val[s] = -INFINITY;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        for (int kk = 0; kk < 64; ++kk) {
            const int k = s * 64 + kk;
            if (k >= a.K) break;
            const float* w = a.Wy + (int64_t)k * a.ldw;
            double sh = 0.0;
            for (int j = lane; j < a.H; j += 64) sh += ais_softplus((double)base[j] + (double)w[j]);
            const double ak = zb + (double)a.by[k] + wave_sum_all(sh);
            if (lane == kk) val[s] = ak;
        }
    }
}

__device__ __forceinline__ double label_logsumexp(const double (&val)[4], int K) {
    const double mx = wave_max_all(fmax(fmax(val[0], val[1]), fmax(val[2], val[3])));
    double sum = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const double e = exp(val[s] - mx);      // an empty slot holds -inf: 0
        for (int kk = 0; kk < 64; ++kk) {
            if (s * 64 + kk >= K) break;
            sum += __shfl(e, kk, 64);
        }
    }
    return mx + log(sum);
}

__global__ __launch_bounds__(64 * ROW_WAVES) void joint_label_loglik(const JointArgs a) {
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.N) return;      // wave-uniform
    double val[4];
    label_class_values(a, row, lane, val);
    const double marg = label_logsumexp(val, a.K);
    const int g = a.gt[row];
    const double at = slots_pick(val, g);
    if (lane == 0) {
        a.joint[row] = (g >= 0 && g < a.K) ? at : (double)NAN;
        a.marg[row] = marg;
    }
}

}  // namespace imdbn
