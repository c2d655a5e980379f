// kernels_gauss_backprop.hpp -- the element-wise half of one back-propagation step through a Gaussian visible layer
// (imdbn_rbm_gauss_backprop_step).
//
// The layer in its two roles, with the log-variance z (sigma_i^2 = e^{z_i}) and n batch rows:
//   output layer (down pair x_h):  m = b + x_h W^T (the logits-only down route),  e_0 = (v - m) e^{-z},
//       gW = e_0^T x_h / n,  gb = colsum(e_0) / n,  gzeta_i = e^{-z_i} sum_b (v_bi - m_bi)^2 / (2 n) - 1/2
//   input layer (up pair e_h):     u = v e^{-z},  gW = u^T e_h / n,  gc = colsum(e_h) / n,  gz_i = -(r_i - t_i) / n
//       r_i = sum_j W_ij S_ij over the statistics S of the weight pass (gauss_apply), t_i = sum_b e_0,bi (m_bi - b_i) the share of
//       the down pair in r_i when both pairs are present (0 otherwise)
//
//   gauss_bp_rows     grid (ceil(V / 256), Bp / 8), 256 threads: the mapping of gauss_rows and backprop_rows, a thread owns one column
//                     and 8 consecutive batch rows.  One pass over v (and m): e_0 row-major (the operand of the error propagation) and
//                     as transposed three-term planes (rows >= B as zeros: the update kernel reads whole 64-row chunks, which is why
//                     the grid covers Bp rows), u row-major, the 8-row column partials of e_0, (v - m)^2 and e_0 (m - b), the block's
//                     partials of the two loss sums (and of sum z, block row 0), and with one pair only the all-zero planes of the
//                     other visible slot.
//   gauss_bp_finish   one small launch: sums the partials in index order, updates the one or two biases and logvar (clamped), and
//                     reduces the two loss figures.
//
// No atomics; every sum has an order fixed by (V, H, B) and the grid.  All loads first, from clamped addresses; stores stay inside
// [B][V] (the planes inside [V][Bp]).
#pragma once
#include "kernels_gauss.hpp"
#include "kernels_backprop.hpp"

namespace imdbn {

struct GaussBpRowsArgs {
    int B, Bp, V;
    const float* v; int64_t ldv;                 // the data [B][V]
    const float* m; int64_t ldm;                 // the decoder's mean [B][V]; null: no down pair
    const float* bias; const float* logvar;
    float* e0;                                   // nullable: e_0 row-major, pitch V
    bf16_t* tr_e0; bf16_t* tr_zero; int terms;   // nullable: planes of e_0 / all-zero planes, term stride V Bp
    float* u;                                    // nullable: u row-major, pitch V
    float* part_e0; float* part_q; float* part_t;      // nullable: [Bp / 8][V]
    float* loss_part;                            // nullable: [3][gridDim.y gridDim.x]: sum (v - m)^2 e^{-z}, sum (v - m)^2, and the
                                                 // block's sum of z over its columns (block row 0 only, zeros elsewhere)
};

__global__ __launch_bounds__(256) void gauss_bp_rows(const GaussBpRowsArgs a) {
    __shared__ float sh[3][256];
    const int tid = threadIdx.x, col = blockIdx.x * 256 + tid, b0 = blockIdx.y * GAUSS_RPT;
    const bool cok = col < a.V;
    const int cc = min(col, a.V - 1);
    const float z = a.logvar[cc], bias = a.bias[cc];
    float v[GAUSS_RPT], m[GAUSS_RPT];
#pragma unroll
    for (int i = 0; i < GAUSS_RPT; ++i) {        // all loads first, from clamped addresses
        const int bc = min(b0 + i, a.B - 1);
        v[i] = a.v[(int64_t)bc * a.ldv + cc];
        m[i] = a.m ? a.m[(int64_t)bc * a.ldm + cc] : 0.f;
    }
    const float iv = expf(-z);
    float e[GAUSS_RPT], ce = 0.f, q = 0.f, t = 0.f;
#pragma unroll
    for (int i = 0; i < GAUSS_RPT; ++i) {
        const int b = b0 + i;
        const bool ok = cok && b < a.B;
        const float dl = v[i] - m[i];
        const float e0 = dl * iv;
        e[i] = ok ? e0 : 0.f;
        if (!ok) continue;
        if (a.e0) a.e0[(int64_t)b * a.V + col] = e0;
        if (a.u) a.u[(int64_t)b * a.V + col] = v[i] * iv;
        ce += e0;
        q += dl * dl;
        t += e0 * (m[i] - bias);
    }
    OperandOut o{};
    o.Bp = a.Bp; o.tr_ts = (int64_t)a.V * a.Bp; o.tr_terms = a.terms; o.tr_negate = 0;
    if (a.tr_e0) {
        o.tr = a.tr_e0;
        store_forms<GAUSS_RPT>(o, e, false, true, b0, col, a.V, a.Bp);
    }
    if (a.tr_zero) {
        const float zr[GAUSS_RPT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        o.tr = a.tr_zero;
        store_forms<GAUSS_RPT>(o, zr, false, true, b0, col, a.V, a.Bp);
    }
    if (cok && a.part_e0) a.part_e0[(int64_t)blockIdx.y * a.V + col] = ce;
    if (cok && a.part_q) a.part_q[(int64_t)blockIdx.y * a.V + col] = q;
    if (cok && a.part_t) a.part_t[(int64_t)blockIdx.y * a.V + col] = t;
    if (a.loss_part) {                           // block-uniform
        sh[0][tid] = q * iv;
        sh[1][tid] = q;
        sh[2][tid] = (cok && blockIdx.y == 0) ? z : 0.f;
        __syncthreads();
        for (int s2 = 128; s2 > 0; s2 >>= 1) {
            if (tid < s2) { sh[0][tid] += sh[0][tid + s2]; sh[1][tid] += sh[1][tid + s2]; sh[2][tid] += sh[2][tid + s2]; }
            __syncthreads();
        }
        if (tid == 0) {
            const int nb = gridDim.x * gridDim.y, k = blockIdx.y * gridDim.x + blockIdx.x;
            a.loss_part[k] = sh[0][0];
            a.loss_part[nb + k] = sh[1][0];
            a.loss_part[2 * nb + k] = sh[2][0];
        }
    }
}

struct GaussBpFinishArgs {
    int V, H, P;                                 // P = Bp / 8 partials per column
    const float* part_h; float* hid_bias; float* hb_m;         // up pair: colsum(e_h) (hid_bias null: no up pair)
    const float* part_e0; float* vis_bias; float* vb_m;        // down pair: colsum(e_0) (vis_bias null: no down pair)
    const float* part_q; const float* part_t;                  // down pair: sum (v - m)^2; both pairs: sum e_0 (m - b)
    const float* row_part; int ctiles;                         // up pair: r from gauss_apply, [ctiles][V]
    float* logvar; float* logvar_m;                            // logvar_m null: the variances stay (lr_z == 0)
    float lr, mom, n, lr_z, z_lo, z_hi;
    const float* loss_part; int n_loss; float* loss_out;       // loss_out[0] = J, loss_out[1] = mean((v - m)^2)
};

// grid = ceil(max(V, H) / 256) + 1: the last block reduces the loss, the others take one hidden and one visible unit per thread
__global__ __launch_bounds__(256) void gauss_bp_finish(const GaussBpFinishArgs a) {
    __shared__ double sh[256];
    if (blockIdx.x == gridDim.x - 1) {
        if (a.loss_out) {                        // sum z comes from the rows kernel's partials: the other blocks of this launch write logvar
            const double s1 = loss_total_256(a.loss_part, a.n_loss, sh);
            __syncthreads();
            const double s2 = loss_total_256(a.loss_part + a.n_loss, a.n_loss, sh);
            __syncthreads();
            const double zs = loss_total_256(a.loss_part + 2 * a.n_loss, a.n_loss, sh);
            if (threadIdx.x == 0) {
                a.loss_out[0] = (float)(0.5 * s1 / (double)a.n + 0.5 * zs);
                a.loss_out[1] = (float)(s2 / ((double)a.n * (double)a.V));
            }
        }
        return;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (a.hid_bias && i < a.H) backprop_bias(a.part_h, a.P, a.H, i, a.hid_bias, a.hb_m, a.lr, a.mom, a.n);
    if (i < a.V) {
        if (a.vis_bias) backprop_bias(a.part_e0, a.P, a.V, i, a.vis_bias, a.vb_m, a.lr, a.mom, a.n);
        if (a.logvar_m) {
            const float z = a.logvar[i];
            float g = 0.f;
            if (a.part_q) g = (expf(-z) * sum_parts(a.part_q, a.P, a.V, i)) / (2.0f * a.n) - 0.5f;
            if (a.row_part) {
                float r = ctr_sum_parts(a.row_part, a.ctiles, a.V, i);
                if (a.part_t) r = r - sum_parts(a.part_t, a.P, a.V, i);
                g = g - r / a.n;
            }
            float mz = a.logvar_m[i] * a.mom;
            mz = mz + a.lr_z * g;
            a.logvar_m[i] = mz;
            a.logvar[i] = fminf(fmaxf(z + mz, a.z_lo), a.z_hi);
        }
    }
}

}  // namespace imdbn
