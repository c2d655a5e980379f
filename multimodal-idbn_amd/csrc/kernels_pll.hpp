// kernels_pll.hpp -- exact pseudo-log-likelihood PLL(v) = sum_sites log p(v_site | v_rest) (imdbn_rbm_pseudo_loglik).
//
// With x = c + v W, sigma = sigmoid(x) and s_i = 1 - 2 v_i, flipping visible column i moves x_j by s_i W_ij, and
// softplus(x + d) - softplus(x) = log1p(sigma(x) expm1(d)) exactly, so
//     g_i = s_i b_i + sum_j log1p(sigma_j expm1(s_i W_ij)) = F(v) - F(v with bit i flipped),      log p(v_i | v_rest) = -softplus(g_i)
// and for a softmax group with observed category t:  g_k = (b_k - b_t) + sum_j log1p(sigma_j expm1(W_kj - W_tj)),
//     log p(v_g | v_rest) = -log sum_{k in g} exp(g_k)      (g_t = 0).
//
//   pll_rows_sigmoid   one wave per row: the logits of the up propagation become sigma in place.  A row holding an element that is
//                      not exactly 0 or 1, or a group without exactly one 1, gets a NaN sigma row -- the mark of an invalid row, which
//                      every term of that row inherits through its arithmetic.
//   pll_sites          the hot kernel: every column as a Bernoulli site.  A block owns PLL_TI visible columns x PLL_TR rows and walks
//                      j over H in chunks of PLL_JC.  Per chunk it stages sigma[rows][chunk] and the two planes expm1(W_ij),
//                      expm1(-W_ij) of its weight tile in LDS -- every weight element is exponentiated once per block, not once per
//                      row; W rows are contiguous in j, so the loads coalesce.  Lane = row, and a thread owns the pairs (its row,
//                      column wave + 4 q), q < 4: the plane of a pair is chosen ONCE, as the LDS address it reads from (v_ri never
//                      changes over j).  Per four j a pair costs one 16-byte plane read (a broadcast: the wave's lanes read one of two
//                      addresses), four fma, three multiplies and one v_log_f32: log2 of the product of four factors
//                      (1 + sigma_j E_ij), each in [min(1, e^d), max(1, e^d)].  The log2 values of a chunk add up in fp32 (32 terms),
//                      the chunks in double, in chunk order.  Columns inside a softmax group get 0 (NaN in an invalid row);
//                      pll_rows_finish overwrites the observed one.
//   pll_rows_finish    one wave per row: each group's term in double (lane l takes j = l, l + 64, ...; the K values of a group are
//                      parked in the label slots of kernels_rows.hpp as in joint_label_loglik), written at the observed column; then
//                      the row total: the fp32 Bernoulli terms in double, lane l the columns l, l + 64, ..., the fixed butterfly,
//                      plus the group terms in group order.
//
// Every sum runs in an order fixed by (V, H, groups): a row gives the same bits alone and inside any batch.  No atomics.
#pragma once
#include "kernels_ais.hpp"

namespace imdbn {

constexpr int PLL_TI = 16;                       // visible columns per block
constexpr int PLL_TR = 64;                       // rows per block = lanes of a wave: a 64-row batch reads W once
constexpr int PLL_JC = 128;                      // hidden units per chunk
constexpr int PLL_SS = PLL_JC + 4;               // sigma row stride (floats): lane l's float4 starts at bank 4 l mod 64 -- the 16 lanes of
                                                 // a ds_read_b128 group cover the 64 banks once
constexpr int PLL_EM = PLL_TI * PLL_JC + 4;      // the expm1(-w) plane starts here: 4 banks off the expm1(w) plane, so the two
                                                 // addresses a wave reads never meet on a bank

struct PllArgs {
    const float* v; int64_t ldv;                 // the caller's rows [N][V]
    float* sig; int64_t ldx;                     // [N][H]: the logits c + v W, sigma after pll_rows_sigmoid
    const float* W; int64_t ldw; const float* vis_bias;
    float* site; int64_t lds;                    // per-column terms [N][V]: the caller's out_site or scratch
    double* pll;                                 // [N]
    int N, V, H;
    GroupSpans sp;
};

__global__ __launch_bounds__(64 * ROW_WAVES) void pll_rows_sigmoid(const PllArgs a) {
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.N) return;      // wave-uniform
    const float* v = a.v + (int64_t)row * a.ldv;
    bool bad = false;
    for (int i = lane; i < a.V; i += 64) {
        const float x = v[i];
        bad |= !(x == 1.f || x == 0.f);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < a.sp.n_groups) {
            int ones = 0;
            for (int i = a.sp.gs[q] + lane; i < a.sp.ge[q]; i += 64) ones += v[i] == 1.f ? 1 : 0;
            bad |= wave_sum_all(ones) != 1;
        }
    }
    const bool any_bad = __ballot(bad) != 0ull;
    float* x = a.sig + (int64_t)row * a.ldx;
    for (int j = lane; j < a.H; j += 64) x[j] = any_bad ? NAN : sigmoidf_ref(x[j]);
}

__global__ __launch_bounds__(256) void pll_sites(const PllArgs a) {
    __shared__ __attribute__((aligned(16))) float sS[PLL_TR * PLL_SS];
    __shared__ __attribute__((aligned(16))) float sE[PLL_EM + PLL_TI * PLL_JC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * PLL_TI, r0 = blockIdx.y * PLL_TR;
    const int row = r0 + lane;
    const float4* e[4];
    bool live[4], one[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ci = wave + 4 * q, col = i0 + ci;
        live[q] = row < a.N && col < a.V;
        one[q] = live[q] && a.v[(int64_t)row * a.ldv + col] == 1.f;
        e[q] = reinterpret_cast<const float4*>(sE + (one[q] ? PLL_EM : 0) + ci * PLL_JC);
    }
    const float4* sg = reinterpret_cast<const float4*>(sS + lane * PLL_SS);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < a.H; j0 += PLL_JC) {
        __syncthreads();      // the previous chunk has been read
#pragma unroll 8
        for (int k = 0; k < PLL_TR * PLL_JC / 256; ++k) {
            const int idx = tid + 256 * k, r = idx / PLL_JC, j = idx % PLL_JC;
            const bool in = r0 + r < a.N && j0 + j < a.H;
            sS[r * PLL_SS + j] = in ? a.sig[(int64_t)(r0 + r) * a.ldx + j0 + j] : 0.f;
        }
#pragma unroll 2
        for (int k = 0; k < PLL_TI * PLL_JC / 256; ++k) {
            const int idx = tid + 256 * k, ci = idx / PLL_JC, j = idx % PLL_JC;
            const bool in = i0 + ci < a.V && j0 + j < a.H;
            const float w = in ? a.W[(int64_t)(i0 + ci) * a.ldw + j0 + j] : 0.f;
            sE[idx] = expm1f(w);
            sE[PLL_EM + idx] = expm1f(-w);
        }
        __syncthreads();
        float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int jq = 0; jq < PLL_JC / 4; ++jq) {
            const float4 s = sg[jq];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 E = e[q][jq];
                const float p = (fmaf(s.x, E.x, 1.f) * fmaf(s.y, E.y, 1.f)) * (fmaf(s.z, E.z, 1.f) * fmaf(s.w, E.w, 1.f));
                part[q] += __log2f(p);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += (double)part[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!live[q]) continue;
        const int col = i0 + wave + 4 * q;
        bool grp = false;
#pragma unroll
        for (int g = 0; g < 4; ++g) grp |= g < a.sp.n_groups && col >= a.sp.gs[g] && col < a.sp.ge[g];
        const double b = (double)a.vis_bias[col];
        const double gi = (one[q] ? -b : b) + 0.6931471805599453 * acc[q];
        a.site[(int64_t)row * a.lds + col] = grp ? (acc[q] != acc[q] ? NAN : 0.f) : (float)(-ais_softplus(gi));
    }
}

__global__ __launch_bounds__(64 * ROW_WAVES) void pll_rows_finish(const PllArgs a) {
    const int lane = wave_lane(), row = wave_row();
    if (row >= a.N) return;      // wave-uniform
    const float* v = a.v + (int64_t)row * a.ldv;
    const float* sig = a.sig + (int64_t)row * a.ldx;
    float* site = a.site + (int64_t)row * a.lds;
    const bool bad = sig[0] != sig[0];      // the mark of pll_rows_sigmoid
    double tot = 0.0;
    for (int i = lane; i < a.V; i += 64) {
        bool grp = false;
#pragma unroll
        for (int g = 0; g < 4; ++g) grp |= g < a.sp.n_groups && i >= a.sp.gs[g] && i < a.sp.ge[g];
        if (!grp) tot += (double)site[i];
    }
    tot = wave_sum_all(tot);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (g >= a.sp.n_groups || bad) continue;
        const int s = a.sp.gs[g], K = a.sp.ge[g] - s;
        int t1 = 0;                                          // observed column + 1 (a valid row holds exactly one)
        for (int i = s + lane; i < s + K; i += 64) t1 += v[i] == 1.f ? i + 1 : 0;
        const int t = wave_sum_all(t1) - 1;
        const float* wt = a.W + (int64_t)t * a.ldw;
        const double bt = (double)a.vis_bias[t];
        double val[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            for (int kk = 0; kk < 64; ++kk) {
                const int k = q * 64 + kk;
                if (k >= K) break;
                const float* wk = a.W + (int64_t)(s + k) * a.ldw;
                double sh = 0.0;
                for (int j = lane; j < a.H; j += 64) sh += log1p((double)sig[j] * expm1((double)wk[j] - (double)wt[j]));
                const double gk = ((double)a.vis_bias[s + k] - bt) + wave_sum_all(sh);
                if (lane == kk) val[q] = gk;
            }
        }
        const double mx = wave_max_all(fmax(fmax(val[0], val[1]), fmax(val[2], val[3])));
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double ex = exp(val[q] - mx);      // an empty slot holds -inf: 0
            for (int kk = 0; kk < 64; ++kk) {
                if (q * 64 + kk >= K) break;
                sum += __shfl(ex, kk, 64);
            }
        }
        const double term = -(mx + log(sum));
        tot += term;
        if (lane == 0) site[t] = (float)term;
    }
    if (lane == 0) a.pll[row] = bad ? (double)NAN : tot;
}

}  // namespace imdbn
