// kernels_centered.hpp -- the centered (enhanced-gradient) parameter update (imdbn_rbm_centered_step).
//
// A centered RBM with offsets mu (visible) and lam (hidden) is the normal RBM with the biases b - W lam and c - W^T mu.  The
// NORMAL parameters stay stored, so only the gradient changes.  With n batch rows, the column sums sv+ / sv- / sh+ / sh- of the
// positive / negative visible and hidden operands, dW = V+^T H+ - V-^T H- (the statistics pass of the update kernel,
// launch_assoc(mode_stats = 1)), dv = (sv+ - sv-) / n and dh = (sh+ - sh-) / n:
//     mv = sv+ / n   (mode 1: (sv+ + sv-) / (2 n)),   mh likewise;      mu' = (1 - slide) mu + slide mv,   lam' likewise
//     gW = dW / n - mu' dh^T - dv lam'^T,     gb = dv - gW lam',     gc = dh - gW^T mu'
//     the momentum rule of rbm.py:212-224 with (gW, gc, gb);  mu := mu', lam := lam'
//
//   centered_apply<VEC4>   grid (column tiles, row stripes), 256 threads.  A block owns a contiguous stripe of <= CTR_ROWS weight
//                          rows and a tile of 64 E cs columns (E = 4 floats per lane with VEC4, else 1; cs <= CTR_CS steps).  It
//                          first forms mu' / dv of its rows and lam' / dh of its columns from the column-sum partials and the old
//                          offsets (LDS, then registers), then every wave takes the rows w, w + 4, ... of the stripe: it streams
//                          dW, W and W_m of the row once, forms gW, does the momentum / decay update, writes W and W_m once, sums
//                          gW_ij lam'_j over its lanes (shuffles: the row is whole inside the wave) into row_part[tile][row], and
//                          keeps mu'_i gW_ij per lane and column.  The four waves' column sums meet in LDS in wave order and
//                          go to col_part[stripe][column].  A layer of at most 64 E CTR_CS columns is one tile: its row dots are
//                          complete inside the block.
//   centered_finish        one small launch: sums col_part over the stripes and row_part over the tiles in index order, updates
//                          both biases and their momenta (sparsity term included), writes mu' and lam', reduces the loss partials.
//
// No floating-point atomics; every sum has an order fixed by (V, H) and the grid, which depends on (V, H) and the CU count only.
// The row padding of W / W_m (pitch > H) is neither read nor written.
#pragma once
#include "kernels_ew.hpp"
#include "kernels_rows.hpp"

namespace imdbn {

constexpr int CTR_CS = 4;                        // column steps of a wave: 64 E CTR_CS columns per tile at most
constexpr int CTR_ROWS = 64;                     // rows of a stripe at most

struct CenteredArgs {
    float* W; float* Wm; int64_t ldw; int V, H;
    const float* dW;                             // [V][H], pitch H: un-normalised statistics
    const float* hpos; const float* hneg; const float* vpos; const float* vneg; int P;      // column-sum partials [P][len]
    float* mu; float* lam;                       // offsets [V], [H]: read by both kernels, overwritten by centered_finish
    float lr, mom, wd, n, slide; int mode;
    int rps, tw, nstripes, ctiles;               // rows per stripe, columns per tile, grid
    float* col_part;                             // [nstripes][H]: sum over the stripe's rows of mu'_i gW_ij
    float* row_part;                             // [ctiles][V]:   sum over the tile's columns of gW_ij lam'_j
    float* hid_bias; float* hb_m; float* vis_bias; float* vb_m;
    int sparsity; float target;
    const float* loss_part; int n_loss; float loss_den; float* loss_out;
};

// the new offset of one unit and its mean difference, from its positive / negative column sums
__device__ __forceinline__ float ctr_offset(const CenteredArgs& a, float sp, float sn, float old, float& diff) {
    diff = (sp - sn) / a.n;
    const float mean = a.mode ? (sp + sn) / (2.0f * a.n) : sp / a.n;
    return (1.0f - a.slide) * old + a.slide * mean;
}

// sum_parts with 32 loads in flight and the same fixed order: centered_finish sums a few hundred stripe partials per column, and
// a dependent round trip per 8 of them was most of its time
__device__ __forceinline__ float ctr_sum_parts(const float* p, int P, int len, int i) {
    float s = 0.f;
    int k = 0;
    for (; k + 32 <= P; k += 32) {
        float t[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) t[j] = p[(int64_t)(k + j) * len + i];
#pragma unroll
        for (int j = 0; j < 32; ++j) s += t[j];
    }
    return s + sum_parts(p + (int64_t)k * len, P - k, len, i);
}

template <bool VEC4>
__global__ __launch_bounds__(256) void centered_apply(const CenteredArgs a) {
    constexpr int E = VEC4 ? 4 : 1;
    __shared__ __attribute__((aligned(16))) float s_lam[64 * E * CTR_CS];
    __shared__ __attribute__((aligned(16))) float s_dh[64 * E * CTR_CS];
    __shared__ __attribute__((aligned(16))) float s_col[4][64 * E * CTR_CS];
    __shared__ float s_mu[CTR_ROWS], s_dv[CTR_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col0 = blockIdx.x * a.tw, ncols = min(a.tw, a.H - col0);
    const int row0 = blockIdx.y * a.rps, nrows = min(a.rps, a.V - row0);
    for (int j = tid; j < ncols; j += 256) {
        const int col = col0 + j;
        float dh;
        s_lam[j] = ctr_offset(a, sum_parts(a.hpos, a.P, a.H, col), sum_parts(a.hneg, a.P, a.H, col), a.lam[col], dh);
        s_dh[j] = dh;
    }
    for (int i = tid; i < nrows; i += 256) {
        const int row = row0 + i;
        float dv;
        s_mu[i] = ctr_offset(a, sum_parts(a.vpos, a.P, a.V, row), sum_parts(a.vneg, a.P, a.V, row), a.mu[row], dv);
        s_dv[i] = dv;
    }
    __syncthreads();
    float lam[CTR_CS][E], dh[CTR_CS][E], cacc[CTR_CS][E];
#pragma unroll
    for (int s = 0; s < CTR_CS; ++s) {
        const int j = (s * 64 + lane) * E;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const bool in = j + e < ncols;       // (VEC4: ncols is a multiple of 4, a float4 is inside or outside as a whole)
            lam[s][e] = in ? s_lam[j + e] : 0.f;
            dh[s][e] = in ? s_dh[j + e] : 0.f;
            cacc[s][e] = 0.f;
        }
    }
    for (int r = w; r < nrows; r += 4) {         // wave-uniform
        const int row = row0 + r;
        const float mu_i = s_mu[r], dv_i = s_dv[r];
        const float* dp = a.dW + (int64_t)row * a.H + col0;
        float* wp = a.W + (int64_t)row * a.ldw + col0;
        float* mp = a.Wm + (int64_t)row * a.ldw + col0;
        float d[CTR_CS][E], w0[CTR_CS][E], m[CTR_CS][E];
#pragma unroll
        for (int s = 0; s < CTR_CS; ++s) {       // the whole row's loads first
            const int j = (s * 64 + lane) * E;
            if (j < ncols) {
                if constexpr (VEC4) {
                    const float4 x = *reinterpret_cast<const float4*>(dp + j);
                    const float4 y = *reinterpret_cast<const float4*>(wp + j);
                    const float4 z = *reinterpret_cast<const float4*>(mp + j);
                    d[s][0] = x.x; d[s][1] = x.y; d[s][2] = x.z; d[s][3] = x.w;
                    w0[s][0] = y.x; w0[s][1] = y.y; w0[s][2] = y.z; w0[s][3] = y.w;
                    m[s][0] = z.x; m[s][1] = z.y; m[s][2] = z.z; m[s][3] = z.w;
                } else {
                    d[s][0] = dp[j]; w0[s][0] = wp[j]; m[s][0] = mp[j];
                }
            }
        }
        float dot = 0.f;
#pragma unroll
        for (int s = 0; s < CTR_CS; ++s) {
            const int j = (s * 64 + lane) * E;
            if (j < ncols) {
                float wn[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float g = d[s][e] / a.n - mu_i * dh[s][e] - dv_i * lam[s][e];
                    dot += g * lam[s][e];
                    cacc[s][e] += mu_i * g;
                    float t = m[s][e] * a.mom;
                    t = t + a.lr * (g - a.wd * w0[s][e]);
                    m[s][e] = t;
                    wn[e] = w0[s][e] + t;
                }
                if constexpr (VEC4) {
                    *reinterpret_cast<float4*>(mp + j) = make_float4(m[s][0], m[s][1], m[s][2], m[s][3]);
                    *reinterpret_cast<float4*>(wp + j) = make_float4(wn[0], wn[1], wn[2], wn[3]);
                } else {
                    mp[j] = m[s][0]; wp[j] = wn[0];
                }
            }
        }
        dot = wave_sum_all(dot);
        if (lane == 0) a.row_part[(int64_t)blockIdx.x * a.V + row] = dot;
    }
#pragma unroll
    for (int s = 0; s < CTR_CS; ++s) {
        const int j = (s * 64 + lane) * E;
#pragma unroll
        for (int e = 0; e < E; ++e) s_col[w][j + e] = cacc[s][e];
    }
    __syncthreads();
    for (int j = tid; j < ncols; j += 256)
        a.col_part[(int64_t)blockIdx.y * a.H + col0 + j] = ((s_col[0][j] + s_col[1][j]) + s_col[2][j]) + s_col[3][j];
}

// grid = ceil(max(V, H) / 256) + 1: the last block reduces the loss partials, the others take one hidden and one visible unit per thread
__global__ __launch_bounds__(256) void centered_finish(const CenteredArgs a) {
    __shared__ double sh[256];
    if (blockIdx.x == gridDim.x - 1) {
        if (a.loss_out) {
            const double t = loss_total_256(a.loss_part, a.n_loss, sh);
            if (threadIdx.x == 0) a.loss_out[0] = (float)(t / (double)a.loss_den);
        }
        return;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.H) {
        const float sp = sum_parts(a.hpos, a.P, a.H, i), sn = sum_parts(a.hneg, a.P, a.H, i);
        float dh;
        const float lam = ctr_offset(a, sp, sn, a.lam[i], dh);
        const float corr = ctr_sum_parts(a.col_part, a.nstripes, a.H, i);       // (gW^T mu')_i
        float m = a.hb_m[i] * a.mom;
        m = m + (a.lr * (sp - sn)) / a.n;
        m = m - a.lr * corr;
        if (a.sparsity) m = m + (-a.lr) * (sp / a.n - a.target);
        a.hb_m[i] = m;
        a.hid_bias[i] += m;
        a.lam[i] = lam;
    }
    if (i < a.V) {
        const float sp = sum_parts(a.vpos, a.P, a.V, i), sn = sum_parts(a.vneg, a.P, a.V, i);
        float dv;
        const float mu = ctr_offset(a, sp, sn, a.mu[i], dv);
        const float corr = ctr_sum_parts(a.row_part, a.ctiles, a.V, i);         // (gW lam')_i
        float m = a.vb_m[i] * a.mom;
        m = m + (a.lr * (sp - sn)) / a.n;
        m = m - a.lr * corr;
        a.vb_m[i] = m;
        a.vis_bias[i] += m;
        a.mu[i] = mu;
    }
}

}  // namespace imdbn
