// kernels_exact.hpp -- exact log Z, and exact model marginals, by enumerating one side of an RBM (imdbn_rbm_exact_logz).
//
// E is the enumerated side (n <= EXACT_NMAX units, bias e), S the other one (D units, bias f).  A state s of E has unit k on iff bit k
// of s is set.  With the dense block Wd [n][D] of exact_prep (row k = the weights between unit k of E and the D units of S) and
// x(s) = f + sum_{k in s} Wd[k] the log-weight of a state is
//     Bernoulli S:   t(s) = e.s + sum_{i outside groups} softplus(x_i) + sum_g log sum_{k in g} exp(x_k)
//     Gaussian S:    t(s) = e.s + sum_i (f_i a_i + a_i^2 / 2) exp(-z_i),    a(s) = x(s) - f = sum_{k in s} Wd[k]    (E hidden, S visible)
// and log Z = LSE_s t(s) (+ sum_i (log 2 pi + z_i) / 2 for Gaussian visibles).
//
//   exact_prep        one launch: Wd from the n columns (E hidden) or rows (E visible) of W -- row padding is never read --, the
//                     marginal partials zeroed.  After it the walk reads W coalesced: lane l reads Wd[k][i0 + l].
//   exact_walk        the enumeration.  A wave owns EXACT_WALK = 32 consecutive states at a time (a "tile": the states 32 g .. 32 g + 31
//                     of the launch); lane l owns the columns i0 + l and i0 + 64 + l of every 128-column chunk i0.  Per chunk a lane
//                     builds a FRESH base x = f + Wd[k] for the set bits k >= 5 of the tile in ascending k, then walks the 32 states
//                     in Gray-code order, one fp32 add or subtract of Wd[bit] per state and column: a pre-activation is reached from
//                     the bias by at most (n - 5) + 31 = n + 26 fp32 additions (the n + 32 of the contract).  The two column terms
//                     of a chunk add in fp32, the chunks in double (the convention of pt_exchange_rows); the 64 lane values of a
//                     state meet in the fixed butterfly.  A softmax group (<= 256 columns, <= 4 of them) is walked on its own, four
//                     columns per lane: max and sum-of-exp per state through the butterfly.
//                     Lane l < 32 keeps the (max, scaled sum) pair of the states 32 g + l it has seen, in double; at the end the
//                     pairs meet in the butterfly, then the four waves in wave order through LDS, and the block writes ONE pair to
//                     slot [launch][block] of the partials.  Tiles are dealt to waves by index (tile = (it * blocks + block) * 4 +
//                     wave), so which wave sums what is fixed by (V, H) alone.
//                     MARG: the second pass, after exact_finish has left LSE_s t(s) in the scratch header.  Per tile the log-weights
//                     as above, w(s) = exp(t(s) - LSE); lane k adds w(s) s_k to its E accumulator; a second sweep over the chunks
//                     repeats the walk and adds w(s) sigmoid(x_i) (softmax_g(x)_k inside a group, f_i + a_i for Gaussian S) in
//                     double per column; the four waves' column sums meet in LDS in wave order and thread c of the block adds them
//                     to column i0 + c of the block's own row of the partials (no other thread ever touches it).
//   exact_finish      one wave: the (max, sum) pairs in a fixed order -- lane l the slots l, l + 64, ... ascending, then the
//                     butterfly --; out = {log Z, log of the largest state weight}; the header keeps LSE_s t(s) for the second pass.
//   exact_finish_marg the per-block partials of a column, blocks in index order, to the fp32 means.
//
// No launch enumerates more than EXACT_LAUNCH_BITS = 22 bits of states; the host loops over the high bits.  No floating-point atomics,
// no inline assembly, nothing waits on another workgroup; every index is bounded by the arguments.
#pragma once
#include "kernels_pt.hpp"

namespace imdbn {

constexpr int EXACT_NMAX = 30;                   // units on the enumerated side
constexpr int EXACT_WALK_BITS = 5;               // a fresh base every 2^5 = 32 states
constexpr int EXACT_WALK = 1 << EXACT_WALK_BITS;
constexpr int EXACT_LAUNCH_BITS = 22;            // states per launch <= 2^22
constexpr int EXACT_BLOCKS = 512;                // blocks per walk launch at most = partial slots per launch = rows of the marginal partials
constexpr int EXACT_JC = 128;                    // columns of S per fp32 chunk (PT_JC)
constexpr int EXACT_HDR = 8;                     // doubles in front of the scratch block: [0] LSE_s t(s)

struct ExactArgs {
    const float* W; int64_t ldw;                 // the caller's weights [V][ldw]
    const float* e_bias; const float* s_bias;    // e [n], f [D]
    const float* logvar;                         // z [D]: Gaussian S (= visible), else null
    int V, H, n, D, e_hidden;                    // E hidden: Wd[k][i] = W[i][k], D = V;  E visible: Wd[k][j] = W[k][j], D = H
    GroupSpans sp;                               // softmax groups of S (E hidden only)
    double* hdr;                                 // [EXACT_HDR]
    double* part;                                // [n_launch][EXACT_BLOCKS][2]  (max, scaled sum)
    float* Wd;                                   // [n][D]
    double* marg_s;                              // [blocks][D]   (marginals only)
    double* marg_e;                              // [blocks][32]
    int n_launch, launch;                        // launches of the call; this one
    unsigned base;                               // first state of this launch
    unsigned tiles;                              // 32-state tiles of this launch
    int blocks;                                  // blocks of every walk launch of the call
    int marg;                                    // prep: zero the marginal partials
    double* out; float* vis_mean; float* hid_mean;
};

__global__ __launch_bounds__(256) void exact_prep(const ExactArgs a) {
    const int64_t nt = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nd = (int64_t)a.n * a.D;
    for (int64_t q = t0; q < nd; q += nt) {
        const int k = (int)(q / a.D), i = (int)(q - (int64_t)k * a.D);
        a.Wd[q] = a.e_hidden ? a.W[(int64_t)i * a.ldw + k] : a.W[(int64_t)k * a.ldw + i];
    }
    if (!a.marg) return;
    const int64_t ns = (int64_t)a.blocks * a.D, ne = (int64_t)a.blocks * 32;      // the rows the walk launches write
    for (int64_t q = t0; q < ns; q += nt) a.marg_s[q] = 0.0;
    for (int64_t q = t0; q < ne; q += nt) a.marg_e[q] = 0.0;
}

// (m, s) <- (m, s) + (m2, s2): a sum of exponentials as (largest exponent, sum scaled by it).  An empty pair is (-inf, 0).
__device__ __forceinline__ void exact_lse_join(double& m, double& s, double m2, double s2) {
    const double M = fmax(m, m2);
    if (M == -INFINITY) { s = 0.0; return; }
    s = s * exp(m - M) + s2 * exp(m2 - M);       // exp(-inf) = 0 for the empty side
    m = M;
}

__device__ __forceinline__ bool exact_in_group(const GroupSpans& sp, int i) {
    bool g = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) g |= q < sp.n_groups && i >= sp.gs[q] && i < sp.ge[q];
    return g;
}

// the code of step t of the Gray walk, and the bit that step t flips (t >= 1)
__host__ __device__ constexpr int exact_gray(int t) { return t ^ (t >> 1); }
__host__ __device__ constexpr int exact_flip(int t) { return (t & 1) ? 0 : (t & 2) ? 1 : (t & 4) ? 2 : (t & 8) ? 3 : 4; }

// One chunk of one tile: the columns i0 + lane and i0 + 64 + lane over the 32 states.  Without WANT_MARG the chunk's fp32 term of
// every state is added to acc (double, per lane).  With it `acc` holds the normalised weights w(s) and the two column means come back.
template <bool GAUSS, bool WANT_MARG>
__device__ __forceinline__ void exact_chunk(const ExactArgs& a, unsigned hi, int i0, int lane, double (&acc)[EXACT_WALK], double (&cm)[2]) {
    int col[2]; bool in[2]; float x[2], f[2], iv[2], wl[EXACT_WALK_BITS][2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        col[c] = i0 + 64 * c + lane;
        in[c] = col[c] < a.D && !(!GAUSS && exact_in_group(a.sp, col[c]));
        f[c] = in[c] ? a.s_bias[col[c]] : 0.f;
        iv[c] = (GAUSS && in[c]) ? expf(-a.logvar[col[c]]) : 0.f;
        x[c] = GAUSS ? 0.f : f[c];
#pragma unroll
        for (int k = 0; k < EXACT_WALK_BITS; ++k) wl[k][c] = (in[c] && k < a.n) ? a.Wd[(int64_t)k * a.D + col[c]] : 0.f;
    }
    for (int k = EXACT_WALK_BITS; k < a.n; ++k) {            // the fresh base: the set high bits in ascending order
        if (!((hi >> k) & 1u)) continue;                     // wave-uniform
#pragma unroll
        for (int c = 0; c < 2; ++c) x[c] += in[c] ? a.Wd[(int64_t)k * a.D + col[c]] : 0.f;
    }
    cm[0] = 0.0; cm[1] = 0.0;
#pragma unroll
    for (int t = 0; t < EXACT_WALK; ++t) {
        const int code = exact_gray(t);
        if (t > 0) {
            const int k = exact_flip(t);
            const bool on = (code >> k) & 1;
#pragma unroll
            for (int c = 0; c < 2; ++c) x[c] = on ? x[c] + wl[k][c] : x[c] - wl[k][c];
        }
        float term[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (!WANT_MARG) term[c] = !in[c] ? 0.f : GAUSS ? (f[c] * x[c] + 0.5f * x[c] * x[c]) * iv[c] : pt_softplus(x[c]);
            else term[c] = !in[c] ? 0.f : GAUSS ? f[c] + x[c] : sigmoidf_ref(x[c]);
        }
        if (!WANT_MARG) acc[code] += (double)(term[0] + term[1]);
        else { cm[0] += acc[code] * (double)term[0]; cm[1] += acc[code] * (double)term[1]; }
    }
}

// One softmax group of one tile: the columns gs + lane + 64 r, r < 4.  Without WANT_MARG lane 0 adds log sum_k exp(x_k) of every state
// to acc; with it `acc` holds w(s) and gm[r] gets sum_s w(s) softmax(x)_k of the lane's columns.
template <bool WANT_MARG>
__device__ __forceinline__ void exact_group(const ExactArgs& a, unsigned hi, int gs, int ge, int lane, double (&acc)[EXACT_WALK], double (&gm)[4]) {
    int col[4]; bool in[4]; float x[4], wl[EXACT_WALK_BITS][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        col[r] = gs + 64 * r + lane;
        in[r] = col[r] < ge;
        x[r] = in[r] ? a.s_bias[col[r]] : 0.f;
#pragma unroll
        for (int k = 0; k < EXACT_WALK_BITS; ++k) wl[k][r] = (in[r] && k < a.n) ? a.Wd[(int64_t)k * a.D + col[r]] : 0.f;
        gm[r] = 0.0;
    }
    for (int k = EXACT_WALK_BITS; k < a.n; ++k) {
        if (!((hi >> k) & 1u)) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] += in[r] ? a.Wd[(int64_t)k * a.D + col[r]] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < EXACT_WALK; ++t) {
        const int code = exact_gray(t);
        if (t > 0) {
            const int k = exact_flip(t);
            const bool on = (code >> k) & 1;
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = on ? x[r] + wl[k][r] : x[r] - wl[k][r];
        }
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = in[r] ? fmaxf(mx, x[r]) : mx;
        mx = wave_max_all(mx);
        float ex[4], es = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { ex[r] = in[r] ? expf(x[r] - mx) : 0.f; es += ex[r]; }
        const double sum = wave_sum_all((double)es);
        if (!WANT_MARG) acc[code] += lane == 0 ? (double)mx + log(sum) : 0.0;
        else {
            const double ws = acc[code] / sum;
#pragma unroll
            for (int r = 0; r < 4; ++r) gm[r] += ws * (double)ex[r];
        }
    }
}

// The log-weights of the 32 states of a tile, the same in every lane: tot[code] for the state hi | code.  Codes >= 2^n (n < 5) are -inf.
template <bool GAUSS>
__device__ __forceinline__ void exact_tile_logw(const ExactArgs& a, unsigned hi, int lane, double (&tot)[EXACT_WALK]) {
    double cm[2];
#pragma unroll
    for (int t = 0; t < EXACT_WALK; ++t) tot[t] = 0.0;
    for (int i0 = 0; i0 < a.D; i0 += EXACT_JC) exact_chunk<GAUSS, false>(a, hi, i0, lane, tot, cm);
    if (!GAUSS) {
        double gm[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < a.sp.n_groups) exact_group<false>(a, hi, a.sp.gs[q], a.sp.ge[q], lane, tot, gm);
    }
    // e.s in double: the high bits once, the low bits per state
    double eh = 0.0, el[EXACT_WALK_BITS];
    for (int k = EXACT_WALK_BITS; k < a.n; ++k) eh += ((hi >> k) & 1u) ? (double)a.e_bias[k] : 0.0;
#pragma unroll
    for (int k = 0; k < EXACT_WALK_BITS; ++k) el[k] = k < a.n ? (double)a.e_bias[k] : 0.0;
    const unsigned n_states = a.n >= 31 ? 0x7fffffffu : (1u << a.n);
#pragma unroll
    for (int t = 0; t < EXACT_WALK; ++t) {
        double es = eh;
#pragma unroll
        for (int k = 0; k < EXACT_WALK_BITS; ++k) es += ((t >> k) & 1) ? el[k] : 0.0;
        const double v = wave_sum_all(tot[t]) + es;
        tot[t] = (hi | (unsigned)t) < n_states ? v : -INFINITY;
    }
}

template <bool GAUSS, bool MARG>
__global__ __launch_bounds__(256) void exact_walk(const ExactArgs a) {
    __shared__ double sm[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned per_it = (unsigned)gridDim.x * 4u;
    const unsigned n_it = (a.tiles + per_it - 1) / per_it;      // the same for every wave of the grid: the barriers below are uniform
    double pm = -INFINITY, ps = 0.0;                            // lane l < 32: the states 32 g + l of this wave's tiles
    double me = 0.0;                                            // MARG, lane k < n: sum w(s) s_k
    const double lse = MARG ? a.hdr[0] : 0.0;
    double tot[EXACT_WALK];
    for (unsigned it = 0; it < n_it; ++it) {
        const unsigned tile = (it * (unsigned)gridDim.x + blockIdx.x) * 4u + wave;
        const bool live = tile < a.tiles;                       // wave-uniform
        const unsigned hi = a.base + tile * EXACT_WALK;
        if (live) {
            exact_tile_logw<GAUSS>(a, hi, lane, tot);
            if (!MARG) {
                double mine = -INFINITY;
#pragma unroll
                for (int t = 0; t < EXACT_WALK; ++t) mine = lane == t ? tot[t] : mine;
                exact_lse_join(pm, ps, mine, mine == -INFINITY ? 0.0 : 1.0);
            } else {
#pragma unroll
                for (int t = 0; t < EXACT_WALK; ++t) {
                    tot[t] = exp(tot[t] - lse);                 // exp(-inf) = 0: a code past 2^n
                    me += (lane < a.n && (((hi | (unsigned)t) >> (lane & 31)) & 1u)) ? tot[t] : 0.0;
                }
            }
        }
        if (!MARG) continue;
        // ---- second sweep: the S side, the four waves' column sums through LDS in wave order
        for (int i0 = 0; i0 < a.D; i0 += EXACT_JC) {
            double cm[2] = {0.0, 0.0};
            if (live) exact_chunk<GAUSS, true>(a, hi, i0, lane, tot, cm);
            __syncthreads();                                    // the previous stage has been read
            sm[wave][lane] = cm[0]; sm[wave][64 + lane] = cm[1];
            __syncthreads();
            const int col = i0 + tid;
            if (tid < EXACT_JC && col < a.D && !(!GAUSS && exact_in_group(a.sp, col)))
                a.marg_s[(int64_t)blockIdx.x * a.D + col] += ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
        }
        if (!GAUSS) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q >= a.sp.n_groups) continue;
                double gm[4] = {0.0, 0.0, 0.0, 0.0};
                if (live) exact_group<true>(a, hi, a.sp.gs[q], a.sp.ge[q], lane, tot, gm);
                __syncthreads();
#pragma unroll
                for (int r = 0; r < 4; ++r) sm[wave][64 * r + lane] = gm[r];
                __syncthreads();
                const int col = a.sp.gs[q] + tid;
                if (col < a.sp.ge[q])
                    a.marg_s[(int64_t)blockIdx.x * a.D + col] += ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
            }
        }
    }
    if (!MARG) {
        for (int o = 32; o >= 1; o >>= 1) {
            const double m2 = __shfl_xor(pm, o), s2 = __shfl_xor(ps, o);
            exact_lse_join(pm, ps, m2, s2);
        }
        if (lane == 0) { sm[0][2 * wave] = pm; sm[0][2 * wave + 1] = ps; }
        __syncthreads();
        if (tid == 0) {
            double m = sm[0][0], s = sm[0][1];
            for (int w = 1; w < 4; ++w) exact_lse_join(m, s, sm[0][2 * w], sm[0][2 * w + 1]);
            double* slot = a.part + ((int64_t)a.launch * EXACT_BLOCKS + blockIdx.x) * 2;
            slot[0] = m; slot[1] = s;
        }
    } else {
        __syncthreads();
        if (lane < 32) sm[wave][lane] = me;
        __syncthreads();
        if (tid < 32) a.marg_e[(int64_t)blockIdx.x * 32 + tid] += ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
    }
}

__global__ __launch_bounds__(64) void exact_finish(const ExactArgs a) {
    const int lane = threadIdx.x;
    double m = -INFINITY, s = 0.0;
    for (int l = 0; l < a.n_launch; ++l)
        for (int b = lane; b < a.blocks; b += 64) {
            const double* slot = a.part + ((int64_t)l * EXACT_BLOCKS + b) * 2;
            exact_lse_join(m, s, slot[0], slot[1]);
        }
    for (int o = 32; o >= 1; o >>= 1) {
        const double m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        exact_lse_join(m, s, m2, s2);
    }
    double cz = 0.0;                                            // Gaussian visibles: sum_i (log 2 pi + z_i) / 2
    if (a.logvar) {
        for (int i = lane; i < a.D; i += 64) cz += 0.5 * (1.8378770664093453 + (double)a.logvar[i]);
        cz = wave_sum_all(cz);
    }
    if (lane == 0) {
        const double lse = m + log(s);
        a.hdr[0] = lse;
        a.out[0] = lse + cz;
        a.out[1] = m + cz;
    }
}

__global__ __launch_bounds__(256) void exact_finish_marg(const ExactArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float* s_out = a.e_hidden ? a.vis_mean : a.hid_mean;
    float* e_out = a.e_hidden ? a.hid_mean : a.vis_mean;
    if (i < a.D) {
        double t = 0.0;
        for (int b = 0; b < a.blocks; ++b) t += a.marg_s[(int64_t)b * a.D + i];
        s_out[i] = (float)t;
    }
    if (i < a.n) {
        double t = 0.0;
        for (int b = 0; b < a.blocks; ++b) t += a.marg_e[(int64_t)b * 32 + i];
        e_out[i] = (float)t;
    }
}

}  // namespace imdbn
