// Pairwise free-energy scores of a joint RBM over [z1 (D1) | z2 (D2)] and what retrieval needs from them
// (imdbn/utils/retrieval.py).
//
//   S[q][n] = -F([z1_q | z2_n]) = sa[q] + sb[n] + sum_j softplus(a[q][j] + b[n][j])
//   a[Q][H] = c + z1 W[:D1]     the logits path of the up propagation on the descriptor cut to its first D1 weight rows
//   b[N][H] = z2 W[D1:]         the same path on the descriptor whose W starts at row D1, V = D2, with a hidden bias of zeros
//                               (a zero vector of H floats in the workspace, cleared by the call)
//   sa[Q] = z1 . b[:D1], sb[N] = z2 . b[D1:]      pair_row_dot: one wave per row, columns l, l + 64, ... then the xor butterfly
//
// The nonlinearity sits inside the pair sum, so no GEMM expresses S: Q N H softplus evaluations, VALU / transcendental bound.
//   * pair_score_list   the matched-pair scores S[q][gt_q[q]] and S[gt_n[n]][n], one thread per pair, BEFORE the sweep; the same
//                       device functions and the same j-order as the sweep, so they carry the bits the sweep gives that pair and
//                       the == of the rank rule means what it says.  An entry of gt outside its range: NaN, nothing read through it.
//   * pair_score_sweep  block = 64 queries x one chunk of the candidates, sub-tiles of 64 candidates (the shape of knn_topk_chunk).
//                       Slices of 32 hidden units of the 64 rows of a and of b are staged through LDS (pitch 33: the 16 candidate rows
//                       a wave reads at one j sit in 16 banks, the 4 query rows are broadcasts); thread (tq, tn) keeps the 4 x 4
//                       pairs (4 tq + i, tn + 16 m) in registers.  Per pair the fp32 terms softplus(a_qj + b_nj) are added, j = 0 ..
//                       H - 1 in order, into a DOUBLE (v_add_f64 is full rate here; 32 of the 96 registers): the sum itself then adds
//                       nothing to the error bound, and a pair scores the same bits whatever Q, N, k, the chunking or the other rows.
//                       The finished 64 x 64 tile goes to LDS, where three waves work side by side: wave 0 counts, per query, the
//                       candidates that rank before the true partner; wave 1 the same per candidate over the 64 queries (the other
//                       direction from the same score bits); wave 2 offers the tile to the queries' top-k lists (KnnList, keyed =
//                       false).  Counts are integers: per-chunk / per-query-tile partials in the workspace, summed by pair_finish.
//                       No score matrix reaches HBM unless the caller asks for it.
//   * pair_finish       rank = sum of the partials (-1 for an invalid gt entry), the public copies of the matched-pair scores.
//   * knn_topk_merge    the chunks' lists into the answer (key = nullptr).
// softplus here is the fast fp32 form max(x, 0) + ln2 * log2(1 + exp2(-|x| log2 e)) on v_exp_f32 / v_log_f32 (8 issue cycles each,
// 4 for the rest: ~40 cycles per pair term and wave), not the double ais_softplus of the per-row kernels.
#pragma once
#include "kernels_knn.hpp"

namespace imdbn {

constexpr int PAIR_KT = 32;                      // hidden units per LDS slice
constexpr int PAIR_LDP = PAIR_KT + 1;            // padded row pitch of the staged slices (floats)
constexpr int PAIR_STATIC_LDS = (int)sizeof(float) * (2 * KNN_QT * PAIR_LDP + KNN_QT * KNN_STP);

inline size_t pair_sweep_lds(int k) { return (size_t)PAIR_STATIC_LDS + knn_merge_lds(k); }

__device__ __forceinline__ float pair_softplus(float x) {
    const float t = __builtin_amdgcn_exp2f(-fabsf(x) * 1.44269504088896341f);        // exp(-|x|), in (0, 1]
    const float l = __builtin_amdgcn_logf(1.0f + t);                                  // log2(1 + t), in (0, 1]
    return __builtin_fmaf(l, 0.693147180559945309f, fmaxf(x, 0.f));
}
// one more term of a pair, then the pair's score: the ONLY two places where a score is put together
__device__ __forceinline__ void pair_term(double& acc, float a, float b) { acc += (double)pair_softplus(a + b); }
__device__ __forceinline__ float pair_total(float sa, float sb, double acc) { return (float)(((double)sa + (double)sb) + acc); }

// out[r] = x[r] . w in fp32: lane l takes columns l, l + 64, ... in order, then the fixed xor butterfly
__global__ __launch_bounds__(64 * ROW_WAVES) void pair_row_dot(const float* __restrict__ x, int64_t ldx, int N, int D,
                                                              const float* __restrict__ w, float* __restrict__ out) {
    const int l = wave_lane();
    const int64_t r = wave_row();
    if (r >= N) return;                                                    // wave-uniform
    const float* row = x + r * ldx;
    float s = 0.f;
    for (int c = l; c < D; c += 64) s = __builtin_fmaf(row[c], w[c], s);
    s = wave_sum_all(s);
    if (l == 0) out[r] = s;
}

struct PairArgs {
    const float* a; const float* b;           // [Q][H], [N][H] of pitch H
    const float* sa; const float* sb;         // [Q], [N]
    int Q, N, H, k, chunk;                    // chunk: candidates per block, a multiple of KNN_BT
    const int32_t* gt_q; const int32_t* gt_n; // [Q] / [N], nullable
    float* ref_q; float* ref_n;               // [Q] / [N] matched-pair scores (workspace)
    int32_t* row_part;                        // [chunks][Q]
    int32_t* col_part;                        // [query tiles][N]
    float* part_s; int32_t* part_i;           // [chunks][Q][k]
    float* scores; int64_t lds;               // [Q][N], nullable
    int32_t* rank_q; int32_t* rank_n; float* score_q; float* score_n;      // the caller's outputs (pair_finish), nullable
    int chunks, qtiles;
};

// grid ceil((Q + N) / 256), 256 threads: thread i < Q scores (i, gt_q[i]), thread Q + n scores (gt_n[n], n)
__global__ __launch_bounds__(256) void pair_score_list(const PairArgs p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)p.Q + p.N) return;
    const bool by_q = i < p.Q;
    if (!(by_q ? p.gt_q : p.gt_n)) return;
    const int own = by_q ? (int)i : (int)(i - p.Q);
    const int g = by_q ? p.gt_q[own] : p.gt_n[own];
    float s = __builtin_nanf("");
    if (g >= 0 && g < (by_q ? p.N : p.Q)) {                                // the entry is compared, then used
        const int q = by_q ? own : g, n = by_q ? g : own;
        const float* ar = p.a + (int64_t)q * p.H;
        const float* br = p.b + (int64_t)n * p.H;
        double acc = 0.0;
        for (int j = 0; j < p.H; ++j) pair_term(acc, ar[j], br[j]);
        s = pair_total(p.sa[q], p.sb[n], acc);
    }
    (by_q ? p.ref_q : p.ref_n)[own] = s;
}

// grid (ceil(Q / 64), chunks), 256 threads; dynamic LDS pair_sweep_lds(k)
__global__ __launch_bounds__(256) void pair_score_sweep(const PairArgs p) {
    extern __shared__ float pair_lds[];
    float* As = pair_lds;                                  // [64][PAIR_LDP]
    float* Bs = As + KNN_QT * PAIR_LDP;                    // [64][PAIR_LDP]
    float* St = Bs + KNN_BT * PAIR_LDP;                    // [64][KNN_STP]
    const KnnList L = knn_list(St + KNN_QT * KNN_STP, p.k);
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const int tq = tid >> 4, tn = tid & 15;                // pairs (4 tq + i, tn + 16 m)
    const int q0 = blockIdx.x * KNN_QT, nq = min(KNN_QT, p.Q - q0);
    const int b_begin = blockIdx.y * p.chunk, b_end = min(p.N, b_begin + p.chunk);
    // wave 0: the row counts and, as wave 2, the lists of query q0 + l
    const int gq_own = q0 + l;
    const bool rows = w == 0 && p.gt_q && gq_own < p.Q, owner = w == 2 && p.k > 0 && gq_own < p.Q;
    const float row_ref = rows ? p.ref_q[gq_own] : 0.f;
    const int row_g = rows ? p.gt_q[gq_own] : 0;
    int row_cnt = 0, n_list = 0;
    float sa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sa[i] = q0 + 4 * tq + i < p.Q ? p.sa[q0 + 4 * tq + i] : 0.f;

    for (int bb = b_begin; bb < b_end; bb += KNN_BT) {
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[i][m] = 0.0;
        for (int h0 = 0; h0 < p.H; h0 += PAIR_KT) {
            __syncthreads();                               // the previous slice is consumed
            for (int e = tid; e < KNN_QT * PAIR_KT; e += 256) {
                const int r = e / PAIR_KT, c = e % PAIR_KT, gj = h0 + c;
                const int gqr = q0 + r, gbr = bb + r;
                As[r * PAIR_LDP + c] = (gqr < p.Q && gj < p.H) ? p.a[(int64_t)gqr * p.H + gj] : 0.f;
                Bs[r * PAIR_LDP + c] = (gbr < b_end && gj < p.H) ? p.b[(int64_t)gbr * p.H + gj] : 0.f;
            }
            __syncthreads();
            const int jn = min(PAIR_KT, p.H - h0);         // no term past H: softplus(0) is not 0
            for (int j = 0; j < jn; ++j) {
                float av[4], bv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) av[i] = As[(4 * tq + i) * PAIR_LDP + j];
#pragma unroll
                for (int m = 0; m < 4; ++m) bv[m] = Bs[(tn + 16 * m) * PAIR_LDP + j];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int m = 0; m < 4; ++m) pair_term(acc[i][m], av[i], bv[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int col = tn + 16 * m, gbr = bb + col;
            const float sbv = gbr < b_end ? p.sb[gbr] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 4 * tq + i, gqr = q0 + row;
                const float s = pair_total(sa[i], sbv, acc[i][m]);
                St[row * KNN_STP + col] = s;
                if (p.scores && gqr < p.Q && gbr < b_end) p.scores[(int64_t)gqr * p.lds + gbr] = s;
            }
        }
        __syncthreads();
        const int nb = min(KNN_BT, b_end - bb);
        if (rows) {                                        // S > ref, or S == ref at a lower index; nothing compares with NaN
            for (int j = 0; j < nb; ++j) {
                const float s = St[l * KNN_STP + j];
                row_cnt += (s > row_ref || (s == row_ref && bb + j < row_g)) ? 1 : 0;
            }
        } else if (w == 1 && p.gt_n && l < nb) {           // candidate bb + l against the tile's queries
            const int gn = bb + l, g = p.gt_n[gn];
            const float ref = p.ref_n[gn];
            int cnt = 0;
            for (int i = 0; i < nq; ++i) {
                const float s = St[i * KNN_STP + l];
                cnt += (s > ref || (s == ref && q0 + i < g)) ? 1 : 0;
            }
            p.col_part[(int64_t)blockIdx.x * p.N + gn] = cnt;
        } else if (owner) {
            for (int j = 0; j < nb; ++j) {
                const float s = St[l * KNN_STP + j];
                const int b = bb + j;
                if (!(s == s)) continue;                                   // NaN scores are never candidates
                if (n_list == p.k && !vi_better(s, b, L.s[(p.k - 1) * KNN_QT + l], L.i[(p.k - 1) * KNN_QT + l])) continue;
                n_list = knn_offer(L, l, n_list, p.k, s, b, false, 0.f, 0.f);
            }
        }
        // the next write of St follows at least two barriers of the h loop (H >= 1)
    }
    if (rows) p.row_part[(int64_t)blockIdx.y * p.Q + gq_own] = row_cnt;
    if (owner) {
        const int64_t o = ((int64_t)blockIdx.y * p.Q + gq_own) * p.k;
        for (int e = 0; e < p.k; ++e) {
            p.part_s[o + e] = e < n_list ? L.s[e * KNN_QT + l] : -INFINITY;
            p.part_i[o + e] = e < n_list ? L.i[e * KNN_QT + l] : -1;
        }
    }
}

// grid ceil(max(Q, N) / 256), 256 threads
__global__ __launch_bounds__(256) void pair_finish(const PairArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (p.gt_q && i < p.Q) {
        const int g = p.gt_q[i];
        int r = -1;
        if (g >= 0 && g < p.N) {
            r = 0;
            for (int c = 0; c < p.chunks; ++c) r += p.row_part[(int64_t)c * p.Q + i];
        }
        if (p.rank_q) p.rank_q[i] = r;
        if (p.score_q) p.score_q[i] = p.ref_q[i];
    }
    if (p.gt_n && i < p.N) {
        const int g = p.gt_n[i];
        int r = -1;
        if (g >= 0 && g < p.Q) {
            r = 0;
            for (int t = 0; t < p.qtiles; ++t) r += p.col_part[(int64_t)t * p.N + i];
        }
        if (p.rank_n) p.rank_n[i] = r;
        if (p.score_n) p.score_n[i] = p.ref_n[i];
    }
}

}  // namespace imdbn
