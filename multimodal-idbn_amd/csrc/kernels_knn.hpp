// Latent nearest-neighbour search over a bank of codes (imdbn/utils/imdbn_logging.py).
//
// The reference scores one query at a time against the whole validation bank on the CPU, sorts the full score row and walks
// it in Python, skipping the query's own row and (dedup="image") every row whose image key was already seen.  Here a batch
// of queries is one pass over the bank:
//   * knn_row_stats    -- per-row sum and sum of squares in a fixed order (image keys; ||z||^2 of banks and queries);
//   * knn_topk_chunk   -- block = 64 queries x one chunk of the bank.  Sub-tiles of 64 bank rows: query and bank rows are
//                         staged through LDS in k-slices of 32, the 64x64 score tile is computed in registers with the
//                         f32-input MFMA (v_mfma_f32_16x16x4_f32: per score one k-ordered fp32 fma chain over the whole row,
//                         zero-padded to a multiple of 32 -- the same bits whatever the tiling or the other rows), the metric
//                         is applied and the tile goes to LDS, where one thread per query offers its 64 candidates, in bank
//                         order, to the query's key-deduplicated top-k list (LDS).  The chunk's list goes to the workspace.
//   * knn_topk_merge   -- one thread per query offers the chunks' lists to a fresh list and writes the answer.
// A list holds, best first, at most k entries with pairwise different keys; an entry is the best-ranked row seen so far of
// its key (rank: score descending, the lower bank index on ties).  Offering a candidate: if its key is in the list it
// replaces that entry only when it ranks higher; otherwise it is appended (list not full) or replaces the last entry when it
// ranks higher than that.  The result does not depend on the order of the offers, so the per-chunk lists (the chunk's top-k
// keys by per-key maximum) merge to the global answer exactly.  No score matrix reaches HBM.
#pragma once
#include "kernels_rows.hpp"

namespace imdbn {

typedef __attribute__((ext_vector_type(4))) float knn_f32x4;

constexpr int KNN_KMAX = 64;
constexpr int KNN_QT = 64;                 // queries per block (= list owners, the threads of wave 0)
constexpr int KNN_BT = 64;                 // bank rows per sub-tile
constexpr int KNN_KT = 32;                 // depth of one LDS k-slice
constexpr int KNN_LDP = KNN_KT + 1;        // padded row pitch of the staged slices (floats)
constexpr int KNN_STP = KNN_BT + 1;        // padded row pitch of the score tile (floats)

// LDS bytes of knn_topk_chunk for a list capacity k
inline size_t knn_chunk_lds(int k) { return sizeof(float) * (2 * KNN_QT * KNN_LDP + KNN_QT * KNN_STP + 4 * KNN_QT * k); }
inline size_t knn_merge_lds(int k) { return sizeof(float) * 4 * KNN_QT * k; }

// one wave per row: lane l sums columns l, l+64, ... in order, then the fixed xor butterfly
__global__ __launch_bounds__(64 * ROW_WAVES) void knn_row_stats(const float* __restrict__ x, int64_t ldx, int N, int D,
                                                               float* __restrict__ out_sum, float* __restrict__ out_sumsq) {
    const int l = wave_lane();
    const int64_t r = wave_row();
    if (r >= N) return;                                                    // wave-uniform
    const float* row = x + r * ldx;
    float a = 0.f, b = 0.f;
    for (int c = l; c < D; c += 64) {
        const float v = row[c];
        a += v;
        b += v * v;
    }
    a = wave_sum_all(a);
    b = wave_sum_all(b);
    if (l == 0) {
        if (out_sum) out_sum[r] = a;
        if (out_sumsq) out_sumsq[r] = b;
    }
}

// the lists of the 64 owners of a block, entry e of owner t at [e * KNN_QT + t] (consecutive owners in consecutive banks)
struct KnnList {
    float* s; int32_t* i; float* k0; float* k1;
    __device__ void at(int e, int t, float s_, int32_t i_, float a, float b) const {
        s[e * KNN_QT + t] = s_; i[e * KNN_QT + t] = i_; k0[e * KNN_QT + t] = a; k1[e * KNN_QT + t] = b;
    }
};

__device__ __forceinline__ KnnList knn_list(float* base, int k) {
    KnnList L;
    L.s = base;
    L.i = reinterpret_cast<int32_t*>(base + KNN_QT * k);
    L.k0 = base + 2 * KNN_QT * k;
    L.k1 = base + 3 * KNN_QT * k;
    return L;
}

// offer (s, b, key) to owner t's list of n <= k entries; returns the new n
__device__ int knn_offer(const KnnList& L, int t, int n, int k, float s, int b, bool keyed, float a, float c) {
    int p = n;                                                             // the slot freed for the candidate
    if (keyed) {
        for (int e = 0; e < n; ++e) {
            if (L.k0[e * KNN_QT + t] == a && L.k1[e * KNN_QT + t] == c) {
                if (!vi_better(s, b, L.s[e * KNN_QT + t], L.i[e * KNN_QT + t])) return n;
                p = e;
                break;
            }
        }
    }
    if (p == n) {                                                          // a key not in the list
        if (n < k) {
            ++n;
        } else {
            if (!vi_better(s, b, L.s[(k - 1) * KNN_QT + t], L.i[(k - 1) * KNN_QT + t])) return n;
            p = k - 1;                                                     // the last entry drops out
        }
    }
    while (p > 0 && vi_better(s, b, L.s[(p - 1) * KNN_QT + t], L.i[(p - 1) * KNN_QT + t])) {
        const int e = p - 1;
        L.at(p, t, L.s[e * KNN_QT + t], L.i[e * KNN_QT + t], L.k0[e * KNN_QT + t], L.k1[e * KNN_QT + t]);
        p = e;
    }
    L.at(p, t, s, b, a, c);
    return n;
}

struct KnnArgs {
    const float* bank; int64_t ldb; int N; int D;
    const float* bss;                 // [N] ||b||^2 (metric 0 / 2)
    const float* q; int64_t ldq; int Q;
    const float* qss;                 // [Q] ||q||^2 (metric 0 / 2)
    int metric; int k; int chunk;     // chunk: bank rows per block, a multiple of KNN_BT
    const int32_t* exclude;           // [Q] nullable
    const float* key;                 // [N][2] nullable
    float* part_s; int32_t* part_i;   // [chunks][Q][k]
};

// grid (ceil(Q / 64), chunks), 256 threads; dynamic LDS knn_chunk_lds(k)
__global__ __launch_bounds__(256) void knn_topk_chunk(const KnnArgs a) {
    extern __shared__ float knn_lds[];
    float* Qs = knn_lds;                                   // [64][KNN_LDP]
    float* Bs = Qs + KNN_QT * KNN_LDP;                     // [64][KNN_LDP]
    float* St = Bs + KNN_BT * KNN_LDP;                     // [64][KNN_STP]
    const KnnList L = knn_list(St + KNN_QT * KNN_STP, a.k);
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const int q0 = blockIdx.x * KNN_QT;
    const int b_begin = blockIdx.y * a.chunk, b_end = min(a.N, b_begin + a.chunk);
    const int wq = w >> 1, wb = w & 1;                     // wave tile: queries [32 wq, +32) x bank rows [32 wb, +32)
    const int fr = l & 15, fk = l >> 4;                    // operand fragment: row fr, k fk (A[i][k] / B[k][j] of 16x16x4)
    // list owner state (wave 0)
    const int gq_own = q0 + l;
    const bool owner = (w == 0) && gq_own < a.Q;
    const int ex = (owner && a.exclude) ? a.exclude[gq_own] : -1;
    int n = 0;

    for (int bb = b_begin; bb < b_end; bb += KNN_BT) {
        knn_f32x4 acc[2][2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = knn_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < a.D; k0 += KNN_KT) {
            __syncthreads();                               // the previous slice is consumed
            for (int e = tid; e < KNN_QT * KNN_KT; e += 256) {
                const int r = e / KNN_KT, c = e % KNN_KT, gk = k0 + c;
                const int gqr = q0 + r, gbr = bb + r;
                Qs[r * KNN_LDP + c] = (gqr < a.Q && gk < a.D) ? a.q[(int64_t)gqr * a.ldq + gk] : 0.f;
                Bs[r * KNN_LDP + c] = (gbr < b_end && gk < a.D) ? a.bank[(int64_t)gbr * a.ldb + gk] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < KNN_KT; kk += 4) {
                const float a0 = Qs[(32 * wq + fr) * KNN_LDP + kk + fk], a1 = Qs[(32 * wq + 16 + fr) * KNN_LDP + kk + fk];
                const float b0 = Bs[(32 * wb + fr) * KNN_LDP + kk + fk], b1 = Bs[(32 * wb + 16 + fr) * KNN_LDP + kk + fk];
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        // metric epilogue: C/D map of 16x16: column = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 32 * wq + 16 * mi + 4 * fk + r, col = 32 * wb + 16 * ni + fr;
                    const int gqr = q0 + row, gbr = bb + col;
                    const float d = acc[mi][ni][r];
                    float s = d;
                    if (a.metric != 1) {
                        const float qv = gqr < a.Q ? a.qss[gqr] : 0.f, bv = gbr < b_end ? a.bss[gbr] : 0.f;
                        if (a.metric == 0) s = d / fmaxf(sqrtf(qv), 1e-12f) / fmaxf(sqrtf(bv), 1e-12f);
                        else s = -((qv + bv) - 2.f * d);
                    }
                    St[row * KNN_STP + col] = s;
                }
        __syncthreads();
        if (owner) {
            const int nb = min(KNN_BT, b_end - bb);
            for (int j = 0; j < nb; ++j) {
                const float s = St[l * KNN_STP + j];
                const int b = bb + j;
                if (!(s == s) || b == ex) continue;                        // NaN scores are never candidates
                if (n == a.k && !vi_better(s, b, L.s[(a.k - 1) * KNN_QT + l], L.i[(a.k - 1) * KNN_QT + l])) continue;
                float ka = 0.f, kb = 0.f;
                if (a.key) { ka = a.key[2 * (int64_t)b]; kb = a.key[2 * (int64_t)b + 1]; }
                n = knn_offer(L, l, n, a.k, s, b, a.key != nullptr, ka, kb);
            }
        }
        // the next write of St follows at least two barriers of the k loop (D >= 1)
    }
    if (owner) {
        const int64_t o = ((int64_t)blockIdx.y * a.Q + gq_own) * a.k;
        for (int e = 0; e < a.k; ++e) {
            a.part_s[o + e] = e < n ? L.s[e * KNN_QT + l] : -INFINITY;
            a.part_i[o + e] = e < n ? L.i[e * KNN_QT + l] : -1;
        }
    }
}

// grid ceil(Q / 64), 64 threads; dynamic LDS knn_merge_lds(k)
__global__ __launch_bounds__(64) void knn_topk_merge(const float* __restrict__ part_s, const int32_t* __restrict__ part_i, int chunks, int Q,
                                                     int k, const float* __restrict__ key, int32_t* __restrict__ out_idx,
                                                     float* __restrict__ out_score) {
    extern __shared__ float knn_lds[];
    const KnnList L = knn_list(knn_lds, k);
    const int t = threadIdx.x, gq = blockIdx.x * KNN_QT + t;
    if (gq >= Q) return;                                                   // no barriers below
    int n = 0;
    for (int c = 0; c < chunks; ++c) {
        const int64_t o = ((int64_t)c * Q + gq) * k;
        for (int e = 0; e < k; ++e) {
            const int b = part_i[o + e];
            if (b < 0) break;                                              // padding: the chunk's list ends
            const float s = part_s[o + e];
            // a chunk's list is sorted: once an entry cannot enter a full list, none after it can
            if (n == k && !vi_better(s, b, L.s[(k - 1) * KNN_QT + t], L.i[(k - 1) * KNN_QT + t])) break;
            float ka = 0.f, kb = 0.f;
            if (key) { ka = key[2 * (int64_t)b]; kb = key[2 * (int64_t)b + 1]; }
            n = knn_offer(L, t, n, k, s, b, key != nullptr, ka, kb);
        }
    }
    for (int e = 0; e < k; ++e) {
        out_score[(int64_t)gq * k + e] = e < n ? L.s[e * KNN_QT + t] : -INFINITY;
        out_idx[(int64_t)gq * k + e] = e < n ? L.i[e * KNN_QT + t] : -1;
    }
}

}  // namespace imdbn
