// Cross-modal label metrics (imdbn/utils/cross_eval.py; reference imdbn.py:615-639 and :764-813) for a batch of p(y | img) rows.
//
// cross_metrics_rows does, per row and without a host round trip: the argmax of p (first maximum), the truth (the first maximum of a
// one-hot / soft row y, or a given index), p_pred / p_true clamped to [1e-9, 1], the rank of the true label in a stable descending
// sort, and the row's binary cross entropy  -(log pt_gt + sum_{j != gt} log(1 - pt_j)),  pt = clamp(p, 1e-6, 1 - 1e-6) in fp32 --
// F.binary_cross_entropy(reduction="sum") against the one-hot truth.  One confusion count per row goes out as an integer atomic.
//
// How the rows are dealt: one wave per row, 4 waves per block, nb = min(ceil(B / 4), CM_MAX_BLOCKS) blocks; wave w of block b takes
// the rows (4 b + w) + i (4 nb), i = 0, 1, ... ascending.  Label c of a row sits in lane c & 63, slot c >> 6 (K <= 256).  A row's
// log sum is: per lane over its slots ascending (in double; the terms are fp32 logf), then the xor butterfly 32, 16, .. 1.  A wave adds
// its rows' sums in the order it meets them and leaves ONE partial record; nothing floating-point is ever added atomically.
//
// cross_metrics_combine then runs 1 + K waves: wave 0 sums the 4 nb partial records (lane l takes records l, l + 64, .. ascending,
// then the same butterfly) and adds the result to acc[0..5]; wave 1 + k sums class k's rows out of the per-row codes (lane l takes
// rows l, l + 64, .. ascending, then the butterfly) and adds to class_sums[k].  Every order depends on (B, K) alone, so the same
// batches leave the same bits; the accumulators are read, added to and written back by one lane each (calls on one stream are ordered).
#pragma once
#include "kernels_rows.hpp"

namespace imdbn {

constexpr int CM_MAX_BLOCKS = 1024;              // 4096 partial records at most (128 KiB of workspace)

struct CmPartial { double ce, mse; int32_t n, top1, topk, skipped; };      // 32 bytes, one per wave of cross_metrics_rows

struct CmArgs {
    const float* p; int64_t ldp;                 // [B][K]
    const float* y; int64_t ldy;                 // [B][K] or null
    const int32_t* gt;                           // [B] or null (exactly one of y / gt)
    const float* row_mse;                        // [B] or null
    int B, K, npix, topk;
    int32_t *pred, *gt_out, *rank;               // [B], nullable
    float *p_pred, *p_true;                      // [B], nullable
    unsigned long long* confusion;               // [K][K] int64 counts, nullable
    int32_t* code;                               // workspace [B]: gt | pred << 8, -1 = skipped row
    CmPartial* part;                             // workspace [4 nb]
};

__global__ __launch_bounds__(64 * ROW_WAVES) void cross_metrics_rows(const CmArgs a) {
    const int l = wave_lane(), wave = wave_row(), stride = gridDim.x * ROW_WAVES;
    const int K = a.K, kk = min(a.topk, K);
    const float lo = 1e-6f, hi = (float)(1.0 - 1e-6);
    double ce = 0.0, mse = 0.0;
    int n = 0, top1 = 0, topk = 0, skipped = 0;
    for (int r = wave; r < a.B; r += stride) {                             // wave-uniform
        float p[4];
        slots_load(p, a.p + (int64_t)r * a.ldp, l, K);
        const int pred = slots_argmax(p, l, K, 0);                         // an all-NaN row gives 0
        int g;
        if (a.y) {
            float yv[4];
            slots_load(yv, a.y + (int64_t)r * a.ldy, l, K);
            g = slots_argmax(yv, l, K, 0);
        } else {
            g = a.gt[r];
        }
        const bool ok = g >= 0 && g < K;
        const float ppred = slots_pick(p, pred);
        if (l == 0) {
            if (a.pred) a.pred[r] = pred;
            if (a.gt_out) a.gt_out[r] = g;
            if (a.p_pred) a.p_pred[r] = fminf(fmaxf(ppred, 1e-9f), 1.0f);
        }
        if (!ok) {                                                         // a caller error: the row is left out and counted
            ++skipped;
            if (l == 0) {
                a.code[r] = -1;
                if (a.p_true) a.p_true[r] = NAN;
                if (a.rank) a.rank[r] = -1;
            }
            continue;
        }
        const float pg = slots_pick(p, g);
        int above = 0;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = l + 64 * q;
            if (c < K) {
                above += (p[q] > pg || (p[q] == pg && c < g)) ? 1 : 0;
                const float pt = fminf(fmaxf(p[q], lo), hi);
                s += (double)(c == g ? logf(pt) : logf(1.0f - pt));
            }
        }
        above = wave_sum_all(above);
        s = wave_sum_all(s);
        ++n;
        top1 += pred == g ? 1 : 0;
        topk += above < kk ? 1 : 0;
        ce -= s;
        if (a.row_mse) mse += (double)a.row_mse[r] * (double)a.npix;
        if (l == 0) {
            a.code[r] = g | (pred << 8);
            if (a.p_true) a.p_true[r] = fminf(fmaxf(pg, 1e-9f), 1.0f);
            if (a.rank) a.rank[r] = above;
            if (a.confusion) atomicAdd(a.confusion + (int64_t)g * K + pred, 1ull);
        }
    }
    if (l == 0) {
        CmPartial o;
        o.ce = ce; o.mse = mse; o.n = n; o.top1 = top1; o.topk = topk; o.skipped = skipped;
        a.part[wave] = o;
    }
}

// block 0: partial records -> acc[0..5]; block 1 + k: the rows of class k -> class_sums[k] = (n, top-1 hits, sum of row_mse)
__global__ __launch_bounds__(64) void cross_metrics_combine(const CmPartial* __restrict__ part, int n_part, const int32_t* __restrict__ code,
                                                            const float* __restrict__ row_mse, int B, double* __restrict__ acc,
                                                            double* __restrict__ class_sums) {
    const int l = threadIdx.x;
    if (blockIdx.x == 0) {
        double ce = 0.0, mse = 0.0;
        int n = 0, top1 = 0, topk = 0, skipped = 0;
        for (int i = l; i < n_part; i += 64) {
            const CmPartial q = part[i];
            ce += q.ce; mse += q.mse; n += q.n; top1 += q.top1; topk += q.topk; skipped += q.skipped;
        }
        ce = wave_sum_all(ce); mse = wave_sum_all(mse);
        n = wave_sum_all(n); top1 = wave_sum_all(top1); topk = wave_sum_all(topk); skipped = wave_sum_all(skipped);
        if (l == 0) {
            acc[0] += (double)n; acc[1] += (double)top1; acc[2] += (double)topk;
            acc[3] += ce; acc[4] += mse; acc[5] += (double)skipped;
        }
        return;
    }
    const int k = blockIdx.x - 1;
    int n = 0, hit = 0;
    double s = 0.0;
    for (int r = l; r < B; r += 64) {
        const int c = code[r];
        if (c >= 0 && (c & 255) == k) {
            ++n;
            hit += (c >> 8) == k ? 1 : 0;
            if (row_mse) s += (double)row_mse[r];
        }
    }
    n = wave_sum_all(n); hit = wave_sum_all(hit); s = wave_sum_all(s);
    if (l == 0) {
        class_sums[3 * k] += (double)n; class_sums[3 * k + 1] += (double)hit; class_sums[3 * k + 2] += s;
    }
}

}  // namespace imdbn
