// Unit moments (imdbn/utils/unit_tuning.py): the sufficient statistics of an activation matrix act[B][H] for per-unit tuning
// curves and regressions, in one pass over act.  With cls[B] a class per row and x[B][R] regressors, z = [1, x_1 .. x_R]:
//   cls_sum[k][h] += sum_{rows of class k} a      cls_sumsq[k][h] += sum a^2      cls_count[k] += #rows
//   xa[q][h] += sum_{used rows} z_q a             aa[h] += sum a^2                xx[p][q] += sum z_p z_q      rows += (used, skipped)
// A row is USED when its class lies in [0, K) (always, without cls) and its R regressors are finite; every other row is skipped
// from every sum and counted.  Every product is formed in double from fp32 factors (exact) and every sum is a double sum.
//
// Three launches, nothing floating-point is ever added atomically:
//   um_sort      one block of 8 waves.  A stable counting sort of the used rows by class into order[]: wave w owns the row range
//                [w per, (w + 1) per), per = ceil(B / 8); the offsets come from a (class-major, wave-minor) exclusive scan of the
//                per-wave histograms, and a wave places its rows 64 at a time, equal classes by ascending lane.  So order[] lists
//                class 0's rows ascending, then class 1's, ...  Each class's run is cut into SEGMENTS of UM_CH rows (the last one
//                shorter); segments are numbered class-major.  Without cls all used rows are one class.  The counts go out here.
//   um_segments  block (column tile of 64, segment s), 4 waves.  Lane l holds column 64 tile + l; wave w adds the segment's rows
//                w, w + 4, w + 8, ... in that order into its own doubles (a, a^2, x_1 a .. x_R a), starting from 0; the four waves'
//                values are then added in wave order 0, 1, 2, 3 and the result is the segment's partial record part[s][q][h].
//                (R + 1)^2 further blocks make xx: entry (p, q) is summed by thread t over the positions t, t + 256, ... of order[],
//                ascending, then the xor butterfly 32 .. 1 within each wave, then the waves in order.
//   um_combine   one thread per column.  Layer k < K adds class k's segment partials in ascending segment order, starting from 0, and
//                adds the total to cls_sum / cls_sumsq; layer K + q adds ALL segments' partials of quantity q (a, a^2, x_1 a, ..) in
//                ascending segment order and adds the total to xa[0] / aa / xa[1 + r].
// Every order is a function of (B, H, K, R) and of which rows are used in which class: the same call leaves the same bits.  The
// accumulators are read, added to and written back by one thread each (calls on one stream are ordered).  Every workspace word that
// is read has been written by an earlier launch of the same call.
#pragma once
#include "kernels_rows.hpp"

namespace imdbn {

constexpr int UM_KMAX = 1024;                    // classes
constexpr int UM_RMAX = 8;                       // regressors
constexpr int UM_CH = 256;                       // rows per segment
constexpr int UM_SORT_WAVES = 8;
constexpr int UM_TILE = 64;                      // columns per block = lanes

struct UmSeg { int32_t start, len; };            // positions [start, start + len) of order[]

struct UmArgs {
    const float* act; int64_t lda;
    const int32_t* cls;                          // nullable
    const float* x; int64_t ldx;                 // nullable with R = 0
    int B, H, K, R;
    int KK;                                      // max(K, 1): classes of the sort
    int tiles, seg_max;                          // ceil(H / 64); KK + ceil(B / UM_CH) >= the number of segments
    // workspace
    int32_t* key;                                // [B] class of a used row, KK for a skipped one
    int32_t* order;                              // [B] used rows, class-major, ascending within a class
    UmSeg* seg;                                  // [seg_max]
    int32_t* cls_seg;                            // [KK + 1] first segment of class k; [KK] = number of segments
    int32_t* hdr;                                // [0] segments, [1] used rows
    double* part;                                // [seg_max][R + 2][H]: a, a^2, x_1 a, .. x_R a
    // accumulators
    double *cls_sum, *cls_sumsq, *xa, *aa, *xx;
    long long *cls_count, *rows;
};

// exclusive scan of v[0 .. 1024) by one wave: lane l owns the 16 entries from 16 l on; returns the total
__device__ __forceinline__ int um_scan_1024(int* v, int l) {
    int loc[16], s = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) { loc[i] = v[16 * l + i]; s += loc[i]; }
    int inc = s;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (l >= o) inc += t;
    }
    int run = inc - s;
#pragma unroll
    for (int i = 0; i < 16; ++i) { v[16 * l + i] = run; run += loc[i]; }
    return __shfl(inc, 63);
}

__global__ __launch_bounds__(64 * UM_SORT_WAVES) void um_sort(const UmArgs a) {
    __shared__ int cnt[UM_SORT_WAVES][UM_KMAX];          // per-wave histogram, then per-wave write offsets
    __shared__ int base[UM_KMAX], nseg[UM_KMAX], tot[UM_KMAX];
    __shared__ int totals[2];
    const int t = threadIdx.x, l = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), KK = a.KK;
    for (int i = t; i < UM_SORT_WAVES * UM_KMAX; i += 64 * UM_SORT_WAVES) (&cnt[0][0])[i] = 0;
    __syncthreads();
    const int64_t per = ((int64_t)a.B + UM_SORT_WAVES - 1) / UM_SORT_WAVES;
    const int64_t B = a.B, lo = per * w < B ? per * w : B, hi = lo + per < B ? lo + per : B;
    for (int64_t r = lo + l; r < hi; r += 64) {
        int k = 0;
        if (a.cls) {
            const int c = a.cls[r];
            k = (c >= 0 && c < a.K) ? c : KK;
        }
        for (int j = 0; j < a.R; ++j)
            if (!(fabsf(a.x[r * a.ldx + j]) <= 3.402823466e+38f)) k = KK;      // inf or NaN
        a.key[r] = k;
        if (k < KK) atomicAdd(&cnt[w][k], 1);
    }
    __syncthreads();
    for (int k = t; k < UM_KMAX; k += 64 * UM_SORT_WAVES) {
        int s = 0;
#pragma unroll
        for (int v = 0; v < UM_SORT_WAVES; ++v) s += cnt[v][k];
        tot[k] = s; base[k] = s; nseg[k] = (s + UM_CH - 1) / UM_CH;
    }
    __syncthreads();
    if (w == 0) {
        const int n = um_scan_1024(base, l), S = um_scan_1024(nseg, l);
        if (l == 0) { totals[0] = S; totals[1] = n; }
    }
    __syncthreads();
    for (int k = t; k < KK; k += 64 * UM_SORT_WAVES) {
        int run = base[k];
#pragma unroll
        for (int v = 0; v < UM_SORT_WAVES; ++v) { const int c = cnt[v][k]; cnt[v][k] = run; run += c; }
        a.cls_seg[k] = nseg[k];
        for (int j = 0, left = tot[k]; left > 0; ++j, left -= UM_CH) {
            UmSeg s; s.start = base[k] + j * UM_CH; s.len = min(left, UM_CH);
            a.seg[nseg[k] + j] = s;
        }
        if (a.cls_count && a.K > 0) a.cls_count[k] += tot[k];
    }
    if (t == 0) {
        a.cls_seg[KK] = totals[0];
        a.hdr[0] = totals[0]; a.hdr[1] = totals[1];
        a.rows[0] += totals[1]; a.rows[1] += (long long)a.B - totals[1];
    }
    __syncthreads();
    volatile int* off = &cnt[w][0];                      // this wave's offsets: read and advanced by this wave alone
    for (int64_t r0 = lo; r0 < hi; r0 += 64) {
        const int64_t r = r0 + l;
        const int k = r < hi ? a.key[r] : KK;
        const bool used = k < KK;
        unsigned long long todo = __ballot(used);
        while (todo) {                                   // wave-uniform: one class of this group of 64 rows per turn
            const int src = __ffsll((long long)todo) - 1;
            const int k0 = __shfl(k, src);
            const unsigned long long m = __ballot(used && k == k0);
            const int b = off[k0];
            if (used && k == k0) a.order[b + __popcll(m & ((1ull << l) - 1ull))] = (int32_t)r;
            if (l == src) off[k0] = b + __popcll(m);
            todo &= ~m;
        }
    }
}

// entry (p, q) of xx over the used rows in the order of order[]
__device__ __forceinline__ void um_xx_block(const UmArgs& a, int e, double* red) {
    const int R1 = a.R + 1, p = e / R1, q = e % R1, n = a.hdr[1], t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += 256) {
        const int64_t r = a.order[i];
        const double zp = p ? (double)a.x[r * a.ldx + p - 1] : 1.0, zq = q ? (double)a.x[r * a.ldx + q - 1] : 1.0;
        s += zp * zq;
    }
    s = wave_sum_all(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0 && n > 0) a.xx[e] += ((red[0] + red[1]) + red[2]) + red[3];
}

template <int R>
__global__ __launch_bounds__(256) void um_segments(const UmArgs a) {
    __shared__ double red[4][R + 2][UM_TILE];
    const int64_t nb = (int64_t)a.tiles * a.seg_max;
    if ((int64_t)blockIdx.x >= nb) {
        um_xx_block(a, (int)((int64_t)blockIdx.x - nb), &red[0][0][0]);
        return;
    }
    const int s = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x % (unsigned)a.tiles);
    if (s >= a.hdr[0]) return;                           // block-uniform
    const int l = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), col = tile * UM_TILE + l;
    const bool in = col < a.H;
    const UmSeg sg = a.seg[s];
    const int32_t* ord = a.order + sg.start;
    const float* ac = a.act + (in ? col : 0);
    double acc[R + 2];
#pragma unroll
    for (int q = 0; q < R + 2; ++q) acc[q] = 0.0;
    auto add = [&](float v, const float* xr) {
        const double d = (double)v;
        acc[0] += d; acc[1] += d * d;
#pragma unroll
        for (int j = 0; j < R; ++j) acc[2 + j] += (double)xr[j] * d;
    };
    int i = w;
    for (; i + 12 < sg.len; i += 16) {                   // four rows of this wave in flight
        const int64_t r0 = ord[i], r1 = ord[i + 4], r2 = ord[i + 8], r3 = ord[i + 12];
        const float v0 = in ? ac[r0 * a.lda] : 0.f, v1 = in ? ac[r1 * a.lda] : 0.f, v2 = in ? ac[r2 * a.lda] : 0.f,
                    v3 = in ? ac[r3 * a.lda] : 0.f;
        add(v0, a.x + r0 * a.ldx); add(v1, a.x + r1 * a.ldx); add(v2, a.x + r2 * a.ldx); add(v3, a.x + r3 * a.ldx);
    }
    for (; i < sg.len; i += 4) {
        const int64_t r0 = ord[i];
        add(in ? ac[r0 * a.lda] : 0.f, a.x + r0 * a.ldx);
    }
#pragma unroll
    for (int q = 0; q < R + 2; ++q) red[w][q][l] = acc[q];
    __syncthreads();
    if (!in) return;
    for (int q = w; q < R + 2; q += 4)
        a.part[((int64_t)s * (R + 2) + q) * a.H + col] = ((red[0][q][l] + red[1][q][l]) + red[2][q][l]) + red[3][q][l];
}

// grid (ceil(H / 256), (K > 0 ? K : 0) + R + 2)
__global__ __launch_bounds__(256) void um_combine(const UmArgs a) {
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= a.H) return;
    const int Q = a.R + 2, nk = a.K > 0 ? a.K : 0, y = blockIdx.y;
    const int64_t qs = (int64_t)Q * a.H;                 // doubles per segment record
    if (y < nk) {
        const int s0 = a.cls_seg[y], s1 = a.cls_seg[y + 1];
        if (s1 == s0) return;                            // an empty class leaves its row untouched
        double u = 0.0, v = 0.0;
        for (int s = s0; s < s1; ++s) { u += a.part[s * qs + col]; v += a.part[s * qs + a.H + col]; }
        a.cls_sum[(int64_t)y * a.H + col] += u; a.cls_sumsq[(int64_t)y * a.H + col] += v;
        return;
    }
    const int q = y - nk, S = a.hdr[0];
    if (S == 0) return;
    double u = 0.0;
    const double* p = a.part + (int64_t)q * a.H + col;
#pragma unroll 8
    for (int s = 0; s < S; ++s) u += p[s * qs];
    double* out = q == 1 ? a.aa + col : a.xa + (int64_t)(q == 0 ? 0 : q - 1) * a.H + col;
    *out += u;
}

}  // namespace imdbn
