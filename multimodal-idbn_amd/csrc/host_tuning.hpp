// host_tuning.hpp -- host side of imdbn_unit_moments (included by engine.hip inside extern "C"; kernels_tuning.hpp).
//
// Workspace, every region rounded up to 256 bytes, in this order (seg_max = max(K, 1) + ceil(B / 256)):
//   key [B] int32      order [B] int32      seg [seg_max] (start, len)      cls_seg [max(K, 1) + 1] int32      hdr [2] int32
//   part [seg_max][R + 2][H] double
// Launch order: um_sort; um_segments<R> (tiles x seg_max blocks and (R + 1)^2 blocks for xx); um_combine.

struct UmSizes { size_t key, seg, cls_seg, hdr, part, total; int KK, tiles, seg_max; };

static bool um_sizes(int B, int H, int K, int R, UmSizes* z) {
    if (B < 1 || H < 1 || K < 0 || K > UM_KMAX || R < 0 || R > UM_RMAX) return false;
    z->KK = std::max(K, 1);
    z->tiles = (int)(((int64_t)H + UM_TILE - 1) / UM_TILE);
    z->seg_max = (int)std::min<int64_t>((int64_t)z->KK + ((int64_t)B + UM_CH - 1) / UM_CH, INT_MAX);
    z->key = knn_align(sizeof(int32_t) * (size_t)B);
    z->seg = knn_align(sizeof(UmSeg) * (size_t)z->seg_max);
    z->cls_seg = knn_align(sizeof(int32_t) * (size_t)(z->KK + 1));
    z->hdr = knn_align(2 * sizeof(int32_t));
    z->part = knn_align(sizeof(double) * (size_t)z->seg_max * (size_t)(R + 2) * (size_t)H);
    z->total = 2 * z->key + z->seg + z->cls_seg + z->hdr + z->part;
    return true;
}

size_t imdbn_unit_moments_ws_bytes(int B, int H, int K, int R) {
    UmSizes z;
    return um_sizes(B, H, K, R, &z) ? z.total : 0;
}

int imdbn_unit_moments(const float* act, int64_t lda, int B, int H, const int32_t* cls, int K, const float* x, int64_t ldx, int R,
                       double* cls_sum, double* cls_sumsq, long long* cls_count, double* xa, double* aa, double* xx, long long* rows,
                       void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    if (B < 1) return fail(IMDBN_E_INVALID, "unit_moments: B = %d (must be >= 1)", B);
    if (H < 1) return fail(IMDBN_E_INVALID, "unit_moments: H = %d (must be >= 1)", H);
    if (R < 0 || R > UM_RMAX) return fail(IMDBN_E_INVALID, "unit_moments: R = %d outside [0, %d]", R, UM_RMAX);
    if (K < 0 || K > UM_KMAX) return fail(IMDBN_E_INVALID, "unit_moments: K = %d outside [0, %d]", K, UM_KMAX);
    if (cls && K < 1) return fail(IMDBN_E_INVALID, "unit_moments: cls given with K = %d (must be >= 1)", K);
    if (!cls && K != 0) return fail(IMDBN_E_INVALID, "unit_moments: K = %d without cls (must be 0)", K);
    if (!act) return fail(IMDBN_E_INVALID, "unit_moments: null act");
    if (lda < H) return fail(IMDBN_E_INVALID, "unit_moments: lda %lld < H %d", (long long)lda, H);
    if ((x != nullptr) != (R > 0)) return fail(IMDBN_E_INVALID, "unit_moments: R = %d with %s x", R, x ? "a non-null" : "a null");
    if (x && ldx < R) return fail(IMDBN_E_INVALID, "unit_moments: ldx %lld < R %d", (long long)ldx, R);
    if (cls && (!cls_sum || !cls_sumsq || !cls_count))
        return fail(IMDBN_E_INVALID, "unit_moments: null accumulator %s with cls given", !cls_sum ? "cls_sum" : (!cls_sumsq ? "cls_sumsq" : "cls_count"));
    if (!xa || !aa || !xx || !rows)
        return fail(IMDBN_E_INVALID, "unit_moments: null accumulator %s", !xa ? "xa" : (!aa ? "aa" : (!xx ? "xx" : "rows")));
    UmSizes z;
    um_sizes(B, H, K, R, &z);
    const int64_t blocks = (int64_t)z.tiles * z.seg_max + (int64_t)(R + 1) * (R + 1);
    if (blocks > INT_MAX) return fail(IMDBN_E_INVALID, "unit_moments: B = %d rows x H = %d columns need %lld blocks (at most %d)", B, H, (long long)blocks, INT_MAX);
    if (!ws || ((uintptr_t)ws & 255) != 0 || ws_bytes < z.total)
        return fail(IMDBN_E_INVALID, "unit_moments: workspace %zu < %zu bytes (or null / not 256-byte aligned)", ws_bytes, z.total);
    UmArgs a;
    memset(&a, 0, sizeof(a));
    a.act = act; a.lda = lda; a.cls = cls; a.x = x; a.ldx = ldx; a.B = B; a.H = H; a.K = K; a.R = R;
    a.KK = z.KK; a.tiles = z.tiles; a.seg_max = z.seg_max;
    char* p = (char*)ws;
    a.key = (int32_t*)p; p += z.key;
    a.order = (int32_t*)p; p += z.key;
    a.seg = (UmSeg*)p; p += z.seg;
    a.cls_seg = (int32_t*)p; p += z.cls_seg;
    a.hdr = (int32_t*)p; p += z.hdr;
    a.part = (double*)p;
    a.cls_sum = cls_sum; a.cls_sumsq = cls_sumsq; a.cls_count = cls_count; a.xa = xa; a.aa = aa; a.xx = xx; a.rows = rows;
    const hipStream_t st = S(stream);
    hipLaunchKernelGGL(um_sort, dim3(1), dim3(64 * UM_SORT_WAVES), 0, st, a);
    HIPCHK(hipGetLastError());
    const unsigned nb = (unsigned)blocks;
    static void (*const segments[UM_RMAX + 1])(const UmArgs) = {um_segments<0>, um_segments<1>, um_segments<2>, um_segments<3>, um_segments<4>,
                                                                um_segments<5>, um_segments<6>, um_segments<7>, um_segments<8>};
    hipLaunchKernelGGL(segments[R], dim3(nb), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(um_combine, dim3((unsigned)(((int64_t)H + 255) / 256), (unsigned)(K + R + 2)), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    return 0;
}
