// host_dbm.hpp -- host side of imdbn_dbm_layer (included by engine.hip inside extern "C"; kernels_dbm.hpp).
//
// Workspace = [counters | slabs | res_part], every region rounded up to 256 bytes.  Nothing of it is read before this call has
// written it: a caller's workspace may hold anything, so the counters are cleared by a memset node at the head of every call that
// splits K.  The kernel's own reset (the last arriver stores zero again) is therefore belt and braces: no test can tell it from the
// memset, as with tap_half.
// Launch order: [memset] dbm_layer [dbm_rows_finish].

struct DbmPlan { int ntiles, zc, ks, kchunk; size_t off_cnt, off_slabs, off_res, bytes; };

static size_t dbm_align(size_t b) { return (b + 255) & ~(size_t)255; }

// K slices of the concatenated axis: about two blocks per CU, at most 16 slices of kchunk >= four stages (128 steps) each; the last
// slice may be shorter.  A function of (K_lo + K_hi, N, B) and the CU count
static DbmPlan dbm_plan(int K_lo, int K_hi, int N, int B) {
    DbmPlan p{};
    const int K = K_lo + K_hi;
    p.ntiles = cdiv(N, DBM_TN);
    p.zc = cdiv(B, DBM_BM);
    int ks = (2 * std::max(cu_count(), 1)) / std::max(1, p.ntiles * p.zc);
    ks = std::max(1, std::min(std::min(ks, 16), K / (4 * DBM_KC)));
    p.kchunk = rup(cdiv(K, ks), DBM_KC);
    p.ks = cdiv(K, p.kchunk);
    p.off_cnt = 0;
    p.off_slabs = dbm_align(sizeof(int) * (size_t)p.zc * p.ntiles);
    p.off_res = p.off_slabs + dbm_align(p.ks > 1 ? sizeof(float) * (size_t)p.zc * p.ks * p.ntiles * DBM_BM * DBM_TN : (size_t)0);
    p.bytes = p.off_res + dbm_align(sizeof(float) * (size_t)p.ntiles * B);
    return p;
}

size_t imdbn_dbm_layer_ws_bytes(int K_lo, int K_hi, int N, int B) {
    if (K_lo < 0 || K_hi < 0 || (int64_t)K_lo + K_hi <= 0 || (int64_t)K_lo + K_hi > INT_MAX || N <= 0 || B <= 0) return 0;
    return dbm_plan(K_lo, K_hi, N, B).bytes;
}

int imdbn_dbm_layer(const float* W_lo, int64_t ldw_lo, int K_lo, const float* x_lo, int64_t ldx_lo, float s_lo,
                    const float* W_hi, int64_t ldw_hi, int K_hi, const float* x_hi, int64_t ldx_hi, float s_hi,
                    const float* bias, int N, int B, int mode, float* m, int64_t ldm, float damp, float* res,
                    imdbn_rng* rng, float* s, int64_t lds, float* p, int64_t ldp, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    if (N <= 0 || B <= 0) return fail(IMDBN_E_INVALID, "dbm_layer: N = %d units, B = %d rows", N, B);
    if (K_lo < 0 || K_hi < 0) return fail(IMDBN_E_INVALID, "dbm_layer: K_lo = %d, K_hi = %d", K_lo, K_hi);
    if (!x_lo) K_lo = 0;                         // a side is absent with x = NULL or K = 0
    if (!x_hi) K_hi = 0;
    if (K_lo == 0 && K_hi == 0) return fail(IMDBN_E_INVALID, "dbm_layer: both sides are absent");
    if ((int64_t)K_lo + K_hi > INT_MAX) return fail(IMDBN_E_INVALID, "dbm_layer: K_lo + K_hi = %lld", (long long)K_lo + K_hi);
    if (K_lo > 0 && (!W_lo || ldw_lo < N || ldx_lo < K_lo))
        return fail(IMDBN_E_INVALID, "dbm_layer: lo side: W %p, ldw %lld (N %d), ldx %lld (K %d)", (const void*)W_lo, (long long)ldw_lo, N, (long long)ldx_lo, K_lo);
    if (K_hi > 0 && (!W_hi || ldw_hi < K_hi || ldx_hi < K_hi))
        return fail(IMDBN_E_INVALID, "dbm_layer: hi side: W %p, ldw %lld, ldx %lld (K %d)", (const void*)W_hi, (long long)ldw_hi, (long long)ldx_hi, K_hi);
    if (!bias) return fail(IMDBN_E_INVALID, "dbm_layer: null bias");
    if (mode != IMDBN_PARITY_F32 && mode != IMDBN_FAST_BF16) return fail(IMDBN_E_INVALID, "dbm_layer: bad mode %d", mode);
    if ((m != nullptr) == (s != nullptr)) return fail(IMDBN_E_INVALID, "dbm_layer: exactly one of m (mean field) and s (sample) must be set");
    if (m) {
        if (ldm < N) return fail(IMDBN_E_INVALID, "dbm_layer: ldm %lld < N %d", (long long)ldm, N);
        if (!(damp >= 0.0f && damp < 1.0f)) return fail(IMDBN_E_INVALID, "dbm_layer: damp = %g outside [0, 1)", (double)damp);
    } else {
        if (lds < N || (p && ldp < N)) return fail(IMDBN_E_INVALID, "dbm_layer: lds %lld / ldp %lld < N %d", (long long)lds, (long long)ldp, N);
        if (!rng) return fail(IMDBN_E_INVALID, "dbm_layer: sample mode needs an rng");
        CHK(tape_room("dbm_layer", rng, (int64_t)B * N, 0));
    }
    if (!ws) return fail(IMDBN_E_WORKSPACE, "dbm_layer: null workspace");
    if (((uintptr_t)ws & 255) != 0) return fail(IMDBN_E_INVALID, "dbm_layer: workspace %p is not 256-byte aligned", ws);
    const DbmPlan pl = dbm_plan(K_lo, K_hi, N, B);
    if (ws_bytes < pl.bytes)
        return fail(IMDBN_E_WORKSPACE, "dbm_layer: workspace %zu < %zu bytes needed for K_lo=%d K_hi=%d N=%d B=%d", ws_bytes, pl.bytes, K_lo, K_hi, N, B);
    hipStream_t st = S(stream);
    char* w8 = (char*)ws;
    DbmLayerArgs a;
    memset(&a, 0, sizeof(a));
    a.W_lo = W_lo; a.ldw_lo = ldw_lo; a.K_lo = K_lo; a.x_lo = x_lo; a.ldx_lo = ldx_lo; a.s_lo = s_lo;
    a.W_hi = W_hi; a.ldw_hi = ldw_hi; a.K_hi = K_hi; a.x_hi = x_hi; a.ldx_hi = ldx_hi; a.s_hi = s_hi;
    a.bias = bias; a.N = N; a.B = B;
    a.m = m; a.ldm = ldm; a.damp = damp; a.res_part = (float*)(w8 + pl.off_res);
    a.s = s; a.lds = lds; a.p = p; a.ldp = ldp;
    a.ks = pl.ks; a.kchunk = pl.kchunk; a.ntiles = pl.ntiles;
    a.slabs = (float*)(w8 + pl.off_slabs); a.counters = (int*)(w8 + pl.off_cnt);
    Rng cur(rng);
    if (s) {
        a.uni = cur.floats(B, N);
        CHK(cur.finish());
    }
    if (pl.ks > 1) HIPCHK(hipMemsetAsync(w8 + pl.off_cnt, 0, sizeof(int) * (size_t)pl.zc * pl.ntiles, st));
    const dim3 grid(pl.ntiles, pl.ks, pl.zc);
    if (s) hipLaunchKernelGGL(dbm_layer<true>, grid, dim3(256), 0, st, a);
    else   hipLaunchKernelGGL(dbm_layer<false>, grid, dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    if (m && res) {
        hipLaunchKernelGGL(dbm_rows_finish, dim3(cdiv(B, 256)), dim3(256), 0, st, (const float*)a.res_part, pl.ntiles, B, res);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
