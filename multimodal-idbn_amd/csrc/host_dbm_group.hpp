// host_dbm_group.hpp -- host side of imdbn_dbm_group_layer (included by engine.hip inside extern "C"; kernels_dbm_group.hpp;
// DESIGN §42).
//
// Workspace = [counters | slabs | logits], dbm_plan's split (host_dbm.hpp) with the residual region replaced by the [B][N] logits.
// Nothing of it is read before this call has written it; the counters are cleared by a memset node when the axis is split.
// Launch order: [memset] dbm_group_logits dbm_group_finish.

struct DbmGroupPlan { DbmPlan d; size_t off_logits, bytes; };

static DbmGroupPlan dbm_group_plan(int K_lo, int K_hi, int N, int B) {
    DbmGroupPlan p{};
    p.d = dbm_plan(K_lo, K_hi, N, B);
    p.off_logits = p.d.off_res;
    p.bytes = p.off_logits + dbm_align(sizeof(float) * (size_t)B * N);
    return p;
}

size_t imdbn_dbm_group_layer_ws_bytes(int K_lo, int K_hi, int N, int B) {
    if (K_lo < 0 || K_hi < 0 || (int64_t)K_lo + K_hi <= 0 || (int64_t)K_lo + K_hi > INT_MAX || N <= 0 || B <= 0) return 0;
    return dbm_group_plan(K_lo, K_hi, N, B).bytes;
}

int imdbn_dbm_group_layer(const float* W_lo, int64_t ldw_lo, int K_lo, const float* x_lo, int64_t ldx_lo, float s_lo,
                          const float* W_hi, int64_t ldw_hi, int K_hi, const float* x_hi, int64_t ldx_hi, float s_hi,
                          const float* bias, int N, int B, int mode, int n_groups, const int* group_end,
                          float* m, int64_t ldm, float damp, float* res,
                          imdbn_rng* rng, float* s, int64_t lds, float* p, int64_t ldp, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    if (N <= 0 || B <= 0) return fail(IMDBN_E_INVALID, "dbm_group_layer: N = %d units, B = %d rows", N, B);
    if (K_lo < 0 || K_hi < 0) return fail(IMDBN_E_INVALID, "dbm_group_layer: K_lo = %d, K_hi = %d", K_lo, K_hi);
    if (!x_lo) K_lo = 0;                         // a side is absent with x = NULL or K = 0
    if (!x_hi) K_hi = 0;
    if (K_lo == 0 && K_hi == 0) return fail(IMDBN_E_INVALID, "dbm_group_layer: both sides are absent");
    if ((int64_t)K_lo + K_hi > INT_MAX) return fail(IMDBN_E_INVALID, "dbm_group_layer: K_lo + K_hi = %lld", (long long)K_lo + K_hi);
    if (K_lo > 0 && (!W_lo || ldw_lo < N || ldx_lo < K_lo))
        return fail(IMDBN_E_INVALID, "dbm_group_layer: lo side: W %p, ldw %lld (N %d), ldx %lld (K %d)", (const void*)W_lo, (long long)ldw_lo, N, (long long)ldx_lo, K_lo);
    if (K_hi > 0 && (!W_hi || ldw_hi < K_hi || ldx_hi < K_hi))
        return fail(IMDBN_E_INVALID, "dbm_group_layer: hi side: W %p, ldw %lld, ldx %lld (K %d)", (const void*)W_hi, (long long)ldw_hi, (long long)ldx_hi, K_hi);
    if (!bias) return fail(IMDBN_E_INVALID, "dbm_group_layer: null bias");
    if (mode != IMDBN_PARITY_F32 && mode != IMDBN_FAST_BF16) return fail(IMDBN_E_INVALID, "dbm_group_layer: bad mode %d", mode);
    if (n_groups < 1 || n_groups > IMDBN_MAX_GROUPS || !group_end)
        return fail(IMDBN_E_INVALID, "dbm_group_layer: %d groups (1 to %d), group_end %p", n_groups, IMDBN_MAX_GROUPS, (const void*)group_end);
    for (int g = 0, g0 = 0; g < n_groups; g0 = group_end[g], ++g) {
        const int64_t wd = (int64_t)group_end[g] - g0;
        if (wd < 2 || wd > GROUP_WMAX)
            return fail(IMDBN_E_INVALID, "dbm_group_layer: group %d = [%d, %d) is %lld wide (2 to %d)", g, g0, group_end[g], (long long)wd, GROUP_WMAX);
    }
    if (group_end[n_groups - 1] != N)
        return fail(IMDBN_E_INVALID, "dbm_group_layer: the groups end at %d, the layer has N = %d units", group_end[n_groups - 1], N);
    if ((m != nullptr) == (s != nullptr)) return fail(IMDBN_E_INVALID, "dbm_group_layer: exactly one of m (mean field) and s (sample) must be set");
    if (m) {
        if (ldm < N) return fail(IMDBN_E_INVALID, "dbm_group_layer: ldm %lld < N %d", (long long)ldm, N);
        if (!(damp >= 0.0f && damp < 1.0f)) return fail(IMDBN_E_INVALID, "dbm_group_layer: damp = %g outside [0, 1)", (double)damp);
    } else {
        if (lds < N || (p && ldp < N)) return fail(IMDBN_E_INVALID, "dbm_group_layer: lds %lld / ldp %lld < N %d", (long long)lds, (long long)ldp, N);
        if (!rng) return fail(IMDBN_E_INVALID, "dbm_group_layer: sample mode needs an rng");
        CHK(tape_room("dbm_group_layer", rng, 0, (int64_t)n_groups * B));
    }
    if (!ws) return fail(IMDBN_E_WORKSPACE, "dbm_group_layer: null workspace");
    if (((uintptr_t)ws & 255) != 0) return fail(IMDBN_E_INVALID, "dbm_group_layer: workspace %p is not 256-byte aligned", ws);
    const DbmGroupPlan pl = dbm_group_plan(K_lo, K_hi, N, B);
    if (ws_bytes < pl.bytes)
        return fail(IMDBN_E_WORKSPACE, "dbm_group_layer: workspace %zu < %zu bytes needed for K_lo=%d K_hi=%d N=%d B=%d", ws_bytes, pl.bytes, K_lo, K_hi, N, B);
    hipStream_t st = S(stream);
    char* w8 = (char*)ws;
    DbmGroupArgs a;
    memset(&a, 0, sizeof(a));
    a.W_lo = W_lo; a.ldw_lo = ldw_lo; a.K_lo = K_lo; a.x_lo = x_lo; a.ldx_lo = ldx_lo; a.s_lo = s_lo;
    a.W_hi = W_hi; a.ldw_hi = ldw_hi; a.K_hi = K_hi; a.x_hi = x_hi; a.ldx_hi = ldx_hi; a.s_hi = s_hi;
    a.bias = bias; a.N = N; a.B = B;
    a.ks = pl.d.ks; a.kchunk = pl.d.kchunk; a.ntiles = pl.d.ntiles;
    a.slabs = (float*)(w8 + pl.d.off_slabs); a.counters = (int*)(w8 + pl.d.off_cnt);
    a.logits = (float*)(w8 + pl.off_logits);
    DbmGroupFinishArgs f;
    memset(&f, 0, sizeof(f));
    f.logits = a.logits; f.N = N; f.B = B; f.n_groups = n_groups;
    for (int g = 0; g < n_groups; ++g) f.end[g] = group_end[g];
    f.m = m; f.ldm = ldm; f.damp = damp; f.res = res;
    f.s = s; f.lds = lds; f.p = p; f.ldp = ldp;
    Rng cur(rng);
    if (s) {
        cur.cats(B, n_groups, &f.cat_tape, &f.cat_uni);
        CHK(cur.finish());
    }
    if (pl.d.ks > 1) HIPCHK(hipMemsetAsync(w8 + pl.d.off_cnt, 0, sizeof(int) * (size_t)pl.d.zc * pl.d.ntiles, st));
    hipLaunchKernelGGL(dbm_group_logits, dim3(pl.d.ntiles, pl.d.ks, pl.d.zc), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    const dim3 grid(cdiv(B, ROW_WAVES)), block(64 * ROW_WAVES);
    if (s) hipLaunchKernelGGL(dbm_group_finish<true>, grid, block, 0, st, f);
    else   hipLaunchKernelGGL(dbm_group_finish<false>, grid, block, 0, st, f);
    HIPCHK(hipGetLastError());
    return 0;
}
