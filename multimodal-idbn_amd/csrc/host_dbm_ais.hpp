// host_dbm_ais.hpp -- host side of imdbn_dbm_rowsum_layer and imdbn_dbm_ais (included by engine.hip inside extern "C";
// kernels_dbm_ais.hpp).
//
// One layer: workspace = [counters | slabs | part], dbm_plan's split (host_dbm.hpp) with the residual region replaced by the
// [tile][B] doubles.  Launch order: [memset] [dbm_rows_bias_dot] dbm_rowsum_layer [dbm_rowsum_finish].
// The whole run: workspace = [counters | slabs | part | state_0 .. state_L], the first three regions the largest any layer needs,
// the states fp32 [M][N_l] (an odd layer whose out_s entry is set lives in the caller's tensor instead).  The counters are cleared
// ONCE, at the head of the call: every launch leaves them zero (the last arriver's store), and the run depends on it.
// Launch order: memset, dbm_rows_bias_dot<draw> per odd layer, then per temperature k = 1 .. K
//     even layers bottom to top   dbm_rowsum_layer<WEIGH> (sampling at beta_k unless k = K), dbm_rowsum_finish (scale 1)
//     odd layers bottom to top    dbm_rowsum_layer<SAMPLE> at beta_k, dbm_rowsum_finish (scale beta_{k+1} - beta_k)     (k < K)

struct DbmRowsumPlan { DbmPlan d; size_t off_part, bytes; };

static DbmRowsumPlan dbm_rowsum_plan(int K_lo, int K_hi, int N, int B) {
    DbmRowsumPlan p{};
    p.d = dbm_plan(K_lo, K_hi, N, B);
    p.off_part = p.d.off_res;
    p.bytes = p.off_part + dbm_align(sizeof(double) * (size_t)p.d.ntiles * B);
    return p;
}

size_t imdbn_dbm_rowsum_layer_ws_bytes(int K_lo, int K_hi, int N, int B) {
    if (K_lo < 0 || K_hi < 0 || (int64_t)K_lo + K_hi <= 0 || (int64_t)K_lo + K_hi > INT_MAX || N <= 0 || B <= 0) return 0;
    return dbm_rowsum_plan(K_lo, K_hi, N, B).bytes;
}

// the operand fields of one layer call; the split comes from `pl`, its regions from the three pointers
static DbmRowsumArgs dbm_rowsum_args(const float* W_lo, int64_t ldw_lo, int K_lo, const float* x_lo, int64_t ldx_lo,
                                     const float* W_hi, int64_t ldw_hi, int K_hi, const float* x_hi, int64_t ldx_hi,
                                     const float* bias, int N, int B, const DbmPlan& pl, int* counters, float* slabs, double* part) {
    DbmRowsumArgs a;
    memset(&a, 0, sizeof(a));
    a.W_lo = W_lo; a.ldw_lo = ldw_lo; a.K_lo = K_lo; a.x_lo = x_lo; a.ldx_lo = ldx_lo; a.s_lo = 1.0f;
    a.W_hi = W_hi; a.ldw_hi = ldw_hi; a.K_hi = K_hi; a.x_hi = x_hi; a.ldx_hi = ldx_hi; a.s_hi = 1.0f;
    a.bias = bias; a.N = N; a.B = B;
    a.ks = pl.ks; a.kchunk = pl.kchunk; a.ntiles = pl.ntiles;
    a.counters = counters; a.slabs = slabs; a.part = part;
    return a;
}

// the layer kernel and, with `acc`, its finish
static int dbm_rowsum_launch(const DbmRowsumArgs& a, const DbmPlan& pl, int mode, double scale, double* acc, hipStream_t st) {
    const dim3 grid(pl.ntiles, pl.ks, pl.zc);
    if (mode == DBM_WEIGH) hipLaunchKernelGGL(dbm_rowsum_layer<DBM_WEIGH>, grid, dim3(256), 0, st, a);
    else if (mode == DBM_SAMPLE) hipLaunchKernelGGL(dbm_rowsum_layer<DBM_SAMPLE>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(dbm_rowsum_layer<DBM_BOUND>, grid, dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    if (acc) {
        hipLaunchKernelGGL(dbm_rowsum_finish, dim3(cdiv(a.B, 256)), dim3(256), 0, st, (const double*)a.part, pl.ntiles, a.B, scale, acc);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

int imdbn_dbm_rowsum_layer(const float* W_lo, int64_t ldw_lo, int K_lo, const float* x_lo, int64_t ldx_lo,
                           const float* W_hi, int64_t ldw_hi, int K_hi, const float* x_hi, int64_t ldx_hi,
                           const float* bias, int N, int B, int mode, float beta, float beta_prev, double dbeta_next,
                           const float* base, const float* mu, int64_t ldmu,
                           imdbn_rng* rng, float* s, int64_t lds, float* p, int64_t ldp, double* acc,
                           void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    if (N <= 0 || B <= 0) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: N = %d units, B = %d rows", N, B);
    if (K_lo < 0 || K_hi < 0) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: K_lo = %d, K_hi = %d", K_lo, K_hi);
    if (!x_lo) K_lo = 0;                         // a side is absent with x = NULL or K = 0
    if (!x_hi) K_hi = 0;
    if (K_lo == 0 && K_hi == 0) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: both sides are absent");
    if ((int64_t)K_lo + K_hi > INT_MAX) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: K_lo + K_hi = %lld", (long long)K_lo + K_hi);
    if (K_lo > 0 && (!W_lo || ldw_lo < N || ldx_lo < K_lo))
        return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: lo side: W %p, ldw %lld (N %d), ldx %lld (K %d)", (const void*)W_lo, (long long)ldw_lo, N, (long long)ldx_lo, K_lo);
    if (K_hi > 0 && (!W_hi || ldw_hi < K_hi || ldx_hi < K_hi))
        return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: hi side: W %p, ldw %lld, ldx %lld (K %d)", (const void*)W_hi, (long long)ldw_hi, (long long)ldx_hi, K_hi);
    if (!bias) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: null bias");
    if (mode != IMDBN_DBM_WEIGH && mode != IMDBN_DBM_SAMPLE && mode != IMDBN_DBM_BOUND) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: bad mode %d", mode);
    if (mode == IMDBN_DBM_BOUND) {
        if (K_hi > 0) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: the bound is one-sided from below, K_hi = %d", K_hi);
        if (!mu || ldmu < N) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: mu %p, ldmu %lld < N %d", (const void*)mu, (long long)ldmu, N);
        if (s || p) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: the bound draws nothing, s and p must be null");
    } else {
        if (!(beta >= 0.0f && beta <= 1.0f)) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: beta = %g outside [0, 1]", (double)beta);
        if (mode == IMDBN_DBM_WEIGH && !(beta_prev >= 0.0f && beta_prev < beta))
            return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: beta_prev = %g is not in [0, beta = %g)", (double)beta_prev, (double)beta);
        if (mode == IMDBN_DBM_SAMPLE && !s) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: sample mode needs s");
        if (!s && p) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: p without s");
        if (s) {
            if (lds < N || (p && ldp < N)) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: lds %lld / ldp %lld < N %d", (long long)lds, (long long)ldp, N);
            if (!rng) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: a draw needs an rng");
            CHK(tape_room("dbm_rowsum_layer", rng, (int64_t)B * N, 0));
        }
    }
    if (mode != IMDBN_DBM_SAMPLE && !acc) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: null acc");
    if (!ws) return fail(IMDBN_E_WORKSPACE, "dbm_rowsum_layer: null workspace");
    if (((uintptr_t)ws & 255) != 0) return fail(IMDBN_E_INVALID, "dbm_rowsum_layer: workspace %p is not 256-byte aligned", ws);
    const DbmRowsumPlan pl = dbm_rowsum_plan(K_lo, K_hi, N, B);
    if (ws_bytes < pl.bytes)
        return fail(IMDBN_E_WORKSPACE, "dbm_rowsum_layer: workspace %zu < %zu bytes needed for K_lo=%d K_hi=%d N=%d B=%d", ws_bytes, pl.bytes, K_lo, K_hi, N, B);
    hipStream_t st = S(stream);
    char* w8 = (char*)ws;
    DbmRowsumArgs a = dbm_rowsum_args(W_lo, ldw_lo, K_lo, x_lo, ldx_lo, W_hi, ldw_hi, K_hi, x_hi, ldx_hi, bias, N, B, pl.d,
                                      (int*)(w8 + pl.d.off_cnt), (float*)(w8 + pl.d.off_slabs), (double*)(w8 + pl.off_part));
    a.beta = beta; a.beta_prev = beta_prev; a.mu = mu; a.ldmu = ldmu;
    a.base = mode == IMDBN_DBM_BOUND ? nullptr : base;
    a.s = s; a.lds = lds; a.p = p; a.ldp = ldp;
    Rng cur(rng);
    if (s) {
        a.uni = cur.floats(B, N);
        CHK(cur.finish());
    }
    if (pl.d.ks > 1) HIPCHK(hipMemsetAsync(w8 + pl.d.off_cnt, 0, sizeof(int) * (size_t)pl.d.zc * pl.d.ntiles, st));
    if (mode == IMDBN_DBM_BOUND && base) {       // the bias term of the layer below: acc[b] += sum_k base_k x_lo[b][k]
        DbmBiasDotArgs d;
        memset(&d, 0, sizeof(d));
        d.bias = base; d.N = K_lo; d.B = B; d.x = x_lo; d.ldx = ldx_lo; d.scale = 1.0; d.first = 0; d.acc = acc;
        hipLaunchKernelGGL(dbm_rows_bias_dot<false>, dim3(cdiv(B, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, st, d);
        HIPCHK(hipGetLastError());
    }
    return dbm_rowsum_launch(a, pl.d, mode, mode == IMDBN_DBM_SAMPLE ? dbeta_next : 1.0, acc, st);
}

// ---- the whole annealing run ---------------------------------------------------------------------------------------------------
struct DbmAisPlan { size_t off_cnt, off_slabs, off_part, off_state[IMDBN_DBM_MAX_LAYERS + 1], bytes, cnt_bytes; };

// layer l of the stack: its sides and its plan
static DbmPlan dbm_ais_layer_plan(int L, const int* sizes, int l, int M) {
    return dbm_plan(l > 0 ? sizes[l - 1] : 0, l < L ? sizes[l + 1] : 0, sizes[l], M);
}

static DbmAisPlan dbm_ais_plan(int L, const int* sizes, int M) {
    DbmAisPlan p{};
    size_t cnt = 0, slabs = 0, part = 0;
    for (int l = 0; l <= L; ++l) {
        const DbmPlan q = dbm_ais_layer_plan(L, sizes, l, M);
        cnt = std::max(cnt, q.off_slabs);
        slabs = std::max(slabs, q.off_res - q.off_slabs);
        part = std::max(part, dbm_align(sizeof(double) * (size_t)q.ntiles * M));
    }
    p.cnt_bytes = cnt;
    p.off_cnt = 0; p.off_slabs = cnt; p.off_part = cnt + slabs;
    size_t off = p.off_part + part;
    for (int l = 0; l <= L; ++l) { p.off_state[l] = off; off += dbm_align(sizeof(float) * (size_t)M * sizes[l]); }
    p.bytes = off;
    return p;
}

static bool dbm_ais_shape_ok(int L, const int* sizes, int M) {
    if (L < 1 || L > IMDBN_DBM_MAX_LAYERS || !sizes || M < 1) return false;
    for (int l = 0; l <= L; ++l)
        if (sizes[l] < 1) return false;
    return true;
}

size_t imdbn_dbm_ais_ws_bytes(int L, const int* sizes, int M) {
    return dbm_ais_shape_ok(L, sizes, M) ? dbm_ais_plan(L, sizes, M).bytes : 0;
}

int imdbn_dbm_ais(int L, const float* const* W, const int64_t* ldw, const int* sizes, const float* const* biases, const float* base,
                  const float* betas, int K, int M, imdbn_rng* rng, double* logw, float* const* out_s, const int64_t* ld_out,
                  void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    if (L < 1 || L > IMDBN_DBM_MAX_LAYERS) return fail(IMDBN_E_INVALID, "dbm_ais: L = %d weight matrices, at most %d", L, IMDBN_DBM_MAX_LAYERS);
    if (!W || !ldw || !sizes || !biases) return fail(IMDBN_E_INVALID, "dbm_ais: null %s", !W ? "W" : (!ldw ? "ldw" : (!sizes ? "sizes" : "biases")));
    // (no descriptor: anneal_check reads it only for the start and output states of an RBM, which this call passes as absent)
    CHK(anneal_check("dbm_ais", nullptr, false, nullptr, 0, M, K, betas, rng, logw, nullptr, 0));
    int64_t odd = 0, all = 0;
    for (int l = 0; l <= L; ++l) {
        if (sizes[l] < 1) return fail(IMDBN_E_INVALID, "dbm_ais: sizes[%d] = %d", l, sizes[l]);
        if (!biases[l]) return fail(IMDBN_E_INVALID, "dbm_ais: null biases[%d]", l);
        if (l < L && (!W[l] || ldw[l] < sizes[l + 1]))
            return fail(IMDBN_E_INVALID, "dbm_ais: W[%d] %p, ldw %lld < N %d", l, (const void*)W[l], (long long)ldw[l], sizes[l + 1]);
        if ((l & 1) && out_s && out_s[l] && (!ld_out || ld_out[l] < sizes[l]))
            return fail(IMDBN_E_INVALID, "dbm_ais: ld_out[%d] %lld < N %d", l, ld_out ? (long long)ld_out[l] : 0ll, sizes[l]);
        all += sizes[l];
        if (l & 1) odd += sizes[l];
    }
    CHK(tape_room("dbm_ais", rng, (int64_t)M * odd + (int64_t)(K - 1) * M * all, 0));
    if (!ws) return fail(IMDBN_E_WORKSPACE, "dbm_ais: null workspace");
    if (((uintptr_t)ws & 255) != 0) return fail(IMDBN_E_INVALID, "dbm_ais: workspace %p is not 256-byte aligned", ws);
    const DbmAisPlan pl = dbm_ais_plan(L, sizes, M);
    if (ws_bytes < pl.bytes) return fail(IMDBN_E_WORKSPACE, "dbm_ais: workspace %zu < %zu bytes needed for L=%d M=%d", ws_bytes, pl.bytes, L, M);
    hipStream_t st = S(stream);
    char* w8 = (char*)ws;
    float* state[IMDBN_DBM_MAX_LAYERS + 1];
    int64_t lds[IMDBN_DBM_MAX_LAYERS + 1];
    for (int l = 0; l <= L; ++l) {
        const bool own = (l & 1) && out_s && out_s[l];
        state[l] = own ? out_s[l] : (float*)(w8 + pl.off_state[l]);
        lds[l] = own ? ld_out[l] : sizes[l];
    }
    Rng cur(rng);
    HIPCHK(hipMemsetAsync(w8 + pl.off_cnt, 0, pl.cnt_bytes, st));
    const double db1 = (double)betas[1] - (double)betas[0];
    for (int l = 1; l <= L; l += 2) {            // the start states and logw = (beta_1 - beta_0) sum_{l odd} b_l s_l
        DbmBiasDotArgs d;
        memset(&d, 0, sizeof(d));
        d.bias = biases[l]; d.N = sizes[l]; d.B = M; d.uni = cur.floats(M, sizes[l]); d.s = state[l]; d.lds = lds[l];
        d.scale = db1; d.first = l == 1; d.acc = logw;
        hipLaunchKernelGGL(dbm_rows_bias_dot<true>, dim3(cdiv(M, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, st, d);
        HIPCHK(hipGetLastError());
    }
    for (int k = 1; k <= K; ++k) {
        for (int parity = 0; parity <= (k < K ? 1 : 0); ++parity) {
            for (int l = parity; l <= L; l += 2) {
                const DbmPlan q = dbm_ais_layer_plan(L, sizes, l, M);
                DbmRowsumArgs a = dbm_rowsum_args(l > 0 ? W[l - 1] : nullptr, l > 0 ? ldw[l - 1] : 0, l > 0 ? sizes[l - 1] : 0,
                                                  l > 0 ? state[l - 1] : nullptr, l > 0 ? lds[l - 1] : 0,
                                                  l < L ? W[l] : nullptr, l < L ? ldw[l] : 0, l < L ? sizes[l + 1] : 0,
                                                  l < L ? state[l + 1] : nullptr, l < L ? lds[l + 1] : 0,
                                                  biases[l], sizes[l], M, q, (int*)(w8 + pl.off_cnt), (float*)(w8 + pl.off_slabs),
                                                  (double*)(w8 + pl.off_part));
                a.beta = betas[k]; a.beta_prev = betas[k - 1];
                a.base = l == 0 ? base : nullptr;
                if (k < K) { a.uni = cur.floats(M, sizes[l]); a.s = state[l]; a.lds = lds[l]; }
                const double scale = parity ? (double)betas[k + 1] - (double)betas[k] : 1.0;
                CHK(dbm_rowsum_launch(a, q, parity ? DBM_SAMPLE : DBM_WEIGH, scale, logw, st));
            }
        }
    }
    return cur.finish();
}
