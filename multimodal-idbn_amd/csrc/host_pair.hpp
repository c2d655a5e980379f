// host_pair.hpp -- host side of imdbn_rbm_pair_scores (included by engine.hip inside extern "C"; kernels_pair.hpp).
//
// Workspace, every region rounded up to 256 bytes, in this order:
//   prop      scratch of the two up propagations, which run one after the other in it: the largest imdbn_ws_bytes(v, H, Q) and
//             imdbn_ws_bytes(v, H, N) over 1 <= v < V (the size helper does not know D1)
//   zero [H]  the hidden bias of the second propagation          a [Q][H], b [N][H]      sa [Q], sb [N]      ref_q [Q], ref_n [N]
//   col_part [ceil(Q / 64)][N]
//   per chunk: row_part [Q], and with k > 0 the chunk's lists: scores [Q][k], indices [Q][k]
// Launch order: clear zero; K1 logits -> a; K1 logits -> b; pair_row_dot -> sa, sb; pair_score_list -> ref; pair_score_sweep ->
// col_part, row_part, lists (and the caller's scores); pair_finish -> the caller's ranks and matched scores; knn_topk_merge.

static size_t pair_prop_bytes(int V, int H, int Q, int N) {
    size_t m = 0;
    for (int v = 1; v < V; ++v) m = std::max(m, std::max(make_layout(v, H, Q, nullptr).bytes, make_layout(v, H, N, nullptr).bytes));
    return m;
}
static size_t pair_head_bytes(size_t prop_bytes, int H, int Q, int N) {      // everything in front of the per-chunk regions
    const size_t f = sizeof(float);
    return prop_bytes + knn_align(f * H) + knn_align(f * (size_t)Q * H) + knn_align(f * (size_t)N * H) +
           2 * knn_align(f * Q) + 2 * knn_align(f * N) + knn_align(sizeof(int32_t) * (size_t)cdiv(Q, KNN_QT) * N);
}
static size_t pair_chunk_bytes(int Q, int k) { return knn_align(sizeof(int32_t) * (size_t)Q) + (k > 0 ? 2 * knn_align(sizeof(float) * (size_t)Q * k) : 0); }

size_t imdbn_pair_ws_bytes(int V, int H, int Q, int N, int k) {
    if (V < 2 || H <= 0 || Q <= 0 || N <= 0 || k < 0 || k > KNN_KMAX) return 0;
    return pair_head_bytes(pair_prop_bytes(V, H, Q, N), H, Q, N) + pair_chunk_bytes(Q, k);
}

// the sweep asks for more than 64 KB of dynamic LDS from k = 29 on: the attribute, once per device ordinal
static int pair_attrs_ready() {
    static std::mutex m;
    static std::vector<char> done;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(m);
    if ((int)done.size() <= dev) done.resize(dev + 1, 0);
    if (done[dev]) return 0;
    HIPCHK(hipFuncSetAttribute((const void*)pair_score_sweep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pair_sweep_lds(KNN_KMAX)));
    done[dev] = 1;
    return 0;
}

// out[B][H] = hid_bias + z W of the cut descriptor `dz`: the logits path of imdbn_rbm_prop_up, as LabelSide::propagate
static int pair_logits(imdbn_rbm_desc dz, const float* z, int64_t ldz, int B, float* out, void* ws, size_t ws_bytes, hipStream_t st) {
    Ctx c(&dz, nullptr, st);
    CHK(setup(c, B, ws, ws_bytes));
    FinishArgs f = new_finish();
    f.logits_only = 1;
    f.out_prob = out; f.ld_prob = dz.H;
    return prep_prop(c, true, z, ldz, f);
}

int imdbn_rbm_pair_scores(const imdbn_rbm_desc* d, int D1, const float* z1, int64_t ld1, int Q, const float* z2, int64_t ld2, int N,
                          const int32_t* gt_q, const int32_t* gt_n, int k, const imdbn_pair_out* out, void* ws, size_t ws_bytes,
                          imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (d->n_groups > 0) return fail(IMDBN_E_UNSUPPORTED, "pair_scores: softmax groups are not supported (n_groups = %d)", d->n_groups);
    if (Q < 1 || N < 1) return fail(IMDBN_E_INVALID, "pair_scores: Q = %d, N = %d (both must be >= 1)", Q, N);
    if (D1 < 1 || D1 >= d->V) return fail(IMDBN_E_INVALID, "pair_scores: D1 = %d outside [1, V = %d)", D1, d->V);
    const int D2 = d->V - D1, H = d->H;
    if (k < 0 || k > KNN_KMAX) return fail(IMDBN_E_INVALID, "pair_scores: k = %d outside [0, %d]", k, KNN_KMAX);
    if (!z1 || !z2 || !out) return fail(IMDBN_E_INVALID, "pair_scores: null %s", !z1 ? "z1" : (!z2 ? "z2" : "out"));
    if (ld1 < D1) return fail(IMDBN_E_INVALID, "pair_scores: ld1 %lld < D1 %d", (long long)ld1, D1);
    if (ld2 < D2) return fail(IMDBN_E_INVALID, "pair_scores: ld2 %lld < D2 %d", (long long)ld2, D2);
    if ((out->rank_q || out->score_q) && !gt_q) return fail(IMDBN_E_INVALID, "pair_scores: rank_q / score_q without gt_q");
    if ((out->rank_n || out->score_n) && !gt_n) return fail(IMDBN_E_INVALID, "pair_scores: rank_n / score_n without gt_n");
    if (k > 0 && (!out->top_idx || !out->top_score)) return fail(IMDBN_E_INVALID, "pair_scores: k = %d without top_idx and top_score", k);
    if (out->scores && out->lds < N) return fail(IMDBN_E_INVALID, "pair_scores: lds %lld < N %d", (long long)out->lds, N);
    const bool want_q = out->rank_q || out->score_q, want_n = out->rank_n || out->score_n;
    if (!want_q && !want_n && k == 0 && !out->scores) return fail(IMDBN_E_INVALID, "pair_scores: no output requested");
    const size_t prop_bytes = pair_prop_bytes(d->V, H, Q, N), head = pair_head_bytes(prop_bytes, H, Q, N), per_chunk = pair_chunk_bytes(Q, k);
    if (!ws || ws_bytes < head + per_chunk) return fail(IMDBN_E_WORKSPACE, "pair_scores: workspace %zu < %zu bytes", ws_bytes, head + per_chunk);
    if (((uintptr_t)ws & 255) != 0) return fail(IMDBN_E_INVALID, "pair_scores: workspace must be 256-byte aligned");
    // about 2048 blocks over (query tiles x candidate chunks), as many chunks as the workspace holds
    const int qtiles = cdiv(Q, KNN_QT);
    int chunks = std::min(std::max(1, cdiv(2048, qtiles)), cdiv(N, KNN_BT));
    chunks = (int)std::min<size_t>((size_t)chunks, (ws_bytes - head) / per_chunk);
    const int chunk = rup(cdiv(N, chunks), KNN_BT);
    chunks = cdiv(N, chunk);
    const size_t f = sizeof(float);
    char* p = (char*)ws + prop_bytes;
    float* zero = (float*)p; p += knn_align(f * H);
    float* a = (float*)p; p += knn_align(f * (size_t)Q * H);
    float* b = (float*)p; p += knn_align(f * (size_t)N * H);
    PairArgs g;
    memset(&g, 0, sizeof(g));
    float* sa = (float*)p; p += knn_align(f * Q);
    float* sb = (float*)p; p += knn_align(f * N);
    g.ref_q = (float*)p; p += knn_align(f * Q);
    g.ref_n = (float*)p; p += knn_align(f * N);
    g.col_part = (int32_t*)p; p += knn_align(sizeof(int32_t) * (size_t)qtiles * N);
    g.row_part = (int32_t*)p; p += knn_align(sizeof(int32_t) * (size_t)Q) * chunks;      // [chunks][Q]: the pitch is Q, the region is larger
    g.part_s = (float*)p; g.part_i = (int32_t*)(p + knn_align(f * (size_t)Q * k) * chunks);
    g.a = a; g.b = b; g.sa = sa; g.sb = sb;
    g.Q = Q; g.N = N; g.H = H; g.k = k; g.chunk = chunk; g.chunks = chunks; g.qtiles = qtiles;
    g.gt_q = want_q ? gt_q : nullptr; g.gt_n = want_n ? gt_n : nullptr;
    g.scores = out->scores; g.lds = out->lds;
    g.rank_q = out->rank_q; g.rank_n = out->rank_n; g.score_q = out->score_q; g.score_n = out->score_n;
    const hipStream_t st = S(stream);
    CHK(kernel_attrs_ready());
    CHK(pair_attrs_ready());
    HIPCHK(hipMemsetAsync(zero, 0, f * H, st));
    imdbn_rbm_desc d1 = *d, d2 = *d;
    d1.V = D1;
    d2.V = D2; d2.W = d->W + (int64_t)D1 * d->ldw; d2.vis_bias = d->vis_bias + D1; d2.hid_bias = zero;
    CHK(pair_logits(d1, z1, ld1, Q, a, ws, prop_bytes, st));
    CHK(pair_logits(d2, z2, ld2, N, b, ws, prop_bytes, st));
    const dim3 rblock(64 * ROW_WAVES);
    hipLaunchKernelGGL(pair_row_dot, dim3(cdiv(Q, ROW_WAVES)), rblock, 0, st, z1, ld1, Q, D1, d1.vis_bias, sa);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(pair_row_dot, dim3(cdiv(N, ROW_WAVES)), rblock, 0, st, z2, ld2, N, D2, d2.vis_bias, sb);
    HIPCHK(hipGetLastError());
    if (g.gt_q || g.gt_n) {
        hipLaunchKernelGGL(pair_score_list, dim3((unsigned)(((int64_t)Q + N + 255) / 256)), dim3(256), 0, st, g);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(pair_score_sweep, dim3(qtiles, chunks), dim3(256), pair_sweep_lds(k), st, g);
    HIPCHK(hipGetLastError());
    if (g.gt_q || g.gt_n) {
        hipLaunchKernelGGL(pair_finish, dim3(cdiv(std::max(Q, N), 256)), dim3(256), 0, st, g);
        HIPCHK(hipGetLastError());
    }
    if (k > 0) {
        hipLaunchKernelGGL(knn_topk_merge, dim3(qtiles), dim3(KNN_QT), knn_merge_lds(k), st, g.part_s, g.part_i, chunks, Q, k,
                           (const float*)nullptr, out->top_idx, out->top_score);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
