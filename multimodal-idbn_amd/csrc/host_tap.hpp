// host_tap.hpp -- host side of imdbn_rbm_tap_iterate / imdbn_rbm_tap_step (included by engine.hip inside extern "C", after the
// centered update whose grid plan tap_apply shares; kernels_tap.hpp).
//
// Workspace = [the layout of imdbn_ws_bytes(V, H, B) | counters | slabs | res_up | res_dn | gam_part], every region rounded up
// to 256 bytes.  tap_iterate touches the tail only.  Nothing of it is read before this call has written it (the counters are
// cleared by a memset node at the head of every call that splits K).
// Launch order of tap_step: [memset] n_iters x (tap_half up, tap_half down); prep_operand(mv), prep_operand(mh, negated);
// prep_operand(data), K1 (H+), [K2 (loss)]; K3 statistics -> dW; [tap_outer -> C]; tap_apply; bias_update.

struct TapDir { int K, N, ntiles, ks, kchunk; };
struct TapPlan { TapDir up, dn; int zc; size_t base, off_cnt, off_slabs, off_res_up, off_res_dn, off_gam, bytes; };

static size_t tap_align(size_t b) { return (b + 255) & ~(size_t)255; }

// K slices: about two blocks per CU, at most 16 slices, none shorter than four stages.  A function of (K, N, B) and the CU count
static TapDir tap_dir(int K, int N, int zc) {
    TapDir t{};
    t.K = K; t.N = N; t.ntiles = cdiv(N, TAP_TN);
    int ks = (2 * std::max(cu_count(), 1)) / std::max(1, t.ntiles * zc);
    ks = std::max(1, std::min(std::min(ks, 16), K / (4 * TAP_KC)));
    t.kchunk = rup(cdiv(K, ks), TAP_KC);
    t.ks = cdiv(K, t.kchunk);
    return t;
}

static TapPlan tap_plan(int V, int H, int B) {
    TapPlan p{};
    p.zc = cdiv(B, TAP_BM);
    p.up = tap_dir(V, H, p.zc);
    p.dn = tap_dir(H, V, p.zc);
    auto slab = [&](const TapDir& t) { return t.ks > 1 ? (size_t)p.zc * t.ks * t.ntiles * 2 * TAP_BM * TAP_TN : (size_t)0; };
    p.base = tap_align(make_layout(V, H, B, nullptr).bytes);
    p.off_cnt = p.base;
    p.off_slabs = p.off_cnt + tap_align(sizeof(int) * (size_t)p.zc * std::max(p.up.ntiles, p.dn.ntiles));
    p.off_res_up = p.off_slabs + tap_align(sizeof(float) * std::max(slab(p.up), slab(p.dn)));
    p.off_res_dn = p.off_res_up + tap_align(sizeof(float) * (size_t)p.up.ntiles * B);
    p.off_gam = p.off_res_dn + tap_align(sizeof(float) * (size_t)p.dn.ntiles * B);
    p.bytes = p.off_gam + tap_align(sizeof(double) * (size_t)p.up.ntiles * B);
    return p;
}

size_t imdbn_rbm_tap_ws_bytes(int V, int H, int B) {
    if (V <= 0 || H <= 0 || B <= 0) return 0;
    return tap_plan(V, H, B).bytes;
}

// [dW V H | pad to 4 | C V H | pad to 4]
size_t imdbn_rbm_tap_scratch_floats(int V, int H) {
    if (V <= 0 || H <= 0) return 0;
    return 2 * centered_dw_floats(V, H);
}

// everything the two entries refuse in common, before any launch
static int tap_check(const char* who, const imdbn_rbm_desc* d, bool momentum, const float* mv, int64_t ldmv, const float* mh, int64_t ldmh,
                     int B, int n_iters, float damp, int order, const void* ws, size_t ws_bytes) {
    if (check_desc(d, momentum) != 0) return IMDBN_E_INVALID;      // (the message of check_desc stands)
    if (d->n_groups != 0) return fail(IMDBN_E_INVALID, "%s: %d softmax groups (Bernoulli units on both sides only)", who, d->n_groups);
    if (!mv || !mh || !ws) return fail(IMDBN_E_INVALID, "%s: null %s", who, !mv ? "mv" : (!mh ? "mh" : "workspace"));
    if (B < 1) return fail(IMDBN_E_INVALID, "%s: B = %d rows", who, B);
    if (ldmv < d->V) return fail(IMDBN_E_INVALID, "%s: ldmv %lld < V %d", who, (long long)ldmv, d->V);
    if (ldmh < d->H) return fail(IMDBN_E_INVALID, "%s: ldmh %lld < H %d", who, (long long)ldmh, d->H);
    if (n_iters < 0) return fail(IMDBN_E_INVALID, "%s: n_iters = %d", who, n_iters);
    if (order != 1 && order != 2) return fail(IMDBN_E_INVALID, "%s: order = %d outside {1, 2}", who, order);
    if (!(damp >= 0.0f && damp < 1.0f)) return fail(IMDBN_E_INVALID, "%s: damp = %g outside [0, 1)", who, (double)damp);
    if (((uintptr_t)ws & 255) != 0) return fail(IMDBN_E_INVALID, "%s: workspace %p is not 256-byte aligned", who, ws);
    const size_t need = tap_plan(d->V, d->H, B).bytes;
    if (ws_bytes < need) return fail(IMDBN_E_INVALID, "%s: workspace %zu < %zu bytes needed for V=%d H=%d B=%d", who, ws_bytes, need, d->V, d->H, B);
    return 0;
}

static int tap_launch_half(const imdbn_rbm_desc* d, const TapPlan& p, char* ws, bool up, float* mv, int64_t ldmv, float* mh, int64_t ldmh,
                           int B, float damp, int order, bool gamma, hipStream_t s) {
    const TapDir& t = up ? p.up : p.dn;
    TapHalfArgs a;
    memset(&a, 0, sizeof(a));
    a.W = d->W; a.ldw = d->ldw; a.K = t.K; a.N = t.N;
    a.m_in = up ? mv : mh; a.ld_in = up ? ldmv : ldmh;
    a.m_out = up ? mh : mv; a.ld_out = up ? ldmh : ldmv;
    a.bias = up ? d->hid_bias : d->vis_bias;
    a.B = B; a.damp = damp;
    a.ks = t.ks; a.kchunk = t.kchunk; a.ntiles = t.ntiles;
    a.slabs = (float*)(ws + p.off_slabs); a.counters = (int*)(ws + p.off_cnt);
    a.res_part = (float*)(ws + (up ? p.off_res_up : p.off_res_dn));
    a.gamma = gamma ? 1 : 0; a.gam_part = (double*)(ws + p.off_gam);
    const dim3 grid(t.ntiles, t.ks, p.zc);
    if (order == 2) {
        if (up) hipLaunchKernelGGL((tap_half<true, true>), grid, dim3(256), 0, s, a);
        else    hipLaunchKernelGGL((tap_half<true, false>), grid, dim3(256), 0, s, a);
    } else {
        if (up) hipLaunchKernelGGL((tap_half<false, true>), grid, dim3(256), 0, s, a);
        else    hipLaunchKernelGGL((tap_half<false, false>), grid, dim3(256), 0, s, a);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// n_iters iterations in place, then (out_gamma) the gamma pass and (either output) the per-row finish
static int tap_run(const imdbn_rbm_desc* d, const TapPlan& p, char* ws, float* mv, int64_t ldmv, float* mh, int64_t ldmh, int B, int n_iters,
                   float damp, int order, double* out_gamma, float* out_res, hipStream_t s) {
    if ((p.up.ks > 1 || p.dn.ks > 1) && (n_iters > 0 || out_gamma))
        HIPCHK(hipMemsetAsync(ws + p.off_cnt, 0, sizeof(int) * (size_t)p.zc * std::max(p.up.ntiles, p.dn.ntiles), s));
    for (int it = 0; it < n_iters; ++it) {
        CHK(tap_launch_half(d, p, ws, true, mv, ldmv, mh, ldmh, B, damp, order, false, s));
        CHK(tap_launch_half(d, p, ws, false, mv, ldmv, mh, ldmh, B, damp, order, false, s));
    }
    if (out_gamma) CHK(tap_launch_half(d, p, ws, true, mv, ldmv, mh, ldmh, B, damp, order, true, s));
    if (out_gamma || out_res) {
        TapRowsArgs r;
        memset(&r, 0, sizeof(r));
        r.B = B; r.V = d->V; r.mv = mv; r.ldmv = ldmv; r.vis_bias = d->vis_bias;
        r.res_up = (const float*)(ws + p.off_res_up); r.nt_up = n_iters > 0 ? p.up.ntiles : 0;
        r.res_dn = (const float*)(ws + p.off_res_dn); r.nt_dn = n_iters > 0 ? p.dn.ntiles : 0;
        r.out_res = out_res;
        r.gam_part = (const double*)(ws + p.off_gam); r.nt_gam = p.up.ntiles; r.out_gamma = out_gamma;
        hipLaunchKernelGGL(tap_rows_finish, dim3(B), dim3(256), 0, s, r);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

int imdbn_rbm_tap_iterate(const imdbn_rbm_desc* d, float* mv, int64_t ldmv, float* mh, int64_t ldmh, int B, int n_iters, float damp,
                          int order, double* out_gamma, float* out_res, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(tap_check("tap_iterate", d, false, mv, ldmv, mh, ldmh, B, n_iters, damp, order, ws, ws_bytes));
    const TapPlan p = tap_plan(d->V, d->H, B);
    return tap_run(d, p, (char*)ws, mv, ldmv, mh, ldmh, B, n_iters, damp, order, out_gamma, out_res, S(stream));
}

// magnetisations -> the negative-phase planes of the statistics kernel (three-term split: real values) and their column sums
static int tap_prep(Ctx& c, const float* in, int64_t ld, int N, int ldrm, bf16_t* tr, float* colsum, int negate) {
    const Layout& L = c.L;
    PrepArgs p;
    memset(&p, 0, sizeof(p));
    p.zero = L.k1s_cnt; p.n_zero = (L.Bp / 64) * L.k1s_tiles;
    c.cnt_ok = true;
    p.in = in; p.ld = ld; p.B = L.B; p.Bp = L.Bp; p.N = N;
    p.op.ldrm = ldrm; p.op.rm_ts = (int64_t)L.Bp * ldrm; p.op.Bp = L.Bp;
    p.op.tr = tr; p.op.tr_ts = (int64_t)N * L.Bp; p.op.tr_terms = c.rt; p.op.tr_negate = negate;
    p.colsum_part = colsum;
    hipLaunchKernelGGL(prep_operand, dim3(cdiv(std::max(N, ldrm), 64), L.P), dim3(256), 0, c.s, p);
    HIPCHK(hipGetLastError());
    return 0;
}

int imdbn_rbm_tap_step(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, float* mv, int64_t ldmv, float* mh, int64_t ldmh,
                       const imdbn_cd_opts* o, int n_iters, float damp, int order, float* loss_out, float* scratch, size_t scratch_floats,
                       void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(tap_check("tap_step", d, true, mv, ldmv, mh, ldmh, B, n_iters, damp, order, ws, ws_bytes));
    if (!data || !o || !scratch) return fail(IMDBN_E_INVALID, "tap_step: null %s", !data ? "data" : (!o ? "opts" : "scratch"));
    if (ldd < d->V) return fail(IMDBN_E_INVALID, "tap_step: ldd %lld < V %d", (long long)ldd, d->V);
    const int V = d->V, H = d->H;
    if (scratch_floats < imdbn_rbm_tap_scratch_floats(V, H))
        return fail(IMDBN_E_INVALID, "tap_step: scratch %zu < %zu floats needed for V=%d H=%d", scratch_floats, imdbn_rbm_tap_scratch_floats(V, H), V, H);
    if (o->data_binary < 0 || o->data_binary > 2) return fail(IMDBN_E_INVALID, "tap_step: data_binary %d outside 0..2", o->data_binary);
    if (o->next_data || o->next_slot || o->data_slot || o->next_binary || o->fwd_out)
        return fail(IMDBN_E_INVALID, "tap_step: the prefetch fields and fwd_out must be zero (next_data %p, next_slot %d, data_slot %d, next_binary %d, fwd_out %p)",
                    (const void*)o->next_data, o->next_slot, o->data_slot, o->next_binary, (const void*)o->fwd_out);
    const TapPlan p = tap_plan(V, H, B);
    Ctx c(d, nullptr, S(stream));
    CHK(setup(c, B, ws, p.base));
    const Layout& L = c.L;
    // negative phase: the stored magnetisations relaxed in place
    CHK(tap_run(d, p, (char*)ws, mv, ldmv, mh, ldmh, B, n_iters, damp, order, nullptr, nullptr, c.s));
    CHK(tap_prep(c, mv, ldmv, V, L.Vpad, L.vis_tr[1], L.cs_vneg, 0));
    CHK(tap_prep(c, mh, ldmh, H, L.Hpad, L.hid_tr[1], L.cs_hneg, 1));
    // positive phase, as pcd_phases: H+ = up(data), and with a loss wanted its mean-field reconstruction
    const bool recon = loss_out != nullptr;
    CHK(prep(c, data, ldd, V, L.vis_rm[0], L.Vpad, L.vis_tr[0], L.flags, L.cs_vpos, 3, L.vis_bits[0]));
    {
        FinishArgs f = new_finish();
        if (recon) { f.op.rm = L.hid_rm; f.op.rm_terms = c.rt; f.rm_src = 1; }
        f.op.tr = L.hid_tr[0]; f.op.tr_terms = c.ht; f.tr_src = 1;
        f.colsum_part = L.cs_hpos; f.colsum_src = 1;
        CHK(prop(c, true, OpIn{L.vis_rm[0], c.nw == 1 ? 1 : 0, L.flags, L.vis_bits[0], data_operand_kind(o->data_binary)}, f));
    }
    if (recon) {
        FinishArgs f = new_finish();
        f.loss_ref = data; f.ld_ref = ldd; f.loss_src = 1; f.loss_part = L.loss_part;
        CHK(prop(c, false, OpIn{L.hid_rm, c.rt, nullptr}, f));
    }
    // dW = V+^T H+ - mv^T mh, un-normalised
    float* dW = scratch;
    float* Cs = order == 2 ? scratch + centered_dw_floats(V, H) : nullptr;
    CHK(launch_assoc(c, 1, o, c.nw == 1 ? 1 : 0, L.flags, c.rt, 1.0f, dW));
    if (Cs) {
        TapOuterArgs q{mv, ldmv, mh, ldmh, B, V, H, Cs};
        hipLaunchKernelGGL(tap_outer, dim3(cdiv(H, 256), cdiv(V, 32)), dim3(256), 0, c.s, q);
        HIPCHK(hipGetLastError());
    }
    const bool vec4 = c.r.vec4 && (((uintptr_t)d->W_m | (uintptr_t)scratch) & 15) == 0;
    const CenteredPlan cp = centered_plan(V, H, vec4);
    TapApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.W = d->W; a.Wm = d->W_m; a.ldw = d->ldw; a.V = V; a.H = H; a.dW = dW; a.C = Cs;
    a.lr = o->lr; a.mom = o->momentum; a.wd = o->weight_decay; a.n = (float)B;
    a.rps = cp.rps; a.tw = cp.tw;
    if (vec4) hipLaunchKernelGGL(tap_apply<true>, dim3(cp.ctiles, cp.nstripes), dim3(256), 0, c.s, a);
    else      hipLaunchKernelGGL(tap_apply<false>, dim3(cp.ctiles, cp.nstripes), dim3(256), 0, c.s, a);
    HIPCHK(hipGetLastError());
    BiasArgs bias = make_bias(c, o, o->sparsity != 0, (float)B, loss_out);
    if (!loss_out) { bias.loss_part = nullptr; bias.n_loss = 0; }
    return launch_bias(c, bias);
}
