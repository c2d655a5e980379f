// host_exact.hpp -- host side of imdbn_rbm_exact_logz (included by engine.hip inside extern "C"; kernels_exact.hpp).
//
// Scratch, every region rounded up to 256 bytes, in this order:
//   hdr    [EXACT_HDR] double        [0]: LSE_s t(s), left by exact_finish for the marginal pass
//   part   [n_launch][EXACT_BLOCKS][2] double        the (max, scaled sum) pair of every block of every walk launch
//   Wd     [n][D] float              the dense block of exact_prep
//   marg_s [blocks][D] double, marg_e [blocks][32] double        per-block partials of the marginals; blocks = the blocks of a walk
//                                    launch = min(ceil(2^min(n, 22) / 128), EXACT_BLOCKS): 8 at n = 10, 512 from n = 16 on
// Launch order: exact_prep; n_launch x exact_walk (2^min(n, 22) states each, the high bits in ascending order); exact_finish; with
// marginals n_launch x exact_walk<MARG> and exact_finish_marg.  Nothing of the scratch is read before this call has written it.

struct ExactPlan { int e_hidden, n, D, n_launch, blocks; unsigned tiles; size_t off_part, off_wd, off_ms, off_me, bytes; };

static size_t exact_align(size_t b) { return (b + 255) & ~(size_t)255; }

// side: 0 the smaller side (ties: hidden), 1 hidden, 2 visible.  n may exceed EXACT_NMAX: the caller decides.
static ExactPlan exact_plan(int V, int H, int side) {
    ExactPlan p{};
    p.e_hidden = side == 1 || (side == 0 && H <= V);
    p.n = p.e_hidden ? H : V;
    p.D = p.e_hidden ? V : H;
    const int nb = std::min(p.n, EXACT_NMAX);
    p.n_launch = nb > EXACT_LAUNCH_BITS ? 1 << (nb - EXACT_LAUNCH_BITS) : 1;
    const int launch_bits = std::min(nb, EXACT_LAUNCH_BITS);
    p.tiles = launch_bits > EXACT_WALK_BITS ? 1u << (launch_bits - EXACT_WALK_BITS) : 1u;
    p.blocks = (int)std::min<unsigned>((p.tiles + 3) / 4, (unsigned)EXACT_BLOCKS);      // four tiles (waves) per block
    p.off_part = exact_align(sizeof(double) * EXACT_HDR);
    p.off_wd = p.off_part + exact_align(sizeof(double) * 2 * EXACT_BLOCKS * (size_t)p.n_launch);
    p.off_ms = p.off_wd + exact_align(sizeof(float) * (size_t)nb * p.D);
    p.off_me = p.off_ms + exact_align(sizeof(double) * (size_t)p.blocks * p.D);
    p.bytes = p.off_me + exact_align(sizeof(double) * (size_t)p.blocks * 32);
    return p;
}

size_t imdbn_exact_scratch_bytes(int V, int H, int side) {
    if (V <= 0 || H <= 0 || side < 0 || side > 2) return 0;
    const ExactPlan p = exact_plan(V, H, side);
    return p.n > EXACT_NMAX ? 0 : p.bytes;
}

static void exact_launch_walk(const ExactArgs& a, bool gauss, bool marg, hipStream_t s) {
    const dim3 grid(a.blocks), block(256);
    if (gauss && marg) hipLaunchKernelGGL((exact_walk<true, true>), grid, block, 0, s, a);
    else if (gauss) hipLaunchKernelGGL((exact_walk<true, false>), grid, block, 0, s, a);
    else if (marg) hipLaunchKernelGGL((exact_walk<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((exact_walk<false, false>), grid, block, 0, s, a);
}

int imdbn_rbm_exact_logz(const imdbn_rbm_desc* d, const float* logvar, int side, double* out, float* vis_mean, float* hid_mean,
                         void* scratch, size_t scratch_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!out || !scratch) return fail(IMDBN_E_INVALID, "exact_logz: null %s", !out ? "out" : "scratch");
    if (side < 0 || side > 2) return fail(IMDBN_E_INVALID, "exact_logz: side = %d outside 0..2", side);
    if ((vis_mean == nullptr) != (hid_mean == nullptr))
        return fail(IMDBN_E_INVALID, "exact_logz: %s given without %s (the marginals come as a pair)", vis_mean ? "vis_mean" : "hid_mean",
                    vis_mean ? "hid_mean" : "vis_mean");
    if (side == 2 && logvar) return fail(IMDBN_E_INVALID, "exact_logz: side = 2 (visible) with logvar: Gaussian visibles cannot be enumerated");
    if (((uintptr_t)scratch & 255) != 0) return fail(IMDBN_E_INVALID, "exact_logz: scratch %p is not 256-byte aligned", scratch);
    const ExactPlan p = exact_plan(d->V, d->H, side);
    if (p.n > EXACT_NMAX)
        return fail(IMDBN_E_UNSUPPORTED, "exact_logz: %d units on the enumerated (%s) side, at most %d", p.n, p.e_hidden ? "hidden" : "visible", EXACT_NMAX);
    if (!p.e_hidden && d->n_groups > 0)
        return fail(IMDBN_E_UNSUPPORTED, "exact_logz: the visible side cannot be enumerated with softmax groups (n_groups = %d)", d->n_groups);
    if (!p.e_hidden && logvar) return fail(IMDBN_E_UNSUPPORTED, "exact_logz: the visible side (side = 0 with V = %d < H = %d) is Gaussian; pass side = 1", d->V, d->H);
    if (logvar && d->n_groups > 0) return fail(IMDBN_E_UNSUPPORTED, "exact_logz: Gaussian visibles with softmax groups (n_groups = %d)", d->n_groups);
    if (scratch_bytes < p.bytes)
        return fail(IMDBN_E_INVALID, "exact_logz: scratch %zu < %zu bytes needed for V=%d H=%d side=%d", scratch_bytes, p.bytes, d->V, d->H, side);
    hipStream_t s = S(stream);
    char* base = (char*)scratch;
    ExactArgs a;
    memset(&a, 0, sizeof(a));
    a.W = d->W; a.ldw = d->ldw;
    a.e_bias = p.e_hidden ? d->hid_bias : d->vis_bias; a.s_bias = p.e_hidden ? d->vis_bias : d->hid_bias;
    a.logvar = logvar;
    a.V = d->V; a.H = d->H; a.n = p.n; a.D = p.D; a.e_hidden = p.e_hidden;
    a.sp.n_groups = d->n_groups;
    for (int g = 0; g < d->n_groups; ++g) { a.sp.gs[g] = d->group_start[g]; a.sp.ge[g] = d->group_end[g]; }
    a.hdr = (double*)base; a.part = (double*)(base + p.off_part); a.Wd = (float*)(base + p.off_wd);
    a.marg_s = (double*)(base + p.off_ms); a.marg_e = (double*)(base + p.off_me);
    a.n_launch = p.n_launch;
    a.tiles = p.tiles; a.blocks = p.blocks;
    a.marg = vis_mean ? 1 : 0;
    a.out = out; a.vis_mean = vis_mean; a.hid_mean = hid_mean;
    const bool prof = g_prof.on && g_prof.used + 2 <= g_prof.ev.size();      // imdbn_profile_read: the whole call between two events
    if (prof) HIPCHK(hipEventRecord(g_prof.ev[g_prof.used], s));
    const int64_t prep_items = std::max<int64_t>((int64_t)p.n * p.D, a.marg ? (int64_t)p.blocks * p.D : 0);
    hipLaunchKernelGGL(exact_prep, dim3((unsigned)std::min<int64_t>((prep_items + 255) / 256, 2048)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    for (int pass = 0; pass < 1 + a.marg; ++pass) {
        for (int l = 0; l < p.n_launch; ++l) {
            a.launch = l;
            a.base = (unsigned)l << EXACT_LAUNCH_BITS;
            exact_launch_walk(a, logvar != nullptr, pass == 1, s);
            HIPCHK(hipGetLastError());
        }
        if (pass == 0) hipLaunchKernelGGL(exact_finish, dim3(1), dim3(64), 0, s, a);
        else hipLaunchKernelGGL(exact_finish_marg, dim3(cdiv(std::max(p.D, p.n), 256)), dim3(256), 0, s, a);
        HIPCHK(hipGetLastError());
    }
    if (prof) { HIPCHK(hipEventRecord(g_prof.ev[g_prof.used + 1], s)); g_prof.used += 2; }
    return 0;
}
