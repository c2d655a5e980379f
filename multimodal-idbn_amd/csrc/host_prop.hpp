// host_prop.hpp -- host side, part 2 (included by engine.hip after Ctx): one launcher per propagation kernel family and
// prop(), which asks the Route (host_layout.hpp) and calls one of them.  Each launcher fills its kernel's argument block,
// completes FinishArgs for that kernel and launches; the tables below name every instantiation that exists.
#pragma once

// ---- instantiations ------------------------------------------------------------------------------
// (one per case: code that a launch does not run -- the general epilogue, the preparation blocks, the loop over bf16 terms --
//  still costs it time; and one body per kernel: several inlined into one make the register allocator spill)
using K1sFn = decltype(&k1_stream<3, 0, false, false>);
struct K1sInst { int nw, na; bool rider, general; K1sFn fn; };      // weight terms, operand terms (0 = bit plane), next-batch blocks, general epilogue
const K1sInst k1s_insts[] = {
    {3, 0, true, false, k1_stream<3, 0, false, true>},  {3, 0, true, true, k1_stream<3, 0, true, true>},
    {3, 0, false, false, k1_stream<3, 0, false, false>}, {3, 0, false, true, k1_stream<3, 0, true, false>},
    {3, 1, false, false, k1_stream<3, 1, false, false>}, {3, 1, false, true, k1_stream<3, 1, true, false>},
    {3, 3, false, false, k1_stream<3, 3, false, false>}, {3, 3, false, true, k1_stream<3, 3, true, false>},
    {1, 0, true, false, k1_stream<1, 0, false, true>},  {1, 0, true, true, k1_stream<1, 0, true, true>},
    {1, 0, false, false, k1_stream<1, 0, false, false>}, {1, 0, false, true, k1_stream<1, 0, true, false>},
    {1, 1, false, false, k1_stream<1, 1, false, false>}, {1, 1, false, true, k1_stream<1, 1, true, false>},
};
using K2sFn = decltype(&k2_stream<3, 1, false>);
const K2sFn k2s_insts[2][3][2] = {      // [nw == 3][16-row MFMA tiles per block - 1][general epilogue]
    {{k2_stream<1, 1, false>, k2_stream<1, 1, true>}, {k2_stream<1, 2, false>, k2_stream<1, 2, true>}, {k2_stream<1, 3, false>, k2_stream<1, 3, true>}},
    {{k2_stream<3, 1, false>, k2_stream<3, 1, true>}, {k2_stream<3, 2, false>, k2_stream<3, 2, true>}, {k2_stream<3, 3, false>, k2_stream<3, 3, true>}}};
using DownFn = decltype(&gemm_down_fused<3, true, 0, false>);
const DownFn down_insts[2][2][4] = {    // [nw == 3][float4 rows][operand: bit plane, 1 term, 3 terms, by the exactness map]
    {{gemm_down_fused<1, false, 1, true>, gemm_down_fused<1, false, 1, false>, gemm_down_fused<1, false, 3, false>, gemm_down_fused<1, false, 0, false>},
     {gemm_down_fused<1, true, 1, true>, gemm_down_fused<1, true, 1, false>, gemm_down_fused<1, true, 3, false>, gemm_down_fused<1, true, 0, false>}},
    {{gemm_down_fused<3, false, 1, true>, gemm_down_fused<3, false, 1, false>, gemm_down_fused<3, false, 3, false>, gemm_down_fused<3, false, 0, false>},
     {gemm_down_fused<3, true, 1, true>, gemm_down_fused<3, true, 1, false>, gemm_down_fused<3, true, 3, false>, gemm_down_fused<3, true, 0, false>}}};
const DownFn down_chunk_insts[2][2] = { // [nw == 3][4 batch chunks per block (else 2)]
    {gemm_down_fused<1, true, 0, false, 2>, gemm_down_fused<1, true, 0, false, 4>},
    {gemm_down_fused<3, true, 0, false, 2>, gemm_down_fused<3, true, 0, false, 4>}};
using DownNextFn = decltype(&gemm_down_fused_next<3, false>);
const DownNextFn down_next_insts[2][2] = {      // [nw == 3][bit-plane operand]
    {gemm_down_fused_next<1, false>, gemm_down_fused_next<1, true>}, {gemm_down_fused_next<3, false>, gemm_down_fused_next<3, true>}};

// Kernels that ask for more than 64 KB of dynamic LDS need the attribute set once per DEVICE: done for all of them the first
// time a launcher meets a device ordinal (any thread), under the lock of g_devices.
int kernel_attrs_ready() {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_devices.m);
    if ((int)g_devices.attrs.size() <= dev) g_devices.attrs.resize(dev + 1, 0);
    if (g_devices.attrs[dev]) return 0;
    const auto attr = hipFuncAttributeMaxDynamicSharedMemorySize;
    for (const K1sInst& k : k1s_insts) HIPCHK(hipFuncSetAttribute((const void*)k.fn, attr, K1S_WAVES * K1S_REGION_REAL + 8 * K1S_MAX_KCHUNK + K1S_LDS_EXTRA));
    for (const auto& nw : k2s_insts) for (const auto& mt : nw) for (K2sFn fn : mt) HIPCHK(hipFuncSetAttribute((const void*)fn, attr, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void*)knn_topk_chunk, attr, (int)knn_chunk_lds(KNN_KMAX)));
    HIPCHK(hipFuncSetAttribute((const void*)knn_topk_merge, attr, (int)knn_merge_lds(KNN_KMAX)));
    g_devices.attrs[dev] = 1;
    return 0;
}

// ---- testing aid: which family the last up / the last down propagation of this THREAD launched (imdbn_debug_last_route).  Written by
// the launchers, each where it launches, never derived again elsewhere; the codes are IMDBN_ROUTE_* of the header
struct RouteRec { int up = -1, up_general = 0, down = -1, down_general = 0, down_groups = 0; };
thread_local RouteRec t_route;
inline void ran_up(int family, bool general) { t_route.up = family; t_route.up_general = general; }
inline void ran_down(int family, bool general) { t_route.down = family; t_route.down_general = general; t_route.down_groups = 0; }

// ---- the epilogue arguments every propagation shares ---------------------------------------------
FinishArgs new_finish() {
    FinishArgs f;
    memset(&f, 0, sizeof(f));
    f.T = 1.0f;
    return f;
}

void common_finish(const Ctx& c, bool up, FinishArgs& f) {
    const Layout& L = c.L;
    f.partial = L.partial;
    f.ks = up ? L.up.ks : L.down.ks;
    f.B = L.B; f.Bp = L.Bp;
    f.N = up ? L.H : L.V;
    f.slab = (int64_t)L.Bp * f.N;
    f.bias = up ? c.d->hid_bias : c.d->vis_bias;
    f.n_groups = up ? 0 : c.d->n_groups;
    for (int g = 0; g < IMDBN_MAX_GROUPS; ++g) { f.gs[g] = up ? 0 : c.d->group_start[g]; f.ge[g] = up ? 0 : c.d->group_end[g]; }
    f.op.ldrm = up ? L.Hpad : L.Vpad;
    f.op.rm_ts = (int64_t)L.Bp * f.op.ldrm;
    f.op.Bp = L.Bp;
    f.op.tr_ts = (int64_t)f.N * L.Bp;
    if (f.T < 1e-6f) f.T = 1e-6f;                           // max(1e-6, T)  rbm.py:92,96
    // lean epilogue specialisation (kernels_ew.hpp finish_rows_impl<R, false>)
    f.simple = (f.T == 1.0f && !(f.sigma > 0.f) && !f.mu && !f.clamp && f.n_groups == 0 && !f.logits_only) ? 1 : 0;
}

// lean epilogue of the streaming kernels (kernels_ew.hpp finish_lean8): decided by the launcher once all outputs are known
int finish_lean(const FinishArgs& g) {
    return g.simple && (g.vmode == 0 || g.vmode == 1) && !g.out_final && !(g.rm_src && g.op.rm) &&
           (g.vmode == 0 || g.uni.tape || (g.uni.row0 & 3) == 0) ? 1 : 0;
}

// K1 epilogues: hidden samples (exactly 0/1, not mixed with clamped values) also leave as a bit plane for the K2 that follows
void hid_bits_out(Ctx& c, FinishArgs& f, int shape, int cols) {
    const bool want = f.op.rm == c.L.hid_rm && f.rm_src == 2 && f.vmode == 1 && !f.clamp && f.n_groups == 0 && !f.logits_only;
    f.op.bits = want ? c.L.hid_bits : nullptr; f.op.bits_shape = shape; f.op.bits_cols = cols;
    if (f.op.rm == c.L.hid_rm) c.hid_bits_ok = want;
}

// ---- K1 ------------------------------------------------------------------------------------------
// short K: fused GEMM + epilogue, no split-K slabs (one launch per half step of a chain)
int launch_up_fused(Ctx& c, const OpIn& in, FinishArgs f) {
    const Layout& L = c.L;
    f.dbg = 0;
    hid_bits_out(c, f, 1, 32);      // epilogue lanes: 32 columns x 2 row octets
    hipLaunchKernelGGL(c.nw == 3 ? gemm_up_fused<3> : gemm_up_fused<1>, dim3(cdiv(L.H, 32), 1, L.Bp / 64), dim3(256), 0, c.s,
                       c.d->W, c.d->ldw, L.V, L.H, in.rm, (int64_t)L.Bp * L.Vpad, L.Vpad, in.flag, in.terms, f);
    HIPCHK(hipGetLastError());
    ran_up(IMDBN_ROUTE_UP_FUSED, !f.simple);
    return 0;
}

// streaming K1: weights through LDS by LDS-DMA, split-K combined by the last arriver, epilogue fused.  The operand is a bit
// plane (0/1 by construction or by the caller's word), bf16 terms (real values), or either per 64-column item (unknown);
// `next`: + block rows that prepare the next batch (one 64-column item each, or a few)
int launch_k1_stream(Ctx& c, const OpIn& in, bool bit_plane, FinishArgs f, const PrepArgs* next) {
    const Layout& L = c.L;
    const Tuning& t = tune();
    const int mb = L.Bp / 64;
    CHK(kernel_attrs_ready());
    if (!c.cnt_ok) {
        HIPCHK(hipMemsetAsync(L.k1s_cnt, 0, (size_t)mb * L.k1s_tiles * sizeof(int), c.s));
        c.cnt_ok = true;
    }
    K1sArgs a;
    memset(&a, 0, sizeof(a));
    a.W = c.d->W; a.ldw = c.d->ldw; a.K = L.V; a.N = L.H;
    a.abits = in.bits; a.Bp = L.Bp;
    a.aflag = in.binary >= 2 ? in.flag : nullptr; a.ncb = cdiv(L.Vpad, 64); a.P = L.P;
    a.slabs = L.partial; a.counters = L.k1s_cnt; a.kchunk = L.k1s_kchunk; a.ks = L.k1s_ks;
    a.amode = bit_plane ? (in.binary == 2 ? K1S_ASSERTED : K1S_BITS) : ((in.binary == 3 && c.r.adaptive_ok) ? K1S_ADAPTIVE : K1S_REAL);
    a.arm = in.rm; a.arm_ts = (int64_t)L.Bp * L.Vpad;
    if (a.amode == K1S_ADAPTIVE && c.fix_slot && in.rm == L.vis_rm[0]) {
        a.fix_tr = L.vis_tr[0]; a.fix_ts = (int64_t)L.V * L.Bp; a.fix_span = 2 * c.r.tpb; a.fix_ranges = cdiv(cdiv(L.V, 128), c.r.tpb);
        if (a.fix_ranges > L.k1s_tiles * a.ks) return fail(IMDBN_E_INVALID, "internal: k1_stream fix-up ranges");
        c.fix_slot = false;
    }
    // terms the kernel multiplies per element: the operand form carries `in.terms` of them (0 = prep's three, nw in FAST mode)
    const int na = bit_plane ? ((t.k1s_force_na && !next) ? c.nw : 0) : ((in.terms == 1 || c.nw == 1) ? 1 : 3);
    f.dbg = c.pos_phase ? ((g_dbg & 2048) ? 64 : 0) : (g_dbg & ~2048);
    hid_bits_out(c, f, 1, 32);
    if (f.op.bits && !t.no_bits) f.op.rm = nullptr, f.rm_src = 0;      // the fused K2 reads the bit plane, nobody reads the bf16 form
    // 80 KB at the headline shape: two workgroups per CU (the bit-plane kernel carries the next batch's preparation blocks)
    a.region = bit_plane ? K1S_RING : K1S_REGION_REAL;
    const size_t lds = (size_t)K1S_WAVES * a.region + (size_t)8 * a.kchunk + (bit_plane ? (next ? 0 : t.k1s_lds_pad) : K1S_LDS_EXTRA);
    f.lean = finish_lean(f);
    PrepArgs pz;
    memset(&pz, 0, sizeof(pz));
    const int items = next ? cdiv(std::max(next->N, next->op.ldrm), 64) : 0;
    const int pr = next ? std::min(8, cdiv(items, L.k1s_tiles)) : 0;
    if (pr > 0 && na != 0) return fail(IMDBN_E_INVALID, "internal: preparation blocks ride on the bit-plane k1_stream only");
    for (const K1sInst& k : k1s_insts) {
        if (k.nw != c.nw || k.na != na || k.rider != (pr > 0) || k.general != !f.lean) continue;
        hipLaunchKernelGGL(k.fn, dim3(L.k1s_tiles, a.ks + pr, mb), dim3(64 * K1S_WAVES), lds, c.s, a, f, next ? *next : pz);
        HIPCHK(hipGetLastError());
        ran_up(bit_plane ? IMDBN_ROUTE_UP_STREAM_BITS : IMDBN_ROUTE_UP_STREAM_REAL, k.general);
        return 0;
    }
    return fail(IMDBN_E_INVALID, "internal: no k1_stream for %d weight and %d operand terms", c.nw, na);
}

// generic K1: split-K partial GEMM into slabs, then `finish` (the epilogue as a launch of its own)
int launch_up_partial(Ctx& c, const OpIn& in, FinishArgs f) {
    const Layout& L = c.L;
    const imdbn_rbm_desc* d = c.d;
    const int mb = L.Bp / 64;
    const int64_t ats = (int64_t)L.Bp * L.Vpad;
    const bool four = L.up4 && c.r.vec4;
    if (four)
        hipLaunchKernelGGL(c.nw == 3 ? gemm_up4_partial<3> : gemm_up4_partial<1>, dim3(cdiv(L.H, 128), L.up.ks, mb), dim3(256), 0, c.s,
                           d->W, d->ldw, L.V, L.H, in.rm, ats, L.Vpad, in.flag, in.terms, L.partial, L.Bp, L.up.kchunk, g_dbg >> 4);
    else
        hipLaunchKernelGGL(c.nw == 3 ? gemm_up_partial<3> : gemm_up_partial<1>, dim3(cdiv(L.H, 64), L.up.ks, mb), dim3(256), 0, c.s,
                           d->W, d->ldw, L.V, L.H, in.rm, ats, L.Vpad, in.flag, in.terms, L.partial, L.Bp, L.up.kchunk);
    HIPCHK(hipGetLastError());
    dim3 fgrid(cdiv(f.N, 64), L.P);
    if ((int)(fgrid.x * fgrid.y) + IMDBN_MAX_GROUPS * mb > L.n_loss_slots) return fail(IMDBN_E_INVALID, "internal: loss slots");
    f.dbg = g_dbg;
    hid_bits_out(c, f, 0, 0);
    hipLaunchKernelGGL(finish, fgrid, dim3(256), 0, c.s, f);
    HIPCHK(hipGetLastError());
    ran_up(four ? IMDBN_ROUTE_UP_PARTIAL4 : IMDBN_ROUTE_UP_PARTIAL, !f.simple);
    return 0;
}

// ---- K2: fused GEMM + epilogue (no split-K slabs).  `blocks`: blocks per batch chunk = squared-error partials left ------
// 0/1 hidden operand as a bit plane: one tile of k2s_tr rows per CU, 16x16x32 MFMA (kernels_stream.hpp)
int launch_k2_stream(Ctx& c, const uint8_t* hbits, FinishArgs& f, const PrepArgs* next, int& blocks) {
    const Layout& L = c.L;
    const int mb = L.Bp / 64;
    CHK(kernel_attrs_ready());
    K2sArgs a;
    memset(&a, 0, sizeof(a));
    a.W = c.d->W; a.ldw = c.d->ldw; a.K = L.H; a.N = L.V; a.abits = hbits; a.Bp = L.Bp; a.TR = L.k2s_tr;
    const int MT = cdiv(a.TR, 16);
    blocks = cdiv(L.Vpad, a.TR);
    if ((blocks + IMDBN_MAX_GROUPS) * mb > L.n_loss_slots) return fail(IMDBN_E_INVALID, "internal: loss slots");
    f.dbg = g_dbg;
    if (f.op.bits && (f.n_groups > 0 || f.vmode == 0)) f.op.bits = nullptr;      // not a pure 0/1 sample
    f.lean = finish_lean(f);
    if (next) return fail(IMDBN_E_INVALID, "internal: k2_stream carries no next-batch blocks");
    const size_t lds = (size_t)((cdiv(L.H, 32) * 256 + 255) & ~255) + (size_t)std::max(K2S_LW * 16 * MT * K2S_LDR * 4, 64);
    if (lds > 160 * 1024 || MT > 3) return fail(IMDBN_E_UNSUPPORTED, "internal: k2_stream LDS");
    hipLaunchKernelGGL(k2s_insts[c.nw == 3][MT - 1][!f.lean], dim3(blocks, 1, mb), dim3(64 * K2S_W), lds, c.s, a, f);
    HIPCHK(hipGetLastError());
    ran_down(IMDBN_ROUTE_DOWN_K2_STREAM, !f.lean);
    return 0;
}

// How the fused K2 of a real-valued (or bf16-form) operand covers a batch of several 64-row chunks: one block per weight tile
// takes 2 or 4 of them, a wave (pair) per chunk, on full 32-row tiles (decode / visible_probs of a 256-row batch: 4 x 500
// blocks of 20 rows in four rounds -> 313 blocks in one) ... and, where the squared-error partials of 32-row tiles fit, the
// LDS-tiled kernel: 128 weight rows x 64 batch rows per block, the activation terms staged once per block (gemm_down_tiled)
struct DownPlan { int mbb, tr; bool tiled; };
DownPlan plan_down(const Ctx& c, const uint8_t* hbits, const FinishArgs& f, const PrepArgs* next) {
    const Layout& L = c.L;
    const Tuning& t = tune();
    const int mb = L.Bp / 64;
    const bool multi = mb >= 2 && !hbits && !next && c.r.vec4 && !(f.rm_src && f.op.rm) && L.Vpad >= 128 * 32;      // (fewer than 128 weight tiles: the per-chunk grid fills the chip better)
    const int mbb = (multi && !t.no_down_chunks) ? (mb % 4 == 0 ? 4 : (mb % 2 == 0 ? 2 : 1)) : 1;
    return {mbb, mbb > 1 ? 32 : L.down_tr,
            multi && !t.no_down_tiled && !t.no_down_chunks && (4 * cdiv(L.Vpad, 128) + IMDBN_MAX_GROUPS) * mb <= L.n_loss_slots};
}
// the epilogue writes a visible bit plane byte-wise: only a pure 0/1 sample, on tiles that are whole bytes wide
void down_bits_out(FinishArgs& f, int tr, int cols) {
    f.dbg = g_dbg;
    if (f.op.bits && (tr % 8 != 0 || f.n_groups > 0 || f.vmode == 0)) f.op.bits = nullptr;
    f.op.bits_shape = 1; f.op.bits_cols = cols;
}

int launch_down_tiled(Ctx& c, const OpIn& in, const DownPlan& p, FinishArgs& f, int& blocks) {
    const Layout& L = c.L;
    dim3 gt(cdiv(L.Vpad, 128), 1, L.Bp / 64);
    blocks = 4 * (int)gt.x;
    down_bits_out(f, p.tr, 32);
    hipLaunchKernelGGL(c.nw == 3 ? gemm_down_tiled<3> : gemm_down_tiled<1>, gt, dim3(256), 0, c.s, c.d->W, c.d->ldw, L.H, L.V,
                       in.rm, (int64_t)L.Bp * L.Hpad, L.Hpad, in.flag, in.terms, f);
    HIPCHK(hipGetLastError());
    ran_down(IMDBN_ROUTE_DOWN_TILED, !f.simple);
    return 0;
}

// tiles cover [0, Vpad): the K16-blocked operand form must have its padding columns [V, Vpad) written (zeros) -- the
// next K1 multiplies them with clamped (non-zero) weight rows.  Tiles of 20 / 24 / 28 rows (chosen for V in
// (4096, 7168]) do not end on a multiple of 16 by themselves; found by tools/stress_parity.py.
// `hbits`: sampled hidden states left by K1 in bit-packed form: 16x less activation traffic per block
// `next`: + one block per (64-column tile, batch chunk) of the NEXT batch behind the weight tiles (prep_item_body)
int launch_down_fused(Ctx& c, const OpIn& in, const uint8_t* hbits, const DownPlan& p, FinishArgs& f, const PrepArgs* next, int& blocks) {
    const Layout& L = c.L;
    const imdbn_rbm_desc* d = c.d;
    const int mb = L.Bp / 64, w3 = c.nw == 3;
    const int64_t ats = (int64_t)L.Bp * L.Hpad;
    dim3 grid(cdiv(L.Vpad, p.tr), 1, mb / p.mbb);
    blocks = (int)grid.x;
    down_bits_out(f, p.tr, p.tr);
    if ((blocks + IMDBN_MAX_GROUPS) * mb > L.n_loss_slots) return fail(IMDBN_E_INVALID, "internal: loss slots");
    if (p.mbb > 1) {
        hipLaunchKernelGGL(down_chunk_insts[w3][p.mbb == 4], grid, dim3(256), 0, c.s, d->W, d->ldw, L.H, L.V, in.rm, ats, L.Hpad,
                           in.flag, in.terms, f, p.tr, hbits, L.ldbits);
    } else if (next) {
        if (!c.r.vec4 || in.terms != 1) return fail(IMDBN_E_INVALID, "internal: next-batch prep on an ineligible K2");
        dim3 gn(grid.x + cdiv(std::max(next->N, next->op.ldrm), 64), 1, mb);
        hipLaunchKernelGGL(down_next_insts[w3][hbits != nullptr], gn, dim3(256), 0, c.s, d->W, d->ldw, L.H, L.V, in.rm, ats, L.Hpad,
                           f, p.tr, hbits, L.ldbits, *next, blocks);
    } else {
        const int kind = hbits ? 0 : (in.terms == 1 ? 1 : (in.terms == 3 ? 2 : 3));
        hipLaunchKernelGGL(down_insts[w3][c.r.vec4][kind], grid, dim3(256), 0, c.s, d->W, d->ldw, L.H, L.V, in.rm, ats, L.Hpad,
                           in.flag, in.terms, f, p.tr, hbits, L.ldbits);
    }
    HIPCHK(hipGetLastError());
    ran_down(p.mbb == 4 ? IMDBN_ROUTE_DOWN_CHUNKS4 : (p.mbb == 2 ? IMDBN_ROUTE_DOWN_CHUNKS2 : IMDBN_ROUTE_DOWN_FUSED), !f.simple);
    return 0;
}

// ---- one propagation -------------------------------------------------------------------------------
int prop(Ctx& c, bool up, OpIn in, FinishArgs f, const PrepArgs* next = nullptr) {
    const Layout& L = c.L;
    common_finish(c, up, f);
    if (up) {
        switch (c.r.up(in, f.logits_only != 0)) {
            case Up::fused: return launch_up_fused(c, in, f);
            case Up::stream_bits: return launch_k1_stream(c, in, true, f, next);
            case Up::stream_real: return launch_k1_stream(c, in, false, f, next);
            case Up::partial: break;
        }
        return launch_up_partial(c, in, f);
    }
    // softmax groups are finished by a kernel of their own, from fp32 copies of v_prob / v (scratch when the caller wants none)
    const bool groups = f.n_groups > 0 && !f.logits_only;
    if (groups && !f.out_prob) f.out_prob = L.f_vp, f.ld_prob = L.V;
    if (groups && !f.out_final) f.out_final = L.f_v[1], f.ld_final = L.V;
    // the hidden operand as the bit plane its K1 left (a sample)
    const uint8_t* hbits = (c.hid_bits_ok && in.rm == L.hid_rm && in.terms == 1 && !tune().no_bits) ? L.hid_bits : nullptr;
    int blocks = 0;
    if (hbits && c.r.k2s) {
        CHK(launch_k2_stream(c, hbits, f, next, blocks));
    } else {
        const DownPlan p = plan_down(c, hbits, f, next);
        if (p.tiled) CHK(launch_down_tiled(c, in, p, f, blocks));
        else CHK(launch_down_fused(c, in, hbits, p, f, next, blocks));
    }
    c.k2_blocks = blocks;
    if (groups) {
        hipLaunchKernelGGL(finish_groups, dim3(f.n_groups, L.Bp / 64), dim3(256), 0, c.s, f, (int)(blocks * (L.Bp / 64)));
        HIPCHK(hipGetLastError());
        t_route.down_groups = 1;
    }
    return 0;
}

// squared-error partials the K2 of this call left (+ one per softmax-group block); a call that ran no K2 (imdbn_rbm_apply_factors)
// reads what the CD pass of imdbn_rbm_cd_factors left
int n_loss_used(const Ctx& c) {
    return ((c.k2_blocks > 0 ? c.k2_blocks : c.r.cd_k2_blocks) + c.d->n_groups) * (c.L.Bp / 64);
}

// caller fp32 tensor -> operand forms in the workspace
int prep(Ctx& c, const float* in, int64_t ld, int N, bf16_t* rm, int ldrm, bf16_t* tr, int* flag,
         float* colsum = nullptr, int terms = 3, uint8_t* bits = nullptr) {
    PrepArgs p;
    memset(&p, 0, sizeof(p));
    // FAST mode reads ONE term of every operand: it must be the nearest bf16 (store_forms, terms == 1), not the first term of the
    // three-term truncation split, which is the operand rounded toward zero
    if (c.nw == 1) terms = 1;
    p.op.bits = bits; p.op.bits_shape = 0;
    p.zero = c.L.k1s_cnt; p.n_zero = (c.L.Bp / 64) * c.L.k1s_tiles;      // first launch of a call: arrival counters of k1_stream
    c.cnt_ok = true;
    p.in = in; p.ld = ld; p.B = c.L.B; p.Bp = c.L.Bp; p.N = N;
    p.op.rm = rm; p.op.ldrm = ldrm; p.op.rm_ts = (int64_t)c.L.Bp * ldrm; p.op.rm_terms = rm ? terms : 0; p.op.Bp = c.L.Bp;
    p.op.tr = tr; p.op.tr_ts = (int64_t)N * c.L.Bp; p.op.tr_terms = terms;
    p.flag = flag;
    p.colsum_part = colsum;
    hipLaunchKernelGGL(prep_operand, dim3(cdiv(std::max(N, ldrm), 64), c.L.P), dim3(256), 0, c.s, p);
    HIPCHK(hipGetLastError());
    return 0;
}

// The data operand of a forward pass at T = 1 -- imdbn_rbm_forward, and the fused forward of imdbn_rbm_cd_step on the forms its
// positive phase read (bit-identical): a 0/1 batch is read as a bit plane by k1_stream, anything else through the bf16 terms
OpIn data_operand(const Ctx& c, int data_binary) {
    const bool bits = c.r.data_bits(data_binary);
    return OpIn{c.L.vis_rm[0], c.nw == 1 ? 1 : 0, c.L.flags, bits ? c.L.vis_bits[0] : nullptr, bits ? data_operand_kind(data_binary) : 0};
}
