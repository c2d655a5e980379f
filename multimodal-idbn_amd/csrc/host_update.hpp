// host_update.hpp -- host side, part 3 (included by engine.hip after host_prop.hpp): launchers of the weight / bias update
// kernels (K3) from the statistics a CD pass left in the workspace, and the profiling bracket around them.
#pragma once

// ---- profiling of the update kernel (bench.py roofline leg) --------------------------------
struct Prof {
    bool on = false;
    std::vector<hipEvent_t> ev;   // pairs
    size_t used = 0;
    unsigned calls = 0;           // only every 8th update launch is bracketed (the 4th, 12th, ...): a bracket costs the stream ~10 us
                                  // (two event records: measured in the kernel trace as +5 us on the bracketed step and +5 on the next)
} g_prof;
struct ProfBracket {              // the update kernel(s) of one call between two HIP events on its stream
    bool on = false;
    int begin(hipStream_t s, bool wanted) {
        on = wanted && g_prof.on && (g_prof.calls++ % 8 == 3) && g_prof.used + 2 <= g_prof.ev.size();
        if (on) HIPCHK(hipEventRecord(g_prof.ev[g_prof.used], s));
        return 0;
    }
    int end(hipStream_t s) {
        if (on) { HIPCHK(hipEventRecord(g_prof.ev[g_prof.used + 1], s)); g_prof.used += 2; }
        return 0;
    }
};

BiasArgs make_bias(Ctx& c, const imdbn_cd_opts* o, bool sparsity, float n, float* loss_out) {
    const Layout& L = c.L;
    BiasArgs b;
    memset(&b, 0, sizeof(b));
    b.hid_bias = c.d->hid_bias; b.hb_m = c.d->hb_m; b.H = L.H; b.hpos = L.cs_hpos; b.hneg = L.cs_hneg;
    b.vis_bias = c.d->vis_bias; b.vb_m = c.d->vb_m; b.V = L.V; b.vpos = L.cs_vpos; b.vneg = L.cs_vneg;
    b.P = L.P; b.lr = o->lr; b.mom = o->momentum; b.n = n;
    b.sparsity = sparsity ? 1 : 0; b.target = o->sparsity_target;
    b.loss_part = L.loss_part; b.n_loss = n_loss_used(c); b.loss_den = n * (float)L.V; b.loss_out = loss_out;
    return b;
}

// bias / sparsity / error tail of the packed statistics buffer (after the V*H delta-W floats): written by the extra block row of the
// statistics kernel (BiasArgs::pack_tail) instead of a launch of its own
BiasArgs make_pack(Ctx& c, float* packed) {
    const imdbn_rbm_desc* d = c.d;
    BiasArgs b;
    memset(&b, 0, sizeof(b));
    b.pack_tail = packed + (size_t)d->V * d->H; b.H = d->H; b.V = d->V;
    b.hpos = c.L.cs_hpos; b.hneg = c.L.cs_hneg; b.vpos = c.L.cs_vpos; b.vneg = c.L.cs_vneg; b.P = c.L.P;
    b.loss_part = c.L.loss_part; b.n_loss = n_loss_used(c);
    return b;
}

int launch_bias(Ctx& c, const BiasArgs& b) {
    hipLaunchKernelGGL(bias_update, dim3(cdiv(std::max(c.L.V, c.L.H), 256) + 1), dim3(256), 0, c.s, b);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- testing aid: which update kernel the last launch_assoc / rank-loop update of this THREAD launched, and with how many visible
// tiles per block (imdbn_debug_last_update; the codes are IMDBN_UPDATE_* of the header).  Written where the launch is made
struct UpdateRec { int kernel = -1, tpb = 0; };
thread_local UpdateRec t_update;
inline void ran_update(int kernel, int tpb) { t_update.kernel = kernel; t_update.tpb = tpb; }

// ---- streaming update kernel: float4 weight tiles, LDS-staged planes, ~one block per CU, each streaming Route::tpb visible
// tiles with its hidden planes resident in LDS.  One launch per 64-row batch chunk or gathered rank block `i` of `n`
// (kernels_gemm.hpp AssocPlanesArgs::pass: only, first, middle, last); `br` extra block rows update the biases / reduce the loss
using K3Fn = decltype(&assoc_update_planes<0, 3, 0>);
const K3Fn k3_insts[2][2][4] = {        // [statistics mode][three hidden terms][pass]
    {{assoc_update_planes<0, 1, 0>, assoc_update_planes<0, 1, 1>, assoc_update_planes<0, 1, 2>, assoc_update_planes<0, 1, 3>},
     {assoc_update_planes<0, 3, 0>, assoc_update_planes<0, 3, 1>, assoc_update_planes<0, 3, 2>, assoc_update_planes<0, 3, 3>}},
    {{assoc_update_planes<1, 1, 0>, assoc_update_planes<1, 1, 1>, assoc_update_planes<1, 1, 2>, assoc_update_planes<1, 1, 3>},
     {assoc_update_planes<1, 3, 0>, assoc_update_planes<1, 3, 1>, assoc_update_planes<1, 3, 2>, assoc_update_planes<1, 3, 3>}}};
int k3_pass(int i, int n) { return n == 1 ? 0 : (i == 0 ? 1 : (i == n - 1 ? 3 : 2)); }
// block rows of a fused bias / loss update: >= 2 blocks, one reduces the loss, the rest stride the biases
int k3_bias_rows(const Layout& L) { return cdiv(L.H, 128) >= 2 ? 1 : 2; }
dim3 k3_grid(const Ctx& c, int br) { return dim3(cdiv(c.L.H, 128), cdiv(cdiv(c.L.V, 128), c.r.tpb) + br); }
// `bin`: the two-plane kernel of a single-chunk update with one-term visible operands (assoc_update_bin: same grid and arguments)
int launch_k3_planes(Ctx& c, int mode_stats, const AssocPlanesArgs& f, int pass, const BiasArgs& bb, int br, bool bin = false) {
    const K3Fn k = bin ? (c.ht == 3 ? assoc_update_bin<3> : assoc_update_bin<1>) : k3_insts[mode_stats != 0][c.ht == 3][pass];
    hipLaunchKernelGGL(k, k3_grid(c, br), dim3(256), 0, c.s, f, c.r.tpb, bb, br);
    HIPCHK(hipGetLastError());
    ran_update(bin ? IMDBN_UPDATE_BIN : IMDBN_UPDATE_PLANES, c.r.tpb);
    return 0;
}

// the update (or, mode_stats, the un-normalised statistics into `delta`) from the operand planes of this call's CD pass
int launch_assoc(Ctx& c, int mode_stats, const imdbn_cd_opts* o, int vpos_terms, const int* vpos_flag, int vneg_terms,
                 float n, float* delta, const BiasArgs* bias = nullptr) {
    const Layout& L = c.L;
    ProfBracket prof;
    CHK(prof.begin(c.s, !mode_stats));
    // fast path: every W / W_m / delta row start 16-B aligned
    if (c.r.vec4 && (((uintptr_t)(mode_stats ? (const void*)delta : (const void*)c.d->W_m)) & 15) == 0 && !tune().no_fast_k3) {
        AssocPlanesArgs f;
        memset(&f, 0, sizeof(f));
        f.W = c.d->W; f.Wm = c.d->W_m; f.ldw = c.d->ldw; f.V = L.V; f.H = L.H;
        f.vpos = L.vis_tr[0]; f.vpos_flag = vpos_flag; f.vpos_terms = vpos_terms;
        f.hpos = L.hid_tr[0]; f.vneg = L.vis_tr[1]; f.vneg_terms = vneg_terms; f.hneg = L.hid_tr[1];
        f.vts = (int64_t)L.V * L.Bp; f.hts = (int64_t)L.H * L.Bp; f.Bp = L.Bp;
        f.lr = o->lr; f.mom = o->momentum; f.wd = o->weight_decay; f.n = n; f.delta = delta; f.dbg = (g_dbg & 512) ? 1 : 0;
        BiasArgs bz;
        memset(&bz, 0, sizeof(bz));
        const int nchunk = L.Bp / 64;      // the bias / loss blocks ride on the last chunk
        // one-term visible operands on both sides: known here, or (vpos_terms == 0: an untagged batch, the bench's default) known
        // only to the device from the exactness map -- the kernel then branches once, at entry, to the old body for anything else
        const bool bin = !mode_stats && nchunk == 1 && vneg_terms == 1 && (vpos_terms == 1 || (vpos_terms == 0 && vpos_flag)) &&
                         !tune().no_update_bin;
        for (int ch = 0; ch < nchunk; ++ch) {
            f.b0 = 64 * ch;
            CHK(launch_k3_planes(c, mode_stats, f, k3_pass(ch, nchunk), bias ? *bias : bz, (bias && ch == nchunk - 1) ? k3_bias_rows(L) : 0, bin));
        }
        return prof.end(c.s);
    }
    AssocArgs a;
    memset(&a, 0, sizeof(a));
    a.W = c.d->W; a.Wm = c.d->W_m; a.ldw = c.d->ldw; a.V = L.V; a.H = L.H;
    a.vpos = L.vis_tr[0]; a.vpos_flag = vpos_flag; a.vpos_terms = vpos_terms;
    a.hpos = L.hid_tr[0]; a.hpos_terms = c.ht;
    a.vneg = L.vis_tr[1]; a.vneg_flag = vpos_flag; a.vneg_terms = vneg_terms;
    a.hneg = L.hid_tr[1]; a.hneg_terms = c.ht;
    a.vts = (int64_t)L.V * L.Bp; a.hts = (int64_t)L.H * L.Bp; a.Bp = L.Bp;
    a.lr = o->lr; a.mom = o->momentum; a.wd = o->weight_decay; a.n = n;
    a.delta = delta;
    hipLaunchKernelGGL(c.ht == 3 ? (mode_stats ? assoc_update<1, 3> : assoc_update<0, 3>) : (mode_stats ? assoc_update<1, 1> : assoc_update<0, 1>),
                       dim3(cdiv(L.H, 128), cdiv(L.V, 64)), dim3(256), 0, c.s, a);
    HIPCHK(hipGetLastError());
    ran_update(IMDBN_UPDATE_GENERIC, 0);
    CHK(prof.end(c.s));
    if (bias) CHK(launch_bias(c, *bias));          // generic K3: bias update as its own launch
    return 0;
}
