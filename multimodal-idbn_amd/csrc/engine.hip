// engine.hip -- C ABI (include/imdbn_engine.h) and host-side launch plans of the CD engine.
//
// Everything here is launch orchestration: carve the caller's workspace, advance the draw cursor in
// the reference's draw order, and enqueue kernels on the caller's stream.
// No host synchronisation, no allocation, no global state besides tuning knobs, the thread-local
// error string, what is known per device ordinal and the optional profiling events.
// The host code is one translation unit in six files: this one (context, CD / chain / factor orchestration, the C entries),
// host_layout.hpp (knobs, workspace layout, Route), host_prop.hpp (propagation launchers), host_update.hpp (update launchers),
// host_delta.hpp (the delta-rule step of a directed layer), host_backprop.hpp (the back-propagation step through a sigmoid layer).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/imdbn_engine.h"
#include "kernels_ew.hpp"
#include "kernels_gemm.hpp"
#include "kernels_chain.hpp"
#include "kernels_stream.hpp"
#include "kernels_trace.hpp"
#include "kernels_knn.hpp"
#include "kernels_energy.hpp"
#include "kernels_metrics.hpp"
#include "kernels_pair.hpp"
#include "kernels_ais.hpp"
#include "kernels_reverse_ais.hpp"
#include "kernels_bound.hpp"
#include "kernels_joint.hpp"
#include "kernels_labelgrad.hpp"
#include "kernels_pll.hpp"
#include "kernels_pt.hpp"
#include "kernels_centered.hpp"
#include "kernels_gauss.hpp"
#include "kernels_gauss_ais.hpp"
#include "kernels_gauss_bound.hpp"
#include "kernels_delta.hpp"
#include "kernels_backprop.hpp"
#include "kernels_gauss_backprop.hpp"
#include "kernels_exact.hpp"
#include "kernels_tuning.hpp"
#include "kernels_tap.hpp"
#include "kernels_dbm.hpp"
#include "kernels_dbm_ais.hpp"
#include "kernels_dbm_group.hpp"

using namespace imdbn;

namespace {

thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail((int)e_, "%s: %s", #expr, hipGetErrorString(e_));    \
    } while (0)
#define CHK(expr)                   \
    do {                            \
        int rc_ = (expr);           \
        if (rc_ != 0) return rc_;   \
    } while (0)

#include "host_layout.hpp"

// ---- draw cursor -----------------------------------------------------------------------------
struct Rng {
    imdbn_rng* r;
    int64_t tpos = 0, cpos = 0;
    uint64_t draws = 0;
    bool bad = false;
    explicit Rng(imdbn_rng* r_) : r(r_) {}
    DrawSrc floats(int B, int N) {
        DrawSrc s{};
        s.N = N;
        if (!r) { bad = true; return s; }
        s.seed = r->seed; s.row0 = r->row0; s.draw = r->offset + draws; s.base = (const unsigned long long*)r->dev_offset;
        if (r->mode == IMDBN_RNG_REPLAY) {
            if (!r->tape || tpos + (int64_t)B * N > r->tape_len) { bad = true; return s; }
            s.tape = r->tape + tpos;
            tpos += (int64_t)B * N;
        }
        ++draws;
        return s;
    }
    // categorical draws for all groups of one sample_visible call
    void cats(int B, int n_groups, const int32_t** tape, DrawSrc* uni) {
        *tape = nullptr;
        DrawSrc s{};
        s.N = 1;
        if (n_groups == 0) { *uni = s; return; }
        if (!r) { bad = true; *uni = s; return; }
        s.seed = r->seed; s.row0 = r->row0; s.draw = r->offset + draws; s.base = (const unsigned long long*)r->dev_offset;
        if (r->mode == IMDBN_RNG_REPLAY) {
            if (!r->cat_tape || cpos + (int64_t)B * n_groups > r->cat_len) { bad = true; *uni = s; return; }
            *tape = r->cat_tape + cpos;
            cpos += (int64_t)B * n_groups;
        }
        draws += n_groups;
        *uni = s;
    }
    int finish() {
        if (r) { r->tape_used = tpos; r->cat_used = cpos; r->draws_used = draws; }
        if (bad) return fail(IMDBN_E_RNG, "random draws requested but rng is null or the replay tape is exhausted");
        return 0;
    }
};

// ---- context -----------------------------------------------------------------------------------
struct Ctx {
    const imdbn_rbm_desc* d;
    Layout L;
    hipStream_t s;
    Rng rng;
    int nw;         // weight terms
    int rt;         // terms of a real-valued activation operand
    int ht;         // terms of the hidden-probability planes of the update kernel (K3) = rt.  Two terms (hi + mid, 16 bits) were tried in
                    // round 2: K3's staging and K1's plane stores shrink by a third, but the 2^-17 relative error of the statistics
                    // random-walks into the weights over thousands of small-batch updates (joint RBM, batch 8: ~1e-5 after 1500 updates)
                    // and flipped a sample of the train_joint fixture (margin 9e-6).  Exact products stay.
    bool hid_bits_ok = false;      // L.hid_bits describes the current contents of L.hid_rm
    bool data_prepped = false;     // cd_phases: the data-side operands are already in place (prefetch slot)
    Route r{};                     // which kernel runs what in this call (setup)
    int k2_blocks = 0;             // blocks (per batch chunk) of the last K2 launch = the squared-error partials it left (prop())
    bool pos_phase = false;        // tuning aid: the propagation being launched is the positive phase of a CD pass (dbg bit 2048 stamps it, bit 64 the others)
    bool cnt_ok = false;           // the arrival counters of k1_stream are known to be zero: a launch of THIS call cleared them (prep / chain_init), or the
                                   // data-side operands come from a prefetch slot (an earlier call on this workspace ran, and every launch leaves them
                                   // zero).  Otherwise prop() clears them itself: a caller's workspace may hold anything
                                   // (tools/stress_chains.py on a NaN-filled workspace: chains of a layer wider than 1024 were all NaN)
    bool fix_slot = false;         // the data-side operands were written item by item (PrepArgs::adaptive): the next k1_stream that reads them
                                   // completes the planes of mixed spans for the update kernel (K1sArgs::fix_tr)
    Ctx(const imdbn_rbm_desc* d_, imdbn_rng* r, hipStream_t s_) : d(d_), s(s_), rng(r) {
        nw = d->mode == IMDBN_FAST_BF16 ? 1 : 3;
        rt = nw;
        ht = rt;
    }
};

int check_desc(const imdbn_rbm_desc* d, bool need_momentum) {
    if (!d) return fail(IMDBN_E_INVALID, "null descriptor");
    if (d->V <= 0 || d->H <= 0) return fail(IMDBN_E_INVALID, "bad shape V=%d H=%d", d->V, d->H);
    if (!d->W || !d->hid_bias || !d->vis_bias) return fail(IMDBN_E_INVALID, "null parameter pointer");
    if (d->ldw < d->H) return fail(IMDBN_E_INVALID, "ldw %lld < H %d", (long long)d->ldw, d->H);
    if (need_momentum && (!d->W_m || !d->hb_m || !d->vb_m)) return fail(IMDBN_E_INVALID, "null momentum buffer");
    if (d->n_groups < 0 || d->n_groups > IMDBN_MAX_GROUPS)
        return fail(IMDBN_E_UNSUPPORTED, "at most %d softmax groups supported, got %d", IMDBN_MAX_GROUPS, d->n_groups);
    for (int g = 0; g < d->n_groups; ++g) {
        if (d->group_start[g] < 0 || d->group_end[g] > d->V || d->group_start[g] >= d->group_end[g])
            return fail(IMDBN_E_INVALID, "softmax group %d = (%d,%d) outside [0,%d)", g, d->group_start[g], d->group_end[g], d->V);
        if (d->group_end[g] - d->group_start[g] > GROUP_WMAX)
            return fail(IMDBN_E_UNSUPPORTED, "softmax group %d is %d wide; at most %d supported", g, d->group_end[g] - d->group_start[g], GROUP_WMAX);
        for (int k = 0; k < g; ++k)
            if (d->group_start[g] < d->group_end[k] && d->group_start[k] < d->group_end[g])
                return fail(IMDBN_E_INVALID, "overlapping softmax groups %d and %d", k, g);
    }
    if (d->mode != IMDBN_PARITY_F32 && d->mode != IMDBN_FAST_BF16) return fail(IMDBN_E_INVALID, "bad mode %d", d->mode);
    return 0;
}

int setup(Ctx& c, int B, void* ws, size_t ws_bytes) {
    if (B <= 0) return fail(IMDBN_E_INVALID, "batch %d", B);
    if (!ws) return fail(IMDBN_E_WORKSPACE, "null workspace");
    if (((uintptr_t)ws & 255) != 0) return fail(IMDBN_E_INVALID, "workspace must be 256-byte aligned");
    c.L = make_layout(c.d->V, c.d->H, B, (char*)ws);
    if (c.L.bytes > ws_bytes)
        return fail(IMDBN_E_WORKSPACE, "workspace %zu < %zu bytes needed for V=%d H=%d B=%d", ws_bytes, c.L.bytes, c.d->V, c.d->H, B);
    c.r = make_route(c.d, c.L);
    return 0;
}

#include "host_prop.hpp"
#include "host_update.hpp"
#include "host_delta.hpp"
#include "host_backprop.hpp"

// The caller's fp32 rows x (visible rows when `up`, hidden rows otherwise) into the row-major operand form of their side, then the
// propagation from it with `f`.
int prep_prop(Ctx& c, bool up, const float* x, int64_t ldx, const FinishArgs& f) {
    const Layout& L = c.L;
    bf16_t* rm = up ? L.vis_rm[0] : L.hid_rm;
    int* flags = up ? L.flags : L.flags_h;
    CHK(prep(c, x, ldx, up ? c.d->V : c.d->H, rm, up ? L.Vpad : L.Hpad, nullptr, flags));
    return prop(c, up, OpIn{rm, c.nw == 1 ? 1 : 0, flags}, f);
}

// The two raw-logit propagations the likelihood calls are built from.  x = c + rows W of fp32 `rows` (pitch ld) into f_h at pitch H:
static int up_logits(Ctx& c, const float* rows, int64_t ld) {
    FinishArgs f = new_finish();
    f.logits_only = 1;
    f.out_prob = c.L.f_h; f.ld_prob = c.L.H;
    return prep_prop(c, true, rows, ld, f);
}
// ... and b + h W^T of the h in hid_rm (one term) into `out` at pitch V.
static int down_logits(Ctx& c, float* out) {
    FinishArgs f = new_finish();
    f.logits_only = 1;
    f.out_prob = out; f.ld_prob = c.L.V;
    return prop(c, false, OpIn{c.L.hid_rm, 1, nullptr}, f);
}

// What imdbn_energy_trace and imdbn_rbm_label_loglik start from: a joint RBM over [z | y | ...] with the code in the first Dz visible
// columns and K labels behind it.  check() opens either call (`name`, for the messages), the call's own checks follow it, then
// propagate() leaves base = z W[:Dz] + c -- the logits path of prop_up on the descriptor cut to its first Dz weight rows -- in the
// workspace.
struct LabelSide {
    imdbn_rbm_desc dz;      // the cut descriptor
    Ctx c;
    const float *base, *bz, *by, *Wy;      // base [N][H] of pitch H; biases of the code and label columns; the labels' weight rows
    static int check(const char* name, const imdbn_rbm_desc* d, int Dz, int K) {
        if (K < 2 || K > LABEL_KMAX) return fail(IMDBN_E_INVALID, "%s: K = %d outside [2, %d]", name, K, LABEL_KMAX);
        if (Dz < 1 || (int64_t)Dz + K > d->V) return fail(IMDBN_E_INVALID, "%s: Dz = %d, K = %d do not fit V = %d", name, Dz, K, d->V);
        return 0;
    }
    LabelSide(const imdbn_rbm_desc* d, int Dz, hipStream_t stream) : dz(*d), c(&dz, nullptr, stream) {
        dz.V = Dz; dz.n_groups = 0;
        bz = d->vis_bias; by = d->vis_bias + Dz; Wy = d->W + (int64_t)Dz * d->ldw;
    }
    LabelSide(const LabelSide&) = delete;      // c.d points at dz
    int propagate(const float* z, int64_t ldz, int N, void* ws, size_t ws_bytes) {
        CHK(setup(c, N, ws, ws_bytes));
        base = c.L.f_h;
        return up_logits(c, z, ldz);
    }
};

// testing aid: how the last CD pass of this THREAD ran (imdbn_debug_last_cd): the families of its positive-phase K1, its first K2 and
// its last K1 as the launchers recorded them (t_route), where the next batch was prepared (IMDBN_CD_NEXT_*), the data slot consumed
// and whether the preparation decided per item.  Written where the decision is made (cd_prologue) / behind the launch (cd_phases)
struct CdRec { int pos_up = -1, first_down = -1, last_up = -1, next_on = 0, slot = 0, adaptive = 0; };
thread_local CdRec t_cd;

// rbm.py:199-209: positive phase, CD-k Gibbs, statistics left in the workspace operand buffers.
int cd_phases(Ctx& c, const float* data, int64_t ldd, const imdbn_cd_opts* o, const PrepArgs* next = nullptr) {
    const Layout& L = c.L;
    const int B = L.B;
    if (o->cd_k < 1) return fail(IMDBN_E_INVALID, "CD=%d (the reference needs CD>=1, rbm.py:204-209)", o->cd_k);
    if (!c.data_prepped) CHK(prep(c, data, ldd, L.V, L.vis_rm[0], L.Vpad, L.vis_tr[0], L.flags, L.cs_vpos, 3, L.vis_bits[0]));
    // (Route: the visible sample of the negative phase leaves its K2 as a bit plane, and which launch carries `next`)
    const bool vbits = c.r.vbits, next_on_k1 = next && c.r.next_on_k1;
    // positive phase: P+ = up(data); h = 1[P+ > U]
    {
        FinishArgs f = new_finish();
        f.vmode = 1; f.uni = c.rng.floats(B, L.H);
        f.op.rm = L.hid_rm; f.op.rm_terms = 1; f.rm_src = 2;
        f.op.tr = L.hid_tr[0]; f.op.tr_terms = c.ht; f.tr_src = 1;
        f.colsum_part = L.cs_hpos; f.colsum_src = 1;
        c.pos_phase = true;
        const int rc = prop(c, true, OpIn{L.vis_rm[0], c.nw == 1 ? 1 : 0, L.flags, L.vis_bits[0], data_operand_kind(o->data_binary)}, f);
        c.pos_phase = false;
        CHK(rc);
        t_cd.pos_up = t_route.up;
        if (next) t_cd.next_on = next_on_k1 ? IMDBN_CD_NEXT_K1_STREAM : IMDBN_CD_NEXT_FUSED_K2;
    }
    for (int it = 0; it < o->cd_k; ++it) {
        const bool last = (it == o->cd_k - 1);
        {   // v_prob = down(h); v = sampleV(v_prob)
            FinishArgs f = new_finish();
            f.vmode = 1; f.uni = c.rng.floats(B, L.V);
            c.rng.cats(B, c.d->n_groups, &f.cat_tape, &f.cat_uni);
            // the fp32 copies of v_prob / v are only read back by the softmax-group kernel (prop() supplies
            // scratch for them when groups exist): without groups nobody needs them -> 5 MB of stores saved
            // the K16-blocked bf16 form only feeds a K1 that cannot read the bit plane (its 2-byte scattered stores were most
            // of the fused K2's 3.8 us epilogue)
            if (c.r.neg_rm) { f.op.rm = L.vis_rm[1]; f.op.rm_terms = 1; f.rm_src = 2; }
            f.op.tr = L.vis_tr[1]; f.op.tr_terms = 1; f.tr_src = 2;
            f.colsum_part = L.cs_vneg; f.colsum_src = 2;
            f.loss_ref = data; f.ld_ref = ldd; f.loss_src = 1; f.loss_part = L.loss_part;
            if (vbits) f.op.bits = L.vis_bits[1];
            CHK(prop(c, false, OpIn{L.hid_rm, 1, nullptr}, f, (it == 0 && !next_on_k1) ? next : nullptr));
            if (it == 0) t_cd.first_down = t_route.down;
        }
        {   // h_prob = up(v); h = 1[h_prob > U]  (the last draw is consumed but unused, rbm.py:208)
            FinishArgs f = new_finish();
            DrawSrc u = c.rng.floats(B, L.H);
            if (!last) { f.vmode = 1; f.uni = u; f.op.rm = L.hid_rm; f.op.rm_terms = 1; f.rm_src = 2; }
            f.op.tr = L.hid_tr[1]; f.op.tr_terms = c.ht; f.tr_src = 1; f.op.tr_negate = 1;
            f.colsum_part = L.cs_hneg; f.colsum_src = 1;
            CHK(prop(c, true, OpIn{L.vis_rm[1], 1, nullptr, vbits ? L.vis_bits[1] : nullptr, 1}, f, (it == 0 && next_on_k1) ? next : nullptr));
            if (last) t_cd.last_up = t_route.up;
        }
    }
    return 0;
}

// ---- row-parallel chain kernel (kernels_chain.hpp) -------------------------------------------
// testing aid: how the last chain call of this THREAD ran (imdbn_debug_last_chain; the codes are IMDBN_CHAIN_* of the header): the
// route, rows per block and blocks of the kernel launch, records of chain 0.  Written where the decision / the launch is made
struct ChainRun { int route = -1, rows = 0, blocks = 0, recs = 0; };
thread_local ChainRun t_chain;
inline void ran_chain(int route, int rows, int blocks, int recs) { t_chain.route = route; t_chain.rows = rows; t_chain.blocks = blocks; t_chain.recs = recs; }

bool chain_kernel_ok(const Ctx& c, int n_steps) {
    const Layout& L = c.L;
    if (tune().no_chain_kernel || !L.k4_planes || n_steps < 2 || n_steps > CHAIN_MAX_STEPS) return false;
    if (c.d->n_groups > 1) return false;                   // the kernel keeps ONE softmax group's logits in LDS
    const int gw = c.d->n_groups ? c.d->group_end[0] - c.d->group_start[0] : 0;
    const size_t lds = (size_t)(c.nw == 3 ? 2 : 1) * K4_ROWS * ((rup(L.V, 32) + 8) + (rup(L.H, 32) + 8)) * 2      // activation terms
                     + (size_t)K4_ROWS * (rup(std::max(L.V, L.H), 16) + 1) * 4                        // fp32 stage
                     + (size_t)K4_ROWS * (gw + 1) * 4 + K4_ROWS * 16                                   // group logits, row stats
                     + (size_t)(K4_ROWS / 2) * gw * 2 * 4;                                             // group-column noise drawn ahead
    return gw <= GROUP_WMAX && lds <= (size_t)K4_LDS_BYTES;
}

// One chain as the host sees it (imdbn_chain_spec + where its final state goes)
struct ChainSpec {
    const float* vk; const float* mask; int64_t ldk; int init_uniform; int n_steps; const imdbn_chain_step* st;
    const float* mu; int64_t ldmu; int Dz; float* out; int64_t ldo;
    const imdbn_chain_trace* tr = nullptr;           // imdbn_rbm_chain_traced: what to record (nullable)
    const imdbn_chain_trace* htr = nullptr;          // imdbn_rbm_chain_traced_vh: the hidden window to record (nullable; never has a baseline)
    int base() const { return tr && tr->with_baseline ? 1 : 0; }
    int n_recs() const { return n_steps + base(); }  // with a baseline, record 0 is an observe-only step (no draws, no state change)
};

// v0 = vk*m + (1-m)*U   (rbm.py:271,333,392) into `out` (and, for the per-launch path, the operand forms of vis_rm[0])
int chain_init(Ctx& c, const ChainSpec& s, bool forms, bool stats_now) {
    const Layout& L = c.L;
    const int B = L.B;
    PrepArgs p;
    memset(&p, 0, sizeof(p));
    p.in = s.vk; p.ld = s.ldk; p.B = B; p.Bp = L.Bp; p.N = L.V;
    if (s.init_uniform) { p.mix = 1; p.mask = s.mask; p.ldm = s.ldk; p.uni = c.rng.floats(B, L.V); }
    p.out_f32 = s.out; p.ldo = s.ldo;
    p.op.ldrm = L.Vpad; p.op.rm_ts = (int64_t)L.Bp * L.Vpad; p.op.Bp = L.Bp;
    if (forms) { p.op.rm = L.vis_rm[0]; p.op.rm_terms = c.rt; }
    if (stats_now) {
        p.op.tr = L.vis_tr[0]; p.op.tr_ts = (int64_t)L.V * L.Bp; p.op.tr_terms = c.rt;
        p.colsum_part = L.cs_vpos;
    }
    p.zero = L.k1s_cnt; p.n_zero = (L.Bp / 64) * L.k1s_tiles;      // (as prep(): the per-launch chain of a wide layer runs k1_stream)
    c.cnt_ok = true;
    hipLaunchKernelGGL(prep_operand, dim3(cdiv(L.Vpad, 64), L.P), dim3(256), 0, c.s, p);
    HIPCHK(hipGetLastError());
    return 0;
}

// draw cursors of a chain's steps in exactly the order of the per-launch path, written as records [off, off + n_steps)
int chain_records(Ctx& c, const ChainSpec& s, int off) {
    const Layout& L = c.L;
    const imdbn_rbm_desc* d = c.d;
    const int B = L.B;
    ChainRecBatch batch;
    const int nr = s.n_recs(), b0 = s.base();
    for (int t0 = 0; t0 < nr; t0 += CHAIN_REC_BATCH) {
        const int n = std::min(CHAIN_REC_BATCH, nr - t0);
        memset(&batch, 0, sizeof(batch));
        for (int i = 0; i < n; ++i) {
            ChainRec& r = batch.r[i];
            if (t0 + i < b0) { r.T = 1.0f; r.flags = 16; continue; }      // the traced baseline p(v | p(h | v0)) at T = 1
            const imdbn_chain_step& st = s.st[t0 + i - b0];
            r.T = st.T; r.sigma = st.sigma; r.eta = st.eta;
            r.flags = (st.sample_h ? 1 : 0) | ((st.vmode & 3) << 1) | (st.clamp ? 8 : 0);
            auto cd = [](const DrawSrc& x) { ChainDraw y; y.tape = x.tape; y.draw = x.draw; return y; };
            if (st.sigma > 0.f) r.noise_h = cd(c.rng.floats(B, L.H));
            if (st.sample_h) r.uni_h = cd(c.rng.floats(B, L.H));
            if (st.sigma > 0.f) r.noise_v = cd(c.rng.floats(B, L.V));
            if (st.vmode != 0) {
                r.uni_v = cd(c.rng.floats(B, L.V));
                DrawSrc cu; c.rng.cats(B, d->n_groups, &r.cat_tape, &cu);
                r.cat_uni = cd(cu);
            }
        }
        hipLaunchKernelGGL(chain_write_recs, dim3(1), dim3(64), 0, c.s, batch, L.chain_recs + off + t0, n);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// the chain kernel for one chain (s1 == nullptr) or two independent ones of the same RBM in one launch
int launch_k4(Ctx& c, const ChainSpec& s0, int off0, const ChainSpec* s1, int off1) {
    const Layout& L = c.L;
    const imdbn_rbm_desc* d = c.d;
    const int B = L.B;
    {
        const dim3 sg(std::max(cdiv(L.H, 16), cdiv(L.V, 16)), std::max(cdiv(L.V, 32), cdiv(L.H, 32)), 2);
        if (c.nw == 3) hipLaunchKernelGGL(k4_split_planes<2>, sg, dim3(64), 0, c.s, d->W, d->ldw, L.V, L.H, L.k4_planes, L.k4_plane_stride);
        else           hipLaunchKernelGGL(k4_split_planes<1>, sg, dim3(64), 0, c.s, d->W, d->ldw, L.V, L.H, L.k4_planes, L.k4_plane_stride);
    }
    K4Args a;
    memset(&a, 0, sizeof(a));
    a.planes = L.k4_planes; a.plane_stride = L.k4_plane_stride;
    a.V = L.V; a.H = L.H; a.nw = c.nw; a.rt = c.rt;
    a.hid_bias = d->hid_bias; a.vis_bias = d->vis_bias;
    a.n_groups = d->n_groups;
    for (int g = 0; g < IMDBN_MAX_GROUPS; ++g) { a.gs[g] = d->group_start[g]; a.ge[g] = d->group_end[g]; }
    a.seed = c.rng.r ? c.rng.r->seed : 0; a.row0 = c.rng.r ? c.rng.r->row0 : 0;
    a.draw_base = c.rng.r ? (const unsigned long long*)c.rng.r->dev_offset : nullptr;
    auto seg = [&](const ChainSpec& s, int off) {
        K4Seg g;
        g.state = s.out; g.lds = s.ldo; g.recs = L.chain_recs + off; g.n_steps = s.n_steps;
        g.mu = s.mu; g.ldmu = s.ldmu; g.Dz = s.Dz; g.vk = s.vk; g.mask = s.mask; g.ldk = s.ldk; g.B = B;
        g.n_steps = s.n_recs();
        g.tr = nullptr; g.tr_ld = g.tr_ss = 0; g.tr_c0 = g.tr_c1 = 0;
        if (s.tr) { g.tr = s.tr->out; g.tr_ld = s.tr->ld_row; g.tr_ss = s.tr->step_stride; g.tr_c0 = s.tr->c0; g.tr_c1 = s.tr->c1; }
        g.htr = nullptr; g.htr_ld = g.htr_ss = 0; g.htr_c0 = g.htr_c1 = 0; g.htr_t0 = s.base();      // hidden slot 0 = the first record that is a chain step
        if (s.htr) { g.htr = s.htr->out; g.htr_ld = s.htr->ld_row; g.htr_ss = s.htr->step_stride; g.htr_c0 = s.htr->c0; g.htr_c1 = s.htr->c1; }
        return g;
    };
    a.s0 = seg(s0, off0);
    a.s1 = s1 ? seg(*s1, off1) : a.s0;
    // rows per block: enough blocks to spread the per-element work (Philox, Box-Muller, sigmoid) over the CUs;
    // one block per CU at most (every block streams all of W from L2)
    const Tuning& t = tune();
    a.dbg = (g_dbg & 1024) ? 1 : 0;
    const int nch = s1 ? 2 : 1, BT = B * nch;
    a.rows = t.k4_rows > 0 ? t.k4_rows : (BT <= 2 * cu_count() ? 2 : (BT <= 4 * cu_count() ? 4 : (BT <= 8 * cu_count() ? 8 : 16)));      // measured: 0.90 / 0.99 / 1.19 / 1.59 ms for 2 / 4 / 8 / 16 rows (30 steps, 532<->256)
    a.nblk0 = cdiv(B, a.rows);
    const dim3 grid(a.nblk0 * nch);
    if (c.nw == 3) hipLaunchKernelGGL(k4_chain<2>, grid, dim3(64 * K4_WAVES), 0, c.s, a);      // PARITY: fp16 hi + lo terms
    else           hipLaunchKernelGGL(k4_chain<1>, grid, dim3(64 * K4_WAVES), 0, c.s, a);
    HIPCHK(hipGetLastError());
    ran_chain(s1 ? IMDBN_CHAIN_KERNEL_PAIR : IMDBN_CHAIN_KERNEL, a.rows, (int)grid.x, s0.n_recs());
    return 0;
}

// chain: init + steps.  The final state ends in fp32 `out` (ld ldo); with want_stats also as operand forms in vis_rm[0] (rt terms),
// the transposed form in vis_tr[0] and column sums in cs_vpos (the positive phase of the clamped update).
int run_chain(Ctx& c, const ChainSpec& s, bool want_stats) {
    const Layout& L = c.L;
    const int B = L.B;
    const float* vk = s.vk; const float* mask = s.mask; const int64_t ldk = s.ldk, ldo = s.ldo, ldmu = s.ldmu;
    const int n_steps = s.n_steps, Dz = s.Dz; const imdbn_chain_step* st = s.st; const float* mu = s.mu; float* out = s.out;
    if (n_steps < 0 || (n_steps > 0 && !st)) return fail(IMDBN_E_INVALID, "bad chain steps");
    if (mu && (Dz <= 0 || Dz > L.V)) return fail(IMDBN_E_INVALID, "mu-pull width %d outside (0,%d]", Dz, L.V);
    const bool k4 = chain_kernel_ok(c, s.n_recs());
    CHK(chain_init(c, s, !k4 || s.n_recs() == 0, want_stats && n_steps == 0));
    if (k4) {
        CHK(chain_records(c, s, 0));
        CHK(launch_k4(c, s, 0, nullptr, 0));
        // operand forms of the final state (what the last v|h launch of the per-launch path leaves behind): only the clamped update reads them
        if (want_stats) CHK(prep(c, out, ldo, L.V, L.vis_rm[0], L.Vpad, L.vis_tr[0], nullptr, L.cs_vpos, c.rt));
        c.hid_bits_ok = false;
        return 0;
    }
    ran_chain(IMDBN_CHAIN_PER_LAUNCH, 0, 0, s.n_recs());
    const int s_base = s.base();
    // the traces of the per-launch path: the window of the step's fp32 v_prob (f_vp), of its fp32 h_prob (f_h)
    auto copy_window = [&](const imdbn_chain_trace* tr, const float* src, int ld, int slot) -> int {
        if (!tr) return 0;
        const int w = tr->c1 - tr->c0;
        const int blocks = (int)std::min<int64_t>(((int64_t)B * w + 255) / 256, 1024);
        hipLaunchKernelGGL(trace_copy, dim3(std::max(blocks, 1)), dim3(256), 0, c.s, src, (int64_t)ld, B, tr->c0, tr->c1,
                           tr->out + (int64_t)slot * tr->step_stride, tr->ld_row);
        HIPCHK(hipGetLastError());
        return 0;
    };
    auto record = [&](int slot) -> int { return copy_window(s.tr, L.f_vp, L.V, slot); };
    const imdbn_chain_trace* const htr = s.htr;
    if (s.base()) {      // observe-only baseline step: p(v | p(h | v0)) at T = 1, no draws; vis_rm[0] keeps v0
        FinishArgs fh = new_finish();
        fh.op.rm = L.hid_rm; fh.op.rm_terms = c.rt; fh.rm_src = 1;
        CHK(prop(c, true, OpIn{L.vis_rm[0], c.rt, nullptr}, fh));
        FinishArgs fv = new_finish();
        fv.out_prob = L.f_vp; fv.ld_prob = L.V;
        CHK(prop(c, false, OpIn{L.hid_rm, c.rt, nullptr}, fv));
        CHK(record(0));
    }
    for (int t = 0; t < n_steps; ++t) {
        const imdbn_chain_step& s = st[t];
        const bool last = (t == n_steps - 1);
        {   // h | v
            FinishArgs f = new_finish();
            f.T = s.T; f.sigma = s.sigma;
            if (s.sigma > 0.f) f.noise = c.rng.floats(B, L.H);
            if (s.sample_h) { f.vmode = 1; f.uni = c.rng.floats(B, L.H); }
            f.op.rm = L.hid_rm; f.op.rm_terms = s.sample_h ? 1 : c.rt; f.rm_src = s.sample_h ? 2 : 1;
            if (htr) { f.out_prob = L.f_h; f.ld_prob = L.H; }      // the probability before sampling, as the chain kernel records it
            CHK(prop(c, true, OpIn{L.vis_rm[0], c.rt, nullptr}, f));
            CHK(copy_window(htr, L.f_h, L.H, t));
        }
        {   // v | h
            FinishArgs f = new_finish();
            f.T = s.T; f.sigma = s.sigma;
            if (s.sigma > 0.f) f.noise = c.rng.floats(B, L.V);
            if (mu && s.eta != 0.f) { f.mu = mu; f.ldmu = ldmu; f.Dz = Dz; f.eta = s.eta; }
            if (s.clamp) { f.clamp = 1; f.vk = vk; f.mask = mask; f.ldk = ldk; }
            f.vmode = s.vmode;
            if (s.vmode != 0) { f.uni = c.rng.floats(B, L.V); c.rng.cats(B, c.d->n_groups, &f.cat_tape, &f.cat_uni); }
            f.out_prob = L.f_vp; f.ld_prob = L.V;
            f.out_final = out; f.ld_final = ldo;
            f.op.rm = L.vis_rm[0]; f.op.rm_terms = c.rt; f.rm_src = 2;
            if (want_stats && last) {
                f.op.tr = L.vis_tr[0]; f.op.tr_terms = c.rt; f.tr_src = 2;
                f.colsum_part = L.cs_vpos; f.colsum_src = 2;
            }
            CHK(prop(c, false, OpIn{L.hid_rm, s.sample_h ? 1 : c.rt, nullptr}, f));
        }
        CHK(record(t + s_base));
    }
    return 0;
}

ChainSpec chain_spec(const imdbn_chain_spec* s, const imdbn_chain_trace* tr = nullptr, const imdbn_chain_trace* htr = nullptr) {
    ChainSpec r{s->v_known, s->mask, s->ldk, s->init_uniform, s->n_steps, s->steps, s->mu, s->ldmu, s->Dz, s->out_v, s->ldo};
    r.tr = tr; r.htr = htr;
    return r;
}
bool chain_spec_ok(const imdbn_rbm_desc* d, const imdbn_chain_spec* s) {
    return s->v_known && s->mask && s->out_v && s->ldk >= d->V && s->ldo >= d->V && s->n_steps >= 0 && (s->n_steps == 0 || s->steps) &&
           (!s->mu || (s->Dz > 0 && s->Dz <= d->V));
}
// two independent chains of one RBM: ONE launch of the chain kernel where it applies (chain a on the first half of the grid,
// chain b on the second), else one after the other; the draws are those of two single runs (a, then b) either way
int run_chain_pair(Ctx& c, const ChainSpec& sa, const ChainSpec& sb) {
    if (chain_kernel_ok(c, sa.n_recs()) && chain_kernel_ok(c, sb.n_recs()) && sa.n_recs() + sb.n_recs() <= CHAIN_MAX_STEPS && !tune().no_chain_pair) {
        CHK(chain_init(c, sa, false, false));
        CHK(chain_records(c, sa, 0));
        CHK(chain_init(c, sb, false, false));
        CHK(chain_records(c, sb, sa.n_recs()));
        CHK(launch_k4(c, sa, 0, &sb, sa.n_recs()));
        c.hid_bits_ok = false;
        return 0;
    }
    CHK(run_chain(c, sa, false));
    CHK(run_chain(c, sb, false));
    t_chain.recs = sa.n_recs();      // the record describes the launch(es) of the LAST chain run, the record count chain 0
    return 0;
}

hipStream_t S(imdbn_stream_t s) { return (hipStream_t)s; }

// the label kernel of imdbn_energy_trace (kernels_energy.hpp): Wy in LDS or global, base / h rows in LDS or global
template <bool WLDS, bool HLDS>
int launch_energy(const EnergyArgs& a, hipStream_t st) {
    const size_t lds = (WLDS ? sizeof(float) * (size_t)a.K * a.H : 0) + (HLDS ? sizeof(float) * 2 * ROW_WAVES * (size_t)a.H : 0);
    hipLaunchKernelGGL((energy_trace_rows<WLDS, HLDS>), dim3(cdiv(a.N, ROW_WAVES)), dim3(64 * ROW_WAVES), lds, st, a);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace

// =================================================================================================
extern "C" {

int imdbn_version(void) { return IMDBN_ABI_VERSION; }

int imdbn_last_error(char* buf, size_t n) {
    if (buf && n) { strncpy(buf, g_err, n - 1); buf[n - 1] = 0; }
    return (int)strlen(g_err);
}

int imdbn_device_info(int* cu_count, char* arch, size_t n) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(IMDBN_E_NODEVICE, "no HIP device");
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, dev));
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (arch && n) { strncpy(arch, p.gcnArchName, n - 1); arch[n - 1] = 0; }
    return 0;
}

size_t imdbn_ws_bytes(int V, int H, int B) {
    if (V <= 0 || H <= 0 || B <= 0) return 0;
    return make_layout(V, H, B, nullptr).bytes;
}

int imdbn_set_tuning(int ksplit_up, int ksplit_down) {
    g_defaults.ks_up = std::max(0, ksplit_up);
    g_defaults.ks_down = std::max(0, ksplit_down);
    return 0;
}

int imdbn_set_option(const char* name, int value) { return set_opt(g_defaults, name, value); }

struct imdbn_options { Tuning t; };
imdbn_options* imdbn_options_create(void) { return new (std::nothrow) imdbn_options{g_defaults}; }      // starts as a copy of the defaults
void imdbn_options_destroy(imdbn_options* o) { if (o && t_bound == &o->t) t_bound = nullptr; delete o; }
int imdbn_options_set(imdbn_options* o, const char* name, int value) {
    if (!o) return fail(IMDBN_E_INVALID, "null options handle");
    if (name && !strcmp(name, "dbg")) return fail(IMDBN_E_INVALID, "dbg is process-wide (imdbn_set_option)");
    return set_opt(o->t, name, value);
}
int imdbn_use_options(const imdbn_options* o) { t_bound = o ? &o->t : nullptr; return 0; }

int imdbn_profile_enable(int on) {
    if (on && g_prof.ev.empty()) {
        g_prof.ev.resize(2 * 4096);
        for (auto& e : g_prof.ev) HIPCHK(hipEventCreate(&e));
    }
    g_prof.on = on != 0;
    g_prof.used = 0;
    g_prof.calls = 0;
    return 0;
}

int imdbn_debug_stamps(long long* out, int n) {
    if (!out || n <= 0 || n > 4096 * 8) return fail(IMDBN_E_INVALID, "imdbn_debug_stamps: bad buffer");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(long long) * (size_t)n, 0, hipMemcpyDeviceToHost));
    static const std::vector<long long> zeros(4096 * 8, 0);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), zeros.data(), sizeof(long long) * zeros.size(), 0, hipMemcpyHostToDevice));
    return 0;
}

int imdbn_debug_ws_offset(int V, int H, int B, const char* name, size_t* offset) {
    if (V <= 0 || H <= 0 || B <= 0 || !name || !offset) return fail(IMDBN_E_INVALID, "debug_ws_offset: bad argument");
    char* fake = reinterpret_cast<char*>((uintptr_t)1 << 30);
    const Layout L = make_layout(V, H, B, fake);
    const void* p = nullptr;
    if (!strcmp(name, "vis_bits0")) p = L.vis_bits[0]; else if (!strcmp(name, "vis_bits1")) p = L.vis_bits[1];
    else if (!strcmp(name, "hid_bits")) p = L.hid_bits; else if (!strcmp(name, "vis_tr0")) p = L.vis_tr[0];
    else if (!strcmp(name, "vis_tr1")) p = L.vis_tr[1]; else if (!strcmp(name, "hid_tr0")) p = L.hid_tr[0];
    else if (!strcmp(name, "hid_tr1")) p = L.hid_tr[1]; else if (!strcmp(name, "cs_hpos")) p = L.cs_hpos;
    else if (!strcmp(name, "cs_hneg")) p = L.cs_hneg; else if (!strcmp(name, "cs_vpos")) p = L.cs_vpos;
    else if (!strcmp(name, "cs_vneg")) p = L.cs_vneg; else if (!strcmp(name, "flags")) p = L.flags;
    else if (!strcmp(name, "partial")) p = L.partial; else if (!strcmp(name, "vis_rm1")) p = L.vis_rm[1];
    else if (!strcmp(name, "pf_tr1")) p = L.pf_tr[0]; else if (!strcmp(name, "pf_tr2")) p = L.pf_tr[1];
    else if (!strcmp(name, "pf_bits1")) p = L.pf_bits[0]; else if (!strcmp(name, "pf_bits2")) p = L.pf_bits[1];
    else return fail(IMDBN_E_INVALID, "debug_ws_offset: unknown buffer %s", name);
    *offset = (size_t)((const char*)p - fake);
    return 0;
}

int imdbn_debug_last_route(int route[5]) {
    if (!route) return fail(IMDBN_E_INVALID, "imdbn_debug_last_route: null buffer");
    route[0] = t_route.up; route[1] = t_route.up_general; route[2] = t_route.down; route[3] = t_route.down_general; route[4] = t_route.down_groups;
    return 0;
}

int imdbn_debug_last_update(int rec[2]) {
    if (!rec) return fail(IMDBN_E_INVALID, "imdbn_debug_last_update: null buffer");
    rec[0] = t_update.kernel; rec[1] = t_update.tpb;
    return 0;
}

int imdbn_debug_last_cd(int rec[6]) {
    if (!rec) return fail(IMDBN_E_INVALID, "imdbn_debug_last_cd: null buffer");
    rec[0] = t_cd.pos_up; rec[1] = t_cd.first_down; rec[2] = t_cd.last_up; rec[3] = t_cd.next_on; rec[4] = t_cd.slot; rec[5] = t_cd.adaptive;
    return 0;
}

int imdbn_debug_last_chain(int rec[4]) {
    if (!rec) return fail(IMDBN_E_INVALID, "imdbn_debug_last_chain: null buffer");
    rec[0] = t_chain.route; rec[1] = t_chain.rows; rec[2] = t_chain.blocks; rec[3] = t_chain.recs;
    return 0;
}

int imdbn_profile_read(double* total_ms, int* launches) {
    double tot = 0.0;
    for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
        HIPCHK(hipEventSynchronize(g_prof.ev[i + 1]));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (int)(g_prof.used / 2);
    g_prof.used = 0;
    return 0;
}

// the device-resident draw counter of imdbn_rng.dev_offset: += n, as a node of the caller's stream (or captured graph)
__global__ void rng_advance_kernel(unsigned long long* p, unsigned long long n) { *p += n; }
int imdbn_rng_advance(uint64_t* dev_offset, uint64_t n, imdbn_stream_t stream) {
    if (!dev_offset) return fail(IMDBN_E_INVALID, "rng_advance: null counter");
    hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, S(stream), (unsigned long long*)dev_offset, (unsigned long long)n);
    HIPCHK(hipGetLastError());
    return 0;
}

int imdbn_rbm_prop_up(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int B, float T, imdbn_rng* rng,
                      float* out_prob, int64_t ldo, float* out_sample, int64_t lds, void* ws, size_t ws_bytes,
                      imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!v || !out_prob || ldv < d->V || ldo < d->H) return fail(IMDBN_E_INVALID, "prop_up: bad tensor argument");
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    FinishArgs f = new_finish();
    f.T = T;
    f.out_prob = out_prob; f.ld_prob = ldo;
    if (out_sample) {
        if (lds < d->H) return fail(IMDBN_E_INVALID, "prop_up: bad sample ld");
        f.vmode = 1; f.uni = c.rng.floats(B, d->H); f.out_final = out_sample; f.ld_final = lds;
    }
    CHK(prep_prop(c, true, v, ldv, f));
    return c.rng.finish();
}

// forward(v) at T = 1 on exactly the path the fused forward of imdbn_rbm_cd_step takes for the same batch (bit-identical):
// a 0/1 batch is read as a bit plane by k1_stream, anything else through the three-term operand form
int imdbn_rbm_forward(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int B, int data_binary, float* out_prob, int64_t ldo,
                      void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!v || !out_prob || ldv < d->V || ldo < d->H) return fail(IMDBN_E_INVALID, "forward: bad tensor argument");
    Ctx c(d, nullptr, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    if (data_binary < 0 || data_binary > 2) return fail(IMDBN_E_INVALID, "forward: data_binary %d", data_binary);
    CHK(prep(c, v, ldv, d->V, c.r.data_needs_rm(data_binary) ? c.L.vis_rm[0] : nullptr, c.L.Vpad, nullptr, c.L.flags, nullptr, 3,
             c.r.data_bits(data_binary) ? c.L.vis_bits[0] : nullptr));
    FinishArgs f = new_finish();
    f.out_prob = out_prob; f.ld_prob = ldo;
    CHK(prop(c, true, data_operand(c, data_binary), f));
    return 0;
}

int imdbn_rbm_free_energy(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int B, float* out_F, void* ws, size_t ws_bytes,
                          imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!v || !out_F || ldv < d->V) return fail(IMDBN_E_INVALID, "free_energy: bad tensor argument");
    Ctx c(d, nullptr, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    CHK(up_logits(c, v, ldv));                             // x = v W + c
    hipLaunchKernelGGL(free_energy_rows, dim3(B), dim3(256), 0, c.s, v, ldv, d->vis_bias, d->V, c.L.f_h, (int64_t)d->H, d->H, out_F);
    HIPCHK(hipGetLastError());
    return 0;
}

// Annealed importance sampling: M chains from the base-rate model (W = 0, visible biases b_A) to the RBM through the
// caller's temperatures.  Per temperature: the up propagation's raw logits, ais_weight_sample_h (weight increment, h, effective
// visible bias), and -- but for the last -- the down propagation at T = 1 / beta_k that samples the next visible state.
// State buffers are scratch that only the softmax-group kernels use otherwise: logits in f_h, the effective bias in f_vp, the
// fp32 state in f_v[0] (or the caller's out_v) -- imdbn_ws_bytes(V, H, M) covers the call.
// With softmax groups: the initial state adds one categorical per group, and the down propagation hands the group
// columns to finish_groups, which reads and writes fp32 copies of p(v | h) and of the state: the call names its own targets for
// them (f_v[1], and the state buffer) because prop()'s defaults are f_vp -- the effective bias here -- and f_v[1].
// Reverse AIS runs the same transitions backwards, T_K first, from the caller's start states.  The anneal_* pieces
// below are what the two calls share; they differ in their first kernel and their loop.

// the argument checks of either call, in their order; `v`: the start states of the call that takes them (has_v)
static int anneal_check(const char* name, const imdbn_rbm_desc* d, bool has_v, const float* v, int64_t ldv, int M, int K,
                        const float* betas, imdbn_rng* rng, double* logw, float* out_v, int64_t ldo) {
    if (M < 1) return fail(IMDBN_E_INVALID, has_v ? "%s: R = %d rows" : "%s: M = %d chains", name, M);
    if (K < 1) return fail(IMDBN_E_INVALID, "%s: K = %d temperatures", name, K);
    if ((has_v && !v) || !betas || !rng || !logw)
        return fail(IMDBN_E_INVALID, "%s: null %s", name, has_v && !v ? "v" : (!betas ? "betas" : (!rng ? "rng" : "logw")));
    if (has_v && ldv < d->V) return fail(IMDBN_E_INVALID, "%s: ldv %lld < V %d", name, (long long)ldv, d->V);
    if (out_v && ldo < d->V) return fail(IMDBN_E_INVALID, "%s: ldo %lld < V %d", name, (long long)ldo, d->V);
    if (betas[0] != 0.0f) return fail(IMDBN_E_INVALID, "%s: betas[0] = %g, must be 0", name, (double)betas[0]);
    if (betas[K] != 1.0f) return fail(IMDBN_E_INVALID, "%s: betas[%d] = %g, must be 1", name, K, (double)betas[K]);
    for (int k = 1; k <= K; ++k)
        if (!(betas[k] > betas[k - 1]))
            return fail(IMDBN_E_INVALID, "%s: betas[%d] = %g is not above betas[%d] = %g", name, k, (double)betas[k], k - 1, (double)betas[k - 1]);
    return 0;
}

struct Anneal {
    imdbn_rbm_desc dl;      // local copy: the down half reads the step's effective visible bias through it
    Ctx c;
    AisArgs a;              // what every kernel of the call is told
    GroupSpans sp;
    dim3 grid, block;
    Anneal(const imdbn_rbm_desc* d, imdbn_rng* rng, imdbn_stream_t stream) : dl(*d), c(&dl, rng, S(stream)) {}
    Anneal(const Anneal&) = delete;      // c.d points at dl
};

static int anneal_setup(Anneal& n, const imdbn_rbm_desc* d, int M, const float* base_vis_bias, double* logw, float* out_v, int64_t ldo,
                        void* ws, size_t ws_bytes) {
    CHK(setup(n.c, M, ws, ws_bytes));
    const Layout& L = n.c.L;
    if (base_vis_bias) n.dl.vis_bias = L.f_vp;
    AisArgs& a = n.a;
    memset(&a, 0, sizeof(a));
    a.M = M; a.Bp = L.Bp; a.V = L.V; a.H = L.H; a.Vpad = L.Vpad; a.Hpad = L.Hpad;
    a.vis_bias = d->vis_bias; a.base_bias = base_vis_bias; a.eff_bias = L.f_vp;
    a.state = out_v ? out_v : L.f_v[0]; a.lds = out_v ? ldo : L.V;
    a.x = L.f_h; a.ldx = L.H; a.logw = logw;
    memset(&n.sp, 0, sizeof(n.sp));
    n.sp.n_groups = d->n_groups;
    for (int g = 0; g < d->n_groups; ++g) { n.sp.gs[g] = d->group_start[g]; n.sp.ge[g] = d->group_end[g]; }
    n.grid = dim3(L.Bp / ROW_WAVES); n.block = dim3(64 * ROW_WAVES);
    return 0;
}

// x = c + v W of the current state; `real`: the state is real-valued fp32 rows of pitch V (imdbn_rbm_gauss_ais: u = v e^{-z}) that
// go through prep_operand first, the route of imdbn_rbm_gauss_free_energy
static int anneal_logits(Anneal& n, const float* real = nullptr) {
    const Layout& L = n.c.L;
    if (real) return up_logits(n.c, real, L.V);
    FinishArgs f = new_finish();
    f.logits_only = 1;
    f.out_prob = L.f_h; f.ld_prob = L.H;
    return prop(n.c, true, OpIn{L.vis_rm[0], 1, nullptr}, f);
}

// The weight step `w` (its k, form and direction are the caller's) on those logits; `sample`: it also draws h for the transition at
// w.beta_draw and writes that transition's effective visible bias.
static int anneal_weigh(Anneal& n, AisArgs w, bool sample) {
    const Layout& L = n.c.L;
    w.sample = sample ? 1 : 0;
    if (sample) {
        w.uni = n.c.rng.floats(w.M, L.H); w.rm = L.hid_rm; w.bits = L.hid_bits;
        w.eff_scale = (1.0f - w.beta_draw) / w.beta_draw;
    }
    hipLaunchKernelGGL(ais_weight_sample_h, n.grid, n.block, 0, n.c.s, w);
    HIPCHK(hipGetLastError());
    return 0;
}

// the next state from that h: v = 1[sigmoid(beta (b + h W^T) + (1 - beta) b_A) > U]; groups: one category each
static int anneal_down(Anneal& n, float beta) {
    Ctx& c = n.c;
    const Layout& L = c.L;
    c.hid_bits_ok = true;              // hid_bits describes hid_rm: the down half may read the bit plane
    FinishArgs f = new_finish();
    f.T = 1.0f / beta;
    f.vmode = 1; f.uni = c.rng.floats(n.a.M, L.V);
    if (n.sp.n_groups > 0) {
        c.rng.cats(n.a.M, n.sp.n_groups, &f.cat_tape, &f.cat_uni);
        f.out_prob = L.f_v[1]; f.ld_prob = L.V;
    }
    f.out_final = n.a.state; f.ld_final = n.a.lds;
    f.op.rm = L.vis_rm[0]; f.op.rm_terms = 1; f.rm_src = 2;
    return prop(c, false, OpIn{L.hid_rm, 1, nullptr}, f);
}

// (the body of imdbn_rbm_ais and imdbn_rbm_ais_groups, after the descriptor checks of either)
static int ais_run(const imdbn_rbm_desc* d, int M, int K, const float* betas, const float* base_vis_bias, imdbn_rng* rng, double* logw,
                   float* out_v, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(anneal_check("ais", d, false, nullptr, 0, M, K, betas, rng, logw, out_v, ldo));
    Anneal n(d, rng, stream);
    CHK(anneal_setup(n, d, M, base_vis_bias, logw, out_v, ldo, ws, ws_bytes));
    {   // v_1 from the base-rate model
        AisGroupsArgs gi;
        memset(&gi, 0, sizeof(gi));
        gi.a = n.a; gi.sp = n.sp;
        gi.a.uni = n.c.rng.floats(M, d->V); gi.a.rm = n.c.L.vis_rm[0];
        n.c.rng.cats(M, d->n_groups, &gi.cat_tape, &gi.cat_uni);
        hipLaunchKernelGGL(ais_init_v_groups, n.grid, n.block, 0, n.c.s, gi);
        HIPCHK(hipGetLastError());
    }
    for (int k = 1; k <= K; ++k) {
        CHK(anneal_logits(n));             // of v_k
        AisArgs w = n.a;
        w.beta_prev = betas[k - 1]; w.beta = w.beta_draw = betas[k];
        CHK(anneal_weigh(n, w, k < K));    // + Delta_k(v_k); the last temperature only weighs
        if (k < K) CHK(anneal_down(n, betas[k]));
    }
    return n.c.rng.finish();
}

int imdbn_rbm_ais(const imdbn_rbm_desc* d, int M, int K, const float* betas, const float* base_vis_bias, imdbn_rng* rng, double* logw,
                  float* out_v, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (d->n_groups > 0) return fail(IMDBN_E_UNSUPPORTED, "ais: softmax groups are not supported (n_groups = %d)", d->n_groups);
    return ais_run(d, M, K, betas, base_vis_bias, rng, logw, out_v, ldo, ws, ws_bytes, stream);
}

// imdbn_rbm_ais over Bernoulli visibles plus softmax groups; without groups it IS imdbn_rbm_ais, launch for launch.
int imdbn_rbm_ais_groups(const imdbn_rbm_desc* d, int M, int K, const float* betas, const float* base_vis_bias, imdbn_rng* rng,
                         double* logw, float* out_v, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    return ais_run(d, M, K, betas, base_vis_bias, rng, logw, out_v, ldo, ws, ws_bytes, stream);
}

// Reverse annealed importance sampling: R chains from the caller's start states, and logw collects
// -F(start) - sum_k Delta_k(u_k).  rais_load_v, then K + 1 weight steps, and between two of them the sampling down propagation at the
// temperature the weight kernel drew h for.
int imdbn_rbm_reverse_ais(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int R, int K, const float* betas, const float* base_vis_bias,
                          imdbn_rng* rng, double* logw, float* out_v, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    CHK(anneal_check("reverse_ais", d, true, v, ldv, R, K, betas, rng, logw, out_v, ldo));
    Anneal n(d, rng, stream);
    CHK(anneal_setup(n, d, R, base_vis_bias, logw, out_v, ldo, ws, ws_bytes));
    {   // u_{K+1} = the caller's rows
        RaisLoadArgs l;
        memset(&l, 0, sizeof(l));
        l.a = n.a; l.a.rm = n.c.L.vis_rm[0]; l.sp = n.sp;
        l.v = v; l.ldv = ldv;
        hipLaunchKernelGGL(rais_load_v, n.grid, n.block, 0, n.c.s, l);
        HIPCHK(hipGetLastError());
    }
    for (int k = K + 1; k >= 1; --k) {     // k = K + 1: the start state's softplus term; k <= K: -Delta_k(u_k)
        const bool first = k == K + 1;
        CHK(anneal_logits(n));             // of u_k
        AisArgs w = n.a;
        w.reverse = 1; w.first = first ? 1 : 0;
        if (!first) { w.beta_prev = betas[k - 1]; w.beta = betas[k]; }
        w.beta_draw = first ? betas[K] : betas[k - 1];      // temperature of the transition that follows
        CHK(anneal_weigh(n, w, k > 1));    // the last step (k = 1) only weighs
        if (k > 1) CHK(anneal_down(n, w.beta_draw));
    }
    return n.c.rng.finish();
}

int imdbn_rows_logmeanexp(const double* logw, int N, int M, double* out_lme, double* out_ess, imdbn_stream_t stream) {
    if (N < 1) return fail(IMDBN_E_INVALID, "rows_logmeanexp: N = %d rows", N);
    if (M < 1) return fail(IMDBN_E_INVALID, "rows_logmeanexp: M = %d chains", M);
    if (!logw || !out_lme || !out_ess)
        return fail(IMDBN_E_INVALID, "rows_logmeanexp: null %s", !logw ? "logw" : (!out_lme ? "out_lme" : "out_ess"));
    hipLaunchKernelGGL(rows_logmeanexp, dim3(cdiv(N, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, S(stream), logw, N, M, out_lme, out_ess);
    HIPCHK(hipGetLastError());
    return 0;
}

int imdbn_rbm_prop_down(const imdbn_rbm_desc* d, const float* h, int64_t ldh, int B, float T, int logits_only,
                        float* out_prob, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!h || !out_prob || ldh < d->H || ldo < d->V) return fail(IMDBN_E_INVALID, "prop_down: bad tensor argument");
    Ctx c(d, nullptr, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    FinishArgs f = new_finish();
    f.T = T; f.logits_only = logits_only;
    f.out_prob = out_prob; f.ld_prob = ldo;
    CHK(prep_prop(c, false, h, ldh, f));
    return 0;
}

int imdbn_rbm_sample_visible(const imdbn_rbm_desc* d, const float* v_prob, int64_t ldp, int B, imdbn_rng* rng,
                             float* out, int64_t ldo, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!v_prob || !out || ldp < d->V || ldo < d->V || B <= 0) return fail(IMDBN_E_INVALID, "sample_visible: bad argument");
    Rng r(rng);
    DrawSrc u = r.floats(B, d->V);
    const int32_t* ct; DrawSrc cu;
    r.cats(B, d->n_groups, &ct, &cu);
    CHK(r.finish());
    const int64_t total = (int64_t)B * d->V;
    hipLaunchKernelGGL(bernoulli_rows, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 2048)), dim3(256), 0, S(stream),
                       v_prob, ldp, B, d->V, u, out, ldo);
    HIPCHK(hipGetLastError());
    for (int g = 0; g < d->n_groups; ++g) {
        DrawSrc cg = cu; cg.draw += g;
        hipLaunchKernelGGL(categorical_rows, dim3(cdiv(B, 64)), dim3(64), 0, S(stream), v_prob, ldp, B,
                           d->group_start[g], d->group_end[g], ct ? ct + (int64_t)g * B : nullptr, cg, out, ldo);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

int imdbn_rbm_gibbs_step(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int B, int sample_h, int sample_v,
                         imdbn_rng* rng, float* v_next, float* v_prob, float* h, float* h_prob, void* ws,
                         size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!v || !v_next || !v_prob || !h || !h_prob || ldv < d->V) return fail(IMDBN_E_INVALID, "gibbs_step: bad argument");
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    const Layout& L = c.L;
    CHK(prep(c, v, ldv, d->V, L.vis_rm[0], L.Vpad, nullptr, L.flags));
    {
        FinishArgs f = new_finish();
        f.out_prob = h_prob; f.ld_prob = d->H; f.out_final = h; f.ld_final = d->H;
        if (sample_h) { f.vmode = 1; f.uni = c.rng.floats(B, d->H); }
        f.op.rm = L.hid_rm; f.op.rm_terms = sample_h ? 1 : c.rt; f.rm_src = 2;
        CHK(prop(c, true, OpIn{L.vis_rm[0], c.nw == 1 ? 1 : 0, L.flags}, f));
    }
    {
        FinishArgs f = new_finish();
        f.out_prob = v_prob; f.ld_prob = d->V; f.out_final = v_next; f.ld_final = d->V;
        if (sample_v) { f.vmode = 1; f.uni = c.rng.floats(B, d->V); c.rng.cats(B, d->n_groups, &f.cat_tape, &f.cat_uni); }
        CHK(prop(c, false, OpIn{L.hid_rm, sample_h ? 1 : c.rt, nullptr}, f));
    }
    return c.rng.finish();
}

// Start of a CD pass (imdbn_rbm_cd_step, imdbn_rbm_cd_factors_wire): the next batch's preparation (imdbn_cd_opts.next_*) and
// the prefetch slot the data sit in.  `pn` = the preparation, `rides` = cd_phases carries it on one of its launches.
static int cd_prologue(Ctx& c, const imdbn_cd_opts* o, PrepArgs& pn, bool& rides, bool allow_compact = true) {
    const imdbn_rbm_desc* d = c.d;
    if (o->data_slot < 0 || o->data_slot > 2 || (o->next_data && (o->next_slot < 1 || o->next_slot > 2 || o->next_slot == o->data_slot || o->ld_next < d->V)))
        return fail(IMDBN_E_INVALID, "cd: bad prefetch slots (data %d, next %d)", o->data_slot, o->next_slot);
    const bool has_next = o->next_data && c.r.prefetch;
    memset(&pn, 0, sizeof(pn));
    t_cd = CdRec{};
    if (has_next) {            // target buffers are taken before the data slot is swapped in
        const Layout& L = c.L;
        const int t = o->next_slot - 1;
        pn.in = o->next_data; pn.ld = o->ld_next; pn.B = L.B; pn.Bp = L.Bp; pn.N = L.V;
        const int terms = c.nw == 1 ? 1 : 3;      // (FAST: the one term every reader takes is the nearest bf16, as prep() writes it)
        pn.op.rm = L.pf_rm[t]; pn.op.ldrm = L.Vpad; pn.op.rm_ts = (int64_t)L.Bp * L.Vpad; pn.op.rm_terms = terms; pn.op.Bp = L.Bp;
        pn.op.tr = L.pf_tr[t]; pn.op.tr_ts = (int64_t)L.V * L.Bp; pn.op.tr_terms = terms;
        pn.flag = L.pf_flags[t]; pn.colsum_part = L.pf_cs[t];
        pn.op.bits = L.pf_bits[t]; pn.op.bits_shape = 0;
    }
    // Where the next batch is prepared: as extra blocks of the fused K2 (gemm_down_fused_next) or of the negative-phase
    // k1_stream (cd_phases decides); where neither can carry them, a prep_operand launch of its own, first thing.
    rides = has_next && c.r.rides;
    if (has_next && allow_compact && c.r.k1s) {
        if (o->next_binary == IMDBN_DATA_BINARY) {
            // a 0/1 batch: the positive phase reads the bit plane, the update kernel one bf16 plane (the exactness map says "one term")
            pn.op.rm = nullptr; pn.op.rm_terms = 0; pn.op.tr_terms = 1;
        } else if (o->next_binary == IMDBN_DATA_UNKNOWN && c.r.adaptive_next) {
            pn.adaptive = 1;      // the same slim set for every 64-column item that turns out to be all 0/1, decided by the preparing block
        }
    }
    if (has_next && !rides) {
        pn.zero = nullptr; pn.n_zero = 0;
        hipLaunchKernelGGL(prep_operand, dim3(cdiv(std::max(pn.N, pn.op.ldrm), 64), c.L.P), dim3(256), 0, c.s, pn);
        HIPCHK(hipGetLastError());
        t_cd.next_on = IMDBN_CD_NEXT_OWN_LAUNCH;
    }
    t_cd.slot = o->data_slot; t_cd.adaptive = pn.adaptive;
    if (o->data_slot) { use_slot(c.L, o->data_slot); c.data_prepped = true; c.cnt_ok = true; c.fix_slot = o->data_binary == IMDBN_DATA_UNKNOWN; }
    return 0;
}

// the CD pass of imdbn_rbm_cd_step / _cd_stats / _cd_factors_wire: next-batch preparation and prefetch slot, phases, draw cursor
static int cd_pass(Ctx& c, const float* data, int64_t ldd, const imdbn_cd_opts* o, bool allow_compact = true) {
    PrepArgs pn;
    bool rides = false;
    CHK(cd_prologue(c, o, pn, rides, allow_compact));
    CHK(cd_phases(c, data, ldd, o, rides ? &pn : nullptr));
    return c.rng.finish();
}

int imdbn_rbm_cd_step(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, const imdbn_cd_opts* o,
                      imdbn_rng* rng, float* loss_out, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, true));
    if (!data || !o || ldd < d->V) return fail(IMDBN_E_INVALID, "cd_step: bad argument");
    if (o->data_binary < 0 || o->data_binary > 2 || o->next_binary < 0 || o->next_binary > 2) return fail(IMDBN_E_INVALID, "cd_step: data_binary / next_binary outside 0..2");
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    CHK(cd_pass(c, data, ldd, o));
    const BiasArgs bias = make_bias(c, o, o->sparsity != 0, (float)B, loss_out);
    CHK(launch_assoc(c, 0, o, c.nw == 1 ? 1 : 0, c.L.flags, 1, (float)B, nullptr, &bias));
    if (o->fwd_out) {
        // forward(data) under the updated weights (idbn.py:195-204: train_epoch(v); v = forward(v)): the positive-phase
        // propagation once more -- same operand forms, still in the workspace -- with the probabilities as the only output
        if (o->ld_fwd < d->H) return fail(IMDBN_E_INVALID, "cd_step: ld_fwd %lld < H %d", (long long)o->ld_fwd, d->H);
        FinishArgs f = new_finish();
        f.out_prob = o->fwd_out; f.ld_prob = o->ld_fwd;
        CHK(prop(c, true, data_operand(c, o->data_binary), f));
    }
    return 0;
}

int imdbn_rbm_prefetch_ok(const imdbn_rbm_desc* d, int B) {
    if (check_desc(d, true) != 0 || B <= 0) return 0;
    return make_route(d, make_layout(d->V, d->H, B, nullptr)).prefetch ? 1 : 0;
}

size_t imdbn_packed_delta_floats(int V, int H) {
    const size_t n = (size_t)V * H + (size_t)2 * H + V + 1;
    return (n + 3) / 4 * 4;
}

int imdbn_rbm_cd_stats(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, const imdbn_cd_opts* o,
                       imdbn_rng* rng, float* packed, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!data || !o || !packed || ldd < d->V) return fail(IMDBN_E_INVALID, "cd_stats: bad argument");
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    CHK(cd_pass(c, data, ldd, o));
    const BiasArgs pack = make_pack(c, packed);
    CHK(launch_assoc(c, 1, o, c.nw == 1 ? 1 : 0, c.L.flags, 1, 1.0f, packed, &pack));
    return 0;
}

// ---- data-parallel "factor exchange" ----------------------------------------------------------
// The statistics are linear in the per-row factors, and the factors of 64 rows (7 MB at 10000 x 1500) are 8x
// smaller than the fp32 delta-W (60 MB): every rank all-gathers the factor blocks and runs the streaming update
// kernel once per rank block (first / middle / last pass) -- the same kernel, bits and order on every rank.
int imdbn_factor_block(int V, int H, int B, size_t* offset, size_t* bytes) {
    if (V <= 0 || H <= 0 || B <= 0 || !offset || !bytes) return fail(IMDBN_E_INVALID, "factor_block: bad argument");
    const Layout L = make_layout(V, H, B, nullptr);
    *offset = L.fb_off; *bytes = L.fb_bytes;
    return 0;
}

static bool factor_mode_ok(const imdbn_rbm_desc* d, int B, bool with_momentum) {
    return B >= 1 && B <= 64 && vec4_rows(d) &&
           (!with_momentum || (d->W_m && (((uintptr_t)d->W_m) & 15) == 0)) && d->n_groups == 0;
}

// offsets of the wire form (kernels_ew.hpp FactorWireArgs) for an (V, H, B) factor block
static FactorWireArgs wire_layout(int V, int H, int B, int binary, size_t* compact_bytes) {
    char* fake = reinterpret_cast<char*>((uintptr_t)1 << 30);          // only differences of the carved pointers are used
    const Layout L = make_layout(V, H, B, fake);
    const char* fb = fake + L.fb_off;
    FactorWireArgs w;
    memset(&w, 0, sizeof(w));
    w.V = V; w.Bp = L.Bp; w.binary = binary ? 1 : 0;
    w.f_vpos = (size_t)((const char*)L.vis_tr[0] - fb);
    w.f_vneg = (size_t)((const char*)L.vis_tr[1] - fb);
    w.f_cs_hpos = (size_t)((const char*)L.cs_hpos - fb);
    // (exact sizes, both multiples of 16: the alignment padding behind them is copied from the block itself either way)
    w.f_flags = (size_t)((const char*)L.flags - fb); w.n_flags = (size_t)L.P * cdiv(L.Vpad, 64) * 4;
    w.f_cs_vpos = (size_t)((const char*)L.cs_vpos - fb); w.n_cs_vpos = (size_t)L.P * V * 4;
    w.head_bytes = w.f_vpos;                                            // flags .. loss_part precede the visible planes
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t bits = up((size_t)V * L.Bp / 8);
    w.c_vneg = w.head_bytes;
    w.c_vpos = w.c_vneg + bits;
    w.c_bad = w.c_vpos + (binary ? bits : up((size_t)3 * V * L.Bp * 2));
    if (compact_bytes) *compact_bytes = w.c_bad + 256;
    return w;
}

int imdbn_factor_compact_bytes(int V, int H, int B, int binary_data, size_t* bytes) {
    if (V <= 0 || H <= 0 || B <= 0 || !bytes) return fail(IMDBN_E_INVALID, "factor_compact_bytes: bad argument");
    (void)wire_layout(V, H, B, binary_data, bytes);
    return 0;
}

// any value >= 1 that changes from call to call (a stale `bad` mark must not match; the caller zero-initialises a fresh compact buffer)
static int next_pack_epoch() {
    static std::atomic<int> epoch{0};
    return epoch.fetch_add(1) % 1000000 + 1;
}

int imdbn_rbm_pack_factors(int V, int H, int B, int binary_data, const void* block, void* compact, imdbn_stream_t stream) {
    if (V <= 0 || H <= 0 || B <= 0 || !block || !compact || (((uintptr_t)block | (uintptr_t)compact) & 15))
        return fail(IMDBN_E_INVALID, "pack_factors: bad argument (blocks must be 16-B aligned)");
    FactorWireArgs w = wire_layout(V, H, B, binary_data, nullptr);
    w.src = (const char*)block; w.dst = (char*)compact; w.n_ranks = 1;
    w.epoch = next_pack_epoch();
    hipLaunchKernelGGL(factor_pack, dim3(std::min(1024, cdiv((int)(w.head_bytes / 16), 256))), dim3(256), 0, S(stream), w);
    HIPCHK(hipGetLastError());
    return 0;
}

int imdbn_rbm_unpack_factors(int V, int H, int B, int binary_data, const void* compact, size_t compact_stride, int n_ranks,
                             void* gathered, size_t full_stride, int planes_only, imdbn_stream_t stream) {
    if (V <= 0 || H <= 0 || B <= 0 || !compact || !gathered || n_ranks < 1 || (((uintptr_t)compact | (uintptr_t)gathered | compact_stride | full_stride) & 15))
        return fail(IMDBN_E_INVALID, "unpack_factors: bad argument (blocks and strides must be 16-B aligned)");
    size_t cb = 0;
    FactorWireArgs w = wire_layout(V, H, B, binary_data, &cb);
    size_t off = 0, fbytes = 0;
    CHK(imdbn_factor_block(V, H, B, &off, &fbytes));
    if (compact_stride < cb || full_stride < fbytes) return fail(IMDBN_E_INVALID, "unpack_factors: strides smaller than the blocks");
    w.src = (const char*)compact; w.dst = (char*)gathered; w.src_stride = compact_stride; w.dst_stride = full_stride; w.n_ranks = n_ranks;
    w.planes_only = planes_only ? 1 : 0;
    hipLaunchKernelGGL(factor_unpack, dim3(std::min(512, cdiv((int)((planes_only ? (size_t)V * w.Bp / 8 * 16 : w.head_bytes) / 16), 256)), n_ranks), dim3(256), 0, S(stream), w);
    HIPCHK(hipGetLastError());
    return 0;
}

int imdbn_rbm_cd_factors(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, const imdbn_cd_opts* o,
                         imdbn_rng* rng, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!data || !o || ldd < d->V) return fail(IMDBN_E_INVALID, "cd_factors: bad argument");
    if (!factor_mode_ok(d, B, false)) return fail(IMDBN_E_UNSUPPORTED, "cd_factors: needs <= 64 rows per rank, 16-B aligned weight rows, no softmax groups");
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    t_cd = CdRec{};      // no prologue: nothing prepared, no slot
    CHK(cd_phases(c, data, ldd, o));
    return c.rng.finish();
}

// The CD pass of this rank's rows straight into the wire form (cd_factors + pack_factors as one call), with the next-batch
// preparation of imdbn_rbm_cd_step (imdbn_cd_opts.next_* / data_slot): the data-side factors then sit in a prefetch slot and
// the pack kernel reads them from there.
int imdbn_rbm_cd_factors_wire(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, const imdbn_cd_opts* o, imdbn_rng* rng,
                              int binary_data, void* wire, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!data || !o || !wire || ldd < d->V || (((uintptr_t)wire) & 15)) return fail(IMDBN_E_INVALID, "cd_factors_wire: bad argument");
    if (!factor_mode_ok(d, B, false)) return fail(IMDBN_E_UNSUPPORTED, "cd_factors_wire: needs <= 64 rows per rank, 16-B aligned weight rows, no softmax groups");
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    // (a wire form that carries the data as three bf16 planes needs all three written: no compact slot form then)
    CHK(cd_pass(c, data, ldd, o, binary_data != 0));
    FactorWireArgs w = wire_layout(d->V, d->H, B, binary_data, nullptr);
    w.src = (const char*)ws + c.L.fb_off; w.dst = (char*)wire; w.n_ranks = 1;
    if (o->data_slot) { w.alt_flags = (const char*)c.L.flags; w.alt_cs_vpos = (const char*)c.L.cs_vpos; w.alt_vpos = (const char*)c.L.vis_tr[0]; }
    w.epoch = next_pack_epoch();
    hipLaunchKernelGGL(factor_pack, dim3(std::min(1024, cdiv((int)(w.head_bytes / 16), 256))), dim3(256), 0, c.s, w);
    HIPCHK(hipGetLastError());
    return 0;
}

// The update from n_ranks factor blocks.  `head` / `planes`: where the blocks' head (exactness map, hidden planes, column-sum
// and error partials) and visible planes are read -- the same buffer and stride for full gathered blocks, or the gathered
// WIRE blocks (whose head is verbatim) plus the buffer imdbn_rbm_unpack_factors(planes_only) expanded the planes into.
static int apply_factors_impl(const imdbn_rbm_desc* d, const void* head, size_t head_stride, const void* planes, size_t planes_stride,
                              int n_ranks, int rows_per_rank, int global_B, const imdbn_cd_opts* o, float* loss_out, imdbn_stream_t stream) {
    CHK(check_desc(d, true));
    if (!head || !planes || !o || n_ranks < 1 || global_B <= 0) return fail(IMDBN_E_INVALID, "apply_factors: bad argument");
    if (!factor_mode_ok(d, rows_per_rank, true)) return fail(IMDBN_E_UNSUPPORTED, "apply_factors: needs <= 64 rows per rank, 16-B aligned weight rows, no softmax groups");
    Ctx c(d, nullptr, S(stream));
    char* fake = reinterpret_cast<char*>((uintptr_t)1 << 30);                   // only offsets inside the factor block are used
    c.L = make_layout(d->V, d->H, rows_per_rank, fake);
    c.r = make_route(d, c.L);
    const Layout& L = c.L;
    const char* fb = fake + L.fb_off;
    if (((head_stride | planes_stride) & 255) || ((((uintptr_t)head) | ((uintptr_t)planes)) & 255) || planes_stride < L.fb_bytes ||
        head_stride < (size_t)((const char*)L.vis_tr[0] - fb))
        return fail(IMDBN_E_INVALID, "apply_factors: the gathered blocks must be 256-B aligned and at least %zu bytes apart", L.fb_bytes);
    auto at_h = [&](const void* layout_ptr, int rk) { return (const char*)head + ((const char*)layout_ptr - fb) + (size_t)rk * head_stride; };
    auto at_v = [&](const void* layout_ptr, int rk) { return (const char*)planes + ((const char*)layout_ptr - fb) + (size_t)rk * planes_stride; };
    AssocPlanesArgs f;
    memset(&f, 0, sizeof(f));
    f.W = d->W; f.Wm = d->W_m; f.ldw = d->ldw; f.V = L.V; f.H = L.H;
    f.vpos_terms = c.nw == 1 ? 1 : 0; f.vneg_terms = 1;
    f.vts = (int64_t)L.V * L.Bp; f.hts = (int64_t)L.H * L.Bp; f.Bp = L.Bp;
    f.lr = o->lr; f.mom = o->momentum; f.wd = o->weight_decay; f.n = (float)global_B;
    BiasArgs b = make_bias(c, o, o->sparsity != 0, (float)global_B, loss_out);      // ... reading rank 0's block, R blocks `rs` floats apart
    b.hpos = (const float*)at_h(L.cs_hpos, 0); b.hneg = (const float*)at_h(L.cs_hneg, 0);
    b.vpos = (const float*)at_h(L.cs_vpos, 0); b.vneg = (const float*)at_h(L.cs_vneg, 0);
    b.loss_part = (const float*)at_h(L.loss_part, 0);
    b.R = n_ranks; b.rs = (int64_t)(head_stride / 4);
    BiasArgs bz;
    memset(&bz, 0, sizeof(bz));
    const int tpb = c.r.tpb, brows = k3_bias_rows(L);
    ProfBracket prof;      // (bench.py roofline at N > 1)
    CHK(prof.begin(c.s, true));
    // all rank blocks inside one launch (the weights move once) when the visible operands need <= 4 plane slices
    if (n_ranks >= tune().min_rank_loop && !tune().no_rank_loop && f.vneg_terms == 1) {
        f.vpos = (const bf16_t*)at_v(L.vis_tr[0], 0); f.vpos_flag = (const int*)at_h(L.flags, 0);
        f.hpos = (const bf16_t*)at_h(L.hid_tr[0], 0);
        f.vneg = (const bf16_t*)at_v(L.vis_tr[1], 0); f.hneg = (const bf16_t*)at_h(L.hid_tr[1], 0);
        RankLoopArgs rl{n_ranks, (int64_t)(head_stride / 2), (int64_t)(planes_stride / 2)};
        const bool acc = tpb <= 4 && !tune().no_rank_acc;       // rank loop outside the tile loop: hidden planes staged once per rank
        const auto k = c.ht == 3 ? (acc ? assoc_update_planes_ranks<3, true> : assoc_update_planes_ranks<3, false>)
                                 : (acc ? assoc_update_planes_ranks<1, true> : assoc_update_planes_ranks<1, false>);
        hipLaunchKernelGGL(k, k3_grid(c, brows), dim3(256), 0, c.s, f, rl, tpb, b, brows);
        HIPCHK(hipGetLastError());
        ran_update(IMDBN_UPDATE_RANKS, tpb);
        return prof.end(c.s);
    }
    for (int rk = 0; rk < n_ranks; ++rk) {
        f.vpos = (const bf16_t*)at_v(L.vis_tr[0], rk); f.vpos_flag = (const int*)at_h(L.flags, rk);
        f.hpos = (const bf16_t*)at_h(L.hid_tr[0], rk);
        f.vneg = (const bf16_t*)at_v(L.vis_tr[1], rk); f.hneg = (const bf16_t*)at_h(L.hid_tr[1], rk);
        const int br = (rk == n_ranks - 1) ? brows : 0;
        CHK(launch_k3_planes(c, 0, f, k3_pass(rk, n_ranks), br ? b : bz, br));
    }
    return prof.end(c.s);
}

int imdbn_rbm_apply_factors(const imdbn_rbm_desc* d, const void* gathered, int n_ranks, size_t rank_stride, int rows_per_rank,
                            int global_B, const imdbn_cd_opts* o, float* loss_out, imdbn_stream_t stream) {
    return apply_factors_impl(d, gathered, rank_stride, gathered, rank_stride, n_ranks, rows_per_rank, global_B, o, loss_out, stream);
}

int imdbn_rbm_apply_factors_wire(const imdbn_rbm_desc* d, const void* wire, size_t wire_stride, const void* planes, size_t planes_stride,
                                 int n_ranks, int rows_per_rank, int global_B, const imdbn_cd_opts* o, float* loss_out, imdbn_stream_t stream) {
    return apply_factors_impl(d, wire, wire_stride, planes, planes_stride, n_ranks, rows_per_rank, global_B, o, loss_out, stream);
}

// unpack(planes_only) + apply_factors_wire as one call: `planes` = scratch of n_ranks x planes_stride bytes (>= the full block size)
int imdbn_rbm_apply_wire(const imdbn_rbm_desc* d, const void* wire, size_t wire_stride, int n_ranks, int rows_per_rank, int global_B,
                         int binary_data, void* planes, size_t planes_stride, const imdbn_cd_opts* o, float* loss_out, imdbn_stream_t stream) {
    CHK(check_desc(d, true));
    CHK(imdbn_rbm_unpack_factors(d->V, d->H, rows_per_rank, binary_data, wire, wire_stride, n_ranks, planes, planes_stride, 1, stream));
    return apply_factors_impl(d, wire, wire_stride, planes, planes_stride, n_ranks, rows_per_rank, global_B, o, loss_out, stream);
}

int imdbn_rbm_apply_delta(const imdbn_rbm_desc* d, const float* packed, int global_B, const imdbn_cd_opts* o,
                          float* loss_out, imdbn_stream_t stream) {
    CHK(check_desc(d, true));
    if (!packed || !o || global_B <= 0) return fail(IMDBN_E_INVALID, "apply_delta: bad argument");
    ApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.W = d->W; a.Wm = d->W_m; a.ldw = d->ldw; a.V = d->V; a.H = d->H; a.packed = packed;
    a.hid_bias = d->hid_bias; a.hb_m = d->hb_m; a.vis_bias = d->vis_bias; a.vb_m = d->vb_m;
    a.lr = o->lr; a.mom = o->momentum; a.wd = o->weight_decay; a.n = (float)global_B;
    a.sparsity = o->sparsity; a.target = o->sparsity_target; a.loss_out = loss_out;
    const int64_t total = (int64_t)d->V * d->H;
    const bool vec4 = vec4_rows(d) && ((((uintptr_t)d->W_m) | ((uintptr_t)packed)) & 15) == 0;
    const int64_t items = vec4 ? total / 4 : total;
    const int grid = (int)std::max<int64_t>(std::min<int64_t>((items + 255) / 256, 8192), cdiv(std::max(d->V, d->H), 256));
    if (vec4) hipLaunchKernelGGL(apply_delta<true>, dim3(grid), dim3(256), 0, S(stream), a);
    else      hipLaunchKernelGGL(apply_delta<false>, dim3(grid), dim3(256), 0, S(stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}

int imdbn_rbm_chain(const imdbn_rbm_desc* d, const float* v_known, const float* mask, int64_t ldk, int B,
                    int init_uniform, int n_steps, const imdbn_chain_step* steps, const float* mu, int64_t ldmu, int Dz,
                    imdbn_rng* rng, float* out_v, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!v_known || !mask || !out_v || ldk < d->V || ldo < d->V) return fail(IMDBN_E_INVALID, "chain: bad argument");
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    CHK(run_chain(c, ChainSpec{v_known, mask, ldk, init_uniform, n_steps, steps, mu, ldmu, Dz, out_v, ldo}, false));
    return c.rng.finish();
}

// Two independent chains of the same RBM and batch size in one call (imdbn.py:419-449: the IMG->TXT and TXT->IMG chains of
// _cross_reconstruct share nothing but the read-only weights).  Draws are assigned in the order of two imdbn_rbm_chain calls (a, then b),
// so the results are those of the two calls, bit for bit; where the row-parallel chain kernel applies both run in ONE launch
// (chain a on the first half of the grid, chain b on the second).
int imdbn_rbm_chain_pair(const imdbn_rbm_desc* d, int B, const imdbn_chain_spec* a, const imdbn_chain_spec* b, imdbn_rng* rng,
                         void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!a || !b) return fail(IMDBN_E_INVALID, "chain_pair: null chain");
    if (!chain_spec_ok(d, a) || !chain_spec_ok(d, b)) return fail(IMDBN_E_INVALID, "chain_pair: bad argument");
    if (a->out_v == b->out_v) return fail(IMDBN_E_INVALID, "chain_pair: the two chains need separate output buffers");
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    CHK(run_chain_pair(c, chain_spec(a), chain_spec(b)));
    return c.rng.finish();
}

// imdbn_rbm_chain / imdbn_rbm_chain_pair with the visible probabilities of a column window recorded at every step (the convergence
// traces of imdbn/utils/conditional_steps.py).  Recording only observes: same draws, same final state as the untraced calls.
static int check_trace(const imdbn_rbm_desc* d, const imdbn_chain_trace* t, bool hidden = false) {
    if (!t) return 0;
    const int width = hidden ? d->H : d->V;
    if (!t->out || t->c0 < 0 || t->c1 <= t->c0 || t->c1 > width || t->ld_row < t->c1 - t->c0 || t->step_stride < 0 ||
        (t->with_baseline != 0 && t->with_baseline != 1))
        return fail(IMDBN_E_INVALID, "chain_traced: bad %s trace [%d, %d) ld %lld", hidden ? "hidden" : "visible", t->c0, t->c1, (long long)t->ld_row);
    if (hidden && t->with_baseline) return fail(IMDBN_E_INVALID, "chain_traced: a hidden trace has no baseline slot");
    return 0;
}

int imdbn_rbm_chain_traced(const imdbn_rbm_desc* d, int B, const imdbn_chain_spec* a, const imdbn_chain_trace* ta,
                           const imdbn_chain_spec* b, const imdbn_chain_trace* tb, imdbn_rng* rng, void* ws, size_t ws_bytes,
                           imdbn_stream_t stream) {
    return imdbn_rbm_chain_traced_vh(d, B, a, ta, nullptr, b, tb, nullptr, rng, ws, ws_bytes, stream);
}

// ... and with the hidden probabilities p(h|v) of a hidden column window recorded too (the joint-hidden trajectories of
// imdbn/utils/bimodal_logging.py): slot t = what step t is about to sample, with that step's T and noise.
int imdbn_rbm_chain_traced_vh(const imdbn_rbm_desc* d, int B, const imdbn_chain_spec* a, const imdbn_chain_trace* va,
                              const imdbn_chain_trace* ha, const imdbn_chain_spec* b, const imdbn_chain_trace* vb,
                              const imdbn_chain_trace* hb, imdbn_rng* rng, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!a || ((vb || hb) && !b)) return fail(IMDBN_E_INVALID, "chain_traced: null chain");
    if (!chain_spec_ok(d, a) || (b && !chain_spec_ok(d, b))) return fail(IMDBN_E_INVALID, "chain_traced: bad argument");
    if (b && a->out_v == b->out_v) return fail(IMDBN_E_INVALID, "chain_traced: the two chains need separate output buffers");
    CHK(check_trace(d, va));
    CHK(check_trace(d, vb));
    CHK(check_trace(d, ha, true));
    CHK(check_trace(d, hb, true));
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    if (b) CHK(run_chain_pair(c, chain_spec(a, va, ha), chain_spec(b, vb, hb)));
    else CHK(run_chain(c, chain_spec(a, va, ha), false));
    return c.rng.finish();
}

int imdbn_trace_label_scan(const float* trace, int64_t step_stride, int64_t ld_row, int T, int B, int K, const int32_t* gt,
                           double eps_l1, int stable_steps, double gap_thresh, float* p_top1, float* p_top2, int32_t* k1, int32_t* k2,
                           float* p_gt, float* l1, int32_t* steps, int32_t* pred, imdbn_stream_t stream) {
    if (!trace || T < 1 || B < 1 || K < 2 || K > LABEL_KMAX || ld_row < K || step_stride < (int64_t)B * ld_row || !p_top1 || !p_top2 ||
        !k1 || !k2 || !l1 || !steps || !pred || (gt && !p_gt))
        return fail(IMDBN_E_INVALID, "trace_label_scan: bad argument (T=%d B=%d K=%d)", T, B, K);
    hipLaunchKernelGGL(trace_label_scan, dim3(cdiv(B, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, S(stream), trace, step_stride, ld_row, T, B, K, gt, eps_l1,
                       stable_steps, gap_thresh, p_top1, p_top2, k1, k2, gt ? p_gt : nullptr, l1, steps, pred);
    HIPCHK(hipGetLastError());
    return 0;
}

int imdbn_trace_code_scan(const float* trace, int64_t step_stride, int64_t ld_row, int T, int B, int Dz, const float* z_init,
                          int64_t ld_init, float ema_beta, float* z_new, float* dz, imdbn_stream_t stream) {
    if (!trace || !z_init || !z_new || !dz || T < 1 || B < 1 || Dz < 1 || ld_row < Dz || ld_init < Dz || step_stride < (int64_t)B * ld_row)
        return fail(IMDBN_E_INVALID, "trace_code_scan: bad argument (T=%d B=%d Dz=%d)", T, B, Dz);
    hipLaunchKernelGGL(trace_code_scan, dim3(cdiv(B, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, S(stream), trace, step_stride, ld_row, T, B, Dz, z_init, ld_init,
                       ema_beta, z_new, dz);
    HIPCHK(hipGetLastError());
    return 0;
}

int imdbn_trace_patience_scan(const float* dz, const float* mse, int T, int B, double eps_z, double mse_tol, int patience,
                              int32_t* steps, float* best_mse, imdbn_stream_t stream) {
    if (!dz || !mse || !steps || !best_mse || T < 1 || B < 1)
        return fail(IMDBN_E_INVALID, "trace_patience_scan: bad argument (T=%d B=%d)", T, B);
    hipLaunchKernelGGL(trace_patience_scan, dim3(cdiv(B, 64)), dim3(64), 0, S(stream), dz, mse, T, B, eps_z, mse_tol, patience, steps, best_mse);
    HIPCHK(hipGetLastError());
    return 0;
}

int imdbn_rbm_prop_down_sqerr(const imdbn_rbm_desc* d, const float* h, int64_t ldh, int B, const float* ref, int64_t ldr,
                              const int32_t* ref_row, float* out_mse, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!h || !ref || !out_mse || ldh < d->H || ldr < d->V || B < 1) return fail(IMDBN_E_INVALID, "prop_down_sqerr: bad tensor argument");
    if (d->n_groups != 0) return fail(IMDBN_E_UNSUPPORTED, "prop_down_sqerr: softmax groups");
    Ctx c(d, nullptr, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    // imdbn_rbm_prop_down at T = 1 into the workspace's [Bp][V] fp32 buffer, then the per-row error in a fixed order
    FinishArgs f = new_finish();
    f.out_prob = c.L.f_vp; f.ld_prob = d->V;
    CHK(prep_prop(c, false, h, ldh, f));
    hipLaunchKernelGGL(row_sqerr, dim3(B), dim3(256), 0, S(stream), c.L.f_vp, (int64_t)d->V, B, d->V, ref, ldr, ref_row, out_mse);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- latent nearest-neighbour search (imdbn/utils/imdbn_logging.py; kernels_knn.hpp) ----------------------------------------
int imdbn_row_stats(const float* x, int64_t ldx, int N, int D, float* out_sum, float* out_sumsq, imdbn_stream_t stream) {
    if (!x || N < 1 || D < 1 || ldx < D || (!out_sum && !out_sumsq)) return fail(IMDBN_E_INVALID, "row_stats: bad argument (N=%d D=%d)", N, D);
    hipLaunchKernelGGL(knn_row_stats, dim3(cdiv(N, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, S(stream), x, ldx, N, D, out_sum, out_sumsq);
    HIPCHK(hipGetLastError());
    return 0;
}

static size_t knn_align(size_t b) { return (b + 255) & ~(size_t)255; }

int imdbn_latent_topk(const float* bank, int64_t ldb, int N, int D, const float* bank_sumsq, const float* queries, int64_t ldq, int Q,
                      int metric, int k, const int32_t* exclude, const float* key, int32_t* out_idx, float* out_score, void* ws,
                      size_t ws_bytes, imdbn_stream_t stream) {
    if (k < 1 || k > KNN_KMAX) return fail(IMDBN_E_INVALID, "latent_topk: k = %d outside [1, %d]", k, KNN_KMAX);
    if (!bank || !queries || !out_idx || !out_score || N < 1 || D < 1 || Q < 1 || ldb < D || ldq < D || metric < 0 || metric > 2)
        return fail(IMDBN_E_INVALID, "latent_topk: bad argument (N=%d D=%d Q=%d metric=%d)", N, D, Q, metric);
    // workspace: ||q||^2 [Q], ||b||^2 [N] (when not given), then the chunk lists (scores, indices) [chunks][Q][k]
    const bool norms = metric != 1, own_bss = norms && !bank_sumsq;
    const size_t head = knn_align(sizeof(float) * (size_t)Q) + (own_bss ? knn_align(sizeof(float) * (size_t)N) : 0);
    const size_t per_chunk = 2 * knn_align(sizeof(float) * (size_t)Q * k);
    if (!ws || ws_bytes < head + per_chunk)
        return fail(IMDBN_E_WORKSPACE, "latent_topk: workspace %zu < %zu bytes", ws_bytes, head + per_chunk);
    // about 2048 blocks over (query tiles x bank chunks), as many chunks as the workspace holds
    const int qtiles = cdiv(Q, KNN_QT), max_chunks = cdiv(N, KNN_BT);
    int chunks = std::min(std::max(1, cdiv(2048, qtiles)), max_chunks);
    chunks = (int)std::min<size_t>((size_t)chunks, (ws_bytes - head) / per_chunk);
    const int chunk = rup(cdiv(N, chunks), KNN_BT);
    chunks = cdiv(N, chunk);
    char* p = (char*)ws;
    float* qss = (float*)p; p += knn_align(sizeof(float) * (size_t)Q);
    const float* bss = bank_sumsq;
    if (own_bss) { bss = (const float*)p; p += knn_align(sizeof(float) * (size_t)N); }
    float* part_s = (float*)p;
    int32_t* part_i = (int32_t*)(p + knn_align(sizeof(float) * (size_t)Q * k) * chunks);
    const hipStream_t st = S(stream);
    if (norms) {
        hipLaunchKernelGGL(knn_row_stats, dim3(cdiv(Q, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, st, queries, ldq, Q, D, nullptr, qss);
        HIPCHK(hipGetLastError());
        if (own_bss) {
            hipLaunchKernelGGL(knn_row_stats, dim3(cdiv(N, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, st, bank, ldb, N, D, nullptr, (float*)bss);
            HIPCHK(hipGetLastError());
        }
    }
    CHK(kernel_attrs_ready());
    KnnArgs a;
    a.bank = bank; a.ldb = ldb; a.N = N; a.D = D; a.bss = bss;
    a.q = queries; a.ldq = ldq; a.Q = Q; a.qss = qss;
    a.metric = metric; a.k = k; a.chunk = chunk; a.exclude = exclude; a.key = key;
    a.part_s = part_s; a.part_i = part_i;
    hipLaunchKernelGGL(knn_topk_chunk, dim3(qtiles, chunks), dim3(256), knn_chunk_lds(k), st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(knn_topk_merge, dim3(qtiles), dim3(KNN_QT), knn_merge_lds(k), st, part_s, part_i, chunks, Q, k, key, out_idx,
                       out_score);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- IMG->TXT energy trace (imdbn/utils/energy_utils.py; kernels_energy.hpp) ------------------------------------------------
int imdbn_energy_trace(const imdbn_rbm_desc* d, const float* z, int64_t ldz, int N, int Dz, int K, int steps, const int32_t* gt,
                       const float* y_start, int64_t ldy, double eps_l1, int stable_steps, double gap_thresh,
                       const imdbn_energy_out* out, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    CHK(LabelSide::check("energy_trace", d, Dz, K));
    if (steps < 1 || N < 1) return fail(IMDBN_E_INVALID, "energy_trace: steps = %d, N = %d (both must be >= 1)", steps, N);
    if (!z || ldz < Dz || (y_start && ldy < K)) return fail(IMDBN_E_INVALID, "energy_trace: bad tensor argument (ldz=%lld ldy=%lld)", (long long)ldz, (long long)ldy);
    if (!out || !out->p_top1 || !out->p_top2 || !out->deltaF_pred || !out->l1 || !out->k1 || !out->steps_to_converge || !out->kstar ||
        !out->predT || !out->margin_energy || !out->fe_top1 || !out->fe_gap || !out->F || (gt && !out->p_gt))
        return fail(IMDBN_E_INVALID, "energy_trace: null output");
    // phase A: base = z W[:Dz] + c
    LabelSide s(d, Dz, S(stream));
    CHK(s.propagate(z, ldz, N, ws, ws_bytes));
    const Ctx& c = s.c;
    // phase B: everything else, one wave per row
    EnergyArgs a{};
    a.base = s.base; a.ldb = d->H;
    a.z = z; a.ldz = ldz;
    a.bz = s.bz; a.by = s.by;
    a.Wy = s.Wy; a.ldw = d->ldw;
    a.N = N; a.Dz = Dz; a.K = K; a.H = d->H; a.steps = steps;
    a.gt = gt; a.y0 = y_start; a.ldy0 = ldy;
    a.eps_l1 = eps_l1; a.stable_steps = stable_steps; a.gap_thresh = gap_thresh;
    a.hscr = (float*)c.L.hid_tr[0];             // 6 H Bp bytes, untouched by a logits-only K1: room for [N][H] floats
    a.p1 = out->p_top1; a.p2 = out->p_top2; a.pgt = gt ? out->p_gt : nullptr; a.dF = out->deltaF_pred; a.l1 = out->l1; a.k1 = out->k1;
    a.conv = out->steps_to_converge; a.kstar = out->kstar; a.predT = out->predT;
    a.margin = out->margin_energy; a.fe_top1 = out->fe_top1; a.fe_gap = out->fe_gap; a.F = out->F; a.y_out = out->y_final;
    const bool wl = sizeof(float) * (size_t)K * d->H <= (size_t)ENERGY_WY_LDS, hl = d->H <= ENERGY_H_LDS;
    if (wl) return hl ? launch_energy<true, true>(a, c.s) : launch_energy<true, false>(a, c.s);
    return hl ? launch_energy<false, true>(a, c.s) : launch_energy<false, false>(a, c.s);
}

// ---- label side of the joint RBM's log-likelihood (imdbn/utils/likelihood.py; kernels_joint.hpp) ---------------------
int imdbn_rbm_label_loglik(const imdbn_rbm_desc* d, const float* z, int64_t ldz, int N, int Dz, int K, const int32_t* gt,
                           double* out_joint, double* out_marg, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    CHK(LabelSide::check("label_loglik", d, Dz, K));
    if (N < 1) return fail(IMDBN_E_INVALID, "label_loglik: N = %d rows", N);
    if (ldz < Dz) return fail(IMDBN_E_INVALID, "label_loglik: ldz %lld < Dz %d", (long long)ldz, Dz);
    if (!z || !gt || !out_joint || !out_marg)
        return fail(IMDBN_E_INVALID, "label_loglik: null %s", !z ? "z" : (!gt ? "gt" : (!out_joint ? "out_joint" : "out_marg")));
    LabelSide s(d, Dz, S(stream));
    CHK(s.propagate(z, ldz, N, ws, ws_bytes));
    const Ctx& c = s.c;
    JointArgs a{};
    a.base = s.base; a.ldb = d->H;
    a.z = z; a.ldz = ldz;
    a.bz = s.bz; a.by = s.by;
    a.Wy = s.Wy; a.ldw = d->ldw;
    a.gt = gt; a.N = N; a.Dz = Dz; a.K = K; a.H = d->H;
    a.joint = out_joint; a.marg = out_marg;
    hipLaunchKernelGGL(joint_label_loglik, dim3(c.L.Bp / ROW_WAVES), dim3(64 * ROW_WAVES), 0, c.s, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- exact pseudo-log-likelihood (imdbn/utils/likelihood.py; kernels_pll.hpp) ------------------------------------------
// The up propagation's raw logits (f_h), pll_rows_sigmoid (sigma in place, NaN rows for invalid input), pll_sites (every column as
// a Bernoulli site, into the caller's out_site or f_vp) and pll_rows_finish (group terms, row totals).
int imdbn_rbm_pseudo_loglik(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int N, double* out_pll, float* out_site, int64_t lds,
                            void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (N < 1) return fail(IMDBN_E_INVALID, "pseudo_loglik: N = %d rows", N);
    if (!v || !out_pll) return fail(IMDBN_E_INVALID, "pseudo_loglik: null %s", !v ? "v" : "out_pll");
    if (ldv < d->V) return fail(IMDBN_E_INVALID, "pseudo_loglik: ldv %lld < V %d", (long long)ldv, d->V);
    if (out_site && lds < d->V) return fail(IMDBN_E_INVALID, "pseudo_loglik: lds %lld < V %d", (long long)lds, d->V);
    Ctx c(d, nullptr, S(stream));
    CHK(setup(c, N, ws, ws_bytes));
    const Layout& L = c.L;
    CHK(up_logits(c, v, ldv));                 // x = c + v W
    PllArgs a;
    memset(&a, 0, sizeof(a));
    a.v = v; a.ldv = ldv; a.sig = L.f_h; a.ldx = L.H;
    a.W = d->W; a.ldw = d->ldw; a.vis_bias = d->vis_bias;
    a.site = out_site ? out_site : L.f_vp; a.lds = out_site ? lds : L.V;
    a.pll = out_pll; a.N = N; a.V = d->V; a.H = d->H;
    a.sp.n_groups = d->n_groups;
    for (int g = 0; g < d->n_groups; ++g) { a.sp.gs[g] = d->group_start[g]; a.sp.ge[g] = d->group_end[g]; }
    const dim3 rows(cdiv(N, ROW_WAVES)), rblock(64 * ROW_WAVES);
    hipLaunchKernelGGL(pll_rows_sigmoid, rows, rblock, 0, c.s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(pll_sites, dim3(cdiv(d->V, PLL_TI), cdiv(N, PLL_TR)), dim3(256), 0, c.s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(pll_rows_finish, rows, rblock, 0, c.s, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- exact log Z and marginals by enumeration (imdbn/utils/likelihood.py; kernels_exact.hpp) ------------------------------
#include "host_exact.hpp"

// ---- cross-modal label metrics (imdbn/utils/cross_eval.py; kernels_metrics.hpp) ---------------------------------------------
int imdbn_cross_metrics(const float* p, int64_t ldp, int B, int K, const float* y, int64_t ldy, const int32_t* gt, const float* row_mse,
                        int npix, int topk, const imdbn_cross_metrics_out* out, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    if (K < 2 || K > LABEL_KMAX) return fail(IMDBN_E_INVALID, "cross_metrics: K = %d outside [2, %d]", K, LABEL_KMAX);
    if (B < 1) return fail(IMDBN_E_INVALID, "cross_metrics: B = %d (must be >= 1)", B);
    if (topk < 1) return fail(IMDBN_E_INVALID, "cross_metrics: topk = %d (must be >= 1)", topk);
    if (npix < 1) return fail(IMDBN_E_INVALID, "cross_metrics: npix = %d (must be >= 1)", npix);
    if ((y != nullptr) == (gt != nullptr))
        return fail(IMDBN_E_INVALID, "cross_metrics: exactly one of y and gt must be given (got %s)", y ? "both" : "neither");
    if (!p || ldp < K) return fail(IMDBN_E_INVALID, "cross_metrics: bad p (ldp = %lld < K = %d or null)", (long long)ldp, K);
    if (y && ldy < K) return fail(IMDBN_E_INVALID, "cross_metrics: ldy = %lld < K = %d", (long long)ldy, K);
    if (!out || !out->acc) return fail(IMDBN_E_INVALID, "cross_metrics: null accumulator acc");
    // workspace: the per-row codes [B], then one partial record per wave of cross_metrics_rows
    const size_t code_bytes = knn_align(sizeof(int32_t) * (size_t)B), need = code_bytes + sizeof(CmPartial) * ROW_WAVES * CM_MAX_BLOCKS;
    if (!ws || ((uintptr_t)ws & 255) != 0 || ws_bytes < need)
        return fail(IMDBN_E_WORKSPACE, "cross_metrics: workspace %zu < %zu bytes (or null / not 256-byte aligned)", ws_bytes, need);
    const int nb = std::min(cdiv(B, ROW_WAVES), CM_MAX_BLOCKS);
    CmArgs a{};
    a.p = p; a.ldp = ldp; a.y = y; a.ldy = ldy; a.gt = gt; a.row_mse = row_mse;
    a.B = B; a.K = K; a.npix = npix; a.topk = topk;
    a.pred = out->pred; a.gt_out = out->gt; a.rank = out->rank; a.p_pred = out->p_pred; a.p_true = out->p_true;
    a.confusion = (unsigned long long*)out->confusion;
    a.code = (int32_t*)ws; a.part = (CmPartial*)((char*)ws + code_bytes);
    hipLaunchKernelGGL(cross_metrics_rows, dim3(nb), dim3(64 * ROW_WAVES), 0, S(stream), a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(cross_metrics_combine, dim3(1 + (out->class_sums ? K : 0)), dim3(64), 0, S(stream), a.part, ROW_WAVES * nb, a.code, row_mse,
                       B, out->acc, out->class_sums);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- pairwise free-energy scores and retrieval ranks (imdbn/utils/retrieval.py; kernels_pair.hpp) -------------------
#include "host_pair.hpp"

// ---- unit moments for tuning curves and per-unit regressions (imdbn/utils/unit_tuning.py; kernels_tuning.hpp) ----------
#include "host_tuning.hpp"

// rbm.py:443-471: v+ by conditional inference, H+, CD-k from v+ (optionally re-clamped / sampled), H-.
// Leaves the statistics operands in the workspace exactly as cd_phases does.
static int clamped_phases(Ctx& c, const float* v_known, const float* mask, int64_t ldk, int n_init,
                          const imdbn_chain_step* init_steps, const float* mu, int64_t ldmu, int Dz, const imdbn_cd_opts* o) {
    const imdbn_rbm_desc* d = c.d;
    const int B = c.L.B;
    const Layout& L = c.L;
    float* vplus = L.f_v[0];
    // positive phase: v+ by conditional inference (rbm.py:443-453), H+ = up(v+) (:455)
    CHK(run_chain(c, ChainSpec{v_known, mask, ldk, 1, n_init, init_steps, mu, ldmu, Dz, vplus, (int64_t)L.V}, true));
    for (int it = 0; it < o->cd_k; ++it) {
        {   // h_prob = up(v_neg) ; first iteration: v_neg == v+ so this is also H+
            FinishArgs f = new_finish();
            if (o->sample_h) { f.vmode = 1; f.uni = c.rng.floats(B, L.H); }
            f.op.rm = L.hid_rm; f.op.rm_terms = o->sample_h ? 1 : c.rt; f.rm_src = o->sample_h ? 2 : 1;
            if (it == 0) {
                f.op.tr = L.hid_tr[0]; f.op.tr_terms = c.ht; f.tr_src = 1;
                f.colsum_part = L.cs_hpos; f.colsum_src = 1;
            }
            CHK(prop(c, true, OpIn{it == 0 ? L.vis_rm[0] : L.vis_rm[1], (it > 0 && o->sample_v) ? 1 : c.rt, nullptr}, f));
        }
        {   // v_neg = down(h) [re-clamped] [sampled]   (rbm.py:463-469)
            const bool last = (it == o->cd_k - 1);
            FinishArgs f = new_finish();
            if (o->reclamp_negative) { f.clamp = 1; f.vk = v_known; f.mask = mask; f.ldk = ldk; }
            if (o->sample_v) { f.vmode = 2; f.uni = c.rng.floats(B, L.V); c.rng.cats(B, d->n_groups, &f.cat_tape, &f.cat_uni); }
            f.out_prob = L.f_vp; f.ld_prob = L.V;
            f.out_final = L.f_v[1]; f.ld_final = L.V;
            f.op.rm = L.vis_rm[1]; f.op.rm_terms = o->sample_v ? 1 : c.rt; f.rm_src = 2;
            if (last) {
                f.op.tr = L.vis_tr[1]; f.op.tr_terms = o->sample_v ? 1 : c.rt; f.tr_src = 2;
                f.colsum_part = L.cs_vneg; f.colsum_src = 2;
                f.loss_ref = vplus; f.ld_ref = L.V; f.loss_src = 2; f.loss_part = L.loss_part;
            }
            CHK(prop(c, false, OpIn{L.hid_rm, o->sample_h ? 1 : c.rt, nullptr}, f));
        }
    }
    {   // H- = up(v_neg)  (rbm.py:471)
        FinishArgs f = new_finish();
        f.op.tr = L.hid_tr[1]; f.op.tr_terms = c.ht; f.tr_src = 1; f.op.tr_negate = 1;
        f.colsum_part = L.cs_hneg; f.colsum_src = 1;
        CHK(prop(c, true, OpIn{L.vis_rm[1], o->sample_v ? 1 : c.rt, nullptr}, f));
    }
    return 0;
}

int imdbn_rbm_clamped_step(const imdbn_rbm_desc* d, const float* v_known, const float* mask, int64_t ldk, int B,
                           int n_init, const imdbn_chain_step* init_steps, const float* mu, int64_t ldmu, int Dz,
                           const imdbn_cd_opts* o, imdbn_rng* rng, float* loss_out, void* ws, size_t ws_bytes,
                           imdbn_stream_t stream) {
    CHK(check_desc(d, true));
    if (!v_known || !mask || !o || ldk < d->V) return fail(IMDBN_E_INVALID, "clamped_step: bad argument");
    if (o->cd_k < 1) return fail(IMDBN_E_INVALID, "CD=%d", o->cd_k);
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    CHK(clamped_phases(c, v_known, mask, ldk, n_init, init_steps, mu, ldmu, Dz, o));
    CHK(c.rng.finish());
    const BiasArgs bias = make_bias(c, o, false, (float)B, loss_out);
    CHK(launch_assoc(c, 0, o, c.rt, nullptr, o->sample_v ? 1 : c.rt, (float)B, nullptr, &bias));
    return 0;
}

// data-parallel half of the clamped update ("train_epoch_clamped shards the same way"): the rank's
// un-normalised statistics in the packed layout of imdbn_rbm_cd_stats; all-reduce, then imdbn_rbm_apply_delta
// (with sparsity off: the clamped update has no sparsity term, rbm.py:473-481).
int imdbn_rbm_clamped_stats(const imdbn_rbm_desc* d, const float* v_known, const float* mask, int64_t ldk, int B,
                            int n_init, const imdbn_chain_step* init_steps, const float* mu, int64_t ldmu, int Dz,
                            const imdbn_cd_opts* o, imdbn_rng* rng, float* packed, void* ws, size_t ws_bytes,
                            imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!v_known || !mask || !o || !packed || ldk < d->V) return fail(IMDBN_E_INVALID, "clamped_stats: bad argument");
    if (o->cd_k < 1) return fail(IMDBN_E_INVALID, "CD=%d", o->cd_k);
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    CHK(clamped_phases(c, v_known, mask, ldk, n_init, init_steps, mu, ldmu, Dz, o));
    CHK(c.rng.finish());
    const BiasArgs pack = make_pack(c, packed);
    CHK(launch_assoc(c, 1, o, c.rt, nullptr, o->sample_v ? 1 : c.rt, 1.0f, packed, &pack));
    return 0;
}


// ---- persistent chains (imdbn/models/rbm.py: train_epoch_persistent; kernels_pt.hpp) -----------------------------------
// a REPLAY tape must hold what the call will draw: checked before the first launch, so that an error leaves nothing touched
static int tape_room(const char* name, const imdbn_rng* rng, int64_t floats, int64_t cats) {
    if (!rng || rng->mode != IMDBN_RNG_REPLAY) return 0;
    if ((floats > 0 && (!rng->tape || rng->tape_len < floats)) || (cats > 0 && (!rng->cat_tape || rng->cat_len < cats)))
        return fail(IMDBN_E_RNG, "%s: the replay tape holds %lld floats / %lld indices, the call draws %lld / %lld", name,
                    (long long)rng->tape_len, (long long)rng->cat_len, (long long)floats, (long long)cats);
    return 0;
}

// rbm.py:199-209 with the negative phase taken from the caller's particles: cd_k Gibbs steps on them (written back in place), H- from
// where they end, then the positive phase of the data -- it draws nothing, so it may come last, and with `recon` its probabilities
// stay in hid_rm for one more down propagation, the mean-field reconstruction whose squared error is the loss.  That K2 is the last
// of the call: its block count is what n_loss_used() reports.  Leaves the statistics operands in the workspace exactly as cd_phases does.
static int pcd_phases(Ctx& c, const float* data, int64_t ldd, float* particles, int64_t ldp, const imdbn_cd_opts* o, bool recon) {
    const Layout& L = c.L;
    const int B = L.B;
    const bool vbits = c.r.vbits;      // (Route: the visible state travels as a bit plane too, as the negative phase of cd_phases)
    // v = particles: a 0/1 state is one bf16 term; with cd_k = 0 they are the negative statistics as they are
    CHK(prep(c, particles, ldp, L.V, L.vis_rm[1], L.Vpad, L.vis_tr[1], nullptr, L.cs_vneg, 1, vbits ? L.vis_bits[1] : nullptr));
    const OpIn vneg{L.vis_rm[1], 1, nullptr, vbits ? L.vis_bits[1] : nullptr, 1};
    for (int it = 0; it < o->cd_k; ++it) {
        {   // h = 1[up(v) > U]
            FinishArgs f = new_finish();
            f.vmode = 1; f.uni = c.rng.floats(B, L.H);
            f.op.rm = L.hid_rm; f.op.rm_terms = 1; f.rm_src = 2;
            CHK(prop(c, true, vneg, f));
        }
        {   // v = sampleV(down(h)), into the particles
            FinishArgs f = new_finish();
            f.vmode = 1; f.uni = c.rng.floats(B, L.V);
            c.rng.cats(B, c.d->n_groups, &f.cat_tape, &f.cat_uni);
            if (c.r.neg_rm) { f.op.rm = L.vis_rm[1]; f.op.rm_terms = 1; f.rm_src = 2; }      // (only a K1 that cannot read the bit plane needs it)
            f.op.tr = L.vis_tr[1]; f.op.tr_terms = 1; f.tr_src = 2;
            f.colsum_part = L.cs_vneg; f.colsum_src = 2;
            if (vbits) f.op.bits = L.vis_bits[1];
            f.out_final = particles; f.ld_final = ldp;
            CHK(prop(c, false, OpIn{L.hid_rm, 1, nullptr}, f));
        }
    }
    {   // H- = up(v): probabilities, no draw
        FinishArgs f = new_finish();
        f.op.tr = L.hid_tr[1]; f.op.tr_terms = c.ht; f.tr_src = 1; f.op.tr_negate = 1;
        f.colsum_part = L.cs_hneg; f.colsum_src = 1;
        CHK(prop(c, true, vneg, f));
    }
    // positive phase: P+ = up(data)
    CHK(prep(c, data, ldd, L.V, L.vis_rm[0], L.Vpad, L.vis_tr[0], L.flags, L.cs_vpos, 3, L.vis_bits[0]));
    {
        FinishArgs f = new_finish();
        if (recon) { f.op.rm = L.hid_rm; f.op.rm_terms = c.rt; f.rm_src = 1; }
        f.op.tr = L.hid_tr[0]; f.op.tr_terms = c.ht; f.tr_src = 1;
        f.colsum_part = L.cs_hpos; f.colsum_src = 1;
        CHK(prop(c, true, OpIn{L.vis_rm[0], c.nw == 1 ? 1 : 0, L.flags, L.vis_bits[0], data_operand_kind(o->data_binary)}, f));
    }
    if (recon) {   // v_rec = down(P+) at T = 1; its squared error against the data
        FinishArgs f = new_finish();
        f.loss_ref = data; f.ld_ref = ldd; f.loss_src = 1; f.loss_part = L.loss_part;
        CHK(prop(c, false, OpIn{L.hid_rm, c.rt, nullptr}, f));
    }
    return 0;
}

int imdbn_rbm_pcd_step(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, float* particles, int64_t ldp,
                       const imdbn_cd_opts* o, imdbn_rng* rng, float* loss_out, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, true));
    if (!data || !particles || !o) return fail(IMDBN_E_INVALID, "pcd_step: null %s", !data ? "data" : (!particles ? "particles" : "opts"));
    if (ldd < d->V) return fail(IMDBN_E_INVALID, "pcd_step: ldd %lld < V %d", (long long)ldd, d->V);
    if (ldp < d->V) return fail(IMDBN_E_INVALID, "pcd_step: ldp %lld < V %d", (long long)ldp, d->V);
    if (B < 1) return fail(IMDBN_E_INVALID, "pcd_step: B = %d rows", B);
    if (o->cd_k < 0) return fail(IMDBN_E_INVALID, "pcd_step: cd_k = %d", o->cd_k);
    if (o->cd_k > 0 && !rng) return fail(IMDBN_E_INVALID, "pcd_step: null rng with cd_k = %d", o->cd_k);
    if (o->data_binary < 0 || o->data_binary > 2) return fail(IMDBN_E_INVALID, "pcd_step: data_binary %d outside 0..2", o->data_binary);
    if (o->next_data || o->next_slot || o->data_slot || o->next_binary || o->fwd_out)
        return fail(IMDBN_E_INVALID, "pcd_step: the prefetch fields and fwd_out must be zero (next_data %p, next_slot %d, data_slot %d, next_binary %d, fwd_out %p)",
                    (const void*)o->next_data, o->next_slot, o->data_slot, o->next_binary, (const void*)o->fwd_out);
    const int G = d->n_groups;
    CHK(tape_room("pcd_step", rng, (int64_t)o->cd_k * B * ((int64_t)d->H + d->V), (int64_t)o->cd_k * G * B));
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    CHK(pcd_phases(c, data, ldd, particles, ldp, o, loss_out != nullptr));
    CHK(c.rng.finish());
    BiasArgs bias = make_bias(c, o, o->sparsity != 0, (float)B, loss_out);
    if (!loss_out) { bias.loss_part = nullptr; bias.n_loss = 0; }
    CHK(launch_assoc(c, 0, o, c.nw == 1 ? 1 : 0, c.L.flags, 1, (float)B, nullptr, &bias));
    return 0;
}

// ---- centered update (imdbn/models/rbm.py: train_epoch_centered; kernels_centered.hpp) ---------------------------------
// The grid of centered_apply: column tiles of `tw` columns (64 E per wave step, at most CTR_CS steps, the steps spread evenly over
// the tiles) times row stripes of `rps` <= CTR_ROWS rows, about two blocks per CU.  A function of (V, H) and the CU count alone.
struct CenteredPlan { int tw, ctiles, rps, nstripes; };
static CenteredPlan centered_plan(int V, int H, bool vec4) {
    const int unit = 64 * (vec4 ? 4 : 1), nunits = cdiv(H, unit);
    CenteredPlan p;
    p.tw = cdiv(nunits, cdiv(nunits, CTR_CS)) * unit;
    p.ctiles = cdiv(H, p.tw);
    const int want = std::max(cdiv(V, CTR_ROWS), std::min(V, cdiv(2 * std::max(cu_count(), 1), p.ctiles)));
    p.rps = cdiv(V, want);
    p.nstripes = cdiv(V, p.rps);
    return p;
}
// scratch = [dW V H | pad to 4 | col_part nstripes H | row_part ctiles V]; sized for whichever of the two plans has more partials
static size_t centered_dw_floats(int V, int H) { return ((size_t)V * H + 3) / 4 * 4; }
size_t imdbn_centered_scratch_floats(int V, int H) {
    if (V <= 0 || H <= 0) return 0;
    size_t tail = 0;
    for (int v4 = 0; v4 < 2; ++v4) {
        const CenteredPlan p = centered_plan(V, H, v4 != 0);
        tail = std::max(tail, (size_t)p.nstripes * H + (size_t)p.ctiles * V);
    }
    return centered_dw_floats(V, H) + (tail + 3) / 4 * 4;
}

int imdbn_rbm_centered_step(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, float* particles, int64_t ldp,
                            const imdbn_cd_opts* o, imdbn_rng* rng, float* mu, float* lam, float slide, int mode,
                            float* loss_out, float* scratch, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, true));
    if (!data || !o || !mu || !lam || !scratch)
        return fail(IMDBN_E_INVALID, "centered_step: null %s", !data ? "data" : (!o ? "opts" : (!mu ? "mu" : (!lam ? "lam" : "scratch"))));
    if (ldd < d->V) return fail(IMDBN_E_INVALID, "centered_step: ldd %lld < V %d", (long long)ldd, d->V);
    if (particles && ldp < d->V) return fail(IMDBN_E_INVALID, "centered_step: ldp %lld < V %d", (long long)ldp, d->V);
    if (B < 1) return fail(IMDBN_E_INVALID, "centered_step: B = %d rows", B);
    if (o->cd_k < (particles ? 0 : 1))
        return fail(IMDBN_E_INVALID, "centered_step: cd_k = %d (%s)", o->cd_k, particles ? "particles need cd_k >= 0" : "CD from the data needs cd_k >= 1");
    const bool draws = !particles || o->cd_k > 0;
    if (draws && !rng) return fail(IMDBN_E_INVALID, "centered_step: null rng with cd_k = %d", o->cd_k);
    if (!(slide >= 0.0f && slide <= 1.0f)) return fail(IMDBN_E_INVALID, "centered_step: slide = %g outside [0, 1]", (double)slide);
    if (mode != 0 && mode != 1) return fail(IMDBN_E_INVALID, "centered_step: mode = %d outside {0, 1}", mode);
    if (o->data_binary < 0 || o->data_binary > 2) return fail(IMDBN_E_INVALID, "centered_step: data_binary %d outside 0..2", o->data_binary);
    if (o->next_data || o->next_slot || o->data_slot || o->next_binary || o->fwd_out)
        return fail(IMDBN_E_INVALID, "centered_step: the prefetch fields and fwd_out must be zero (next_data %p, next_slot %d, data_slot %d, next_binary %d, fwd_out %p)",
                    (const void*)o->next_data, o->next_slot, o->data_slot, o->next_binary, (const void*)o->fwd_out);
    const int G = d->n_groups, V = d->V, H = d->H;
    if (particles) CHK(tape_room("centered_step", rng, (int64_t)o->cd_k * B * ((int64_t)H + V), (int64_t)o->cd_k * G * B));
    else CHK(tape_room("centered_step", rng, (int64_t)B * H + (int64_t)o->cd_k * B * ((int64_t)H + V), (int64_t)o->cd_k * G * B));
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    if (particles) CHK(pcd_phases(c, data, ldd, particles, ldp, o, loss_out != nullptr));
    else { t_cd = CdRec{}; CHK(cd_phases(c, data, ldd, o)); }
    CHK(c.rng.finish());
    CHK(launch_assoc(c, 1, o, c.nw == 1 ? 1 : 0, c.L.flags, 1, 1.0f, scratch));
    const Layout& L = c.L;
    const bool vec4 = c.r.vec4 && (((uintptr_t)c.d->W_m | (uintptr_t)scratch) & 15) == 0;
    const CenteredPlan p = centered_plan(V, H, vec4);
    CenteredArgs a;
    memset(&a, 0, sizeof(a));
    a.W = d->W; a.Wm = d->W_m; a.ldw = d->ldw; a.V = V; a.H = H; a.dW = scratch;
    a.hpos = L.cs_hpos; a.hneg = L.cs_hneg; a.vpos = L.cs_vpos; a.vneg = L.cs_vneg; a.P = L.P;
    a.mu = mu; a.lam = lam;
    a.lr = o->lr; a.mom = o->momentum; a.wd = o->weight_decay; a.n = (float)B; a.slide = slide; a.mode = mode;
    a.rps = p.rps; a.tw = p.tw; a.nstripes = p.nstripes; a.ctiles = p.ctiles;
    a.col_part = scratch + centered_dw_floats(V, H); a.row_part = a.col_part + (size_t)p.nstripes * H;
    a.hid_bias = d->hid_bias; a.hb_m = d->hb_m; a.vis_bias = d->vis_bias; a.vb_m = d->vb_m;
    a.sparsity = o->sparsity != 0; a.target = o->sparsity_target;
    a.loss_part = L.loss_part; a.n_loss = n_loss_used(c); a.loss_den = (float)B * (float)V;
    a.loss_out = loss_out;
    if (vec4) hipLaunchKernelGGL(centered_apply<true>, dim3(p.ctiles, p.nstripes), dim3(256), 0, c.s, a);
    else      hipLaunchKernelGGL(centered_apply<false>, dim3(p.ctiles, p.nstripes), dim3(256), 0, c.s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(centered_finish, dim3(cdiv(std::max(V, H), 256) + 1), dim3(256), 0, c.s, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- extended mean field: TAP training and log Z (imdbn/utils/tap.py; kernels_tap.hpp) -----------------------------------
#include "host_tap.hpp"

// ---- deep Boltzmann machine: the two-sided layer half-step (imdbn/models/dbm.py; kernels_dbm.hpp) -------------------------
#include "host_dbm.hpp"

// ---- deep Boltzmann machine: AIS log Z and the variational bound (imdbn/utils/likelihood.py; kernels_dbm_ais.hpp) ----------
#include "host_dbm_ais.hpp"

// ---- multimodal deep Boltzmann machine: the half-step of a layer of categorical units (imdbn/models/mdbm.py; kernels_dbm_group.hpp) ----
#include "host_dbm_group.hpp"

// ---- Gaussian visible units (imdbn/models/grbm.py; kernels_gauss.hpp) ----------------------------------------------------
// p(h | v) is the Bernoulli engine applied to u = v e^{-z}, the mean of p(v | h) its logits path: K1 / K2 / K3 are called as they are.
static int gauss_check(const char* name, const imdbn_rbm_desc* d, bool need_momentum, const float* logvar) {
    CHK(check_desc(d, need_momentum));
    if (d->n_groups > 0) return fail(IMDBN_E_UNSUPPORTED, "%s: %d softmax groups on a Gaussian visible layer", name, d->n_groups);
    if (!logvar) return fail(IMDBN_E_INVALID, "%s: null logvar", name);
    return 0;
}

// one gauss_rows launch over [B][V]
static int launch_gauss_rows(const Ctx& c, const imdbn_rbm_desc* d, const float* logvar, int B, GaussRowsArgs a) {
    a.bias = d->vis_bias; a.logvar = logvar; a.B = B; a.V = d->V;
    hipLaunchKernelGGL(gauss_rows, dim3(cdiv(d->V, 256), cdiv(B, GAUSS_RPT)), dim3(256), 0, c.s, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// u = v e^{-z} into `u` (pitch V)
static int gauss_scale(const Ctx& c, const imdbn_rbm_desc* d, const float* logvar, const float* v, int64_t ldv, int B, float* u) {
    GaussRowsArgs a;
    memset(&a, 0, sizeof(a));
    a.in = v; a.ldi = ldv; a.out_u = u; a.ldu = d->V;
    return launch_gauss_rows(c, d, logvar, B, a);
}

int imdbn_rbm_gauss_prop_up(const imdbn_rbm_desc* d, const float* logvar, const float* v, int64_t ldv, int B, float T, imdbn_rng* rng,
                            float* out_prob, int64_t ldo, float* out_sample, int64_t lds, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(gauss_check("gauss_prop_up", d, false, logvar));
    if (!v || !out_prob) return fail(IMDBN_E_INVALID, "gauss_prop_up: null %s", !v ? "v" : "out_prob");
    if (ldv < d->V) return fail(IMDBN_E_INVALID, "gauss_prop_up: ldv %lld < V %d", (long long)ldv, d->V);
    if (ldo < d->H) return fail(IMDBN_E_INVALID, "gauss_prop_up: ldo %lld < H %d", (long long)ldo, d->H);
    if (out_sample && lds < d->H) return fail(IMDBN_E_INVALID, "gauss_prop_up: lds %lld < H %d", (long long)lds, d->H);
    if (out_sample && !rng) return fail(IMDBN_E_INVALID, "gauss_prop_up: null rng with a sample");
    if (B < 1) return fail(IMDBN_E_INVALID, "gauss_prop_up: B = %d rows", B);
    if (out_sample) CHK(tape_room("gauss_prop_up", rng, (int64_t)B * d->H, 0));
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    CHK(gauss_scale(c, d, logvar, v, ldv, B, c.L.f_v[0]));
    FinishArgs f = new_finish();
    f.T = T;
    f.out_prob = out_prob; f.ld_prob = ldo;
    if (out_sample) { f.vmode = 1; f.uni = c.rng.floats(B, d->H); f.out_final = out_sample; f.ld_final = lds; }
    CHK(prep_prop(c, true, c.L.f_v[0], d->V, f));
    return c.rng.finish();
}

int imdbn_rbm_gauss_prop_down(const imdbn_rbm_desc* d, const float* logvar, const float* h, int64_t ldh, int B, imdbn_rng* rng,
                              float* out_mean, int64_t ldo, float* out_sample, int64_t lds, void* ws, size_t ws_bytes,
                              imdbn_stream_t stream) {
    CHK(gauss_check("gauss_prop_down", d, false, logvar));
    if (!h || !out_mean) return fail(IMDBN_E_INVALID, "gauss_prop_down: null %s", !h ? "h" : "out_mean");
    if (ldh < d->H) return fail(IMDBN_E_INVALID, "gauss_prop_down: ldh %lld < H %d", (long long)ldh, d->H);
    if (ldo < d->V) return fail(IMDBN_E_INVALID, "gauss_prop_down: ldo %lld < V %d", (long long)ldo, d->V);
    if (out_sample && lds < d->V) return fail(IMDBN_E_INVALID, "gauss_prop_down: lds %lld < V %d", (long long)lds, d->V);
    if (out_sample && !rng) return fail(IMDBN_E_INVALID, "gauss_prop_down: null rng with a sample");
    if (B < 1) return fail(IMDBN_E_INVALID, "gauss_prop_down: B = %d rows", B);
    if (out_sample) CHK(tape_room("gauss_prop_down", rng, (int64_t)B * d->V, 0));
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    FinishArgs f = new_finish();
    f.logits_only = 1;                                     // the mean: b + h W^T
    f.out_prob = out_mean; f.ld_prob = ldo;
    CHK(prep_prop(c, false, h, ldh, f));
    if (out_sample) {
        GaussRowsArgs a;
        memset(&a, 0, sizeof(a));
        a.in = out_mean; a.ldi = ldo; a.sample = 1; a.nz = c.rng.floats(B, d->V); a.out_v = out_sample; a.ldv = lds;
        CHK(launch_gauss_rows(c, d, logvar, B, a));
    }
    return c.rng.finish();
}

int imdbn_rbm_gauss_sample_visible(const imdbn_rbm_desc* d, const float* logvar, const float* mean, int64_t ldm, int B, imdbn_rng* rng,
                                   float* out, int64_t ldo, imdbn_stream_t stream) {
    CHK(gauss_check("gauss_sample_visible", d, false, logvar));
    if (!mean || !out || !rng) return fail(IMDBN_E_INVALID, "gauss_sample_visible: null %s", !mean ? "mean" : (!out ? "out" : "rng"));
    if (ldm < d->V) return fail(IMDBN_E_INVALID, "gauss_sample_visible: ldm %lld < V %d", (long long)ldm, d->V);
    if (ldo < d->V) return fail(IMDBN_E_INVALID, "gauss_sample_visible: ldo %lld < V %d", (long long)ldo, d->V);
    if (B < 1) return fail(IMDBN_E_INVALID, "gauss_sample_visible: B = %d rows", B);
    CHK(tape_room("gauss_sample_visible", rng, (int64_t)B * d->V, 0));
    Ctx c(d, rng, S(stream));
    GaussRowsArgs a;
    memset(&a, 0, sizeof(a));
    a.in = mean; a.ldi = ldm; a.sample = 1; a.nz = c.rng.floats(B, d->V); a.out_v = out; a.ldv = ldo;
    CHK(launch_gauss_rows(c, d, logvar, B, a));
    return c.rng.finish();
}

int imdbn_rbm_gauss_free_energy(const imdbn_rbm_desc* d, const float* logvar, const float* v, int64_t ldv, int B, float* out_F,
                                void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(gauss_check("gauss_free_energy", d, false, logvar));
    if (!v || !out_F) return fail(IMDBN_E_INVALID, "gauss_free_energy: null %s", !v ? "v" : "out_F");
    if (ldv < d->V) return fail(IMDBN_E_INVALID, "gauss_free_energy: ldv %lld < V %d", (long long)ldv, d->V);
    if (B < 1) return fail(IMDBN_E_INVALID, "gauss_free_energy: B = %d rows", B);
    Ctx c(d, nullptr, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    CHK(gauss_scale(c, d, logvar, v, ldv, B, c.L.f_v[0]));
    CHK(up_logits(c, c.L.f_v[0], d->V));                   // x = u W + c
    hipLaunchKernelGGL(gauss_free_energy_rows, dim3(B), dim3(256), 0, c.s, v, ldv, d->vis_bias, logvar, d->V, c.L.f_h, (int64_t)d->H, d->H, out_F);
    HIPCHK(hipGetLastError());
    return 0;
}

// Annealed importance sampling over Gaussian visibles (kernels_gauss_ais.hpp): M chains from the base-rate model (W = 0,
// c = 0, the same variances, visible bias b_A; null = the RBM's own b) to the RBM.  The start kernel, then per temperature:
// prep_operand on u, the up propagation's raw logits (the route of gauss_free_energy), gauss_ais_weight_sample_h and -- but for the
// last -- the down propagation's raw mean b + h W^T and gauss_ais_visible, which leaves v, u and the row's visible weight term.
// Built from the anneal_* pieces of imdbn_rbm_ais.  State buffers are scratch of the workspace no propagation of this call touches:
// logits in f_h, the mean in f_vp, the fp32 state in f_v[0] (or the caller's out_v), u in f_v[1], the M visible terms (doubles) at
// the head of vis_rm[1] (>= 96 Bp bytes) -- imdbn_ws_bytes(V, H, M) covers the call.  The reverse call runs the same
// transitions backwards from the caller's rows; the gauss_anneal_* pieces below are what the two share.

// what every kernel of either Gaussian annealing call is told, after anneal_setup; `rows`: M chains or R rows
static GaussAisArgs gauss_anneal_args(const Anneal& n, const imdbn_rbm_desc* d, const float* logvar, const float* base_vis_bias, int rows,
                                      double* logw) {
    const Layout& L = n.c.L;
    GaussAisArgs g;
    memset(&g, 0, sizeof(g));
    g.M = rows; g.Bp = L.Bp; g.V = L.V; g.H = L.H; g.Hpad = L.Hpad;
    g.vis_bias = d->vis_bias; g.base_bias = base_vis_bias ? base_vis_bias : d->vis_bias; g.logvar = logvar;
    g.state = n.a.state; g.lds = n.a.lds; g.u = L.f_v[1]; g.ldu = L.V;
    g.tv = reinterpret_cast<double*>(L.vis_rm[1]);
    g.x = L.f_h; g.ldx = L.H; g.logw = logw;
    return g;
}

// The weight step `w` (its k, form and direction are the caller's) on the logits of the current state; `sample`: it also draws h for
// the transition at w.beta_draw.
static int gauss_anneal_weigh(Anneal& n, GaussAisArgs w, bool sample) {
    const Layout& L = n.c.L;
    w.sample = sample ? 1 : 0;
    if (sample) { w.uni = n.c.rng.floats(w.M, L.H); w.rm = L.hid_rm; w.bits = L.hid_bits; }
    hipLaunchKernelGGL(gauss_ais_weight_sample_h, n.grid, n.block, 0, n.c.s, w);
    HIPCHK(hipGetLastError());
    return 0;
}

// the next state from that h: m = b + h W^T, then v = ((1 - beta) b_A + beta m) + e^{z/2} n, with u and the visible weight term
static int gauss_anneal_visible(Anneal& n, GaussAisArgs s, float beta) {
    Ctx& c = n.c;
    const Layout& L = c.L;
    c.hid_bits_ok = true;                  // hid_bits describes hid_rm: the down half may read the bit plane
    CHK(down_logits(c, L.f_vp));
    s.mean = L.f_vp; s.ldm = L.V; s.beta = beta;
    s.nz = c.rng.floats(s.M, L.V);
    hipLaunchKernelGGL(gauss_ais_visible, n.grid, n.block, 0, c.s, s);
    HIPCHK(hipGetLastError());
    return 0;
}

int imdbn_rbm_gauss_ais(const imdbn_rbm_desc* d, const float* logvar, const float* betas, int K, int M, const float* base_vis_bias,
                        imdbn_rng* rng, double* logw, float* out_v, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(gauss_check("gauss_ais", d, false, logvar));
    CHK(anneal_check("gauss_ais", d, false, nullptr, 0, M, K, betas, rng, logw, out_v, ldo));
    CHK(tape_room("gauss_ais", rng, (int64_t)M * d->V + (int64_t)(K - 1) * M * ((int64_t)d->H + d->V), 0));
    Anneal n(d, rng, stream);
    CHK(anneal_setup(n, d, M, nullptr, logw, out_v, ldo, ws, ws_bytes));
    const GaussAisArgs g = gauss_anneal_args(n, d, logvar, base_vis_bias, M, logw);
    {   // v_1 = b_A + e^{z/2} n, logw = 0
        GaussAisArgs s = g;
        s.nz = n.c.rng.floats(M, d->V);
        hipLaunchKernelGGL(gauss_ais_visible, n.grid, n.block, 0, n.c.s, s);
        HIPCHK(hipGetLastError());
    }
    for (int k = 1; k <= K; ++k) {
        CHK(anneal_logits(n, g.u));        // x = c + u_k W
        GaussAisArgs w = g;
        w.beta_prev = betas[k - 1]; w.beta = w.beta_draw = betas[k];
        CHK(gauss_anneal_weigh(n, w, k < K));      // + Delta_k(v_k); the last temperature only weighs
        if (k < K) CHK(gauss_anneal_visible(n, g, betas[k]));
    }
    return n.c.rng.finish();
}

// Reverse annealed importance sampling over Gaussian visibles: R chains from the caller's rows, and logw collects
// -F(v) - sum_k Delta_k(u_k).  gauss_rais_load_v, then K + 1 weight steps, and between two of them the transition at the temperature
// the weight kernel drew h for: per temperature the launches of imdbn_rbm_gauss_ais, on its state buffers.
int imdbn_rbm_gauss_reverse_ais(const imdbn_rbm_desc* d, const float* logvar, const float* v, int64_t ldv, int R, int K,
                                const float* betas, const float* base_vis_bias, imdbn_rng* rng, double* logw, float* out_v, int64_t ldo,
                                void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(gauss_check("gauss_reverse_ais", d, false, logvar));
    CHK(anneal_check("gauss_reverse_ais", d, true, v, ldv, R, K, betas, rng, logw, out_v, ldo));
    CHK(tape_room("gauss_reverse_ais", rng, (int64_t)K * R * ((int64_t)d->H + d->V), 0));
    Anneal n(d, rng, stream);
    CHK(anneal_setup(n, d, R, nullptr, logw, out_v, ldo, ws, ws_bytes));
    const GaussAisArgs g = gauss_anneal_args(n, d, logvar, base_vis_bias, R, logw);
    {   // u_{K+1} = the caller's rows, logw = -q_B(v)
        GaussRaisLoadArgs l;
        memset(&l, 0, sizeof(l));
        l.a = g; l.v = v; l.ldv = ldv;
        hipLaunchKernelGGL(gauss_rais_load_v, n.grid, n.block, 0, n.c.s, l);
        HIPCHK(hipGetLastError());
    }
    for (int k = K + 1; k >= 1; --k) {     // k = K + 1: the start row's softplus term; k <= K: -Delta_k(u_k)
        const bool first = k == K + 1;
        CHK(anneal_logits(n, g.u));        // x = c + u_k W
        GaussAisArgs w = g;
        w.reverse = 1; w.first = first ? 1 : 0;
        if (!first) { w.beta_prev = betas[k - 1]; w.beta = betas[k]; }
        w.beta_draw = first ? betas[K] : betas[k - 1];      // temperature of the transition that follows
        CHK(gauss_anneal_weigh(n, w, k > 1));               // the last step (k = 1) only weighs
        if (k > 1) CHK(gauss_anneal_visible(n, g, w.beta_draw));
    }
    return n.c.rng.finish();
}

// One directed layer of the DBN lower bound, and its bottom bracket under a Gaussian visible layer (DESIGN §31;
// `logvar`, null = Bernoulli visibles).  The up propagation's raw logits, bound_entropy_sample_h (h ~ q(h | v) in the caller's fp32
// form and both operand forms, entropy / -log q in double), the down propagation's raw logits from that h, and bound_loglik_rows
// (log p(v | h) in double).  Gaussian: acc[row] += log N(v; b + h W^T, e^z) + E with q(h | v) = Bernoulli(sigmoid(c + u W)),
// u = v e^{-z} -- the scale launch of gauss_prop_up in front, the up propagation reads u, gauss_bound_loglik_rows closes.
// Scratch as in imdbn_rbm_ais: the up logits in f_h, the down logits / the mean in f_v[0], u in f_v[1] -- imdbn_ws_bytes(V, H, M)
// covers the call.  (the body of either entry, after its descriptor checks)
static int bound_run(const char* name, const imdbn_rbm_desc* d, const float* logvar, const float* v, int64_t ldv, int M, int mode,
                     imdbn_rng* rng, double* acc, float* out_h, int64_t ldh, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    if (M < 1) return fail(IMDBN_E_INVALID, "%s: M = %d rows", name, M);
    if (mode != IMDBN_BOUND_ENTROPY && mode != IMDBN_BOUND_LOGQ) return fail(IMDBN_E_INVALID, "%s: unknown mode %d", name, mode);
    if (!v || !rng || !acc || !out_h) return fail(IMDBN_E_INVALID, "%s: null %s", name, !v ? "v" : (!rng ? "rng" : (!acc ? "acc" : "out_h")));
    if (ldv < d->V) return fail(IMDBN_E_INVALID, "%s: ldv %lld < V %d", name, (long long)ldv, d->V);
    if (ldh < d->H) return fail(IMDBN_E_INVALID, "%s: ldh %lld < H %d", name, (long long)ldh, d->H);
    if (logvar) CHK(tape_room(name, rng, (int64_t)M * d->H, 0));
    Ctx c(d, rng, S(stream));
    CHK(setup(c, M, ws, ws_bytes));
    const Layout& L = c.L;
    BoundArgs a;
    memset(&a, 0, sizeof(a));
    a.M = M; a.Bp = L.Bp; a.V = L.V; a.H = L.H; a.Hpad = L.Hpad; a.mode = mode;
    a.x = L.f_h; a.ldx = L.H; a.a = L.f_v[0]; a.lda = L.V; a.v = v; a.ldv = ldv;
    a.out_h = out_h; a.ldh = ldh; a.rm = L.hid_rm; a.bits = L.hid_bits; a.acc = acc;
    a.uni = c.rng.floats(M, L.H);
    if (c.rng.bad) return c.rng.finish();      // a short replay tape is an error like the others: before the first launch (the
                                               // Gaussian entry has refused it above, in tape_room's words)
    if (logvar) {
        CHK(gauss_scale(c, d, logvar, v, ldv, M, L.f_v[1]));       // u = v e^{-z}
        CHK(up_logits(c, L.f_v[1], L.V));                          // x = c + u W
    } else {
        CHK(up_logits(c, v, ldv));                                 // x = c + v W
    }
    const dim3 grid(L.Bp / ROW_WAVES), block(64 * ROW_WAVES);
    hipLaunchKernelGGL(bound_entropy_sample_h, grid, block, 0, c.s, a);
    HIPCHK(hipGetLastError());
    c.hid_bits_ok = true;                      // hid_bits describes hid_rm: the down half may read the bit plane
    CHK(down_logits(c, L.f_v[0]));             // a = b + h W^T (Gaussian: the mean)
    if (logvar) {
        GaussBoundArgs g;
        memset(&g, 0, sizeof(g));
        g.M = M; g.V = L.V; g.mean = L.f_v[0]; g.ldm = L.V; g.v = v; g.ldv = ldv; g.logvar = logvar; g.acc = acc;
        hipLaunchKernelGGL(gauss_bound_loglik_rows, grid, block, 0, c.s, g);
    } else {
        hipLaunchKernelGGL(bound_loglik_rows, grid, block, 0, c.s, a);
    }
    HIPCHK(hipGetLastError());
    return c.rng.finish();
}

int imdbn_rbm_bound_step(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int M, int mode, imdbn_rng* rng, double* acc,
                         float* out_h, int64_t ldh, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (d->n_groups > 0) return fail(IMDBN_E_UNSUPPORTED, "bound_step: softmax groups are not supported (n_groups = %d)", d->n_groups);
    return bound_run("bound_step", d, nullptr, v, ldv, M, mode, rng, acc, out_h, ldh, ws, ws_bytes, stream);
}

// The bottom bracket of the DBN lower bound under a Gaussian visible layer (kernels_gauss_bound.hpp): bound_run with z.
int imdbn_rbm_gauss_bound_step(const imdbn_rbm_desc* d, const float* logvar, const float* v, int64_t ldv, int M, int mode,
                               imdbn_rng* rng, double* acc, float* out_h, int64_t ldh, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(gauss_check("gauss_bound_step", d, false, logvar));
    return bound_run("gauss_bound_step", d, logvar, v, ldv, M, mode, rng, acc, out_h, ldh, ws, ws_bytes, stream);
}

// scratch = [S V H | mean B V | u B V | sum u0, sum u1, q0, q1: RP V each | row_part ctiles V | loss partials], every piece padded
// to 4 floats; the row partials are sized for whichever plan of gauss_apply (the tiling of centered_apply) has more column tiles
struct GaussScratch { size_t mean, u, su0, su1, q0, q1, row_part, loss, total; int RP, n_loss; };
static GaussScratch gauss_scratch(int V, int H, int B) {
    auto r4 = [](size_t n) { return (n + 3) / 4 * 4; };
    GaussScratch g;
    g.RP = cdiv(B, GAUSS_RPT); g.n_loss = cdiv(V, 256) * g.RP;
    const size_t bv = r4((size_t)B * V), pv = r4((size_t)g.RP * V);
    const int ctiles = std::max(centered_plan(V, H, false).ctiles, centered_plan(V, H, true).ctiles);
    g.mean = centered_dw_floats(V, H); g.u = g.mean + bv;
    g.su0 = g.u + bv; g.su1 = g.su0 + pv; g.q0 = g.su1 + pv; g.q1 = g.q0 + pv;
    g.row_part = g.q1 + pv; g.loss = g.row_part + r4((size_t)ctiles * V); g.total = g.loss + r4((size_t)g.n_loss);
    return g;
}
size_t imdbn_gauss_scratch_floats(int V, int H, int B) {
    if (V <= 0 || H <= 0 || B <= 0) return 0;
    return gauss_scratch(V, H, B).total;
}

int imdbn_rbm_gauss_cd_step(const imdbn_rbm_desc* d, float* logvar, float* logvar_m, const float* data, int64_t ldd, int B,
                            const imdbn_cd_opts* o, float lr_z, float z_lo, float z_hi, int sample_v, imdbn_rng* rng, float* loss_out,
                            float* scratch, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(gauss_check("gauss_cd_step", d, true, logvar));
    if (!data || !o || !scratch || !rng)
        return fail(IMDBN_E_INVALID, "gauss_cd_step: null %s", !data ? "data" : (!o ? "opts" : (!scratch ? "scratch" : "rng")));
    if (lr_z != 0.0f && !logvar_m) return fail(IMDBN_E_INVALID, "gauss_cd_step: null logvar_m with lr_z = %g", (double)lr_z);
    if (ldd < d->V) return fail(IMDBN_E_INVALID, "gauss_cd_step: ldd %lld < V %d", (long long)ldd, d->V);
    if (B < 1) return fail(IMDBN_E_INVALID, "gauss_cd_step: B = %d rows", B);
    if (o->cd_k < 1) return fail(IMDBN_E_INVALID, "gauss_cd_step: cd_k = %d (CD from the data needs cd_k >= 1)", o->cd_k);
    if (!(lr_z == lr_z)) return fail(IMDBN_E_INVALID, "gauss_cd_step: lr_z = %g", (double)lr_z);
    if (!(z_lo <= z_hi)) return fail(IMDBN_E_INVALID, "gauss_cd_step: clamp [%g, %g] is empty", (double)z_lo, (double)z_hi);
    if (sample_v != 0 && sample_v != 1) return fail(IMDBN_E_INVALID, "gauss_cd_step: sample_v = %d outside {0, 1}", sample_v);
    if (o->next_data || o->next_slot || o->data_slot || o->next_binary || o->fwd_out)
        return fail(IMDBN_E_INVALID, "gauss_cd_step: the prefetch fields and fwd_out must be zero (next_data %p, next_slot %d, data_slot %d, next_binary %d, fwd_out %p)",
                    (const void*)o->next_data, o->next_slot, o->data_slot, o->next_binary, (const void*)o->fwd_out);
    const int V = d->V, H = d->H;
    CHK(tape_room("gauss_cd_step", rng, (int64_t)o->cd_k * B * H + (int64_t)(sample_v ? o->cd_k : 0) * B * V, 0));
    Ctx c(d, rng, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    const Layout& L = c.L;
    const GaussScratch g = gauss_scratch(V, H, B);
    float* mean = scratch + g.mean;
    float* u = scratch + g.u;
    t_cd = CdRec{};
    {   // u0 = data e^{-z}, its column sums and q0
        GaussRowsArgs a;
        memset(&a, 0, sizeof(a));
        a.in = data; a.ldi = ldd; a.out_u = u; a.ldu = V; a.su_part = scratch + g.su0; a.q_part = scratch + g.q0;
        CHK(launch_gauss_rows(c, d, logvar, B, a));
    }
    CHK(prep(c, u, V, V, L.vis_rm[0], L.Vpad, L.vis_tr[0], L.flags, nullptr, 3));
    {   // positive phase: P0 = up(u0); h = 1[P0 > U]
        FinishArgs f = new_finish();
        f.vmode = 1; f.uni = c.rng.floats(B, H);
        f.op.rm = L.hid_rm; f.op.rm_terms = 1; f.rm_src = 2;
        f.op.tr = L.hid_tr[0]; f.op.tr_terms = c.ht; f.tr_src = 1;
        f.colsum_part = L.cs_hpos; f.colsum_src = 1;
        CHK(prop(c, true, OpIn{L.vis_rm[0], c.nw == 1 ? 1 : 0, L.flags}, f));
    }
    for (int it = 0; it < o->cd_k; ++it) {
        const bool last = (it == o->cd_k - 1);
        CHK(down_logits(c, mean));         // m = b + h W^T
        {   // v = m (+ e^{z/2} n); u = v e^{-z}; on the last step its column sums, q1 and the loss
            GaussRowsArgs a;
            memset(&a, 0, sizeof(a));
            a.in = mean; a.ldi = V; a.out_u = u; a.ldu = V;
            if (sample_v) { a.sample = 1; a.nz = c.rng.floats(B, V); }
            if (last) {
                a.su_part = scratch + g.su1; a.q_part = scratch + g.q1;
                if (loss_out) { a.ref = data; a.ldr = ldd; a.loss_part = scratch + g.loss; }
            }
            CHK(launch_gauss_rows(c, d, logvar, B, a));
        }
        CHK(prep(c, u, V, V, L.vis_rm[1], L.Vpad, last ? L.vis_tr[1] : nullptr, nullptr, nullptr, c.rt));
        {   // P = up(u); h = 1[P > U] on every step but the last
            FinishArgs f = new_finish();
            if (!last) {
                f.vmode = 1; f.uni = c.rng.floats(B, H);
                f.op.rm = L.hid_rm; f.op.rm_terms = 1; f.rm_src = 2;
            } else {
                f.op.tr = L.hid_tr[1]; f.op.tr_terms = c.ht; f.tr_src = 1; f.op.tr_negate = 1;
                f.colsum_part = L.cs_hneg; f.colsum_src = 1;
            }
            CHK(prop(c, true, OpIn{L.vis_rm[1], c.rt, nullptr}, f));
        }
    }
    CHK(c.rng.finish());
    CHK(launch_assoc(c, 1, o, c.nw == 1 ? 1 : 0, L.flags, c.rt, 1.0f, scratch));
    const bool vec4 = c.r.vec4 && (((uintptr_t)d->W_m | (uintptr_t)scratch) & 15) == 0;
    const CenteredPlan p = centered_plan(V, H, vec4);
    GaussArgs a;
    memset(&a, 0, sizeof(a));
    a.W = d->W; a.Wm = d->W_m; a.ldw = d->ldw; a.V = V; a.H = H; a.S = scratch;
    a.lr = o->lr; a.mom = o->momentum; a.wd = o->weight_decay; a.n = (float)B;
    a.rps = p.rps; a.tw = p.tw; a.nstripes = p.nstripes; a.ctiles = p.ctiles;
    a.row_part = scratch + g.row_part;
    a.hpos = L.cs_hpos; a.hneg = L.cs_hneg; a.P = L.P;
    a.su0 = scratch + g.su0; a.su1 = scratch + g.su1; a.q0 = scratch + g.q0; a.q1 = scratch + g.q1; a.RP = g.RP;
    a.hid_bias = d->hid_bias; a.hb_m = d->hb_m; a.vis_bias = d->vis_bias; a.vb_m = d->vb_m; a.logvar = logvar; a.logvar_m = logvar_m;
    a.lr_z = lr_z; a.z_lo = z_lo; a.z_hi = z_hi;
    a.sparsity = o->sparsity != 0; a.target = o->sparsity_target;
    a.loss_part = scratch + g.loss; a.n_loss = g.n_loss; a.loss_den = (float)B * (float)V; a.loss_out = loss_out;
    if (vec4) hipLaunchKernelGGL(gauss_apply<true>, dim3(p.ctiles, p.nstripes), dim3(256), 0, c.s, a);
    else      hipLaunchKernelGGL(gauss_apply<false>, dim3(p.ctiles, p.nstripes), dim3(256), 0, c.s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(gauss_finish, dim3(cdiv(std::max(V, H), 256) + 1), dim3(256), 0, c.s, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- one back-propagation step through a Gaussian visible layer (host_gauss_backprop.hpp; kernels_gauss_backprop.hpp) ------
#include "host_gauss_backprop.hpp"

size_t imdbn_gauss_backprop_scratch_floats(int V, int H, int B) {
    if (V <= 0 || H <= 0 || B <= 0) return 0;
    return gauss_bp_scratch(V, H, B).total;
}

int imdbn_rbm_gauss_backprop_step(const imdbn_rbm_desc* d, float* logvar, float* logvar_m, const float* v, int64_t ldv, const float* e_h,
                                  int64_t ldeh, const float* x_h, int64_t ldxh, int B, const imdbn_cd_opts* o, float lr_z, float z_lo,
                                  float z_hi, float* err_h_out, int64_t ldoh, float* loss_out, float* scratch, void* ws, size_t ws_bytes,
                                  imdbn_stream_t stream) {
    return gauss_backprop_step(d, logvar, logvar_m, v, ldv, e_h, ldeh, x_h, ldxh, B, o, lr_z, z_lo, z_hi, err_h_out, ldoh, loss_out, scratch,
                               ws, ws_bytes, S(stream));
}

// ---- one delta-rule step of a directed layer (host_delta.hpp; kernels_delta.hpp) ------------------------------------------
int imdbn_rbm_delta_step(const imdbn_rbm_desc* d, int dir, const float* in, int64_t ldi, const float* target, int64_t ldt, int B,
                         const imdbn_cd_opts* o, double* out_rowlp, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    return delta_step(d, dir, in, ldi, target, ldt, B, o, out_rowlp, ws, ws_bytes, S(stream));
}

// ---- one back-propagation step through a sigmoid layer (host_backprop.hpp; kernels_backprop.hpp) -------------------------
int imdbn_rbm_backprop_step(const imdbn_rbm_desc* d, const float* x_v, int64_t ldxv, const float* e_h, int64_t ldeh,
                            const float* x_h, int64_t ldxh, const float* e_v, int64_t ldev, int B, const imdbn_cd_opts* o,
                            float* err_v_out, int64_t ldov, float* err_h_out, int64_t ldoh, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    return backprop_step(d, x_v, ldxv, e_h, ldeh, x_h, ldxh, e_v, ldev, B, o, err_v_out, ldov, err_h_out, ldoh, ws, ws_bytes, S(stream));
}

// rows [row, row + ...) of a draw tensor that spans more rows than the launch it feeds
static DrawSrc draw_rows(DrawSrc s, int64_t row, int N) {
    s.row0 += row;
    if (s.tape) s.tape += row * N;
    return s;
}

int imdbn_rbm_pt_sweep(const imdbn_rbm_desc* d, float* state, int64_t lds, int R, int M, const float* betas, int n_sweeps, imdbn_rng* rng,
                       int64_t* swap_try, int64_t* swap_acc, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, false));
    if (!state || !betas || !rng || !swap_try || !swap_acc)
        return fail(IMDBN_E_INVALID, "pt_sweep: null %s", !state ? "state" : (!betas ? "betas" : (!rng ? "rng" : (!swap_try ? "swap_try" : "swap_acc"))));
    if (lds < d->V) return fail(IMDBN_E_INVALID, "pt_sweep: lds %lld < V %d", (long long)lds, d->V);
    if (R < 1) return fail(IMDBN_E_INVALID, "pt_sweep: R = %d replicas", R);
    if (M < 1) return fail(IMDBN_E_INVALID, "pt_sweep: M = %d chains", M);
    if (n_sweeps < 0) return fail(IMDBN_E_INVALID, "pt_sweep: n_sweeps = %d", n_sweeps);
    if (R > PT_RMAX) return fail(IMDBN_E_UNSUPPORTED, "pt_sweep: R = %d replicas; at most %d supported", R, PT_RMAX);
    if ((int64_t)R * M > (int64_t)INT_MAX / 2) return fail(IMDBN_E_INVALID, "pt_sweep: R M = %lld rows", (long long)R * M);
    if (!(betas[0] > 0.0f)) return fail(IMDBN_E_INVALID, "pt_sweep: betas[0] = %g, must be above 0", (double)betas[0]);
    if (betas[R - 1] != 1.0f) return fail(IMDBN_E_INVALID, "pt_sweep: betas[%d] = %g, must be 1", R - 1, (double)betas[R - 1]);
    for (int r = 1; r < R; ++r)
        if (!(betas[r] > betas[r - 1]))
            return fail(IMDBN_E_INVALID, "pt_sweep: betas[%d] = %g is not above betas[%d] = %g", r, (double)betas[r], r - 1, (double)betas[r - 1]);
    const int G = d->n_groups, RM = R * M, V = d->V, H = d->H;
    // finish_groups finds group g's indices at cat_tape + g B, B the rows of its launch: a replica's rows of a tape over R M rows
    // are there for one group only
    if (rng->mode == IMDBN_RNG_REPLAY && R >= 2 && G >= 2)
        return fail(IMDBN_E_UNSUPPORTED, "pt_sweep: a replay tape serves R >= 2 replicas with at most one softmax group (n_groups = %d)", G);
    CHK(tape_room("pt_sweep", rng, (int64_t)n_sweeps * RM * ((int64_t)H + V + (R >= 2 ? 1 : 0)), (int64_t)n_sweeps * G * RM));
    Ctx call(d, rng, S(stream));       // all R M rows: the draw cursor, the logits of the exchange
    CHK(setup(call, RM, ws, ws_bytes));
    Ctx rep(d, nullptr, S(stream));    // one replica's rows: its Gibbs step (the same workspace, one launch after the other)
    CHK(setup(rep, M, ws, ws_bytes));
    PtArgs x;
    memset(&x, 0, sizeof(x));
    x.state = state; x.lds = lds; x.x = call.L.f_h; x.ldx = H; x.vis_bias = d->vis_bias;
    x.R = R; x.M = M; x.V = V; x.H = H;
    x.swap_try = (unsigned long long*)swap_try; x.swap_acc = (unsigned long long*)swap_acc;
    for (int r = 0; r < R; ++r) x.beta[r] = betas[r];
    for (int s = 0; s < n_sweeps; ++s) {
        // part 1: one Gibbs step per replica at T = 1 / beta_r -- imdbn_rbm_gibbs_step(sample_h, sample_v) on the replica's rows
        const DrawSrc uh = call.rng.floats(RM, H), uv = call.rng.floats(RM, V);
        const int32_t* ct; DrawSrc cu;
        call.rng.cats(RM, G, &ct, &cu);
        for (int r = 0; r < R; ++r) {
            const int64_t row = (int64_t)r * M;
            float* rows = state + row * lds;
            const Layout& L = rep.L;
            CHK(prep(rep, rows, lds, V, L.vis_rm[0], L.Vpad, nullptr, L.flags));
            {
                FinishArgs f = new_finish();
                f.T = 1.0f / betas[r];
                f.vmode = 1; f.uni = draw_rows(uh, row, H);
                f.op.rm = L.hid_rm; f.op.rm_terms = 1; f.rm_src = 2;
                CHK(prop(rep, true, OpIn{L.vis_rm[0], rep.nw == 1 ? 1 : 0, L.flags}, f));
            }
            {
                FinishArgs f = new_finish();
                f.T = 1.0f / betas[r];
                f.vmode = 1; f.uni = draw_rows(uv, row, V);
                f.cat_tape = ct ? ct + row : nullptr; f.cat_uni = draw_rows(cu, row, 1);
                f.out_final = rows; f.ld_final = lds;
                CHK(prop(rep, false, OpIn{L.hid_rm, 1, nullptr}, f));
            }
        }
        if (R < 2) continue;
        // part 2: exchange between the pairs (r, r + 1), r = s mod 2, s mod 2 + 2, ...; the draw is consumed with or without a pair
        x.uni = call.rng.floats(RM, 1);
        x.parity = s & 1; x.n_pairs = (R - x.parity) / 2;
        if (x.n_pairs == 0) continue;
        CHK(up_logits(call, state, lds));      // x = c + v W of every row
        hipLaunchKernelGGL(pt_exchange_rows, dim3(cdiv(x.n_pairs * M, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, call.s, x);
        HIPCHK(hipGetLastError());
    }
    return call.rng.finish();
}

// ---- K3 alone: rbm.py:209-224 from caller-supplied phase tensors ------------------------------------------------------
// operand planes + column sums of the four tensors (exact three-term planes wherever a value is not exactly bf16), then the update
static int assoc_from_tensors(Ctx& c, const float* vpos, int64_t ldvp, const float* hpos, int64_t ldhp, const float* vneg, int64_t ldvn,
                              const float* hneg, int64_t ldhn, const imdbn_cd_opts* o, bool sparsity) {
    const Layout& L = c.L;
    CHK(prep(c, vpos, ldvp, L.V, nullptr, L.Vpad, L.vis_tr[0], L.flags, L.cs_vpos, c.rt));
    CHK(prep(c, vneg, ldvn, L.V, nullptr, L.Vpad, L.vis_tr[1], nullptr, L.cs_vneg, c.rt));
    CHK(prep(c, hpos, ldhp, L.H, nullptr, L.Hpad, L.hid_tr[0], L.flags_h, L.cs_hpos, c.ht));
    {
        PrepArgs p;
        memset(&p, 0, sizeof(p));
        p.in = hneg; p.ld = ldhn; p.B = L.B; p.Bp = L.Bp; p.N = L.H;
        p.op.ldrm = L.Hpad; p.op.Bp = L.Bp; p.op.tr = L.hid_tr[1]; p.op.tr_ts = (int64_t)L.H * L.Bp; p.op.tr_terms = c.ht; p.op.tr_negate = 1;
        p.colsum_part = L.cs_hneg;
        hipLaunchKernelGGL(prep_operand, dim3(cdiv(L.Hpad, 64), L.P), dim3(256), 0, c.s, p);
        HIPCHK(hipGetLastError());
    }
    BiasArgs bias = make_bias(c, o, sparsity, (float)L.B, nullptr);
    bias.loss_part = nullptr; bias.n_loss = 0;
    CHK(launch_assoc(c, 0, o, c.nw == 1 ? 1 : 0, L.flags, c.rt, (float)L.B, nullptr, &bias));
    return 0;
}

int imdbn_rbm_assoc_update(const imdbn_rbm_desc* d, const float* vpos, int64_t ldvp, const float* hpos, int64_t ldhp,
                           const float* vneg, int64_t ldvn, const float* hneg, int64_t ldhn, int B, const imdbn_cd_opts* o,
                           void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    CHK(check_desc(d, true));
    if (!vpos || !hpos || !vneg || !hneg || !o || ldvp < d->V || ldvn < d->V || ldhp < d->H || ldhn < d->H)
        return fail(IMDBN_E_INVALID, "assoc_update: bad tensor argument");
    Ctx c(d, nullptr, S(stream));
    CHK(setup(c, B, ws, ws_bytes));
    return assoc_from_tensors(c, vpos, ldvp, hpos, ldhp, vneg, ldvn, hneg, ldhn, o, o->sparsity != 0);
}

// ---- one ascent step on log p(y | z) of the joint RBM (imdbn/models/rbm.py: train_epoch_labels; kernels_labelgrad.hpp) ---
// base = z W[:Dz] + c as imdbn_rbm_label_loglik leaves it (f_h); label_grad_rows (logp, r, hpos, hneg into the caller's scratch);
// label_grad_update (the label rows of W / W_m and the label entries of the visible bias and its momentum, from base and the old
// label rows); then the update path of imdbn_rbm_assoc_update on the descriptor cut to its first Dz rows with vpos = vneg = z:
// W[:Dz] gets z^T hpos - z^T hneg, hid_bias the column sums of hpos - hneg, the code columns of vis_bias their momentum.
// Its operand preparation writes vis_tr / hid_tr / flags / column sums: f_h and the scratch are out of its way, and the label kernel
// has read base and the label rows before the update kernel starts (one stream), so both halves see the parameters on entry.
// label_grad_call is that step (bp = false) and imdbn_rbm_label_backprop_step (bp = true; o may then be NULL: nothing is written).
static int label_grad_call(const char* name, bool bp, const imdbn_rbm_desc* d, const float* z, int64_t ldz, int N, int Dz, int K, const int32_t* gt,
                           const imdbn_cd_opts* o, double* out_logp, int32_t* out_pred, float* err_z, int64_t lde, float* scratch,
                           void* ws, size_t ws_bytes, hipStream_t stream) {
    CHK(check_desc(d, o != nullptr || !bp));
    CHK(LabelSide::check(name, d, Dz, K));
    if (Dz + K != d->V) return fail(IMDBN_E_INVALID, "%s: Dz + K = %d is not V = %d", name, Dz + K, d->V);
    if (N < 1) return fail(IMDBN_E_INVALID, "%s: N = %d rows", name, N);
    if (ldz < Dz) return fail(IMDBN_E_INVALID, "%s: ldz %lld < Dz %d", name, (long long)ldz, Dz);
    if (!z || !gt || (!o && !bp) || !out_logp || !scratch)
        return fail(IMDBN_E_INVALID, "%s: null %s", name, !z ? "z" : (!gt ? "gt" : (!o && !bp ? "opts" : (!out_logp ? "out_logp" : "scratch"))));
    if (bp) {
        if (!err_z) return fail(IMDBN_E_INVALID, "%s: null err_z", name);
        if (lde < Dz) return fail(IMDBN_E_INVALID, "%s: lde %lld < Dz %d", name, (long long)lde, Dz);
        if (o && (o->cd_k || o->sparsity || o->next_data || o->next_slot || o->data_slot || o->next_binary || o->fwd_out))
            return fail(IMDBN_E_INVALID, "%s: cd_k, sparsity, the prefetch fields and fwd_out must be zero (cd_k %d, sparsity %d, next_data %p, "
                        "next_slot %d, data_slot %d, next_binary %d, fwd_out %p)", name, o->cd_k, o->sparsity, (const void*)o->next_data, o->next_slot,
                        o->data_slot, o->next_binary, (const void*)o->fwd_out);
    }
    LabelSide s(d, Dz, stream);
    CHK(s.propagate(z, ldz, N, ws, ws_bytes));
    Ctx& c = s.c;
    const Layout& L = c.L;
    const int H = d->H;
    LabelBackpropArgs g{};
    JointArgs& j = g.g.j;
    j.base = s.base; j.ldb = H;
    j.z = z; j.ldz = ldz;
    j.bz = s.bz; j.by = s.by;
    j.Wy = s.Wy; j.ldw = d->ldw;
    j.gt = gt; j.N = N; j.Dz = Dz; j.K = K; j.H = H;
    g.g.logp = out_logp;
    g.g.r = scratch; g.g.hpos = scratch + (size_t)N * K; g.g.hneg = g.g.hpos + (size_t)N * H;
    g.pred = out_pred; g.e = g.g.hneg + (size_t)N * H;
    if (bp) {
        hipLaunchKernelGGL(label_backprop_rows, dim3(cdiv(N, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, c.s, g);
    } else {
        hipLaunchKernelGGL(label_grad_rows, dim3(cdiv(N, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, c.s, g.g);
    }
    HIPCHK(hipGetLastError());
    if (o) {
        LabelUpdateArgs u{};
        u.base = s.base; u.ldb = H; u.r = g.g.r;
        u.U = d->W + (int64_t)Dz * d->ldw; u.Um = d->W_m + (int64_t)Dz * d->ldw; u.ldw = d->ldw;
        u.by = d->vis_bias + Dz; u.bym = d->vb_m + Dz;
        u.N = N; u.K = K; u.H = H;
        u.lr = o->lr; u.mom = o->momentum; u.wd = o->weight_decay; u.n = (float)N;
        hipLaunchKernelGGL(label_grad_update, dim3((unsigned)(((int64_t)K * H + K + 255) / 256)), dim3(256), 0, c.s, u);
        HIPCHK(hipGetLastError());
    }
    if (bp) {   // err_z = (e W[:Dz]^T) z (1 - z): host_backprop.hpp's err_v_out on the cut descriptor, its visible bias at zeros
        HIPCHK(hipMemsetAsync(L.cs_vneg, 0, (size_t)Dz * sizeof(float), c.s));
        float* vis_bias = s.dz.vis_bias;
        s.dz.vis_bias = L.cs_vneg;
        CHK(prep(c, g.e, H, H, L.hid_rm, L.Hpad, nullptr, L.flags_h));
        FinishArgs f = new_finish();
        f.logits_only = 1;
        f.out_prob = L.f_v[0]; f.ld_prob = Dz;
        CHK(prop(c, false, OpIn{L.hid_rm, c.nw == 1 ? 1 : 0, L.flags_h}, f));
        s.dz.vis_bias = vis_bias;
        BackpropApplyArgs a;
        memset(&a, 0, sizeof(a));
        a.B = N; a.N = Dz; a.q = L.f_v[0]; a.ldq = Dz; a.x = z; a.ldx = ldz; a.out = err_z; a.ldo = lde;
        hipLaunchKernelGGL(backprop_apply, dim3(cdiv(Dz, 256), cdiv(N, 8)), dim3(256), 0, c.s, a);
        HIPCHK(hipGetLastError());
    }
    if (!o) return 0;
    return assoc_from_tensors(c, z, ldz, g.g.hpos, H, z, ldz, g.g.hneg, H, o, false);
}

int imdbn_rbm_label_step(const imdbn_rbm_desc* d, const float* z, int64_t ldz, int N, int Dz, int K, const int32_t* gt,
                         const imdbn_cd_opts* o, double* out_logp, float* scratch, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    return label_grad_call("label_step", false, d, z, ldz, N, Dz, K, gt, o, out_logp, nullptr, nullptr, 0, scratch, ws, ws_bytes, S(stream));
}

// ---- log p(y | z) of the joint RBM as an output layer: its error at the code, and optionally the step above ----------
// Launch order, plain, on the caller's stream: the propagation of base (prep_operand of z, the up route) into f_h; label_backprop_rows
// (logp, pred, r, hpos, hneg, e into the caller's arrays); with o, label_grad_update -- it writes W[Dz:] only and is the last reader
// of base; a memset of the zero bias, prep_operand of e (hid_rm, flags_h), the logits-only down propagation on the cut descriptor
// (its partial buffer and f_v[0]: not f_h, not the scratch) and backprop_apply (err_z) -- they read W[:Dz] only; with o, the code-side
// update of label_step (operand planes, column sums, the update kernel: the only writer of W[:Dz], hid_bias and their momenta, last).
int imdbn_rbm_label_backprop_step(const imdbn_rbm_desc* d, const float* z, int64_t ldz, int N, int Dz, int K, const int32_t* gt,
                                  const imdbn_cd_opts* o, double* out_logp, int32_t* out_pred, float* err_z, int64_t lde,
                                  float* scratch, void* ws, size_t ws_bytes, imdbn_stream_t stream) {
    return label_grad_call("label_backprop_step", true, d, z, ldz, N, Dz, K, gt, o, out_logp, out_pred, err_z, lde, scratch, ws, ws_bytes, S(stream));
}

// ---- C1: collectives over RCCL for callers that do not go through torch.distributed ------------------------------------
// librccl is opened on first use (dlopen: the engine has no link-time dependency on it; a process that already runs
// torch.distributed's nccl backend gets that same library).  One communicator per (process, GPU); the caller moves the
// 128-byte unique id from rank 0 to the other ranks by whatever channel it has.
namespace {
struct Id128 { char b[128]; };      // ncclUniqueId, passed by value
struct Rccl {
    void* h = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id128, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
} g_rccl;

int rccl_load() {
    if (g_rccl.h) return 0;
    void* h = nullptr;
    for (const char* nm : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"}) { h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) return fail(IMDBN_E_UNSUPPORTED, "librccl not found: %s", dlerror());
    auto sym = [&](const char* n) { return dlsym(h, n); };
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))sym("ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))sym("ncclCommInitRank");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))sym("ncclCommDestroy");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))sym("ncclAllReduce");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))sym("ncclAllGather");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))sym("ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllReduce || !g_rccl.AllGather)
        return fail(IMDBN_E_UNSUPPORTED, "librccl lacks an expected symbol");
    g_rccl.h = h;
    return 0;
}
int rccl_fail(int rc, const char* what) {
    return fail(rc > 0 ? rc : IMDBN_E_INVALID, "%s: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error");
}
}  // namespace

int imdbn_comm_unique_id(void* id128) {
    if (!id128) return fail(IMDBN_E_INVALID, "comm_unique_id: null buffer");
    CHK(rccl_load());
    const int rc = g_rccl.GetUniqueId(id128);
    return rc ? rccl_fail(rc, "ncclGetUniqueId") : 0;
}

int imdbn_comm_init(void** comm, int world, int rank, const void* id128) {
    if (!comm || !id128 || world < 1 || rank < 0 || rank >= world) return fail(IMDBN_E_INVALID, "comm_init: bad argument");
    CHK(rccl_load());
    Id128 id;
    memcpy(id.b, id128, 128);
    const int rc = g_rccl.CommInitRank(comm, world, id, rank);
    return rc ? rccl_fail(rc, "ncclCommInitRank") : 0;
}

int imdbn_comm_destroy(void* comm) {
    if (!comm) return 0;
    CHK(rccl_load());
    const int rc = g_rccl.CommDestroy(comm);
    return rc ? rccl_fail(rc, "ncclCommDestroy") : 0;
}

int imdbn_allreduce_sum_f32(void* comm, float* buf, size_t count, imdbn_stream_t stream) {
    if (!comm || !buf) return fail(IMDBN_E_INVALID, "allreduce: bad argument");
    CHK(rccl_load());
    const int rc = g_rccl.AllReduce(buf, buf, count, /* ncclFloat32 */ 7, /* ncclSum */ 0, comm, S(stream));
    return rc ? rccl_fail(rc, "ncclAllReduce") : 0;
}

int imdbn_allgather_bytes(void* comm, const void* send, void* recv, size_t bytes_per_rank, imdbn_stream_t stream) {
    if (!comm || !send || !recv) return fail(IMDBN_E_INVALID, "allgather: bad argument");
    CHK(rccl_load());
    const int rc = g_rccl.AllGather(send, recv, bytes_per_rank, /* ncclUint8 */ 1, comm, S(stream));
    return rc ? rccl_fail(rc, "ncclAllGather") : 0;
}

}  // extern "C"
