// host_layout.hpp -- host side, part 1 (included by engine.hip, inside its anonymous namespace): the tuning knobs and their
// option table, the workspace layout, and the Route: every "which kernel runs this" decision of a call, made once.
#pragma once

// Tuning / testing knobs.  The process-wide defaults are set by imdbn_set_option / imdbn_set_tuning; a caller that wants its own
// (two engines with different settings in one process) creates an imdbn_options handle and binds it to its thread with
// imdbn_use_options: every engine call made by that thread then reads the handle instead of the defaults.  Knobs that shape the
// workspace layout (split-K factors, tile heights) must be the same for all calls that share a workspace.
struct Tuning {
    int ks_up = 0, ks_down = 0;      // split-K factors of the generic propagation kernels (0 = automatic)
    int no_fast_k3 = 0;              // testing: force the unaligned-shape update kernel
    int no_fast_k1 = 0;
    int no_fused_up = 0;
    int k4_rows = 0;                 // tuning: batch rows per chain-kernel block (0 = automatic)
    int no_rank_loop = 0;            // testing: one update-kernel launch per gathered rank block
    int no_chain_kernel = 0;         // testing: run chains as one launch per half step
    int no_rank_acc = 0;             // testing: tile-wise rank loop (k3_body_ranks) even when the accumulating form applies
    int min_rank_loop = 2;           // apply_factors: rank blocks from which the single-launch rank loop is used (1 block: the plain update kernel, 46 vs 60 us)
    int no_prefetch = 0;             // testing: ignore imdbn_cd_opts.next_data
    int no_bits = 0;                 // testing: never use the bit-packed hidden operand
    int down_tr = 0;                 // tuning: rows per fused-K2 block (0 = automatic)
    int no_k1s = 0;                  // testing: never use the LDS-DMA streaming K1 for binary operands (k1_stream)
    int k1s_ks = 0;                  // tuning: K slices of k1_stream (0 = automatic)
    int no_k2s = 0;                  // testing: never use k2_stream (the fused K2 for a bit-plane hidden operand, one tile per CU)
    int k2s_tr = 0;                  // tuning: rows per k2_stream block (0 = automatic; multiple of 8, <= 48)
    int no_k1s_real = 0;             // testing: real-valued operands of K1 take the partial GEMM + finish launches, not k1_stream
    int no_adaptive = 0;             // testing: a prefetched batch of unknown content gets all three-term forms (no per-item choice)
    int k1s_lds_pad = 0;             // experiment: extra dynamic LDS (bytes) for the bit-plane k1_stream
    int no_chain_pair = 0;           // testing: imdbn_rbm_chain_pair runs its chains one after the other
    int no_down_tiled = 0;           // testing: multi-chunk real-valued K2 without the LDS-tiled kernel
    int no_update_bin = 0;           // testing: single-chunk updates of one-term visible operands run assoc_update_planes, not assoc_update_bin
    int k3_tpb = 0;                  // testing: visible tiles per block of the streaming update kernels (0 = automatic: ~one block per CU)
    int no_down_chunks = 0;          // testing: the fused K2 of a multi-chunk batch runs one block per (tile, 64-row chunk)
    int k1s_force_na = 0;            // experiment: bit-plane operands run on the kernel instantiation that can also read bf16 terms
};
Tuning g_defaults;
thread_local const Tuning* t_bound = nullptr;
inline const Tuning& tune() { return t_bound ? *t_bound : g_defaults; }
int g_dbg = 0;    // tuning aid: kernels that record per-block timeline stamps (64 K1, 128 K2, 256 finish, 512 K3; tools/stamps_probe.py)

// imdbn_set_option / imdbn_options_set: name -> knob.  FLAG stores value != 0, CLAMP clamps into [lo, hi], CHECKED accepts 0 and the
// multiples of `step` in [lo, hi] and rejects everything else; "dbg" (process-wide, not a Tuning member) is handled by set_opt.
enum OptKind { OPT_SET, OPT_FLAG, OPT_CLAMP, OPT_CHECKED };
struct Opt { const char* name; int Tuning::*knob; OptKind kind = OPT_SET; int lo = 0, hi = 0, step = 1; };
const Opt g_opts[] = {
    {"ksplit_up", &Tuning::ks_up, OPT_CLAMP, 0, INT_MAX}, {"ksplit_down", &Tuning::ks_down, OPT_CLAMP, 0, INT_MAX},
    {"k1s_ks", &Tuning::k1s_ks, OPT_CLAMP, 0, INT_MAX}, {"k1s_lds_pad", &Tuning::k1s_lds_pad, OPT_CLAMP, 0, 64 * 1024},
    {"down_rows", &Tuning::down_tr, OPT_CHECKED, 4, 32, 4}, {"k2s_rows", &Tuning::k2s_tr, OPT_CHECKED, 8, 48, 8},
    {"chain_rows", &Tuning::k4_rows, OPT_CHECKED, 0, 16, 1},
    {"generic_k3", &Tuning::no_fast_k3, OPT_FLAG}, {"generic_k1", &Tuning::no_fast_k1, OPT_FLAG}, {"no_fused_up", &Tuning::no_fused_up, OPT_FLAG},
    {"no_rank_loop", &Tuning::no_rank_loop}, {"no_rank_acc", &Tuning::no_rank_acc}, {"min_rank_loop", &Tuning::min_rank_loop},
    {"no_chain_kernel", &Tuning::no_chain_kernel}, {"no_chain_pair", &Tuning::no_chain_pair}, {"no_bits", &Tuning::no_bits},
    {"no_prefetch", &Tuning::no_prefetch}, {"no_adaptive", &Tuning::no_adaptive}, {"k1s_force_na", &Tuning::k1s_force_na},
    {"no_k1s", &Tuning::no_k1s}, {"no_k1s_real", &Tuning::no_k1s_real}, {"no_k2s", &Tuning::no_k2s},
    {"no_down_chunks", &Tuning::no_down_chunks}, {"no_down_tiled", &Tuning::no_down_tiled},
    {"no_update_bin", &Tuning::no_update_bin}, {"k3_tpb", &Tuning::k3_tpb, OPT_CLAMP, 0, 64},
};

int set_opt(Tuning& t, const char* name, int value) {
    if (!name) return fail(IMDBN_E_INVALID, "null option name");
    if (!strcmp(name, "dbg")) { g_dbg = value; return 0; }
    for (const Opt& o : g_opts) {
        if (strcmp(name, o.name)) continue;
        if (o.kind == OPT_CHECKED && value != 0 && (value < o.lo || value > o.hi || value % o.step)) {
            if (o.step > 1) return fail(IMDBN_E_INVALID, "%s must be 0 or a multiple of %d in [%d, %d]", o.name, o.step, o.lo, o.hi);
            return fail(IMDBN_E_INVALID, "%s must be in [%d, %d]", o.name, o.lo, o.hi);
        }
        t.*o.knob = o.kind == OPT_FLAG ? (value != 0) : (o.kind == OPT_CLAMP ? std::max(o.lo, std::min(value, o.hi)) : value);
        return 0;
    }
    return fail(IMDBN_E_INVALID, "unknown option %s", name);
}

inline int rup(int x, int m) { return (x + m - 1) / m * m; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- split-K plan --------------------------------------------------------------------------
struct Split { int ks; int kchunk; };
Split plan_split(int Kpad, int n_tiles, int m_blocks, int forced, int cap) {
    int ks = forced;
    if (ks <= 0) {
        const int target = 768;    // ~3 workgroups per CU on 256 CUs
        ks = std::max(1, (int)((double)target / (double)(n_tiles * m_blocks) + 0.5));
    }
    ks = std::min(ks, cap);
    ks = std::min(ks, cdiv(Kpad, 64));
    ks = std::max(ks, 1);
    const int kchunk = rup(cdiv(Kpad, ks), 64);
    return {cdiv(Kpad, kchunk), kchunk};
}

// ---- workspace layout ----------------------------------------------------------------------
struct Layout {
    int V, H, B, Bp, Vpad, Hpad, P;
    Split up, down;
    bool up4;
    int* flags; int* flags_h;
    bf16_t* vis_rm[2];
    bf16_t* vis_tr[2];
    bf16_t* hid_rm;
    bf16_t* hid_tr[2];
    uint8_t* hid_bits; int ldbits;       // bit plane of the sampled hidden states, byte-major [Hpad64/8][Bp]
    uint8_t* vis_bits[2];                // bit planes of the visible operands (0: data, 1: negative-phase sample), [Vpad64/8][Bp]
    uint8_t* pf_bits[2];                 // ... of the prefetch slots
    float* partial;
    float* f_h;
    float* f_vp;
    float* f_v[2];
    float* cs_hpos; float* cs_hneg; float* cs_vpos; float* cs_vneg;
    float* loss_part; int n_loss_slots;
    size_t fb_off, fb_bytes;      // the factor block inside the workspace
    // prefetch slots 1 / 2: operand forms of a batch prepared ahead of its CD step (imdbn_cd_opts.next_data)
    bf16_t* pf_rm[2]; bf16_t* pf_tr[2]; int* pf_flags[2]; float* pf_cs[2];
    ChainRec* chain_recs;   // per-step schedule of the row-parallel chain kernel
    bf16_t* k4_planes; int64_t k4_plane_stride;      // fragment-ordered bf16 weight planes [2 directions][3 terms]
    int down_tr;            // visible rows per block of the fused K2 (<= 32): balances the row tiles over the CUs
    int k2s_tr;             // rows per k2_stream block: one tile per CU where the layer is large enough
    int k1s_tiles, k1s_ks, k1s_kchunk; int* k1s_cnt;      // k1_stream: 32-column tiles, K slices, arrival counters [Bp/64][tiles]
    size_t bytes;
};

// What the process knows per device ORDINAL (not per process: a second device gets its own): CU count, kernel attributes set
struct DeviceOnce {
    std::mutex m;
    std::vector<int> cus;      // by ordinal; 0 = not seen yet
    std::vector<char> attrs;   // by ordinal; 1 = kernel attributes set (host_prop.hpp kernel_attrs_ready)
} g_devices;

int cu_count() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 256;
    std::lock_guard<std::mutex> lock(g_devices.m);
    if ((int)g_devices.cus.size() <= dev) g_devices.cus.resize(dev + 1, 0);
    if (g_devices.cus[dev] <= 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
        g_devices.cus[dev] = n;
    }
    return g_devices.cus[dev];
}

// Fused K2 streams W once, one tile of `tr` visible rows per block, and every block costs the same; the kernel
// ends when the CU with the most rows ends (blocks are dealt round-robin).  10000 rows as 313 tiles of 32 put two
// tiles (64 rows) on 57 of the 256 CUs and one on the rest: the main loop ran 13 us at the median and 20 us on
// those 57.  20-row tiles (500 blocks, two per CU, 40 rows each) level it.  The MFMA tile stays 32 wide.
int plan_down_rows(int V, int cus) {
    if (tune().down_tr > 0) return tune().down_tr;
    int best = 32, best_cost = 1 << 30;
    for (int tr = 32; tr >= 16; tr -= 4) {
        const int cost = cdiv(cdiv(V, tr), cus) * tr;       // rows streamed by the busiest CU
        if (cost < best_cost) { best_cost = cost; best = tr; }
    }
    return best;
}

inline bool cols_vec4(int H) { return H % 4 == 0 && H >= 4; }
// float4 weight rows: every row of W starts 16-byte aligned and holds whole float4s.  THE definition (Route::vec4)
bool vec4_rows(const imdbn_rbm_desc* d) { return cols_vec4(d->H) && d->ldw % 4 == 0 && (((uintptr_t)d->W) & 15) == 0; }

Layout make_layout(int V, int H, int B, char* base) {
    const Tuning& t = tune();
    const int cus = cu_count();
    Layout L{};
    L.V = V; L.H = H; L.B = B;
    L.Bp = rup(std::max(B, 1), 64);
    L.Vpad = rup(V, 16); L.Hpad = rup(H, 16);
    L.P = L.Bp / 8;
    const int mb = L.Bp / 64;
    L.up4 = cols_vec4(H) && !t.no_fast_k1;      // float4 K1 (also needs 16-B aligned W: Route::vec4)
    if (L.up4) {
        const int tiles = cdiv(H, 128) * mb;
        const int want = t.ks_up > 0 ? t.ks_up : std::max(1, 252 / std::max(1, tiles));
        L.up = plan_split(L.Vpad, cdiv(H, 128), mb, want, 64);
    } else {
        L.up = plan_split(L.Vpad, cdiv(H, 64), mb, t.ks_up, 64);
    }
    L.down = plan_split(L.Hpad, cdiv(V, 64), mb, t.ks_down, 16);
    L.down_tr = plan_down_rows(V, cus);
    L.k2s_tr = t.k2s_tr > 0 ? t.k2s_tr : std::min(48, std::max(8, 8 * cdiv(V, 8 * cus)));
    size_t off = 0;
    auto take = [&](size_t nbytes) { char* p = base ? base + off : nullptr; off += (nbytes + 255) / 256 * 256; return p; };
    // exactness maps of caller-supplied operands (prep rewrites them every call): visible side, hidden side
    // ---- factor block: everything the weight / bias update needs from one CD pass, contiguous, so that the
    // data-parallel "factor exchange" can all-gather it in one piece (imdbn_factor_block): exactness map of the data,
    // hidden planes (pos, negated neg), column-sum and squared-error partials, visible planes (pos: 3 terms; neg: its
    // FIRST term only is inside the block -- the negative visible state of train_epoch is a sample, one term)
    L.fb_off = off;
    L.flags = (int*)take((size_t)L.P * cdiv(L.Vpad, 64) * 4);
    for (int i = 0; i < 2; ++i) L.hid_tr[i] = (bf16_t*)take((size_t)3 * H * L.Bp * 2);
    L.cs_hpos = (float*)take((size_t)L.P * H * 4);
    L.cs_hneg = (float*)take((size_t)L.P * H * 4);
    L.cs_vpos = (float*)take((size_t)L.P * V * 4);
    L.cs_vneg = (float*)take((size_t)L.P * V * 4);
    L.n_loss_slots = std::max(cdiv(std::max(V, H), 64) * L.P, (cdiv(V, 8) + 2) * (L.Bp / 64)) + IMDBN_MAX_GROUPS * (L.Bp / 64);
    L.loss_part = (float*)take((size_t)L.n_loss_slots * 4);
    for (int i = 0; i < 2; ++i) {
        L.vis_tr[i] = (bf16_t*)take((size_t)3 * V * L.Bp * 2);
        if (i == 1) L.fb_bytes = (off - (((size_t)3 * V * L.Bp * 2 + 255) / 256 * 256)) + ((size_t)V * L.Bp * 2 + 255) / 256 * 256 - L.fb_off;
    }
    // ---- the rest
    L.flags_h = (int*)take((size_t)L.P * cdiv(L.Hpad, 64) * 4);
    for (int i = 0; i < 2; ++i) L.vis_rm[i] = (bf16_t*)take((size_t)3 * L.Bp * L.Vpad * 2);
    L.hid_rm = (bf16_t*)take((size_t)3 * L.Bp * L.Hpad * 2);
    L.ldbits = 2 * cdiv(L.Hpad, 64);
    L.hid_bits = (uint8_t*)take((size_t)L.Bp * rup(H, 64) / 8);
    for (int i = 0; i < 2; ++i) L.vis_bits[i] = (uint8_t*)take((size_t)L.Bp * rup(V, 64) / 8);
    {   // k1_stream: ~one block per CU; a K slice is a multiple of 64 rows and at most K1S_MAX_KCHUNK (its bits sit in LDS)
        L.k1s_tiles = cdiv(H, 32);
        int ks = t.k1s_ks > 0 ? t.k1s_ks : std::max(1, (int)((double)cus / (double)(L.k1s_tiles * mb) + 0.5));
        ks = std::min(ks, std::max(1, L.Vpad / 192));      // at least three K16 steps per wave and slice (1500 <-> 500: 8 slices of 192 rows, 45.5 us per update against 47.9 with 12 of 128)
        ks = std::max(ks, cdiv(L.Vpad, K1S_MAX_KCHUNK));
        L.k1s_kchunk = rup(cdiv(L.Vpad, ks), 64);
        L.k1s_ks = cdiv(L.Vpad, L.k1s_kchunk);
    }
    const size_t pf = std::max(std::max((size_t)L.up.ks * L.Bp * H, (size_t)L.down.ks * L.Bp * V), (size_t)L.k1s_ks * L.Bp * 32 * L.k1s_tiles);
    L.partial = (float*)take(pf * 4);
    L.k1s_cnt = (int*)take((size_t)mb * L.k1s_tiles * 4);
    L.f_h = (float*)take((size_t)L.Bp * H * 4);
    L.f_vp = (float*)take((size_t)L.Bp * V * 4);
    for (int i = 0; i < 2; ++i) L.f_v[i] = (float*)take((size_t)L.Bp * V * 4);
    L.chain_recs = (ChainRec*)take(sizeof(ChainRec) * CHAIN_MAX_STEPS);
    for (int i = 0; i < 2; ++i) {
        L.pf_rm[i] = (bf16_t*)take((size_t)3 * L.Bp * L.Vpad * 2);
        L.pf_tr[i] = (bf16_t*)take((size_t)3 * V * L.Bp * 2);
        L.pf_flags[i] = (int*)take((size_t)L.P * cdiv(L.Vpad, 64) * 4);
        L.pf_cs[i] = (float*)take((size_t)L.P * V * 4);
        L.pf_bits[i] = (uint8_t*)take((size_t)L.Bp * rup(V, 64) / 8);
    }
    L.k4_plane_stride = 0; L.k4_planes = nullptr;
    if (V <= 1024 && H <= 1024) {
        L.k4_plane_stride = (int64_t)std::max(cdiv(H, 16) * cdiv(V, 32), cdiv(V, 16) * cdiv(H, 32)) * 512;
        L.k4_planes = (bf16_t*)take((size_t)6 * L.k4_plane_stride * 2);
    }
    L.bytes = off;
    return L;
}

// the CD step reads its data-side operands from prefetch slot `slot` (1 / 2) instead of the default buffers
void use_slot(Layout& L, int slot) {
    if (slot < 1 || slot > 2) return;
    std::swap(L.vis_rm[0], L.pf_rm[slot - 1]);
    std::swap(L.vis_tr[0], L.pf_tr[slot - 1]);
    std::swap(L.flags, L.pf_flags[slot - 1]);
    std::swap(L.cs_vpos, L.pf_cs[slot - 1]);
    std::swap(L.vis_bits[0], L.pf_bits[slot - 1]);
}

// An activation operand in row-major form: pointer + static term count (0 = look at flag)
// bits / binary: the operand also exists as a bit plane; binary = 1: it is 0/1 by construction (a sample), 2: the caller
// says so (checked on the device against the exactness map `flag`), 3: nobody knows -- the streaming K1 decides per
// 64-column item from the exactness map (bit plane where the item is all 0/1, the bf16 terms in `rm` elsewhere)
struct OpIn { const bf16_t* rm; int terms; const int* flag; const uint8_t* bits = nullptr; int binary = 0; };
// imdbn_cd_opts.data_binary (0 unknown, 1 asserted 0/1, 2 real) -> OpIn::binary of the data operand
int data_operand_kind(int data_binary) { return data_binary == IMDBN_DATA_BINARY ? 2 : (data_binary == IMDBN_DATA_UNKNOWN ? 3 : 0); }

// ---- route -------------------------------------------------------------------------------------
// Which kernel family a propagation of this call runs, and what the callers may leave unwritten because of it.  Computed once
// per call (setup) from the descriptor, the layout and the bound knobs; prop() chooses from it and the CD orchestration reads
// the same fields, so "what will run" and "what runs" cannot part.
enum class Up { fused, stream_bits, stream_real, partial };
struct Route {
    bool vec4;         // float4 weight rows (vec4_rows)
    bool up_fused;     // K1: short K, gemm_up_fused (no split-K slabs)
    bool k1s;          // K1: k1_stream takes every operand that has a form it reads (up())
    bool k1s_real;     // ... bf16 terms included (else only bit planes)
    bool k2s;          // K2: k2_stream takes a 0/1 hidden operand that exists as a bit plane
    bool k2s_cd;       // ... which the K2 of a CD pass always is (a sample): the K2 of cd_phases is k2_stream, else the fused K2
    bool vbits;        // CD: the negative visible sample leaves its K2 as a bit plane too (whole-byte tiles, no softmax group)
    bool neg_rm;       // CD: ... and is still needed as vis_rm[1] (its K1 cannot read the bit plane)
    bool prefetch;     // CD: a next batch can be prepared ahead (imdbn_cd_opts.next_data is honoured)
    bool next_on_k1;   // CD: its preparation rides on the negative-phase k1_stream (k2_stream: a 512-thread block per CU, nothing fits beside it)
    bool rides;        // CD: ... or on the fused K2 (gemm_down_fused_next); false: a prep_operand launch of its own, first thing
    bool adaptive_ok;  // k1_stream's per-item choice (K1S_ADAPTIVE) fits this shape
    bool adaptive_next;// CD: a next batch of unknown content is prepared item by item (PrepArgs::adaptive)
    int tpb;           // visible tiles (128 rows) per block of the streaming update kernel
    int cd_k2_blocks;  // blocks per batch chunk (= squared-error partials) of the K2 of a CD pass on <= 64 rows

    // the family of one up propagation, from the forms its operand has
    Up up(const OpIn& in, bool logits_only) const {
        if (up_fused) return Up::fused;
        if (!k1s || logits_only) return Up::partial;
        if (in.bits && (in.binary == 1 || in.binary == 2)) return Up::stream_bits;
        return (in.rm && k1s_real && (in.binary == 0 || (in.binary == 3 && in.bits && in.flag))) ? Up::stream_real : Up::partial;
    }
    // the data operand of a forward pass / positive phase: read as a bit plane (or per item), and then without its bf16 form?
    bool data_bits(int data_binary) const { return k1s && data_binary != IMDBN_DATA_REAL; }
    bool data_needs_rm(int data_binary) const { return !(k1s && data_binary == IMDBN_DATA_BINARY); }
};

Route make_route(const imdbn_rbm_desc* d, const Layout& L) {
    const Tuning& t = tune();
    Route r{};
    r.vec4 = vec4_rows(d);
    r.up_fused = L.Vpad <= 1024 && !t.no_fused_up;
    r.k1s = r.vec4 && !t.no_k1s && !r.up_fused;
    r.k1s_real = r.k1s && !t.no_k1s_real;
    r.k2s = r.vec4 && !t.no_k2s;
    r.k2s_cd = r.k2s && !t.no_bits;
    r.vbits = d->n_groups == 0 && (r.k2s_cd || L.down_tr % 8 == 0);
    r.neg_rm = !(r.vbits && r.k1s);
    r.prefetch = r.vec4 && !t.no_prefetch;
    r.next_on_k1 = r.k2s_cd && r.vbits && r.k1s;
    r.rides = !r.k2s_cd || r.next_on_k1;
    r.tpb = t.k3_tpb > 0 ? t.k3_tpb : std::max(1, cdiv(cdiv(L.H, 128) * cdiv(L.V, 128), std::max(cu_count(), 1)));
    // The per-item choice of k1_stream holds one exactness-map entry per thread for a K slice's items (<= 32) and one for a span
    // of the update kernel (<= 256 entries); layers outside that read data of unknown content from the bf16 terms throughout
    // (same numbers, all three-term forms prepared) ... and one block of the (first batch chunk of the) positive-phase K1 per
    // span of the update kernel for the fix-up of mixed spans: a narrow hidden layer has too few (found by
    // tools/stress_parity.py: 1576 x 12, 1437 x 32, 2116 x 28)
    r.adaptive_ok = L.k1s_kchunk <= 2048 && 2 * r.tpb * L.P <= 256 && cdiv(cdiv(L.V, 128), r.tpb) <= L.k1s_tiles * L.k1s_ks;
    r.adaptive_next = r.rides && !t.no_adaptive && r.k1s_real && r.adaptive_ok;
    r.cd_k2_blocks = cdiv(L.Vpad, r.k2s_cd ? L.k2s_tr : L.down_tr);
    return r;
}
