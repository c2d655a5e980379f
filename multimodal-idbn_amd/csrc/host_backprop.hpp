// host_backprop.hpp -- host side, part 5 (included by engine.hip after host_delta.hpp): one back-propagation step through a sigmoid
// layer (imdbn_rbm_backprop_step; kernels_backprop.hpp).
//
// Launches, plain, on the caller's stream, in this order:
//   per error output wanted: prep_operand of the error rows (the row-major form the propagation reads), the logits-only
//     propagation of prop() WITHOUT a bias (down for err_v_out, up for err_h_out), backprop_apply;
//   when applying, per pair present: prep_operand of the input rows (their transposed planes only) and backprop_rows of the error
//     rows; then backprop_finish and the update kernel through launch_assoc.
// Every launch that reads W precedes the update kernel, which is the last launch of the call.
// The bias-free product: prop() adds the descriptor's bias in its epilogue, so the propagation runs on a copy of the descriptor whose
// bias of the output side points at zeros in the workspace (a column-partial buffer no launch of this call uses, cleared by a
// memset node on the stream): x + 0.0f is x, no bias is added and taken back.
// Slots of the weight pass (the update kernel adds vpos^T hpos + vneg^T hneg, hneg being STORED negated by a CD pass: here both
// hidden slots hold what is to be added, as host_delta.hpp has it):
//   up pair    (vpos, hpos) = (x_v, e_h)      vis_tr[0] by prep_operand (with its exactness map), hid_tr[0] by backprop_rows
//   down pair  (vneg, hneg) = (e_v, x_h)      vis_tr[1] by backprop_rows, hid_tr[1] by prep_operand
//   up only:   hid_tr[1] = zeros (backprop_rows), the visible slot 1 aliased to slot 0 -- the call of delta_step UP
//   down only: vis_tr[0] = zeros (backprop_rows), the hidden slot 0 aliased to slot 1 -- the call of delta_step DOWN
// The update kernel's own bias rows are off (bias == nullptr): backprop_finish moves the biases.
#pragma once

int backprop_step(const imdbn_rbm_desc* d, const float* x_v, int64_t ldxv, const float* e_h, int64_t ldeh,
                  const float* x_h, int64_t ldxh, const float* e_v, int64_t ldev, int B, const imdbn_cd_opts* o,
                  float* err_v_out, int64_t ldov, float* err_h_out, int64_t ldoh, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!d) return fail(IMDBN_E_INVALID, "backprop_step: null descriptor");
    CHK(check_desc(d, false));
    if (d->n_groups > 0) return fail(IMDBN_E_UNSUPPORTED, "backprop_step: softmax groups are not supported (n_groups = %d)", d->n_groups);
    if (!x_v != !e_h) return fail(IMDBN_E_INVALID, "backprop_step: half an up pair (x_v %p, e_h %p)", (const void*)x_v, (const void*)e_h);
    if (!x_h != !e_v) return fail(IMDBN_E_INVALID, "backprop_step: half a down pair (x_h %p, e_v %p)", (const void*)x_h, (const void*)e_v);
    const bool has_up = x_v != nullptr, has_dn = x_h != nullptr;
    if (!has_up && !has_dn) return fail(IMDBN_E_INVALID, "backprop_step: no pair at all (x_v, e_h, x_h, e_v are NULL)");
    if (err_v_out && !has_up) return fail(IMDBN_E_INVALID, "backprop_step: err_v_out %p without the up pair", (const void*)err_v_out);
    if (err_h_out && !has_dn) return fail(IMDBN_E_INVALID, "backprop_step: err_h_out %p without the down pair", (const void*)err_h_out);
    if (!o && !err_v_out && !err_h_out) return fail(IMDBN_E_INVALID, "backprop_step: opts == NULL and both outputs NULL: nothing to do");
    const int V = d->V, H = d->H;
    if (has_up && ldxv < V) return fail(IMDBN_E_INVALID, "backprop_step: ldxv %lld < %d", (long long)ldxv, V);
    if (has_up && ldeh < H) return fail(IMDBN_E_INVALID, "backprop_step: ldeh %lld < %d", (long long)ldeh, H);
    if (has_dn && ldxh < H) return fail(IMDBN_E_INVALID, "backprop_step: ldxh %lld < %d", (long long)ldxh, H);
    if (has_dn && ldev < V) return fail(IMDBN_E_INVALID, "backprop_step: ldev %lld < %d", (long long)ldev, V);
    if (err_v_out && ldov < V) return fail(IMDBN_E_INVALID, "backprop_step: ldov %lld < %d", (long long)ldov, V);
    if (err_h_out && ldoh < H) return fail(IMDBN_E_INVALID, "backprop_step: ldoh %lld < %d", (long long)ldoh, H);
    if (B < 1) return fail(IMDBN_E_INVALID, "backprop_step: B = %d rows", B);
    if (o) {
        if (!d->W_m || !d->hb_m || !d->vb_m) return fail(IMDBN_E_INVALID, "backprop_step: null momentum buffer (W_m %p, hb_m %p, vb_m %p)",
                                                         (const void*)d->W_m, (const void*)d->hb_m, (const void*)d->vb_m);
        if (o->cd_k || o->sparsity || o->next_data || o->next_slot || o->data_slot || o->next_binary || o->fwd_out)
            return fail(IMDBN_E_INVALID, "backprop_step: cd_k, sparsity, the prefetch fields and fwd_out must be zero (cd_k %d, sparsity %d, next_data %p, "
                        "next_slot %d, data_slot %d, next_binary %d, fwd_out %p)", o->cd_k, o->sparsity, (const void*)o->next_data, o->next_slot,
                        o->data_slot, o->next_binary, (const void*)o->fwd_out);
    }
    imdbn_rbm_desc dz = *d;                          // the descriptor the propagations see: its biases become zeros below
    Ctx c(&dz, nullptr, stream);
    CHK(setup(c, B, ws, ws_bytes));
    Layout& L = c.L;
    const int one = c.nw == 1 ? 1 : 0;               // operand terms of a propagation: one in FAST mode, else by the exactness map
    // ---- the errors at the layer's inputs, from the parameters on entry
    auto apply = [&](const float* q, int N, const float* x, int64_t ldx, float* out, int64_t ldo) {
        BackpropApplyArgs a;
        memset(&a, 0, sizeof(a));
        a.B = B; a.N = N; a.q = q; a.ldq = N; a.x = x; a.ldx = ldx; a.out = out; a.ldo = ldo;
        hipLaunchKernelGGL(backprop_apply, dim3(cdiv(N, 256), cdiv(B, 8)), dim3(256), 0, c.s, a);
        HIPCHK(hipGetLastError());
        return 0;
    };
    if (err_v_out) {                                 // (e_h W^T) x_v (1 - x_v)
        HIPCHK(hipMemsetAsync(L.cs_vneg, 0, (size_t)V * sizeof(float), c.s));
        dz.vis_bias = L.cs_vneg;
        CHK(prep(c, e_h, ldeh, H, L.hid_rm, L.Hpad, nullptr, L.flags_h));
        FinishArgs f = new_finish();
        f.logits_only = 1;
        f.out_prob = L.f_v[0]; f.ld_prob = V;
        CHK(prop(c, false, OpIn{L.hid_rm, one, L.flags_h}, f));
        CHK(apply(L.f_v[0], V, x_v, ldxv, err_v_out, ldov));
    }
    if (err_h_out) {                                 // (e_v W) x_h (1 - x_h)
        HIPCHK(hipMemsetAsync(L.cs_hneg, 0, (size_t)H * sizeof(float), c.s));
        dz.hid_bias = L.cs_hneg;
        CHK(prep(c, e_v, ldev, V, L.vis_rm[0], L.Vpad, nullptr, L.flags));
        FinishArgs f = new_finish();
        f.logits_only = 1;
        f.out_prob = L.f_h; f.ld_prob = H;
        CHK(prop(c, true, OpIn{L.vis_rm[0], one, L.flags}, f));
        CHK(apply(L.f_h, H, x_h, ldxh, err_h_out, ldoh));
    }
    if (!o) return 0;
    // ---- the operands of the weight pass and the column partials of the bias gradients
    auto rows = [&](const float* e, int64_t lde, int N, bf16_t* tr_e, bf16_t* tr_zero, float* part) {
        BackpropRowsArgs a;
        memset(&a, 0, sizeof(a));
        a.B = B; a.Bp = L.Bp; a.N = N; a.e = e; a.lde = lde; a.tr_e = tr_e; a.tr_zero = tr_zero; a.terms = c.ht; a.colsum_part = part;
        hipLaunchKernelGGL(backprop_rows, dim3(cdiv(N, 256), L.Bp / 8), dim3(256), 0, c.s, a);
        HIPCHK(hipGetLastError());
        return 0;
    };
    if (has_up) {
        CHK(prep(c, x_v, ldxv, V, nullptr, L.Vpad, L.vis_tr[0], L.flags, nullptr, c.rt));
        CHK(rows(e_h, ldeh, H, L.hid_tr[0], has_dn ? nullptr : L.hid_tr[1], L.cs_hpos));
    }
    if (has_dn) {
        CHK(prep(c, x_h, ldxh, H, nullptr, L.Hpad, L.hid_tr[1], L.flags_h, nullptr, c.rt));
        CHK(rows(e_v, ldev, V, L.vis_tr[1], has_up ? nullptr : L.vis_tr[0], L.cs_vpos));
    }
    BackpropFinishArgs b;
    memset(&b, 0, sizeof(b));
    b.P = L.P; b.H = H; b.V = V; b.lr = o->lr; b.mom = o->momentum; b.n = (float)B;
    if (has_up) { b.part_h = L.cs_hpos; b.hid_bias = d->hid_bias; b.hb_m = d->hb_m; }
    if (has_dn) { b.part_v = L.cs_vpos; b.vis_bias = d->vis_bias; b.vb_m = d->vb_m; }
    hipLaunchKernelGGL(backprop_finish, dim3(cdiv(std::max(V, H), 256)), dim3(256), 0, c.s, b);
    HIPCHK(hipGetLastError());
    // ---- weight pass: W_m = mom W_m + lr ((x_v^T e_h + e_v^T x_h) / B - wd W), W += W_m
    if (!has_dn) {
        L.vis_tr[1] = L.vis_tr[0];                   // vneg = vpos = x_v against the zero planes of hid_tr[1]
        return launch_assoc(c, 0, o, one, L.flags, c.rt, (float)B, nullptr, nullptr);
    }
    if (!has_up) {
        L.hid_tr[0] = L.hid_tr[1];                   // hpos = hneg = x_h against the zero planes of vis_tr[0]
        return launch_assoc(c, 0, o, c.rt, nullptr, c.rt, (float)B, nullptr, nullptr);
    }
    return launch_assoc(c, 0, o, one, L.flags, c.rt, (float)B, nullptr, nullptr);
}
