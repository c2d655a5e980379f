// host_delta.hpp -- host side, part 4 (included by engine.hip after host_update.hpp): one delta-rule step of a directed layer
// (imdbn_rbm_delta_step; kernels_delta.hpp).
//
// Launches, plain, on the caller's stream: prep_operand of `in` (the row-major form the propagation reads and, when applying, the
// transposed planes the weight pass reads), the logits-only propagation (f_h for UP, f_v[0] for DOWN), delta_rows, delta_finish, and
// when applying the update kernel through launch_assoc with the pairs (in, target) and (in, p): the output side's slot 0 holds the
// planes of `target`, its slot 1 those of -p, and the input side reads ITS slot 0 in both phases -- the Layout of this call aliases
// slot 1 to slot 0 on the input side (the copy in Ctx; the workspace is not touched by that).  The update kernel's own bias rows are
// off (bias == nullptr): delta_finish moves the predicting bias only.
// Scratch: the row partials of the log-probability sit in L.partial, which the propagation has finished with (one stream):
// ceil(N / 64) Bp doubles <= Bp max(N, 32) floats, the least make_layout gives that buffer.
#pragma once

int delta_step(const imdbn_rbm_desc* d, int dir, const float* in, int64_t ldi, const float* target, int64_t ldt, int B,
               const imdbn_cd_opts* o, double* out_rowlp, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!d) return fail(IMDBN_E_INVALID, "delta_step: null descriptor");
    if (!in || !target) return fail(IMDBN_E_INVALID, "delta_step: null %s", !in ? "in" : "target");
    if (dir != IMDBN_DELTA_UP && dir != IMDBN_DELTA_DOWN) return fail(IMDBN_E_INVALID, "delta_step: dir = %d outside {0, 1}", dir);
    CHK(check_desc(d, false));
    const bool up = dir == IMDBN_DELTA_UP;
    const int Nin = up ? d->V : d->H, N = up ? d->H : d->V;
    if (ldi < Nin) return fail(IMDBN_E_INVALID, "delta_step: ldi %lld < %d", (long long)ldi, Nin);
    if (ldt < N) return fail(IMDBN_E_INVALID, "delta_step: ldt %lld < %d", (long long)ldt, N);
    if (B < 1) return fail(IMDBN_E_INVALID, "delta_step: B = %d rows", B);
    if (!o && !out_rowlp) return fail(IMDBN_E_INVALID, "delta_step: opts == NULL and out_rowlp == NULL: nothing to do");
    if (o) {
        if (!d->W_m || !d->hb_m || !d->vb_m) return fail(IMDBN_E_INVALID, "delta_step: null momentum buffer (W_m %p, hb_m %p, vb_m %p)",
                                                         (const void*)d->W_m, (const void*)d->hb_m, (const void*)d->vb_m);
        if (o->cd_k || o->sparsity || o->next_data || o->next_slot || o->data_slot || o->next_binary || o->fwd_out)
            return fail(IMDBN_E_INVALID, "delta_step: cd_k, sparsity, the prefetch fields and fwd_out must be zero (cd_k %d, sparsity %d, next_data %p, "
                        "next_slot %d, data_slot %d, next_binary %d, fwd_out %p)", o->cd_k, o->sparsity, (const void*)o->next_data, o->next_slot,
                        o->data_slot, o->next_binary, (const void*)o->fwd_out);
    }
    if (!up && d->n_groups > 0) return fail(IMDBN_E_UNSUPPORTED, "delta_step: DOWN with softmax groups is not supported (n_groups = %d)", d->n_groups);
    Ctx c(d, nullptr, stream);
    CHK(setup(c, B, ws, ws_bytes));
    Layout& L = c.L;
    // in -> operand forms of its side; the planes only when the weight pass follows
    bf16_t* in_tr = up ? L.vis_tr[0] : L.hid_tr[0];
    int* in_flags = up ? L.flags : L.flags_h;
    bf16_t* in_rm = up ? L.vis_rm[0] : L.hid_rm;
    CHK(prep(c, in, ldi, Nin, in_rm, up ? L.Vpad : L.Hpad, o ? in_tr : nullptr, in_flags, nullptr, c.rt));
    float* logits = up ? L.f_h : L.f_v[0];
    {
        FinishArgs f = new_finish();
        f.logits_only = 1;
        f.out_prob = logits; f.ld_prob = N;
        CHK(prop(c, up, OpIn{in_rm, c.nw == 1 ? 1 : 0, in_flags}, f));
    }
    DeltaArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.Bp = L.Bp; a.N = N;
    a.a = logits; a.lda = N; a.t = target; a.ldt = ldt;
    if (o) {
        a.tr_t = up ? L.hid_tr[0] : L.vis_tr[0];
        a.tr_p = up ? L.hid_tr[1] : L.vis_tr[1];
        a.terms = c.ht;
        a.colsum_part = up ? L.cs_hpos : L.cs_vpos;
        a.bias = up ? d->hid_bias : d->vis_bias;
        a.bias_m = up ? d->hb_m : d->vb_m;
        a.lr = o->lr; a.mom = o->momentum; a.n = (float)B;
    }
    if (out_rowlp) { a.lp_part = (double*)L.partial; a.out_rowlp = out_rowlp; }
    hipLaunchKernelGGL(delta_rows, dim3(cdiv(N, 256), L.Bp / 8), dim3(256), 0, c.s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(delta_finish, dim3(cdiv(std::max(N, B), 256)), dim3(256), 0, c.s, a);
    HIPCHK(hipGetLastError());
    if (!o) return 0;
    // weight pass: W_m = mom W_m + lr ((in^T target - in^T p) / B - wd W), W += W_m, in the [V][H] layout whichever side predicts
    if (up) {
        L.vis_tr[1] = L.vis_tr[0];                  // vneg = vpos = in; hpos = target, hneg = -p (stored negated, as the kernel expects)
        return launch_assoc(c, 0, o, c.nw == 1 ? 1 : 0, L.flags, c.rt, (float)B, nullptr, nullptr);
    }
    L.hid_tr[1] = L.hid_tr[0];                      // hpos = in and, un-negated, hneg = in: the sign rides on the visible side, vneg = -p
    return launch_assoc(c, 0, o, c.rt, nullptr, c.rt, (float)B, nullptr, nullptr);
}
