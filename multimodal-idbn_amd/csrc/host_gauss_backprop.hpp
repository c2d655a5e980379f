// host_gauss_backprop.hpp -- host side, part 6 (included by engine.hip behind the Gaussian calls): one back-propagation step through
// a Gaussian visible layer (imdbn_rbm_gauss_backprop_step; kernels_gauss_backprop.hpp).
//
// Launches, plain, on the caller's stream, in this order:
//   with the down pair: prep_operand of x_h and the logits-only down propagation WITH the bias -- the two launches of
//     imdbn_rbm_gauss_prop_down, the mean m bit for bit;
//   gauss_bp_rows over v (and m);
//   for err_h_out: prep_operand of e_0, a memset node for the zero bias, the logits-only up propagation without a bias and
//     backprop_apply (the sequence of host_backprop.hpp);
//   when applying: with the up pair prep_operand of u (its planes) and backprop_rows of e_h, with the down pair prep_operand of x_h
//     (its planes); then the weight pass and gauss_bp_finish.
// The weight pass.  With the up pair the log-variance needs r_i = sum_j W_ij S_ij, so the update kernel runs in its statistics mode
// (launch_assoc(mode_stats = 1): S into the scratch) and gauss_apply streams S, W and W_m once, as imdbn_rbm_gauss_cd_step does.  With
// the down pair alone no r is needed and the update kernel applies the step itself, as imdbn_rbm_backprop_step does.  Slots:
//   up pair    (vpos, hpos) = (u, e_h)        vis_tr[0] by prep_operand (with its exactness map), hid_tr[0] by backprop_rows
//   down pair  (vneg, hneg) = (e_0, x_h)      vis_tr[1] by gauss_bp_rows, hid_tr[1] by prep_operand
//   up only:   hid_tr[1] = zeros (backprop_rows), the visible slot 1 aliased to slot 0
//   down only: vis_tr[0] = zeros (gauss_bp_rows), the hidden slot 0 aliased to slot 1
// Every launch that reads W, a bias or logvar on entry precedes the launch that writes it: the weight pass and gauss_bp_finish come last.
#pragma once

// scratch = [S V H | mean B V | e_0 B V | u B V | colsum e_0, q, t: P V each | row_part ctiles V | loss partials 3 n_loss], every piece
// padded to 4 floats; P = Bp / 8 (the rows kernel covers the padded rows), the row partials sized as gauss_scratch sizes them
struct GaussBpScratch { size_t mean, e0, u, pe, pq, pt, row_part, loss, total; int P, n_loss; };
static GaussBpScratch gauss_bp_scratch(int V, int H, int B) {
    auto r4 = [](size_t n) { return (n + 3) / 4 * 4; };
    GaussBpScratch g;
    g.P = rup(std::max(B, 1), 64) / 8; g.n_loss = cdiv(V, 256) * g.P;
    const size_t bv = r4((size_t)B * V), pv = r4((size_t)g.P * V);
    const int ctiles = std::max(centered_plan(V, H, false).ctiles, centered_plan(V, H, true).ctiles);
    g.mean = centered_dw_floats(V, H); g.e0 = g.mean + bv; g.u = g.e0 + bv;
    g.pe = g.u + bv; g.pq = g.pe + pv; g.pt = g.pq + pv;
    g.row_part = g.pt + pv; g.loss = g.row_part + r4((size_t)ctiles * V); g.total = g.loss + r4((size_t)3 * g.n_loss);
    return g;
}

static int gauss_backprop_step(const imdbn_rbm_desc* d, float* logvar, float* logvar_m, const float* v, int64_t ldv, const float* e_h, int64_t ldeh,
                        const float* x_h, int64_t ldxh, int B, const imdbn_cd_opts* o, float lr_z, float z_lo, float z_hi,
                        float* err_h_out, int64_t ldoh, float* loss_out, float* scratch, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!d) return fail(IMDBN_E_INVALID, "gauss_backprop_step: null descriptor");
    CHK(gauss_check("gauss_backprop_step", d, false, logvar));
    if (!v || !scratch) return fail(IMDBN_E_INVALID, "gauss_backprop_step: null %s", !v ? "v" : "scratch");
    const bool has_up = e_h != nullptr, has_dn = x_h != nullptr;
    if (!has_up && !has_dn) return fail(IMDBN_E_INVALID, "gauss_backprop_step: no pair at all (e_h and x_h are NULL)");
    if (err_h_out && !has_dn) return fail(IMDBN_E_INVALID, "gauss_backprop_step: err_h_out %p without the down pair", (const void*)err_h_out);
    if (loss_out && !has_dn) return fail(IMDBN_E_INVALID, "gauss_backprop_step: loss_out %p without the down pair", (const void*)loss_out);
    if (!o && !err_h_out && !loss_out) return fail(IMDBN_E_INVALID, "gauss_backprop_step: opts == NULL and both outputs NULL: nothing to do");
    const int V = d->V, H = d->H;
    if (ldv < V) return fail(IMDBN_E_INVALID, "gauss_backprop_step: ldv %lld < %d", (long long)ldv, V);
    if (has_up && ldeh < H) return fail(IMDBN_E_INVALID, "gauss_backprop_step: ldeh %lld < %d", (long long)ldeh, H);
    if (has_dn && ldxh < H) return fail(IMDBN_E_INVALID, "gauss_backprop_step: ldxh %lld < %d", (long long)ldxh, H);
    if (err_h_out && ldoh < H) return fail(IMDBN_E_INVALID, "gauss_backprop_step: ldoh %lld < %d", (long long)ldoh, H);
    if (B < 1) return fail(IMDBN_E_INVALID, "gauss_backprop_step: B = %d rows", B);
    if (!(lr_z == lr_z)) return fail(IMDBN_E_INVALID, "gauss_backprop_step: lr_z = %g", (double)lr_z);
    if (!(z_lo <= z_hi)) return fail(IMDBN_E_INVALID, "gauss_backprop_step: clamp [%g, %g] is empty", (double)z_lo, (double)z_hi);
    if (lr_z != 0.0f && !logvar_m) return fail(IMDBN_E_INVALID, "gauss_backprop_step: null logvar_m with lr_z = %g", (double)lr_z);
    if (o) {
        if (!d->W_m || !d->hb_m || !d->vb_m)
            return fail(IMDBN_E_INVALID, "gauss_backprop_step: null momentum buffer (W_m %p, hb_m %p, vb_m %p)", (const void*)d->W_m,
                        (const void*)d->hb_m, (const void*)d->vb_m);
        if (o->cd_k || o->sparsity || o->next_data || o->next_slot || o->data_slot || o->next_binary || o->fwd_out)
            return fail(IMDBN_E_INVALID, "gauss_backprop_step: cd_k, sparsity, the prefetch fields and fwd_out must be zero (cd_k %d, sparsity %d, "
                        "next_data %p, next_slot %d, data_slot %d, next_binary %d, fwd_out %p)", o->cd_k, o->sparsity, (const void*)o->next_data,
                        o->next_slot, o->data_slot, o->next_binary, (const void*)o->fwd_out);
    }
    imdbn_rbm_desc dz = *d;                          // the descriptor the propagations see: its hidden bias becomes zeros for err_h
    Ctx c(&dz, nullptr, stream);
    CHK(setup(c, B, ws, ws_bytes));
    Layout& L = c.L;
    const GaussBpScratch g = gauss_bp_scratch(V, H, B);
    const int one = c.nw == 1 ? 1 : 0;               // operand terms of a propagation: one in FAST mode, else by the exactness map
    const bool learn_z = o && lr_z != 0.0f;
    float* mean = scratch + g.mean;
    float* e0 = scratch + g.e0;
    float* u = scratch + g.u;
    // ---- the decoder's mean, from the parameters on entry: the launches of imdbn_rbm_gauss_prop_down
    if (has_dn) {
        FinishArgs f = new_finish();
        f.logits_only = 1;
        f.out_prob = mean; f.ld_prob = V;
        CHK(prep_prop(c, false, x_h, ldxh, f));
    }
    {   // ---- one pass over v (and m)
        GaussBpRowsArgs a;
        memset(&a, 0, sizeof(a));
        a.B = B; a.Bp = L.Bp; a.V = V; a.v = v; a.ldv = ldv; a.bias = d->vis_bias; a.logvar = logvar; a.terms = c.ht;
        if (has_dn) {
            a.m = mean; a.ldm = V;
            if (err_h_out) a.e0 = e0;
            if (o) { a.tr_e0 = L.vis_tr[1]; a.part_e0 = scratch + g.pe; }
            if (o && !has_up) a.tr_zero = L.vis_tr[0];
            if (learn_z) a.part_q = scratch + g.pq;
            if (learn_z && has_up) a.part_t = scratch + g.pt;
            if (loss_out) a.loss_part = scratch + g.loss;
        }
        if (has_up && o) a.u = u;
        hipLaunchKernelGGL(gauss_bp_rows, dim3(cdiv(V, 256), g.P), dim3(256), 0, c.s, a);
        HIPCHK(hipGetLastError());
    }
    GaussBpFinishArgs b;
    memset(&b, 0, sizeof(b));
    b.V = V; b.H = H; b.P = L.P; b.n = (float)B;
    b.loss_part = scratch + g.loss; b.n_loss = g.n_loss; b.loss_out = loss_out;
    const dim3 fin_grid(cdiv(std::max(V, H), 256) + 1);
    // ---- the error at the hidden layer's pre-activations: (e_0 W) x_h (1 - x_h)
    if (err_h_out) {
        HIPCHK(hipMemsetAsync(L.cs_hneg, 0, (size_t)H * sizeof(float), c.s));
        dz.hid_bias = L.cs_hneg;
        CHK(prep(c, e0, V, V, L.vis_rm[0], L.Vpad, nullptr, L.flags));
        FinishArgs f = new_finish();
        f.logits_only = 1;
        f.out_prob = L.f_h; f.ld_prob = H;
        CHK(prop(c, true, OpIn{L.vis_rm[0], one, L.flags}, f));
        BackpropApplyArgs a;
        memset(&a, 0, sizeof(a));
        a.B = B; a.N = H; a.q = L.f_h; a.ldq = H; a.x = x_h; a.ldx = ldxh; a.out = err_h_out; a.ldo = ldoh;
        hipLaunchKernelGGL(backprop_apply, dim3(cdiv(H, 256), cdiv(B, 8)), dim3(256), 0, c.s, a);
        HIPCHK(hipGetLastError());
    }
    if (!o) {
        if (loss_out) {                              // the loss block alone: no bias, no logvar
            hipLaunchKernelGGL(gauss_bp_finish, fin_grid, dim3(256), 0, c.s, b);
            HIPCHK(hipGetLastError());
        }
        return 0;
    }
    // ---- the operands of the weight pass and the column partials of the hidden bias
    if (has_up) {
        CHK(prep(c, u, V, V, nullptr, L.Vpad, L.vis_tr[0], L.flags, nullptr, c.rt));
        BackpropRowsArgs a;
        memset(&a, 0, sizeof(a));
        a.B = B; a.Bp = L.Bp; a.N = H; a.e = e_h; a.lde = ldeh; a.tr_e = L.hid_tr[0]; a.tr_zero = has_dn ? nullptr : L.hid_tr[1];
        a.terms = c.ht; a.colsum_part = L.cs_hpos;
        hipLaunchKernelGGL(backprop_rows, dim3(cdiv(H, 256), L.Bp / 8), dim3(256), 0, c.s, a);
        HIPCHK(hipGetLastError());
        b.part_h = L.cs_hpos; b.hid_bias = d->hid_bias; b.hb_m = d->hb_m;
    }
    if (has_dn) {
        CHK(prep(c, x_h, ldxh, H, nullptr, L.Hpad, L.hid_tr[1], L.flags_h, nullptr, c.rt));
        b.part_e0 = scratch + g.pe; b.vis_bias = d->vis_bias; b.vb_m = d->vb_m;
    }
    b.lr = o->lr; b.mom = o->momentum; b.lr_z = lr_z; b.z_lo = z_lo; b.z_hi = z_hi;
    if (learn_z) {
        b.logvar = logvar; b.logvar_m = logvar_m;
        if (has_dn) b.part_q = scratch + g.pq;
        if (has_dn && has_up) b.part_t = scratch + g.pt;
    }
    // ---- weight pass: W_m = mom W_m + lr ((u^T e_h + e_0^T x_h) / B - wd W), W += W_m
    if (!has_up) {
        L.hid_tr[0] = L.hid_tr[1];                   // hpos = hneg = x_h against the zero planes of vis_tr[0]
        CHK(launch_assoc(c, 0, o, c.rt, nullptr, c.rt, (float)B, nullptr, nullptr));
    } else {
        if (!has_dn) L.vis_tr[1] = L.vis_tr[0];      // vneg = vpos = u against the zero planes of hid_tr[1]
        CHK(launch_assoc(c, 1, o, one, L.flags, c.rt, 1.0f, scratch));
        const bool vec4 = c.r.vec4 && (((uintptr_t)d->W_m | (uintptr_t)scratch) & 15) == 0;
        const CenteredPlan p = centered_plan(V, H, vec4);
        GaussArgs a;
        memset(&a, 0, sizeof(a));
        a.W = d->W; a.Wm = d->W_m; a.ldw = d->ldw; a.V = V; a.H = H; a.S = scratch;
        a.lr = o->lr; a.mom = o->momentum; a.wd = o->weight_decay; a.n = (float)B;
        a.rps = p.rps; a.tw = p.tw; a.nstripes = p.nstripes; a.ctiles = p.ctiles;
        a.row_part = scratch + g.row_part;
        if (vec4) hipLaunchKernelGGL(gauss_apply<true>, dim3(p.ctiles, p.nstripes), dim3(256), 0, c.s, a);
        else      hipLaunchKernelGGL(gauss_apply<false>, dim3(p.ctiles, p.nstripes), dim3(256), 0, c.s, a);
        HIPCHK(hipGetLastError());
        if (learn_z) { b.row_part = scratch + g.row_part; b.ctiles = p.ctiles; }
    }
    hipLaunchKernelGGL(gauss_bp_finish, fin_grid, dim3(256), 0, c.s, b);
    HIPCHK(hipGetLastError());
    return 0;
}
