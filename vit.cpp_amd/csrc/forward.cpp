// forward.cpp -- the forward pass of the MI355X ViT engine on an execution context (context.h).
// Replaces vit_encode_image + the compute half of vit_predict of the reference (vit.cpp:718-941, 1004-1040): the batch is n images, cut
// into sub-batches that run beside each other on HIP streams, and the ~90 launches of a forward are enqueued without host synchronisation.
#include "context.h"

namespace {

// One GEMM launch (+ its profile record).  `fused` != nullptr: W is that q4_0 matrix and the GEMM expands the blocks in its own LDS-fill path
// (small batches).  `fix`: the GemmLn of the LayerNorm-fusing GEMM that produced A (GemmArgs::fix); when the kernel this shape selects cannot
// recompute the row blocks that GEMM left behind, they are fixed by a launch of their own first.  `rows_alg`: the rows the profile counts
// (0 = a.M_real).
int gemm(vitx_ctx *c, hipStream_t st, int pc, int epi, GemmArgs a, const QuantW *fused = nullptr, const GemmLn *ln = nullptr,
         const GemmLn *fix = nullptr, long hilo_off = 0, int rows_alg = 0) {
    a.hilo_off = hilo_off; a.ln = ln;
    if (fix) {
        if (!fused && gemm_fix_capable(*c->tune, a)) a.fix = fix;
        else {
            ProfScope ps(c, st, PC_LAYERNORM, 0, 0);
            HIP_TRY(launch_layernorm_fixup(c->dtype, fix->x, fix->w, fix->b, fix->out, a.M, a.K, fix->eps, fix->todo, fix->epoch, st));
        }
    }
    // algorithmic work of the launch: the REAL rows (a LayerNorm-fusing launch computes and stores its pad rows too -- GemmLn -- but they are not work
    // the forward asked for: r03 counted them, +0.46 % on the fc2 figure)
    double flops, bytes;
    gemm_work(epi, rows_alg > 0 ? rows_alg : a.M_real, a.N, a.K, fused != nullptr, ln != nullptr, &flops, &bytes);
    ProfScope ps(c, st, pc, flops, bytes);
    if (fused) {
        a.W = fused->blocks; a.Wscale = fused->scales;
        HIP_TRY(launch_gemm_q4(c->dtype, epi, a, st));
        return VITX_OK;
    }
    HIP_TRY(launch_gemm(*c->tune, c->dtype, epi, a, st));
    return VITX_OK;
}

// One MXFP8 GEMM (gemm_mx8.hip) on rows A / As of `rows` rows; the profile counts operand bytes as 1 per element + 1 per 32 (scales)
int gemm_mx(vitx_ctx *c, hipStream_t st, int pc, int epi, const uint8_t *A, const uint8_t *As, const MxW &w, const float *bias, void *out, uint8_t *out_s,
            int rows, int ldo) {
    const GemmArgs a = dense_gemm(A, w.q, bias, out, rows, rows, w.N, w.n_pad, w.k_pad, ldo);
    constexpr double mxb = 1.0 + 1.0 / kMxBlock;
    double bytes = (double)rows * w.k_pad * mxb + (double)w.n_pad * w.k_pad * mxb + (epi == EPI_BIAS_GELU ? (double)rows * ldo * mxb : (double)rows * w.N * epi_out_bytes(epi));
    if (epi == EPI_BIAS_RESID) bytes += (double)rows * w.N * 4;
    ProfScope ps(c, st, pc, 2.0 * rows * (double)w.N * w.K, bytes);
    HIP_TRY(launch_gemm_mx8(epi, a, As, w.s, out_s, st));
    return VITX_OK;
}

// Attention maps of layer il (vitx_attn_enable) for the n images first_img .. of a sub-batch, from the QKV its qkv projection has just written
// (lo_off: the parity mode's lo plane).  The kernels only read QKV and write the context's map buffers at the images' global positions.
// Rollout: A^_l goes to roll[l & 1] and becomes R_l = A^_l R_(l-1) in place; the last layer contributes row 0 of its factor only,
// built from its class-token maps -- the rows a cls_tail context still has.
static int attention_maps(vitx_ctx *c, hipStream_t st, const void *qkv, long lo_off, int il, int first_img, int n) {
    const AttnMaps &am = *c->attn;
    const int N = c->N, D = c->D, H = c->H, L = c->L, fpi = am.fpi;
    const size_t NN = (size_t)N * N;
    const bool rollout = (am.flags & VITX_ATTN_ROLLOUT) != 0;
    float *const roll[2] = {am.roll[0].as<float>(), am.roll[1].as<float>()};
    const double qk_bytes = (double)n * N * 2 * D * 2 * (lo_off ? 2 : 1);        // q and k of every token (both planes in the parity mode)
    float *out_img = am.out.as<float>() + (size_t)first_img * fpi;
    float *cls = nullptr;
    long cls_stride = 0;
    if ((am.mask >> il) & 1) {
        cls = out_img + (size_t)layer_slot(am.mask, il) * H * N; cls_stride = fpi;
    } else if (rollout && il + 1 == L) {
        cls = am.cls_last.as<float>() + (size_t)first_img * H * N; cls_stride = (long)H * N;
    }
    if (cls) {
        ProfScope ps(c, st, PC_ATTN_MAP, 2.0 * n * (double)N * D, qk_bytes / 2 + (double)n * H * N * 4);
        HIP_TRY(launch_attention_cls_map(c->dtype, qkv, lo_off, cls, cls_stride, n, N, D, H, st));
    }
    if (!rollout) return VITX_OK;
    if (il + 1 < L) {
        float *a = roll[il & 1] + (size_t)first_img * NN;
        {
            ProfScope ps(c, st, PC_ATTN_MAP, 2.0 * n * (double)NN * D, qk_bytes + (double)n * NN * 4);
            HIP_TRY(launch_attention_head_mean(c->dtype, qkv, lo_off, a, n, N, D, H, true, st));
        }
        if (il > 0) {
            ProfScope ps(c, st, PC_ATTN_MAP, 2.0 * n * (double)NN * N, (double)n * NN * 12);
            HIP_TRY(launch_rollout_step(a, roll[(il + 1) & 1] + (size_t)first_img * NN, n, N, st));
        }
        return VITX_OK;
    }
    const float *r = L > 1 ? roll[(L - 2) & 1] + (size_t)first_img * NN : nullptr;
    ProfScope ps(c, st, PC_ATTN_MAP, 2.0 * n * (double)NN, (double)n * NN * 4);
    HIP_TRY(launch_rollout_row(cls, cls_stride, r, out_img + (fpi - N), fpi, n, N, H, st));
    return VITX_OK;
}

// The forward of one sub-batch: the n images first_img .. on slice `sl` and stream `st`.  The members are what every step shares; the member
// functions are the steps, each one launch (or one group of launches) + its profile record.  run() enqueues them in order.
struct SliceForward {
    vitx_ctx *c; vitx_ctx::Slice &sl; hipStream_t st; int first_img, n;
    const WeightSet &ws = *c->wset;
    const size_t si = &sl - &c->slices[0];                          // the slice's index: the per-slice buffers of the opt-in outputs
    const HeadLaunch head{*c->tune, c->dtype, st, c};               // how the head sequences (heads.cpp) launch, recorded in this context's profile
    const int D = c->D, N = c->N, tm = c->tm, tn = c->tn, dt = c->dtype;
    const int F = c->F, F1 = c->F1;                                 // MLP widths: fc2's K and fc1's N (4 D both, or F and 2 F of a `glu` context)
    static constexpr double eb = 2.0;                               // operand bytes
    const int M_real = n * N, M = round_up(M_real, tm);            // token rows
    const long lo_off = c->prec_attn ? (long)M * 3 * D : 0;         // F16 parity mode: the lo plane of q, k, v right behind this sub-batch's hi plane (elements)
    const int Dk = mx_k_pad(D);
#ifdef VITX_LAB
    const int skip = c->skip;
#else
    static constexpr int skip = 0;
#endif
    bool fuse = false;                 // LayerNorm fusion, decided per forward (run)
    // The rows a layer carries past its attention (proj + norm2, fc1, fc2 + the next norm1): every token row of the sub-batch, or -- the last
    // layer of a cls_tail context (vitx_ctx::cls_tail) -- the n class-token rows Xc, padded to Mc, never LayerNorm-fused
    struct Rows { float *X; int M, M_real, pc_proj, pc_fc1, pc_fc2; bool fuse; };
    GemmLn fix_u{}, fix_u2{};          // fused LayerNorm launches whose output (U / U2) has not been consumed yet
    // the current layer's matrices: Wl = expanded operand-type (the file's, or the slice's just-in-time scratch), Fl = those the fused q4_0 kernel takes
    const void *Wl[W_PER_LAYER]; const QuantW *Fl[W_PER_LAYER];
    // residual-stream trace: copy X of the traced images that live in this sub-batch (stage 0 = after patch embedding, il + 1 = after layer il)
    int trace(int stage) {
        const size_t per = (size_t)c->N * c->D;
        for (size_t k = 0; k < c->trace_ids.size(); ++k) {
            const int id = c->trace_ids[k];
            if (id < first_img || id >= first_img + n) continue;
            HIP_TRY(hipMemcpyAsync(c->trace_buf + ((size_t)stage * c->trace_ids.size() + k) * per, sl.X + (size_t)(id - first_img) * per, per * 4, hipMemcpyDeviceToDevice, st));
        }
        return VITX_OK;
    }
    // embeddings and token features of layer il (vitx_feat_enable), from the residual stream its fc2 has just completed: one launch writes this
    // sub-batch's images straight into the packed per-image layout.  cls_rows: X is the compact class rows Xc of the class-rows-only last layer.
    // z != nullptr (the last layer of a pooled-head context): the same launch also writes the head's operand rows RNE(cls) ‖ RNE(mean), with or
    // without features of that layer selected -- one pass over the residual stream serves both.
    int features(int il, bool cls_rows, void *z = nullptr) {
        const Features *ft = c->feat.get();
        const bool sel = ft && ft->selects(il);
        if (!sel && !z) return VITX_OK;
        const int fl = sel ? ft->flags : 0, Tp = c->Tp;
        float *o_cls = nullptr, *o_mean = nullptr, *o_tok = nullptr;
        if (sel) ft->slots(first_img, il, &o_cls, &o_mean, &o_tok);
        if (c->map) {        // no class row: VITX_FEAT_CLS of such a context is the pooled embedding, written by pooled_tail
            o_cls = nullptr;
            if (!o_mean && !o_tok) return VITX_OK;
        }
        const double rows = (double)n * ((o_cls || z ? 1 : 0) + (o_mean || o_tok || z ? N - Tp : 0));
        ProfScope ps(c, st, sel ? PC_FEATURES : PC_HEAD_POOL, 0, rows * D * 4 + (double)n * D * 4 * ((o_cls ? 1 : 0) + (o_mean ? 1 : 0) + (o_tok ? N - Tp : 0)) + (z ? (double)n * 2 * D * eb : 0.0));
        HIP_TRY(launch_features(cls_rows ? sl.Xc : sl.X, D, cls_rows ? (long)D : (long)N * D, ws.norm_w, ws.norm_b, o_cls, o_mean, o_tok, ft ? ft->fpi : 0,
                                n, cls_rows ? 1 : N, D, c->hp.eps, (fl & VITX_FEAT_L2) != 0, st, cls_rows ? 1 : Tp, z, dt));
        return VITX_OK;
    }
    // The attention-pooling head (VITX_POOL_MAP; include/vitx.h) on the n images of this sub-batch, after the last layer: the pooling pass over the
    // residual stream (attention_pool.hip) -> Mp = RNE(M) [n][H][D]; the value projection, H launches of the short-M GEMM on strided operands (head h
    // reads Mp[:, h, :] and writes columns h d .. (h + 1) d of U); proj -> a (f32, Xc); LayerNorm -> U2; fc1 + activation -> Hbuf; fc2 + residual
    // -> e (Xc, in place); Z = RNE(e) and the VITX_FEAT_CLS feature.  6 + H launches; all but the first work on one row per image.
    int pooled_tail() {
        int rc;
        const int H = c->H, d = D / H, Mc = round_up(n, tm);
        {
            ProfScope ps(c, st, PC_HEAD_POOL, 4.0 * n * H * (double)N * D, (double)M_real * D * 4 + (double)n * H * D * eb);
            HIP_TRY(launch_attention_pool(sl.X, D, (long)N * D, ws.norm_w, ws.norm_b, c->hp.eps, ws.map_u, nullptr, sl.Mp, dt, nullptr, n, N, D, H, st));
        }
        for (int h = 0; h < H; ++h) {
            GemmArgs a = dense_gemm((const char *)sl.Mp + (size_t)h * D * 2, (const char *)ws.map_v_w + (size_t)h * d * D * 2, ws.map_v_b + h * d, (char *)sl.U + (size_t)h * d * 2,
                                    Mc, n, d, round_up(d, 128), D, D);
            a.lda = H * D;
            if ((rc = gemm(c, st, PC_GEMM_TAIL, EPI_BIAS, a))) return rc;
        }
        if ((rc = gemm(c, st, PC_GEMM_TAIL, EPI_BIAS_F32, dense_gemm(sl.U, ws.map_proj_w, ws.map_proj_b, sl.Xc, Mc, n, D, round_up(D, tn), D)))) return rc;
        if ((rc = layernorm(sl.Xc, D, ws.map_ln_w, ws.map_ln_b, sl.U2, n))) return rc;
        if ((rc = gemm(c, st, PC_GEMM_TAIL, c->fc1_epi, dense_gemm(sl.U2, ws.map_fc1_w, ws.map_fc1_b, sl.Hbuf, Mc, n, 4 * D, round_up(4 * D, tn), D)))) return rc;
        if ((rc = gemm(c, st, PC_GEMM_TAIL, EPI_BIAS_RESID, dense_gemm(sl.Hbuf, ws.map_fc2_w, ws.map_fc2_b, sl.Xc, Mc, n, D, round_up(D, tn), 4 * D)))) return rc;
        float *o_cls = nullptr, *o_mean, *o_tok;
        const Features *ft = c->feat.get();
        const bool sel = ft && ft->selects(c->L - 1);
        if (sel) ft->slots(first_img, c->L - 1, &o_cls, &o_mean, &o_tok);
        ProfScope ps(c, st, sel && o_cls ? PC_FEATURES : PC_HEAD_POOL, 0, (double)n * D * (4 + eb + (o_cls ? 4 : 0)));
        HIP_TRY(launch_pool_embed(sl.Xc, sl.Z, dt, o_cls, ft ? ft->fpi : 0, ft && (ft->flags & VITX_FEAT_L2), n, D, st));
        return VITX_OK;
    }
    // The four heads after the classifier, each one sequence of heads.cpp on this slice's buffers, its results at the images' global positions.
    // lg: this sub-batch's f32 logits rows (row stride ldl).  Zero-shot (vitx_zeroshot_set) embeds the pooled embedding e of an attention-pooling
    // head, else the logits row; nearest neighbours (vitx_nn_set) the logits row, or the head GEMM's operand rows Z.
    int heads(const float *lg, long ldl) {
        if (const ZeroShot *zs = c->zs.get()) {
            float *out = zs->out.as<float>() + (size_t)first_img * 2 * zs->K;
            HIP_TRY(head_zeroshot(head, c->map ? sl.Xc : lg, c->map ? (long)D : ldl, zs->a[si].p, zs->bank.p, zs->zero.as<float>(), zs->acc[si].as<float>(), out, out + zs->K,
                                  2L * zs->K, n, zs->K, zs->E, zs->kind, zs->scale, zs->bias));
        }
        if (const Gallery *nn = c->nn.get()) {
            const bool operand = nn->source != VITX_NN_LOGITS;
            HIP_TRY(head_nearest(head, operand ? (const void *)sl.Z : lg, operand ? (long)nn->E : ldl, operand, nn->a[si].p, nn->gallery.p, nn->zero.as<float>(), nn->acc[si].as<float>(),
                                 nn->state[si].p, nn->G, nn->E, nn->k, Gallery::kChunk, nn->labels.as<int>(), nn->nlabels, nn->T, nn->out.as<float>() + (size_t)first_img * nn->k * 2,
                                 nn->vote ? nn->vote.as<float>() + (size_t)first_img * nn->nlabels : nullptr, n));
        }
        const size_t Np = N - c->Tp;
        if (const DenseHead *dn = c->dense.get()) {
            const size_t px = (size_t)dn->oh * dn->ow;
            HIP_TRY(head_dense(head, dn->a[si].p, dn->W.p, dn->bias.as<float>(), dn->acc[si].as<float>(), n, c->gh, c->gw, dn->K, dn->Dc, dn->oh, dn->ow,
                               dn->labels.as<uint8_t>() + (size_t)first_img * px, dn->score ? dn->score.as<float>() + (size_t)first_img * px : nullptr,
                               dn->logits ? dn->logits.as<float>() + (size_t)first_img * Np * dn->K : nullptr));
        }
        if (const DepthHead *dp = c->depth.get()) {
            const size_t px = (size_t)dp->oh * dp->ow, fpx = (size_t)dp->u * c->gh * dp->u * c->gw;
            const bool cls = (bool)dp->Wc;
            HIP_TRY(head_depth(head, dp->a[si].p, dp->Wp.p, dp->zero.as<float>(), dp->acc[si].as<float>(), cls ? dp->ac[si].p : nullptr, dp->Wc.p, dp->bias.as<float>(),
                               cls ? dp->o[si].as<float>() : nullptr, dp->bins.as<float>(), n, c->gh, c->gw, dp->K, dp->Dc, dp->u, dp->oh, dp->ow, dp->lo, dp->hi,
                               dp->fine.as<float>() + (size_t)first_img * fpx, dp->depth.as<float>() + (size_t)first_img * px,
                               dp->logits ? dp->logits.as<float>() + (size_t)first_img * Np * dp->K : nullptr, dp->off ? dp->off.as<float>() + (size_t)first_img * dp->K : nullptr));
        }
        return VITX_OK;
    }
    // The operand rows of the dense and the depth head, as layer il finishes (where features(il, ..) is called).  head_rows, the one step: `rows` rows of
    // the f32 residual stream (x, ldx, group, gstride as launch_layernorm reads them) -- their final norm through the stand-alone LayerNorm (no kernel
    // of its own), or, raw, through the streaming conversion -- rounded to the operand type into y, rows of Dc elements: a column slot of compact rows.
    int head_rows(int pc, bool norm, const float *x, long ldx, void *y, int Dc, int rows, int group = 1, long gstride = 0) {
        ProfScope ps(c, st, pc, 0, (double)rows * D * (4 + eb));
        if (norm) HIP_TRY(launch_layernorm(dt, x, ldx, ws.norm_w, ws.norm_b, y, Dc, rows, D, c->hp.eps, st, group, gstride));
        else HIP_TRY(launch_depth_rows(dt, x, ldx, y, Dc, rows, D, st, group, gstride));
        return VITX_OK;
    }
    // the patch rows of this sub-batch's images into columns slot * D .. of h's operand rows [n * Np][Dc]
    int patch_rows(const PatchHead &h, int il, int pc, bool norm) {
        const int Np = N - c->Tp;
        return head_rows(pc, norm, sl.X + (size_t)c->Tp * D, D, h.a[si].as<char>() + h.col(il, D) * 2, h.Dc, n * Np, Np, (long)N * D);
    }
    // the dense head (vitx_dense_set) reads the final norm; the depth head (vitx_depth_set) the raw stream or (VITX_DEPTH_NORM) the final norm, and
    // with a class half the class-token row of every image the same way (one row per image)
    int patch_head_rows(int il) {
        int rc;
        if (c->dense && c->dense->selects(il) && (rc = patch_rows(*c->dense, il, PC_DENSE, true))) return rc;
        const DepthHead *dp = c->depth.get();
        if (!dp || !dp->selects(il)) return VITX_OK;
        const bool norm = (dp->flags & VITX_DEPTH_NORM) != 0;
        if ((rc = patch_rows(*dp, il, PC_DEPTH, norm))) return rc;
        return dp->Wc ? head_rows(PC_DEPTH, norm, sl.X, (long)N * D, dp->ac[si].as<char>() + dp->col(il, D) * 2, dp->Dc, n) : VITX_OK;
    }
    // Quantised matrices (block form in HBM): a q4_0 GEMM with few rows expands the blocks in its own LDS-fill path; everything else
    // is expanded just in time, one launch per layer, into the slice's scratch and then streamed by the wide-tile kernels.
    bool fused_ok(const QuantW &q, int rows) const { return q.blocks && q.type == T_Q4_0 && rows <= c->q4_fused_rows && rows % 128 == 0 && q.n_pad % 128 == 0 && q.K % 64 == 0; }
    int expand(const QuantW *const *qs, void *const *dst, int count) {
        bool done[W_PER_LAYER] = {false, false, false, false};
        for (int k = 0; k < count; ++k) {
            if (done[k] || !qs[k]) continue;
            DequantJob jobs[4]; int nj = 0; double bytes = 0;
            for (int m = k; m < count; ++m) {
                if (done[m] || !qs[m] || qs[m]->type != qs[k]->type) continue;
                jobs[nj++] = DequantJob{qs[m]->blocks, qs[m]->scales, dst[m], qs[m]->N, qs[m]->n_pad, qs[m]->K / 32};
                bytes += (double)qs[m]->N * qs[m]->K / 32 * type_block_bytes(qs[m]->type) + (double)qs[m]->n_pad * qs[m]->K * eb;
                done[m] = true;
            }
            ProfScope ps(c, st, PC_DEQUANT, 0, bytes);
            HIP_TRY(launch_dequant(dt, qs[k]->type, jobs, nj, st));
        }
        return VITX_OK;
    }
    // one LayerNorm launch (+ its profile record): `rows` rows of x (row stride ldx; group > 1: see launch_layernorm) -> y [rows][D]
    int layernorm(const float *x, long ldx, const float *lw, const float *lb, void *y, int rows, int group = 1, long gstride = 0) {
        ProfScope ps(c, st, PC_LAYERNORM, 0, (double)rows * D * (4 + eb));
        HIP_TRY(launch_layernorm(dt, x, ldx, lw, lb, y, D, rows, D, c->hp.eps, st, group, gstride));
        return VITX_OK;
    }
    // VITX_MXFP8: a LayerNorm whose output is the A operand of an MX GEMM (norm1, norm2) writes MX elements + scales
    int layernorm_mx(const float *x, const float *lw, const float *lb, uint8_t *q, uint8_t *s, int rows) {
        if (skip & 2) return VITX_OK;
        ProfScope ps(c, st, PC_LAYERNORM, 0, (double)rows * D * 4 + (double)rows * Dk * (1.0 + 1.0 / kMxBlock));
        HIP_TRY(launch_layernorm_mx8(x, D, lw, lb, q, s, Dk, rows, D, c->hp.eps, st));
        return VITX_OK;
    }
    // residual GEMM (+ the LayerNorm that follows it, fused when r.fuse; otherwise its own launch) -- proj + norm2, fc2 + the next norm1
    // `pend` receives the launch's GemmLn when the LayerNorm was fused: the GEMM that consumes ln_out next gets it as its `fix` argument
    int resid_gemm_ln(const Rows &r, int pc, const void *A, const void *W, const float *bias, int K, const QuantW *fq, const float *lw, const float *lb, void *ln_out, GemmLn *pend) {
        int rc2;
        pend->todo = nullptr;
        GemmArgs a = dense_gemm(A, W, bias, r.X, r.M, r.M_real, D, round_up(D, tn), K);
        if (r.fuse && lw && !fq) {
            GemmLn ln{};
            ln.w = lw; ln.b = lb; ln.x = r.X; ln.out = ln_out; ln.eps = c->hp.eps; ln.sync = sl.ln_sync; ln.todo = sl.ln_todo; ln.fallbacks = sl.ln_todo + sl.ln_blocks;
            if (++c->ln_epoch == 0) c->ln_epoch = 1;
            ln.epoch = c->ln_epoch; ln.timeout = c->ln_timeout; ln.test = c->ln_test;
            a.M_real = r.M;             // the pad rows are stored too; the profile counts the real ones
            if ((rc2 = gemm(c, st, pc, EPI_BIAS_RESID, a, nullptr, &ln, nullptr, 0, r.M_real))) return rc2;
            *pend = ln;
            return VITX_OK;
        }
        if ((rc2 = gemm(c, st, pc, EPI_BIAS_RESID, a, fq))) return rc2;
        if (lw && !(skip & 2)) return layernorm(r.X, D, lw, lb, ln_out, r.M_real);
        return VITX_OK;
    }
    // The front of layer il, shared by the dense and the MX tail: just-in-time dequant, (norm1 of the first layer,) the qkv projection, the
    // (rotary position embeddings,) attention maps, then the attention -- or, tail_now, the class token's attention alone
    int layer_front(int il, const LayerW &w, bool tail_now, const Rows &r) {
        int rc;
        const void *Wfile[W_PER_LAYER] = {w.qkv_w, w.proj_w, w.fc1_w, w.fc2_w};
        for (int k = 0; k < W_PER_LAYER; ++k) { Wl[k] = Wfile[k]; Fl[k] = nullptr; }
        {
            const QuantW *todo[W_PER_LAYER] = {nullptr, nullptr, nullptr, nullptr};
            bool any = false;
            for (int k = 0; k < W_PER_LAYER; ++k) {
                if (!w.q[k].blocks) continue;
                if (fused_ok(w.q[k], k == W_QKV ? M : r.M)) Fl[k] = &w.q[k];
                else { todo[k] = &w.q[k]; Wl[k] = sl.Wq[k]; any = true; }
            }
            if (any && (rc = expand(todo, sl.Wq, W_PER_LAYER))) return rc;
        }
        // norm1 of the first layer (vit.cpp:808-812); every later norm1 comes out of the previous layer's fc2
        if (c->mx) {
            if (il == 0 && (rc = layernorm_mx(sl.X, w.ln1_w, w.ln1_b, sl.Umx, sl.Umx_s, M_real))) return rc;
            if ((rc = gemm_mx(c, st, PC_GEMM_QKV, EPI_BIAS, sl.Umx, sl.Umx_s, w.mx[W_QKV], w.qkv_b, sl.QKV, nullptr, M_real, 3 * D))) return rc;
        } else {
            if (il == 0 && !(skip & 2) && (rc = layernorm(sl.X, D, w.ln1_w, w.ln1_b, sl.U, M_real))) return rc;
            // qkv projection (vit.cpp:820-821); `fix_u`: row blocks of U the previous layer's fc2 left to the fix-up are normalised in its prologue
            if ((rc = gemm(c, st, PC_GEMM_QKV, c->prec_attn ? EPI_BIAS_HILO : EPI_BIAS, dense_gemm(sl.U, Wl[W_QKV], w.qkv_b, sl.QKV, M, M_real, 3 * D, round_up(3 * D, tn), D),
                           Fl[W_QKV], nullptr, fix_u.todo ? &fix_u : nullptr, lo_off))) return rc;
        }
        // rotary position embeddings of a file with `rope`: q and k of the patch rows, in place, before anything reads them
        if (c->rope_cos) {
            ProfScope ps(c, st, PC_ROPE, 6.0 * n * (N - c->Tp) * (double)D, (double)n * (N - c->Tp) * 2 * D * eb * 2 * (c->prec_attn ? 2 : 1));
            HIP_TRY(launch_rope(dt, sl.QKV, lo_off, c->rope_cos, c->rope_sin, n, N, c->Tp, D, c->H, st));
        }
        if (c->attn && (rc = attention_maps(c, st, sl.QKV, lo_off, il, first_img, n))) return rc;
        if (tail_now) {   // attention of token 0 (vit.cpp:848-858 for the one row vit.cpp:910-911 keeps) -> compact rows U[b]; class rows of X -> Xc[b]
            ProfScope ps(c, st, PC_ATTENTION_CLS, 4.0 * n * c->H * (double)N * (D / c->H), (double)M_real * 2 * D * eb * (c->prec_attn ? 2 : 1) + (double)n * D * (eb + 8));
            HIP_TRY(launch_attention_cls(dt, sl.QKV, lo_off, sl.U, sl.X, sl.Xc, n, N, D, c->H, st));
        } else {          // attention (vit.cpp:826-866)
            ProfScope ps(c, st, PC_ATTENTION, 4.0 * n * c->H * (double)N * N * (D / c->H), (double)M_real * (c->prec_attn ? 7 : 4) * D * eb);
            if (!(skip & 1)) {
                if (c->prec_attn) HIP_TRY(launch_attention_stream(dt, true, sl.QKV, sl.U, n, N, D, c->H, lo_off, st));
                else HIP_TRY(launch_attention(*c->tune, dt, sl.QKV, sl.U, n, N, D, c->H, st));
            }
        }
        return VITX_OK;
    }
    // VITX_MXFP8 tail of a layer: proj in bf16, norm2 -> MX, fc1 -> MX (GELU epilogue), fc2 into X, the next norm1 -> MX
    int mx_tail(int il, const LayerW &w, const LayerW *nx, bool tail_now, const Rows &r) {
        int rc;
        if ((rc = gemm(c, st, r.pc_proj, EPI_BIAS_RESID, dense_gemm(sl.U, Wl[W_PROJ], w.proj_b, r.X, r.M, r.M_real, D, round_up(D, tn), D), Fl[W_PROJ]))) return rc;
        if ((rc = layernorm_mx(r.X, w.ln2_w, w.ln2_b, sl.U2mx, sl.U2mx_s, r.M_real))) return rc;
        if ((rc = gemm_mx(c, st, r.pc_fc1, EPI_BIAS_GELU, sl.U2mx, sl.U2mx_s, w.mx[W_FC1], w.fc1_b, sl.Hmx, sl.Hmx_s, r.M_real, mx_k_pad(F)))) return rc;
        if ((rc = gemm_mx(c, st, r.pc_fc2, EPI_BIAS_RESID, sl.Hmx, sl.Hmx_s, w.mx[W_FC2], w.fc2_b, r.X, nullptr, r.M_real, D))) return rc;
        if (nx && (rc = layernorm_mx(r.X, nx->ln1_w, nx->ln1_b, sl.Umx, sl.Umx_s, r.M_real))) return rc;
        if (!c->trace_ids.empty() && (rc = trace(il + 1))) return rc;
        if (c->feat && (rc = features(il, tail_now))) return rc;
        return patch_head_rows(il);
    }
    // Dense tail of a layer
    int dense_tail(int il, const LayerW &w, const LayerW *nx, bool tail_now, const Rows &r) {
        int rc;
        // output projection + residual (vit.cpp:868-873), then norm2 (vit.cpp:881-885) -> U2
        if ((rc = resid_gemm_ln(r, r.pc_proj, sl.U, Wl[W_PROJ], w.proj_b, D, Fl[W_PROJ], w.ln2_w, w.ln2_b, sl.U2, &fix_u2))) return rc;
        // MLP (vit.cpp:889-900), then the NEXT layer's norm1 (vit.cpp:808-812) -> U; the last layer is followed by the final norm instead
        // a `glu` context (include/vitx.h "gated MLP"): fc1 with the plain bias epilogue -> gate | up [M][2 F]; the gate kernel -> the compact
        // Hg [M][F] = silu(gate) . up; fc2 from that, lda == K as in any other model
        if ((rc = gemm(c, st, r.pc_fc1, c->fc1_epi, dense_gemm(sl.U2, Wl[W_FC1], w.fc1_b, sl.Hbuf, r.M, r.M_real, F1, round_up(F1, tn), D), Fl[W_FC1], nullptr,
                       fix_u2.todo ? &fix_u2 : nullptr))) return rc;
        if (c->glu) {
            ProfScope ps(c, st, PC_SWIGLU, 0, (double)r.M_real * 3 * F * eb);
            HIP_TRY(launch_swiglu(dt, sl.Hbuf, F1, sl.Hg, F, r.M_real, F, st));
        }
        if ((rc = resid_gemm_ln(r, r.pc_fc2, c->glu ? sl.Hg : sl.Hbuf, Wl[W_FC2], w.fc2_b, F, Fl[W_FC2], nx ? nx->ln1_w : nullptr, nx ? nx->ln1_b : nullptr, sl.U, &fix_u))) return rc;
        if (!c->trace_ids.empty() && (rc = trace(il + 1))) return rc;
        if ((rc = features(il, tail_now, c->pool && il + 1 == c->L ? sl.Z : nullptr))) return rc;
        return patch_head_rows(il);
    }
    int run(const void *d_imgs, void *d_probs, void *d_logits) {
        const int Mp_real = n * c->gh * c->gw;                          // patch rows
        // patch embedding (vit.cpp:747-797) in one launch: im2col gather, GEMM, + bias + pos, token scatter, class rows (patch_embed.hip)
        int rc;
        {
            ProfScope ps(c, st, PC_GEMM_PATCH, 2.0 * Mp_real * (double)D * c->Kpe, (double)n * c->img_floats() * 4 + (double)M_real * D * 4);
            HIP_TRY(launch_patch_embed(dt, (const float *)d_imgs, ws.pe_w, ws.pe_b, c->pos, ws.cls, ws.reg, c->nreg, sl.X, n, c->Sh, c->Sw, c->P, c->Cin, D, round_up(D, tn), c->Kpe_pad, st));
        }
        // pre-norm of a file with pre_norm.* (CLIP's pre_layrnorm): every token row, in place, before layer 0 -- trace stage 0 is the stream that enters it
        if (ws.pre_w) {
            ProfScope ps(c, st, PC_LAYERNORM, 0, (double)M_real * D * 8);
            HIP_TRY(launch_layernorm_f32(sl.X, ws.pre_w, ws.pre_b, sl.X, M_real, D, c->hp.eps, st));
        }
        if (!c->trace_ids.empty() && (rc = trace(0))) return rc;
        // LayerNorm fusion: decided per forward (the GEMM shape of this sub-batch must take the wide persistent kernel; never while the caller is
        // capturing a graph -- the epoch tag of a captured launch would be replayed).  The padded rows M_real .. M of X are then computed and
        // stored as well (GemmLn): they belong to this slice's scratch, start as zeros and stay finite.
        if (c->ln_fuse && sl.ln_sync) {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusActive; }
            fuse = cs == hipStreamCaptureStatusNone && gemm_ln_fusable(*c->tune, dense_gemm(nullptr, nullptr, nullptr, nullptr, M, M, D, round_up(D, tn), D)) &&
                   gemm_ln_fusable(*c->tune, dense_gemm(nullptr, nullptr, nullptr, nullptr, M, M, D, round_up(D, tn), F));
        }
        const Rows all_rows{sl.X, M, M_real, PC_GEMM_PROJ, PC_GEMM_FC1, PC_GEMM_FC2, fuse};
        const Rows cls_rows{sl.Xc, round_up(n, tm), n, PC_GEMM_TAIL, PC_GEMM_TAIL, PC_GEMM_TAIL, false};
        const bool tail = c->cls_tail && c->trace_ids.empty() && !c->outputs_need_last_rows();      // the last layer carries only the class-token rows past its qkv projection (vitx_ctx::cls_tail)
        for (int il = 0; il < c->L; ++il) {
            const LayerW &w = ws.layers[il], *nx = il + 1 < c->L ? &ws.layers[il + 1] : nullptr;
            const bool tail_now = tail && il + 1 == c->L;
            const Rows &r = tail_now ? cls_rows : all_rows;
            if ((rc = layer_front(il, w, tail_now, r))) return rc;
            if ((rc = c->mx ? mx_tail(il, w, nx, tail_now, r) : dense_tail(il, w, nx, tail_now, r))) return rc;
        }
        // cls pooling + final norm (vit.cpp:910-919): row b*N of X, i.e. row stride N*D.  ViTSTR (vitstr.cpp:864-895) keeps the first
        // R = 25 tokens of every image instead: output row r = image r / R, token r % R.
        const int nR = n * c->R;
        // classifier: one row per image, row stride N*D; ViTSTR: groups of R consecutive token rows (stride D), group stride N*D
        // pooled head: Z [n][2 D] was written by the last layer's feature launch above (final norm of row 0 ‖ mean of the patch rows' final norm)
        // attention-pooling head: one row per image comes out of pooled_tail
        if (c->pool) rc = VITX_OK;
        else if (c->map) rc = pooled_tail();             // Z = RNE(e), the attention-pooled embedding
        else if (tail) rc = layernorm(sl.Xc, D, ws.norm_w, ws.norm_b, sl.Z, n);
        else rc = layernorm(sl.X, c->R == 1 ? (long)N * D : (long)D, ws.norm_w, ws.norm_b, sl.Z, nR, c->R, (long)N * D);
        if (rc) return rc;
        // classifier (vit.cpp:927-928) and class softmax (vit.cpp:931-933)
        float *lg = d_logits ? (float *)d_logits : sl.logits;
        const int ldl = d_logits ? c->C : c->C_pad;
        const void *head_w = ws.head_w; const QuantW *head_f = nullptr;
        if (ws.head_q.blocks) {
            if (fused_ok(ws.head_q, round_up(nR, tm))) head_f = &ws.head_q;
            else { const QuantW *todo[1] = {&ws.head_q}; void *dst[1] = {sl.Wq_head}; if ((rc = expand(todo, dst, 1))) return rc; head_w = sl.Wq_head; }
        }
        if ((rc = gemm(c, st, PC_GEMM_HEAD, EPI_BIAS_F32, dense_gemm(sl.Z, head_w, ws.head_b, lg, round_up(nR, tm), nR, c->C, c->C_pad, c->pool ? 2 * D : D, ldl), head_f))) return rc;
        {
            ProfScope ps(c, st, PC_SOFTMAX, 0, (double)nR * c->C * 8);
            HIP_TRY(launch_softmax(dt, lg, (float *)d_probs, nR, c->C, ldl, st));
        }
        if ((rc = heads(lg, ldl))) return rc;
        if (fuse && c->ln_fb_host) HIP_TRY(hipMemcpyAsync(c->ln_fb_host + si, sl.ln_todo + sl.ln_blocks, sizeof(unsigned), hipMemcpyDeviceToHost, st));       // fall-back budget
        return VITX_OK;
    }
};

// Sub-batch sizes.  One 256x256 GEMM tile per CU per round means a sub-batch is cheapest when its tile counts land just
// under whole rounds: for ViT-B on 256 CUs 110 images are 85 row tiles = 255 / 765 / 1020 tiles for N = 768 / 2304 / 3072
// (1, 3 and 4 rounds) while 128 images cost 2 rounds' worth of time for 1.15 rounds of proj / fc2 work.  The first
// sub-batch size is the minimiser of a tile-round model of the four GEMMs of a layer (same tiling rules as launch_gemm);
// vitx_ctx_options::split_first overrides it.  More than two sub-batches are split evenly.
static double gemm_round_cost(long rows, int N, int K, int n_cu) {
    const long ntm = (rows + 255) / 256, ntn = (N + 255) / 256, tiles = ntm * ntn, rounds = tiles / n_cu, rem = tiles % n_cu;
    const double slots = K / 32.0, t_tile = slots * 0.98 + 3.5, t_half = slots * 0.6 + 3.0;
    if (rounds >= 1 && rem > 0 && rem <= n_cu * 6 / 10) {
        const long m_main = rounds * n_cu / ntn, half_tiles = ((ntm - m_main) * 2) * ntn;
        return rounds * t_tile + (double)((half_tiles + n_cu - 1) / n_cu) * t_half;
    }
    if (tiles < 128) return (double)(((rows + 127) / 128 * ntn + n_cu - 1) / n_cu) * t_half;
    return (double)((tiles + n_cu - 1) / n_cu) * t_tile;
}
// the LayerNorm-fusing residual GEMMs (proj, fc2) run rounds of gemm_ln_grid() workgroups: whole row blocks per XCD, column tiles of a
// row block in the same round; + 2 units per tile for the statistics exchange and the normalised store
static double gemm_round_cost_ln(long rows, int N, int K, int n_cu) {
    const long ntm = (rows + 255) / 256, ntn = N / 256;
    const int grid = gemm_ln_grid(n_cu, (int)(ntm * 256), N);
    const long most = ((ntm + 7) / 8) * ntn, wgx = grid / 8;
    return (double)((most + wgx - 1) / wgx) * (K / 32.0 * 0.98 + 3.5 + 2.0);
}
static void split_batch(const vitx_ctx *c, int n, int ns, int *m) {
    const int base = n / ns, extra = n % ns;
    for (int i = 0; i < ns; ++i) m[i] = base + (i < extra ? 1 : 0);
    if (c->split_first > 0 && ns == 2 && c->split_first < n) { m[0] = c->split_first; m[1] = n - c->split_first; return; }
    if (ns != 2) return;
    const int n_cu = c->tune->n_cu;
    const int D = c->D, F = c->F, F1 = c->F1;
    const bool ln = c->ln_fuse && c->slices[0].ln_sync;
    if (ln) {
        // LayerNorm-fusing residual GEMMs run rounds of (CUs / 8 / ntn) * ntn workgroups per XCD: the first sub-batch takes as many images as
        // ONE such round holds (ViT-B on 256 CUs: 10 row blocks per XCD = 80 blocks = 103 images), the second the rest -- measured (r03a,
        // interleaved, ms per 256-image forward): 72 | 103 | model's 110 | 128 images first = 9.95 | 9.90 | 10.09 | 10.21
        const int ntn = D / 256, per_xcd = std::max(n_cu / 8, ntn) / ntn;
        const int s1 = (int)((long)8 * per_xcd * 256 / c->N);
        if (s1 >= n / 4 && s1 <= n / 2 && (long)s1 * c->N / 256 * ntn >= 128) { m[0] = s1; m[1] = n - s1; return; }
    }
    auto layer = [&](int imgs) {
        const long rows = (long)imgs * c->N;
        const bool fl = ln && ((rows + 255) / 256) * (D / 256) >= 128;        // the fused kernel needs the wide path (is_wide, gemm.hip)
        return gemm_round_cost(rows, 3 * D, D, n_cu) + gemm_round_cost(rows, F1, D, n_cu) +
               (fl ? gemm_round_cost_ln(rows, D, D, n_cu) + gemm_round_cost_ln(rows, D, F, n_cu) : gemm_round_cost(rows, D, D, n_cu) + gemm_round_cost(rows, D, F, n_cu));
    };
    double best = layer(m[0]) + layer(m[1]);
    for (int s1 = std::max(8, n / 4); s1 <= n / 2; ++s1) {
        const double cost = layer(s1) + layer(n - s1);
        if (cost < best * 0.97) { best = cost; m[0] = s1; m[1] = n - s1; }   // move off the even split only for a clear (>3 %) modelled gain
    }
}

// Replay (or, the second time a call repeats, capture) the single-stream forward as a hipGraph.  *done = the forward was enqueued
// through a graph; otherwise the caller launches it directly (unless an error is returned).
static int forward_graph(vitx_ctx *c, hipStream_t st, const void *d_imgs, int n, void *d_probs, void *d_logits, bool *done) {
    *done = false;
    for (auto &ge : c->graphs)
        if (ge.imgs == d_imgs && ge.n == n && ge.probs == d_probs && ge.logits == d_logits) {
            if (hipGraphLaunch(ge.exec, st) == hipSuccess) { *done = true; ++c->graph_launches; return VITX_OK; }
            (void)hipGetLastError(); c->graphs_on = false; return VITX_OK;       // never seen; stay on the direct path from here on
        }
    vitx_ctx::GraphEntry &last = c->graph_last;
    const bool repeat = last.imgs == d_imgs && last.n == n && last.probs == d_probs && last.logits == d_logits;
    last = vitx_ctx::GraphEntry{d_imgs, d_probs, d_logits, n, nullptr};
    if (!repeat) return VITX_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return VITX_OK; }   // the caller is capturing: our launches join ITS graph
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); c->graphs_on = false; return VITX_OK; }
    const int rc = SliceForward{c, c->slices[0], st, 0, n}.run(d_imgs, d_probs, d_logits);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    hipGraphExec_t exec = nullptr;
    if (rc != VITX_OK || e != hipSuccess || !g || hipGraphInstantiate(&exec, g, nullptr, nullptr, 0) != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError(); c->graphs_on = false;
        return rc;                               // nothing ran: a launch error is reported, a capture problem falls back to direct launches
    }
    (void)hipGraphDestroy(g);
    if (c->graphs.size() >= 8) { (void)hipGraphExecDestroy(c->graphs.front().exec); c->graphs.erase(c->graphs.begin()); }
    c->graphs.push_back(vitx_ctx::GraphEntry{d_imgs, d_probs, d_logits, n, exec});
    if (hipGraphLaunch(exec, st) != hipSuccess) { set_error("vitx_forward_device: hipGraphLaunch: %s", hipGetErrorString(hipGetLastError())); return VITX_ERR_HIP; }
    *done = true;
    ++c->graph_launches;
    return VITX_OK;
}

// Do the internal sub-batch streams really run BESIDE the caller's stream?  The HIP runtime maps streams onto a pool of hardware queues and
// the queues onto the command processor's slots; which streams end up serialised depends on every other stream alive in the process
// (measured r03, tools/ctx_order_probe.py: with earlier contexts still alive the 2nd and the 7th context of a process ran 11.6 instead of
// 9.9 ms per forward -- with 8 hardware queues the 2nd, 4th and 6th, with 2 none; per-kernel times unchanged).  Nothing in the API tells,
// so it is measured: a 40 us do-nothing kernel on each stream, forked and joined like a forward; ~40 us = concurrent, ~80 us = serialised.
// For a serialised internal stream up to 8 candidate streams are created and kept alive TOGETHER (a stream created after another was
// destroyed gets the same queue back), the first one that runs beside the caller's stream is adopted, the rest are destroyed.
// Once per context (on the first forward of >= 16 images: the first caller stream it sees), ~0.2 ms, synchronous -- documented in vitx.h;
// skipped while the caller captures a graph.
static int probe_pair(vitx_ctx *c, hipStream_t st, hipStream_t s1, hipEvent_t done, float *best_ms) {
    *best_ms = 1e9f;
    for (int rep = 0; rep < 3; ++rep) {        // the first pass also wakes the queues up
        HIP_TRY(hipEventRecord(c->probe_a, st));
        HIP_TRY(hipStreamWaitEvent(s1, c->probe_a, 0));
        HIP_TRY(launch_spin(40, s1));
        HIP_TRY(hipEventRecord(done, s1));
        HIP_TRY(launch_spin(40, st));
        HIP_TRY(hipStreamWaitEvent(st, done, 0));
        HIP_TRY(hipEventRecord(c->probe_b, st));
        HIP_TRY(hipEventSynchronize(c->probe_b));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, c->probe_a, c->probe_b));
        *best_ms = std::min(*best_ms, ms);
    }
    return VITX_OK;
}
static int ensure_concurrent(vitx_ctx *c, hipStream_t st, int ns) {
    if (ns < 2 || std::find(c->probed_streams.begin(), c->probed_streams.end(), st) != c->probed_streams.end()) return VITX_OK;
    // Only the FIRST caller stream a context sees is probed (and may get the internal streams replaced): a caller that alternates streams
    // must not pay a synchronising probe per call, and replacing an internal stream for the second caller stream could undo what was
    // found for the first (r03 advisor).  Later caller streams are remembered and left alone.
    if (!c->probed_streams.empty()) { if (c->probed_streams.size() < 16) c->probed_streams.push_back(st); return VITX_OK; }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return VITX_OK; }
    if (!c->probe_a) { HIP_TRY(hipEventCreate(&c->probe_a)); HIP_TRY(hipEventCreate(&c->probe_b)); }
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const float kSerialised = 0.064f;
    for (int i = 1; i < ns; ++i) {
        vitx_ctx::Slice &sl = c->slices[i];
        float ms = 0.0f;
        int rc = probe_pair(c, st, sl.stream, sl.done, &ms);
        if (rc) return rc;
        if (ms < kSerialised) continue;
        hipStream_t cand[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        int pick = -1;
        for (int k = 0; k < 8 && pick < 0; ++k) {
            HIP_TRY(hipStreamCreateWithPriority(&cand[k], hipStreamNonBlocking, (k & 1) ? 0 : greatest));
            ++c->stream_retries;
            if ((rc = probe_pair(c, st, cand[k], sl.done, &ms))) break;
            if (ms < kSerialised) pick = k;
        }
        for (int k = 0; k < 8; ++k) if (cand[k] && k != pick) (void)hipStreamDestroy(cand[k]);
        if (rc) return rc;
        if (pick >= 0) { (void)hipStreamDestroy(sl.stream); sl.stream = cand[pick]; }       // otherwise keep the original: nothing better exists
    }
    c->probed_streams.push_back(st);
    return VITX_OK;
}

static int forward_pass(vitx_ctx *c, const void *d_imgs, int n, void *d_probs, void *d_logits, hipStream_t st) {
    // Fall-back budget of the fused LayerNorm.  The counters are what the PREVIOUS forwards copied to pinned memory behind their last kernel
    // (no event between that copy and this read: a value that is one forward stale, or mid-update, moves the decision by one window at most --
    // the reads are volatile so that each is one 32-bit load).  Test mode: only with bit 4.
    if (c->ln_fb_host && (!c->ln_test || (c->ln_test & 4))) {
        constexpr int kLnWindow = 16, kLnBudget = 8;
        auto counters = [&]() { unsigned long long t = 0; for (int i = 0; i < c->nslices && i < 4; ++i) t += *(volatile unsigned *)(c->ln_fb_host + i); return t; };
        if (c->ln_fuse) {
            if (++c->ln_fb_forwards >= kLnWindow) {
                const unsigned long long total = counters();
                if (total - c->ln_fb_base > (unsigned long long)kLnWindow * kLnBudget) {
                    c->ln_fuse = false; c->ln_fuse_disabled = true;
                    c->ln_cool_left = c->ln_cool_len; c->ln_cool_len = std::min(c->ln_cool_len * 2, 1 << 16);
                }
                c->ln_fb_base = total; c->ln_fb_forwards = 0;
            }
        } else if (c->ln_fuse_disabled && --c->ln_cool_left <= 0) {       // cool-down over: try the fused path again (same bits either way)
            c->ln_fuse = true; c->ln_fuse_disabled = false;
            c->ln_fb_base = counters(); c->ln_fb_forwards = 0;
        }
    }
    // while per-kernel profiling is on, sub-batches run back to back on the caller's stream so that every
    // event pair brackets one kernel running alone (exclusive durations, comparable with rocprofv3 --stats)
    const bool serial = c->prof_on;
    const int ns = (c->nslices > 1 && n >= 8 * c->nslices) ? c->nslices : 1;
    if (ns == 1) {
        if (c->graphs_on && !c->prof_on && c->trace_ids.empty() && !c->any_output()) {
            bool done = false;
            const int rc = forward_graph(c, st, d_imgs, n, d_probs, d_logits, &done);
            if (rc != VITX_OK || done) return rc;
        }
        return SliceForward{c, c->slices[0], st, 0, n}.run(d_imgs, d_probs, d_logits);
    }
    int m[4];
    split_batch(c, n, ns, m);
    if (!serial) { const int rc = ensure_concurrent(c, st, ns); if (rc) return rc; }
    // fork: slices 1.. wait for the caller's stream and run their contiguous sub-batches on the internal streams, slice 0 runs on the caller's
    // stream itself, which finally joins the others (slice 0 is enqueued LAST so that the host has already fed the other streams)
    if (!serial) HIP_TRY(hipEventRecord(c->fork, st));
    int off[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < ns; ++i) off[i + 1] = off[i] + m[i];
    for (int k = 0; k < ns; ++k) {
        const int i = serial ? k : (k + 1) % ns;           // 1, 2, .., 0
        vitx_ctx::Slice &sl = c->slices[i];
        hipStream_t ss = (serial || i == 0) ? st : sl.stream;
        if (!serial && i > 0) HIP_TRY(hipStreamWaitEvent(sl.stream, c->fork, 0));
        int rc = SliceForward{c, sl, ss, off[i], m[i]}.run((const float *)d_imgs + (size_t)off[i] * c->img_floats(), (float *)d_probs + (size_t)off[i] * c->R * c->C,
                                                           d_logits ? (float *)d_logits + (size_t)off[i] * c->R * c->C : nullptr);
        if (rc) return rc;
        if (!serial && i > 0) HIP_TRY(hipEventRecord(sl.done, sl.stream));
    }
    if (!serial) for (int i = 1; i < ns; ++i) HIP_TRY(hipStreamWaitEvent(st, c->slices[i].done, 0));
    return VITX_OK;
}

}  // namespace

extern "C" {

int vitx_ctx_split(const vitx_ctx *c, int n, int32_t *images, int max_parts) {
    if (!c || !images || max_parts <= 0 || n <= 0 || n > c->max_batch) return 0;
    n = std::min(n, c->call_limit);              // a batch beyond the kernels' window runs as several passes: this is the first one's cut
    const int ns = (c->nslices > 1 && n >= 8 * c->nslices) ? c->nslices : 1;
    if (ns > max_parts) return 0;
    int m[4] = {n, 0, 0, 0};
    if (ns > 1) split_batch(c, n, ns, m);
    for (int i = 0; i < ns; ++i) images[i] = m[i];
    return ns;
}
int vitx_forward_device(vitx_ctx *c, const void *d_imgs, int n, void *d_probs, void *d_logits, void *stream) {
    if (!c || !d_imgs || !d_probs) { set_error("vitx_forward_device: NULL argument"); return VITX_ERR_ARG; }
    if (n <= 0 || n > c->max_batch) { set_error("vitx_forward_device: batch %d outside 1..%d", n, c->max_batch); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    // one pass of the kernels takes call_limit images (32-bit buffer window, vitx_ctx_create_ex); a larger batch is several passes, back to back on the
    // caller's stream through the same scratch -- images are independent, so the results are the ones a single pass would give
    if (n > c->call_limit && !c->trace_ids.empty()) { set_error("vitx_forward_device: the residual-stream trace takes one pass (at most %d images)", c->call_limit); return VITX_ERR_ARG; }
    if (n > c->call_limit) {
        const char *who = nullptr;
        c->each_output([&](const Output &o) { if (!who) who = o.one_pass; });
        if (who) { set_error("vitx_forward_device: %s one pass (at most %d images)", who, c->call_limit); return VITX_ERR_ARG; }
    }
    for (int i0 = 0; i0 < n; i0 += c->call_limit) {
        const int ni = std::min(c->call_limit, n - i0);
        const int rc = forward_pass(c, (const float *)d_imgs + (size_t)i0 * c->img_floats(), ni, (float *)d_probs + (size_t)i0 * c->R * c->C,
                                    d_logits ? (float *)d_logits + (size_t)i0 * c->R * c->C : nullptr, st);
        if (rc) return rc;
    }
    c->each_output([n](Output &o) { o.n = n; });
    return VITX_OK;
}
int vitx_forward(vitx_ctx *c, const float *imgs, int n, float *probs, float *logits) {
    if (!c || !imgs || !probs) { set_error("vitx_forward: NULL argument"); return VITX_ERR_ARG; }
    if (n <= 0 || n > c->max_batch) { set_error("vitx_forward: batch %d outside 1..%d", n, c->max_batch); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    const size_t img_bytes = (size_t)n * c->img_floats() * 4;
    HIP_TRY(hipMemcpyAsync(c->img, imgs, img_bytes, hipMemcpyHostToDevice, c->stream));
    int rc = vitx_forward_device(c, c->img, n, c->probs, logits ? c->logits_all : nullptr, c->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(probs, c->probs, (size_t)n * c->R * c->C * 4, hipMemcpyDeviceToHost, c->stream));
    if (logits) HIP_TRY(hipMemcpyAsync(logits, c->logits_all, (size_t)n * c->R * c->C * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VITX_OK;
}

int vitx_ctx_synchronize(vitx_ctx *c) {
    if (!c) return VITX_ERR_ARG;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VITX_OK;
}

}  // extern "C"
