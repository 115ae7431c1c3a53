// packed_outputs.cpp -- what a packed context gives besides probabilities (packed_context.h; include/vitx.h "packed batches"): the last layer's
// features, attention maps, the dense head and the depth head.  All opt-in; the forward (packed_forward.cpp) launches nothing for an output that
// is off.  A set call checks every argument before its first device call, waits for the context (pack_quiesce), builds the new state in a local --
// each buffer through alloc_counted, so the state's `bytes` are what it allocated -- and ends with pack_commit and the move in: a refused or failed
// set leaves what was set.  The heads' own argument checks and their uploads are the image context's (heads.h: dense_head_args,
// dense_head_values, dense_head_upload and depth_head_*); what the two packed heads add in front is pack_head_pixels and pack_head_window.
#include <algorithm>

#include "packed_context.h"

namespace {

// The last forward's patch rows of d_rows, which holds `width` floats for every row of the pack, gathered on the host: the images end to end,
// without their prefix rows
int read_patch_rows(const vitx_pack *p, int n, const float *d_rows, size_t width, float *out) {
    for (int i = 0; i < n; ++i)
        HIP_TRY(hipMemcpy(out + p->patch_at(i) * width, d_rows + (size_t)(p->row0[i] + p->Tp) * width, p->patch_rows(i) * width * 4, hipMemcpyDeviceToHost));
    return VITX_OK;
}

// What vitx_pack_dense_set and vitx_pack_depth_set refuse besides the image context's checks, in pieces as those sit between them
int pack_head_pixels(const char *api, long max_pixels) {
    if (max_pixels < 1) { set_error("%s: max_pixels = %ld", api, max_pixels); return VITX_ERR_ARG; }
    return VITX_OK;
}
int pack_head_window(const char *api, const vitx_pack *p, size_t Mp, int Dc, size_t Kpad) {
    if (Mp * Dc * 2 > 0xf0000000u || Mp * Kpad * 4 > 0xf0000000u) {
        set_error("%s: the operand or logit rows of max_tokens = %d rows leave the GEMM's 32-bit byte window", api, p->max_tokens);
        return VITX_ERR_UNSUPPORTED;
    }
    return VITX_OK;
}

}  // namespace

extern "C" {

int vitx_pack_feat_enable(vitx_pack *p, int flags) {
    if (!p || (flags & ~(VITX_FEAT_CLS | VITX_FEAT_TOKENS))) { set_error("vitx_pack_feat_enable: flags are VITX_FEAT_CLS | VITX_FEAT_TOKENS (0 = off)"); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(p->device));
    if (flags && !p->feat) {
        const size_t bytes = (size_t)p->max_tokens * p->D * 4;
        HIP_TRY(hipMalloc(&p->feat.p, bytes));
        p->scratch_bytes += bytes;
    }
    p->feat_flags = flags; p->feat_n = 0;
    return VITX_OK;
}

// The last forward's final-norm rows, gathered on the host: cls [n][D] = row row0[i], tokens = image i's patch rows, images end to end
int vitx_pack_feat_read(vitx_pack *p, float *cls, float *tokens) {
    if (!p || (!cls && !tokens)) { set_error("vitx_pack_feat_read: NULL argument"); return VITX_ERR_ARG; }
    if (!p->feat_flags || !p->feat_n) { set_error("vitx_pack_feat_read: no forward has run with features on since vitx_pack_feat_enable"); return VITX_ERR_ARG; }
    if ((cls && !(p->feat_flags & VITX_FEAT_CLS)) || (tokens && !(p->feat_flags & VITX_FEAT_TOKENS))) { set_error("vitx_pack_feat_read: an output was asked for that vitx_pack_feat_enable did not select"); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(p->device));
    if (p->done_pending) HIP_TRY(hipEventSynchronize(p->done));
    const int n = p->feat_n;
    const size_t D = (size_t)p->D;
    if (cls) for (int i = 0; i < n; ++i) HIP_TRY(hipMemcpy(cls + i * D, p->feat.as<float>() + p->row0[i] * D, D * 4, hipMemcpyDeviceToHost));
    return tokens ? read_patch_rows(p, n, p->feat.as<float>(), D, tokens) : VITX_OK;
}

// Attention maps of a packed context (include/vitx.h "packed batches")
int vitx_pack_attn_enable(vitx_pack *p, uint64_t layer_mask, int flags, long max_sq_tokens) {
    if (!p) { set_error("vitx_pack_attn_enable: NULL context"); return VITX_ERR_ARG; }
    if (const int rc = pack_attn_args("vitx_pack_attn_enable", p->L, layer_mask, flags, max_sq_tokens)) return rc;
    const bool on = layer_mask != 0 || flags != 0, rollout = (flags & VITX_ATTN_ROLLOUT) != 0;
    HIP_TRY(hipSetDevice(p->device));
    if (const int rc = pack_quiesce(p)) return rc;
    if (!on) {
        if (p->attn) { p->scratch_bytes -= p->attn->bytes; p->attn.reset(); }
        return resize_tables(p, "vitx_pack_attn_enable", p->parts() & ~kRollout);
    }
    auto am = std::make_unique<PackAttn>();
    const size_t T = (size_t)p->max_tokens, H = (size_t)p->H;
    am->mask = layer_mask; am->flags = flags; am->max_sq = rollout ? max_sq_tokens : 0;
    am->fpt = layer_slot(layer_mask, p->L) * p->H + (rollout ? 1 : 0);
    bool ok = alloc_counted(am->out, T * am->fpt * 4, &am->bytes);
    if (ok && rollout) ok = alloc_counted(am->roll[0], (size_t)max_sq_tokens * 4, &am->bytes) && alloc_counted(am->roll[1], (size_t)max_sq_tokens * 4, &am->bytes);
    if (ok && rollout && !am->selects(p->L - 1)) ok = alloc_counted(am->cls_last, T * H * 4, &am->bytes);
    if (!ok) { set_error("vitx_pack_attn_enable: cannot allocate the map buffers for %d token rows", p->max_tokens); return VITX_ERR_NOMEM; }
    const unsigned parts = rollout ? p->parts() | kRollout : p->parts() & ~kRollout;
    if (const int rc = pack_commit(p, "vitx_pack_attn_enable", parts, p->attn ? p->attn->bytes : 0, am->bytes)) return rc;
    p->attn = std::move(am);
    return VITX_OK;
}

int vitx_pack_attn_floats(const vitx_pack *p) { return p && p->attn ? p->attn->fpt : 0; }
const void *vitx_pack_attn_device(const vitx_pack *p) { return p && p->attn ? p->attn->out.p : nullptr; }

// The last forward's maps, the images end to end as they lie on the device: image i's floats start at row0[i] * fpt
int vitx_pack_attn_read(vitx_pack *p, float *out, size_t n_floats) {
    if (!p || !out) { set_error("vitx_pack_attn_read: NULL argument"); return VITX_ERR_ARG; }
    const PackAttn *am = p->attn.get();
    const int n = am ? am->n : 0;
    if (n == 0) { set_error("vitx_pack_attn_read: no forward has run with attention maps on since vitx_pack_attn_enable"); return VITX_ERR_ARG; }
    const size_t need = (size_t)p->row0[n] * am->fpt;
    if (n_floats < need) { set_error("vitx_pack_attn_read: the buffer holds %zu floats, the last forward's maps %zu", n_floats, need); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(p->device));
    if (p->done_pending) HIP_TRY(hipEventSynchronize(p->done));
    HIP_TRY(hipMemcpy(out, am->out.p, need * 4, hipMemcpyDeviceToHost));
    return VITX_OK;
}

// The dense head of a packed context (include/vitx.h "packed batches")
int vitx_pack_dense_set(vitx_pack *p, const float *W, const float *bias, int K, int Dc, uint64_t layer_mask, long max_pixels, int flags) {
    const char *api = "vitx_pack_dense_set";
    if (!p) { set_error("vitx_pack_dense_set: NULL context"); return VITX_ERR_ARG; }
    const bool off = !W && K == 0;
    uint64_t mask = layer_mask;
    const size_t Mp = (size_t)round_up(p->max_tokens, p->tm), Kpad = K > 0 ? (size_t)round_up(K, p->tn) : 0;
    if (!off) {
        if (const int rc = dense_head_args(api, W, K, Dc, flags, p->L, p->D, &mask)) return rc;
        if (const int rc = pack_head_pixels(api, max_pixels)) return rc;
        if (const int rc = dense_head_values(api, W, bias, K, Dc)) return rc;
        if (const int rc = pack_head_window(api, p, Mp, Dc, Kpad)) return rc;
    }
    HIP_TRY(hipSetDevice(p->device));
    if (const int rc = pack_quiesce(p)) return rc;
    if (off) {
        if (p->dense) { p->scratch_bytes -= p->dense->bytes; p->dense.reset(); }
        return resize_tables(p, api, p->parts() & ~kDense);
    }
    auto dn = std::make_unique<PackDense>();
    dn->K = K; dn->Kpad = (int)Kpad; dn->Dc = Dc; dn->mask = mask; dn->flags = flags; dn->cap = p->max_images; dn->max_pixels = max_pixels;
    dn->a.resize(1); dn->acc.resize(1);
    bool ok = alloc_counted(dn->W, Kpad * Dc * 2, &dn->bytes) && alloc_counted(dn->bias, Kpad * 4, &dn->bytes) && alloc_counted(dn->a[0], Mp * Dc * 2, &dn->scratch) &&
              alloc_counted(dn->acc[0], Mp * Kpad * 4, &dn->scratch) && alloc_counted(dn->labels, (size_t)max_pixels, &dn->bytes);
    if (ok && (flags & VITX_DENSE_SCORE)) ok = alloc_counted(dn->score, (size_t)max_pixels * 4, &dn->bytes);
    if (ok && (flags & VITX_DENSE_LOGITS)) ok = alloc_counted(dn->logits, (size_t)p->max_tokens * K * 4, &dn->bytes);
    if (!ok) { set_error("vitx_pack_dense_set: cannot allocate the buffers for %d classes, %ld pixels and %d token rows", K, max_pixels, p->max_tokens); return VITX_ERR_NOMEM; }
    dn->bytes += dn->scratch;            // the operand and logit rows (vitx_pack_dense_scratch_bytes) are part of what the head adds
    // the head goes up as in an image context; the operand rows start as zeros (a forward writes its rows and zeroes the pad rows behind them)
    HIP_TRY(dense_head_upload(*dn, p->dtype, W, bias));
    HIP_TRY(hipMemset(dn->a[0].p, 0, Mp * Dc * 2));
    HIP_TRY(hipDeviceSynchronize());
    if (const int rc = pack_commit(p, api, p->parts() | kDense, p->dense ? p->dense->bytes : 0, dn->bytes)) return rc;
    p->dense = std::move(dn);
    return VITX_OK;
}

int vitx_pack_dense_out(vitx_pack *p, const int32_t *out_shapes, int n) {
    if (!p || !p->dense) { set_error("vitx_pack_dense_out: no dense head is set"); return VITX_ERR_ARG; }
    return pack_next_shapes(p, "vitx_pack_dense_out", out_shapes, n, &p->dense->next_out);
}

const void *vitx_pack_dense_device(const vitx_pack *p) { return p && p->dense ? p->dense->labels.p : nullptr; }
size_t vitx_pack_dense_scratch_bytes(const vitx_pack *p) { return p && p->dense ? p->dense->scratch : 0; }

// The last forward's maps, the images end to end, and the kept logits of its patch rows (behind each image's prefix rows in the pack's rows)
int vitx_pack_dense_read(vitx_pack *p, uint8_t *labels, float *score, float *logits) {
    if (!p || !labels) { set_error("vitx_pack_dense_read: NULL argument"); return VITX_ERR_ARG; }
    const PackDense *dn = p->dense.get();
    const int n = dn ? dn->n : 0;
    if (n == 0) { set_error("vitx_pack_dense_read: no forward has run with a dense head set since vitx_pack_dense_set"); return VITX_ERR_ARG; }
    if (score && !dn->score) { set_error("vitx_pack_dense_read: the head was set without VITX_DENSE_SCORE"); return VITX_ERR_ARG; }
    if (logits && !dn->logits) { set_error("vitx_pack_dense_read: the head was set without VITX_DENSE_LOGITS"); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(p->device));
    if (p->done_pending) HIP_TRY(hipEventSynchronize(p->done));
    const size_t px = (size_t)dn->last.pix0[n];
    HIP_TRY(hipMemcpy(labels, dn->labels.p, px, hipMemcpyDeviceToHost));
    if (score) HIP_TRY(hipMemcpy(score, dn->score.p, px * 4, hipMemcpyDeviceToHost));
    return logits ? read_patch_rows(p, n, dn->logits.as<float>(), (size_t)dn->K, logits) : VITX_OK;
}

// The depth head of a packed context (include/vitx.h "packed batches")
int vitx_pack_depth_set(vitx_pack *p, const float *Wp, const float *Wc, const float *bias, const float *bins, int K, int Dc, uint64_t layer_mask, int upsample,
                        float min_depth, float max_depth, long max_pixels, int flags) {
    const char *api = "vitx_pack_depth_set";
    if (!p) { set_error("vitx_pack_depth_set: NULL context"); return VITX_ERR_ARG; }
    const bool off = !Wp && K == 0;
    uint64_t mask = layer_mask;
    const size_t Mp = (size_t)round_up(p->max_tokens, p->tm), Bp = (size_t)round_up(p->max_images, p->tm), Kpad = K > 0 ? (size_t)round_up(K, p->tn) : 0;
    if (!off) {
        if (const int rc = depth_head_args(api, Wp, bins, K, Dc, flags, p->L, p->D, &mask)) return rc;
        if (const int rc = pack_head_pixels(api, max_pixels)) return rc;
        if (const int rc = depth_head_values(api, Wp, Wc, bias, bins, K, Dc, min_depth, max_depth, upsample)) return rc;
        if (const int rc = pack_head_window(api, p, Mp, Dc, Kpad)) return rc;
    }
    HIP_TRY(hipSetDevice(p->device));
    if (const int rc = pack_quiesce(p)) return rc;
    if (off) {
        if (p->depth) { p->scratch_bytes -= p->depth->bytes; p->depth.reset(); }
        return resize_tables(p, api, p->parts() & ~kDepth);
    }
    auto dp = std::make_unique<PackDepth>();
    dp->K = K; dp->Kpad = (int)Kpad; dp->Dc = Dc; dp->mask = mask; dp->flags = flags; dp->cap = p->max_images; dp->max_pixels = max_pixels;
    dp->u = upsample; dp->lo = min_depth; dp->hi = max_depth;
    dp->bias_host.assign(K, 0.0f);
    if (bias) std::copy(bias, bias + K, dp->bias_host.begin());
    dp->a.resize(1); dp->acc.resize(1);
    const size_t fine_floats = (size_t)upsample * upsample * p->max_tokens;
    bool ok = alloc_counted(dp->Wp, Kpad * Dc * 2, &dp->bytes) && (!Wc || alloc_counted(dp->Wc, Kpad * Dc * 2, &dp->bytes)) && alloc_counted(dp->bias, Kpad * 4, &dp->bytes) &&
              alloc_counted(dp->zero, Kpad * 4, &dp->bytes) && alloc_counted(dp->bins, Kpad * 4, &dp->bytes) && alloc_counted(dp->a[0], Mp * Dc * 2, &dp->scratch) &&
              alloc_counted(dp->acc[0], Mp * Kpad * 4, &dp->scratch) && alloc_counted(dp->depth, (size_t)max_pixels * 4, &dp->bytes) &&
              alloc_counted(dp->fine, fine_floats * 4, &dp->bytes);
    if (ok && Wc) {
        dp->ac.resize(1); dp->o.resize(1);
        ok = alloc_counted(dp->ac[0], Bp * Dc * 2, &dp->scratch) && alloc_counted(dp->o[0], Bp * Kpad * 4, &dp->scratch);
    }
    if (ok && (flags & VITX_DEPTH_LOGITS))
        ok = alloc_counted(dp->logits, (size_t)p->max_tokens * K * 4, &dp->bytes) && (!Wc || alloc_counted(dp->off, (size_t)p->max_images * K * 4, &dp->bytes));
    if (!ok) { set_error("vitx_pack_depth_set: cannot allocate the buffers for %d bins, %ld pixels and %d token rows", K, max_pixels, p->max_tokens); return VITX_ERR_NOMEM; }
    dp->bytes += dp->scratch;            // the operand, logit, class and offset rows (vitx_pack_depth_scratch_bytes) are part of what the head adds
    // the head goes up as in an image context; the operand rows start as zeros (a forward writes its rows and zeroes the pad rows behind them)
    HIP_TRY(depth_head_upload(*dp, p->dtype, Wp, Wc, bias, bins));
    HIP_TRY(hipMemset(dp->a[0].p, 0, Mp * Dc * 2));
    if (Wc) HIP_TRY(hipMemset(dp->ac[0].p, 0, Bp * Dc * 2));
    HIP_TRY(hipDeviceSynchronize());
    if (const int rc = pack_commit(p, api, p->parts() | kDepth, p->depth ? p->depth->bytes : 0, dp->bytes)) return rc;
    p->depth = std::move(dp);
    return VITX_OK;
}

int vitx_pack_depth_out(vitx_pack *p, const int32_t *out_shapes, int n) {
    if (!p || !p->depth) { set_error("vitx_pack_depth_out: no depth head is set"); return VITX_ERR_ARG; }
    return pack_next_shapes(p, "vitx_pack_depth_out", out_shapes, n, &p->depth->next_out);
}

const void *vitx_pack_depth_device(const vitx_pack *p) { return p && p->depth ? p->depth->depth.p : nullptr; }
size_t vitx_pack_depth_scratch_bytes(const vitx_pack *p) { return p && p->depth ? p->depth->scratch : 0; }

// The last forward's maps and fine planes, the images end to end, the kept logits of its patch rows (behind each image's prefix rows in the pack's
// rows) and the kept offsets, one row per image
int vitx_pack_depth_read(vitx_pack *p, float *depth, float *fine, float *logits, float *offsets) {
    if (!p || !depth) { set_error("vitx_pack_depth_read: NULL argument"); return VITX_ERR_ARG; }
    const PackDepth *dp = p->depth.get();
    const int n = dp ? dp->n : 0;
    if (n == 0) { set_error("vitx_pack_depth_read: no forward has run with a depth head set since vitx_pack_depth_set"); return VITX_ERR_ARG; }
    if (fine && !(dp->flags & VITX_DEPTH_FINE)) { set_error("vitx_pack_depth_read: the head was set without VITX_DEPTH_FINE"); return VITX_ERR_ARG; }
    if ((logits || offsets) && !dp->logits) { set_error("vitx_pack_depth_read: the head was set without VITX_DEPTH_LOGITS"); return VITX_ERR_ARG; }
    const int K = dp->K;
    HIP_TRY(hipSetDevice(p->device));
    if (p->done_pending) HIP_TRY(hipEventSynchronize(p->done));
    HIP_TRY(hipMemcpy(depth, dp->depth.p, (size_t)dp->last.pix0[n] * 4, hipMemcpyDeviceToHost));
    if (fine) HIP_TRY(hipMemcpy(fine, dp->fine.p, (size_t)dp->last.fine0[n] * 4, hipMemcpyDeviceToHost));
    if (logits) if (const int rc = read_patch_rows(p, n, dp->logits.as<float>(), (size_t)K, logits)) return rc;
    if (offsets && dp->off) HIP_TRY(hipMemcpy(offsets, dp->off.p, (size_t)n * K * 4, hipMemcpyDeviceToHost));
    if (offsets && !dp->off) for (int i = 0; i < n; ++i) std::copy(dp->bias_host.begin(), dp->bias_host.end(), offsets + (size_t)i * K);
    return VITX_OK;
}

}  // extern "C"
