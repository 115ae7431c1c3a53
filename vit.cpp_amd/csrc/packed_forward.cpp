// packed_forward.cpp -- a call of a packed context (packed_context.h; include/vitx.h "packed batches"): its host-only checks, made once, and
// the forward, and the entry points of both.
// The checks: check_shapes for every call, then one check_* per opt-in part that is on (dense, depth, attention rollout, u8), each filling its
// part's struct of the PackCall (packed_context.h); check_call runs them for a forward, the vitx_pack_*_check entry points run one each and
// copy out of the same struct.
// The forward: pack_forward takes the call's structs over with one swap per part, resolves the grids, has every part write its tables into the
// staging buffer (*_tables, in layout order) and uploads them in one copy; then the launches.  The blocks are the image forward's row-wise
// launches through the same dispatchers (GEMMs, LayerNorm, activation, gate, pre-norm do not care where one image ends); new are the three
// launches that must know: the variable-length attention (attention_packed.hip), the rotary embeddings by a segment table (rope.hip) and the
// class-row gather (text_embed.hip).  The patch embedding is the rectangular context's kernel, one launch per run of consecutive images of
// one shape.  With u8 sources declared for the call one launch in front of it stretches every source to its image's shape into the context's
// pixel buffer (image_preprocess.hip).  Attention maps are the image forward's launch sequence on the packed map kernels (attention_map.hip), in
// front of each layer's attention.  The dense and the depth head: the operand rows and the head GEMM over all rows of the pack, then the label
// launch (dense_label.hip) or the fine and resize launches (depth_map.hip) by their own segment tables, one map per image at its own size.
// No LayerNorm fusion, no class-token tail.
#include <algorithm>

#include "depth_bins.h"
#include "packed_context.h"

namespace {

// The checks of a forward call that need no device (vitx_pack_check's text): row0 [n + 1] on success
int check_shapes(const char *api, const vitx_model *m, const int32_t *shapes, int n, int max_tokens, int max_images, int32_t *row0) {
    if (!m || !shapes) { set_error("%s: NULL argument", api); return VITX_ERR_ARG; }
    if (m->kind != VITX_KIND_IMAGE) { set_error("%s: a text-tower model takes a text context (vitx_text_create), not a packed context", api); return VITX_ERR_ARG; }
    if (max_images < 1 || n < 1 || n > max_images) { set_error("%s: n = %d is outside 1 .. max_images = %d", api, n, max_images); return VITX_ERR_ARG; }
    const int P = m->hp.patch_size, Tp = vitx_model_num_prefix(m);
    long rows = 0;
    for (int i = 0; i < n; ++i) {
        const int h = shapes[2 * i], w = shapes[2 * i + 1];
        if (P <= 0 || h <= 0 || w <= 0 || h % P || w % P) { set_error("%s: image %d: %d x %d is not a positive multiple of the patch size %d", api, i, h, w, P); return VITX_ERR_ARG; }
        if (row0) row0[i] = (int32_t)rows;
        rows += (long)(h / P) * (w / P) + Tp;
        if (rows > max_tokens) { set_error("%s: images 0 .. %d hold %ld tokens, above max_tokens = %d", api, i, rows, max_tokens); return VITX_ERR_ARG; }
    }
    if (row0) row0[n] = (int32_t)rows;
    return VITX_OK;
}

// What a forward call adds to check_shapes while a dense head of K classes and max_pixels is set (vitx_pack_dense_check's text; `shapes` has passed
// check_shapes): the output shapes -- out_shapes [n_out][2], or the images' own -- against the grids and the buffers.  On success the head's
// tables of the call in *c.
int check_dense(const char *api, const vitx_model *m, const int32_t *shapes, const int32_t *out_shapes, int n_out, int n, int K, long max_pixels, PackDenseCall *c) {
    if (K < 1) { set_error("%s: K = %d classes", api, K); return VITX_ERR_ARG; }
    if (K > kDenseMaxK) { set_error("%s: K = %d classes above %d (labels are bytes)", api, K, kDenseMaxK); return VITX_ERR_UNSUPPORTED; }
    if (max_pixels < 1) { set_error("%s: max_pixels = %ld", api, max_pixels); return VITX_ERR_ARG; }
    if (out_shapes && n_out != n) { set_error("%s: output shapes were given for %d images, the call has %d", api, n_out, n); return VITX_ERR_ARG; }
    const int P = m->hp.patch_size;
    c->grids.resize((size_t)2 * n); c->outs.resize((size_t)2 * n); c->pix0.resize((size_t)n + 1); c->tile0.resize((size_t)n + 1);
    for (int i = 0; i < n; ++i) {
        const int gh = shapes[2 * i] / P, gw = shapes[2 * i + 1] / P;
        const int oh = out_shapes ? out_shapes[2 * i] : shapes[2 * i], ow = out_shapes ? out_shapes[2 * i + 1] : shapes[2 * i + 1];
        if (oh < gh || ow < gw || oh > kDenseMaxOut || ow > kDenseMaxOut) {
            set_error("%s: image %d: output %d x %d outside the patch grid %d x %d .. %d (upsampling only)", api, i, oh, ow, gh, gw, kDenseMaxOut);
            return VITX_ERR_ARG;
        }
        c->grids[2 * i] = gh; c->grids[2 * i + 1] = gw; c->outs[2 * i] = oh; c->outs[2 * i + 1] = ow;
    }
    if (!dense_pack_tables(c->grids.data(), c->outs.data(), n, c->pix0.data(), c->tile0.data(), &c->cells)) { set_error("%s: the call's outputs hold more than 2^31 - 1 tiles", api); return VITX_ERR_ARG; }
    if (c->pix0[n] > (int64_t)max_pixels) { set_error("%s: the call's outputs hold %lld pixels, above max_pixels = %ld", api, (long long)c->pix0[n], max_pixels); return VITX_ERR_ARG; }
    return VITX_OK;
}

// The same for a depth head of K bins, upsampling u and max_pixels (vitx_pack_depth_check's text): the output shapes against the fine planes and the
// buffers.  On success the head's tables of the call in *c.
int check_depth(const char *api, const vitx_model *m, const int32_t *shapes, const int32_t *out_shapes, int n_out, int n, int K, int u, long max_pixels, PackDepthCall *c) {
    if (K < 1) { set_error("%s: K = %d bins", api, K); return VITX_ERR_ARG; }
    if (K > kDepthMaxK) { set_error("%s: K = %d bins above %d", api, K, kDepthMaxK); return VITX_ERR_UNSUPPORTED; }
    if (u != 1 && u != 2 && u != 4) { set_error("%s: upsample = %d, not 1, 2 or 4", api, u); return VITX_ERR_UNSUPPORTED; }
    if (max_pixels < 1) { set_error("%s: max_pixels = %ld", api, max_pixels); return VITX_ERR_ARG; }
    if (out_shapes && n_out != n) { set_error("%s: output shapes were given for %d images, the call has %d", api, n_out, n); return VITX_ERR_ARG; }
    const int P = m->hp.patch_size;
    c->grids.resize((size_t)2 * n); c->outs.resize((size_t)2 * n);
    c->pix0.resize((size_t)n + 1); c->fine0.resize((size_t)n + 1); c->ftile0.resize((size_t)n + 1); c->otile0.resize((size_t)n + 1);
    for (int i = 0; i < n; ++i) {
        const int gh = shapes[2 * i] / P, gw = shapes[2 * i + 1] / P;
        const int oh = out_shapes ? out_shapes[2 * i] : shapes[2 * i], ow = out_shapes ? out_shapes[2 * i + 1] : shapes[2 * i + 1];
        if ((long)u * gh > kDepthMaxOut || (long)u * gw > kDepthMaxOut) {
            set_error("%s: image %d: fine plane %ld x %ld above %d", api, i, (long)u * gh, (long)u * gw, kDepthMaxOut);
            return VITX_ERR_UNSUPPORTED;
        }
        if (oh < u * gh || ow < u * gw || oh > kDepthMaxOut || ow > kDepthMaxOut) {
            set_error("%s: image %d: output %d x %d outside the fine plane %d x %d .. %d (upsampling only)", api, i, oh, ow, u * gh, u * gw, kDepthMaxOut);
            return VITX_ERR_ARG;
        }
        c->grids[2 * i] = gh; c->grids[2 * i + 1] = gw; c->outs[2 * i] = oh; c->outs[2 * i + 1] = ow;
    }
    if (!depth_pack_tables(c->grids.data(), c->outs.data(), n, u, c->pix0.data(), c->fine0.data(), c->ftile0.data(), c->otile0.data(), &c->cells)) {
        set_error("%s: the call's outputs hold more than 2^31 - 1 tiles", api);
        return VITX_ERR_ARG;
    }
    if (c->pix0[n] > (int64_t)max_pixels) { set_error("%s: the call's outputs hold %lld pixels, above max_pixels = %ld", api, (long long)c->pix0[n], max_pixels); return VITX_ERR_ARG; }
    return VITX_OK;
}

// What a forward call adds while u8 sources are declared for it (vitx_pack_u8_check's text; `shapes` has passed check_shapes): the sources' shapes
// [n_src][2] = (ny, nx) against the call, the tables (pp_pack_tables: its refusals) and the bytes against max_src_bytes (0: no bound).  On success the
// preprocessing's tables of the call in *c.
int check_u8(const char *api, const vitx_preproc &pp, const int32_t *src_shapes, int n_src, const int32_t *shapes, int n, size_t max_src_bytes, PackU8Call *c, int64_t *src0) {
    if (!src_shapes) { set_error("%s: NULL argument", api); return VITX_ERR_ARG; }
    if (n_src != n) { set_error("%s: u8 sources were declared for %d images, the call has %d", api, n_src, n); return VITX_ERR_ARG; }
    std::vector<int64_t> s0((size_t)n + 1);
    c->tile0.resize((size_t)n + 1); c->seg.resize((size_t)n * kPpSegInts);
    if (const int rc = pp_pack_tables(api, pp, src_shapes, shapes, n, s0.data(), nullptr, c->tile0.data(), c->seg.data(), &c->lds)) return rc;
    if (max_src_bytes && (uint64_t)s0[n] > (uint64_t)max_src_bytes) {
        set_error("%s: the call's sources hold %lld bytes, above max_src_bytes = %zu", api, (long long)s0[n], max_src_bytes);
        return VITX_ERR_ARG;
    }
    c->src_bytes = s0[n]; c->on = true;
    if (src0) std::copy(s0.begin(), s0.end(), src0);
    return VITX_OK;
}

// What a forward call adds while attention rollout is on with arenas of max_sq floats (vitx_pack_attn_check's text; row0 [n + 1] is check_shapes's):
// every image within the rollout kernels' token bound, the call's matrices within the arenas.  On success the rollout's tables of the call in *c.
// (Class maps alone refuse nothing: they live in max_tokens rows.)
int check_attn(const char *api, const int32_t *row0, int n, long max_sq, PackRolloutCall *c) {
    for (int i = 0; i < n; ++i)
        if (row0[i + 1] - row0[i] > kAttnMeanMaxTokens) {
            set_error("%s: image %d: rollout keeps two N x N matrices per image and takes at most %d tokens (this image: %d)", api, i, kAttnMeanMaxTokens, row0[i + 1] - row0[i]);
            return VITX_ERR_UNSUPPORTED;
        }
    c->rblk0.resize((size_t)n + 1); c->sq0.resize((size_t)n + 1);
    int64_t sq = 0;
    for (int i = 0; i < n; ++i) { const int64_t N = row0[i + 1] - row0[i]; sq += N * N; }
    if (sq > (int64_t)max_sq || !attn_pack_tables(row0, n, c->rblk0.data(), c->sq0.data(), &c->n_max)) {
        set_error("%s: the call's rollout matrices hold %lld floats (the sum of N_i^2), above max_sq_tokens = %ld", api, (long long)sq, max_sq);
        return VITX_ERR_ARG;
    }
    return VITX_OK;
}

// the distinct grids of a call, in order of first appearance, as (gh << 32 | gw)
std::vector<uint64_t> distinct_grids(const int32_t *shapes, int n, int P) {
    std::vector<uint64_t> g;
    for (int i = 0; i < n; ++i) {
        const uint64_t k = (uint64_t)(uint32_t)(shapes[2 * i] / P) << 32 | (uint32_t)(shapes[2 * i + 1] / P);
        if (std::find(g.begin(), g.end(), k) == g.end()) g.push_back(k);
    }
    return g;
}

// THE check of a forward call, for both entry points: everything the call can be refused for, before its first device call.  It consumes
// vitx_pack_dense_out's and vitx_pack_depth_out's shapes and vitx_pack_u8_sources's declaration, passed or refused, and touches nothing else of the
// context: a refused call leaves row0 and the parts' tables of the last forward that ran (vitx_pack_feat_read, vitx_pack_dense_read) alone.  d_imgs is
// only looked at, never read.
int check_call(vitx_pack *p, const void *d_imgs, const int32_t *shapes, int n, PackCall *c) {
    int rc;
    PackDense *dn = p->dense.get();
    PackDepth *dp = p->depth.get();
    PackU8 *u8 = p->u8.get();
    std::vector<int32_t> next_out, next_depth, next_src;
    if (dn) next_out.swap(dn->next_out);
    if (dp) next_depth.swap(dp->next_out);
    if (u8) next_src.swap(u8->next_src);
    const bool from_u8 = !next_src.empty();
    c->row0.resize((size_t)p->max_images + 1);
    if ((rc = check_shapes("vitx_pack_forward", p->model, shapes, n, p->max_tokens, p->max_images, c->row0.data()))) return rc;
    c->want = distinct_grids(shapes, n, p->P);
    if (c->want.size() > (size_t)p->max_grids) { set_error("vitx_pack_forward: the call names %d distinct grids, the table cache holds max_grids = %d", (int)c->want.size(), p->max_grids); return VITX_ERR_ARG; }
    if (dn && (rc = check_dense("vitx_pack_forward", p->model, shapes, next_out.empty() ? nullptr : next_out.data(), (int)(next_out.size() / 2), n, dn->K, dn->max_pixels, &c->dense))) return rc;
    if (dp && (rc = check_depth("vitx_pack_forward", p->model, shapes, next_depth.empty() ? nullptr : next_depth.data(), (int)(next_depth.size() / 2), n, dp->K, dp->u, dp->max_pixels, &c->depth))) return rc;
    if (p->rollout() && (rc = check_attn("vitx_pack_forward", c->row0.data(), n, p->attn->max_sq, &c->roll))) return rc;
    if (from_u8) {
        if ((uintptr_t)d_imgs & 3) { set_error("vitx_pack_forward: the u8 sources must be 4-byte aligned"); return VITX_ERR_ARG; }
        rc = check_u8("vitx_pack_forward", u8->pp, next_src.data(), (int)(next_src.size() / 2), shapes, n, u8->max_src_bytes, &c->u8, nullptr);
    }
    return rc;
}

// Attention maps of layer il (vitx_pack_attn_enable) from the QKV its qkv projection (and launch_rope_packed) has just written: the launch sequence of
// the image forward's attention_maps, per image of the pack.  The kernels only read QKV and write the maps' own buffers.  Rollout: A^_l goes to arena
// l & 1 and becomes R_l = A^_l R_(l-1) in place; the last layer contributes row 0 of its factor only, built from its class-token maps.
int pack_attention_maps(vitx_pack *p, const PackLayout &at, int il, int n, hipStream_t st) {
    PackAttn &am = *p->attn;
    const int D = p->D, H = p->H, L = p->L, dt = p->dtype, fpt = am.fpt;
    const int *d_row0 = p->tab + at.row0();
    float *const roll[2] = {am.roll[0].as<float>(), am.roll[1].as<float>()};
    const float *cls = nullptr;
    long cfpt = 0;
    int cslot = 0;
    if (am.selects(il)) { cls = am.out.as<float>(); cfpt = fpt; cslot = layer_slot(am.mask, il); }
    else if (am.rollout() && il + 1 == L) { cls = am.cls_last.as<float>(); cfpt = H; }
    if (cls) { HIP_TRY(launch_attention_cls_map_packed(dt, p->QKV, (float *)cls, cfpt, cslot, d_row0, n, D, H, st)); ++p->launches; }
    if (!am.rollout()) return VITX_OK;
    const int *d_rblk0 = p->tab + at.rblk0(), *d_sq0 = p->tab + at.sq0();
    const int blocks = am.last.rblk0[n], n_max = am.last.n_max;
    if (il + 1 < L) {
        float *a = roll[il & 1];
        HIP_TRY(launch_attention_head_mean_packed(dt, p->QKV, a, d_row0, d_rblk0, d_sq0, n, blocks, n_max, D, H, true, st)); ++p->launches;
        if (il > 0) { HIP_TRY(launch_rollout_step_packed(a, roll[(il + 1) & 1], d_row0, d_rblk0, d_sq0, n, blocks, n_max, st)); ++p->launches; }
        return VITX_OK;
    }
    HIP_TRY(launch_rollout_row_packed(cls, cfpt, cslot, L > 1 ? roll[(L - 2) & 1] : nullptr, am.out.as<float>(), fpt, fpt - 1, d_row0, d_sq0, n, n_max, H, st));
    ++p->launches;
    return VITX_OK;
}

int pack_gemm(vitx_pack *p, int epi, const GemmArgs &a, hipStream_t st) {
    HIP_TRY(launch_gemm(*p->tune, p->dtype, epi, a, st));
    ++p->launches;
    return VITX_OK;
}

// Each part's tables of a call into the staging buffer `host`, where the layout puts them.  lrow [n]: image i's first logit row, behind its prefix rows
void dense_tables(const PackDenseCall &c, const int32_t *lrow, int n, const PackLayout &at, int *host) {
    std::copy(c.tile0.begin(), c.tile0.end(), host + at.tile0());
    dense_pack_seg(c.grids.data(), c.outs.data(), lrow, c.pix0.data(), n, host + at.seg());
}
// image i's offsets are row i of the offsets (or, without a class half, the bias for every image)
void depth_tables(const PackDepthCall &c, const int32_t *lrow, int n, int u, const PackLayout &at, int *host) {
    std::vector<int32_t> orow(n);
    for (int i = 0; i < n; ++i) orow[i] = i;
    std::copy(c.ftile0.begin(), c.ftile0.end(), host + at.ftile0());
    std::copy(c.otile0.begin(), c.otile0.end(), host + at.otile0());
    depth_pack_seg(c.grids.data(), c.outs.data(), lrow, orow.data(), c.fine0.data(), c.pix0.data(), n, u, host + at.dseg());
}
void u8_tables(const PackU8Call &c, const PackLayout &at, int *host) {
    std::copy(c.tile0.begin(), c.tile0.end(), host + at.ptile0());
    std::copy(c.seg.begin(), c.seg.end(), host + at.pseg());
}
void rollout_tables(const PackRolloutCall &c, const PackLayout &at, int *host) {
    std::copy(c.rblk0.begin(), c.rblk0.end(), host + at.rblk0());
    std::copy(c.sq0.begin(), c.sq0.end(), host + at.sq0());
}

// A call that passed check_call: its rows and its parts' tables take the place of the last forward's, its grids are resolved; then the segment tables
// go up in one copy, then the launches
int pack_forward(vitx_pack *p, PackCall &c, const void *d_imgs, const int32_t *shapes, int n, float *d_probs, float *d_logits, hipStream_t st) {
    int rc;
    PackDense *dn = p->dense.get();
    PackDepth *dp = p->depth.get();
    PackAttn *am = p->attn.get();
    HIP_TRY(hipSetDevice(p->device));
    p->row0.swap(c.row0); p->feat_n = 0;
    if (dn) { std::swap(dn->last, c.dense); dn->n = 0; }
    if (dp) { std::swap(dp->last, c.depth); dp->n = 0; }
    if (am) { std::swap(am->last, c.roll); am->n = 0; }
    p->launches = p->pe_launches = 0;
    if ((rc = resolve_grids(p, c.want, st))) return rc;
    const WeightSet &ws = *p->wset;
    const PackLayout at = p->layout();
    const int D = p->D, H = p->H, P = p->P, Tp = p->Tp, tm = p->tm, tn = p->tn, dt = p->dtype, half = D / H / 2;
    const int rows = p->row0[n], M = round_up(rows, tm), Mh = round_up(n, tm);
    // staging: the previous call's upload may still be reading the buffer (this call only enqueues) -- wait for the upload, not for its forward
    if (p->uploaded_pending) { HIP_TRY(hipEventSynchronize(p->uploaded)); p->uploaded_pending = false; }
    int *host = p->host.data(), *h_row0 = host + at.row0(), *h_qb0 = host + at.qb0(), *h_toff = host + at.toff();
    std::vector<int32_t> lrow(n);
    long qblocks = 0;
    for (int i = 0; i < n; ++i) {
        h_row0[i] = p->row0[i]; h_qb0[i] = (int)qblocks; lrow[i] = p->row0[i] + Tp;
        qblocks += (p->row0[i + 1] - p->row0[i] + 63) / 64;
        h_toff[i] = (int)find_grid(p, shapes[2 * i] / P, shapes[2 * i + 1] / P)->rope_off;
    }
    h_row0[n] = rows; h_qb0[n] = (int)qblocks;
    // the parts' tables (check_call built them), in layout order
    if (dn) dense_tables(dn->last, lrow.data(), n, at, host);
    if (dp) depth_tables(dp->last, lrow.data(), n, dp->u, at, host);
    if (c.u8.on) u8_tables(c.u8, at, host);
    if (at.parts & kRollout) rollout_tables(am->last, at, host);
    HIP_TRY(hipMemcpyAsync(p->tab, p->host.data(), p->host.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(p->uploaded, st));
    p->uploaded_pending = true;
    const int *d_row0 = p->tab + at.row0(), *d_qb0 = p->tab + at.qb0(), *d_toff = p->tab + at.toff();
    // u8 sources: ONE launch stretches every source to its image's own shape into the context's pixel buffer, which the forward below reads
    const float *px = (const float *)d_imgs;
    if (c.u8.on) {
        const hipError_t e = launch_preprocess_pack(p->u8->pp, d_imgs, p->img.as<float>(), p->tab + at.ptile0(), p->tab + at.pseg(), n, c.u8.tile0[n], c.u8.lds, st);
        if (e != hipSuccess) { set_error("vitx_pack_forward: the u8 preprocessing: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
        ++p->launches;
        px = p->img.as<float>();
    }
    // patch embedding: one launch of the rectangular context's kernel per run of consecutive images of one shape, at the run's rows of X with the
    // position table of its grid -- the rows a rectangular context of that shape computes
    for (int i = 0; i < n;) {
        const int h = shapes[2 * i], w = shapes[2 * i + 1];
        int j = i + 1;
        while (j < n && shapes[2 * j] == h && shapes[2 * j + 1] == w) ++j;
        HIP_TRY(launch_patch_embed(dt, px, ws.pe_w, ws.pe_b, find_grid(p, h / P, w / P)->pos, ws.cls, ws.reg, p->nreg, p->X + (size_t)p->row0[i] * D, j - i, h, w, P, 3, D,
                                   round_up(D, tn), p->Kpe_pad, st));
        ++p->launches; ++p->pe_launches;
        px += (size_t)(j - i) * h * w * 3;
        i = j;
    }
    if (ws.pre_w) { HIP_TRY(launch_layernorm_f32(p->X, ws.pre_w, ws.pre_b, p->X, rows, D, p->eps, st)); ++p->launches; }
    int il = -1;
    for (const LayerW &w : ws.layers) {
        ++il;
        HIP_TRY(launch_layernorm(dt, p->X, D, w.ln1_w, w.ln1_b, p->U, D, rows, D, p->eps, st)); ++p->launches;
        if ((rc = pack_gemm(p, EPI_BIAS, dense_gemm(p->U, w.qkv_w, w.qkv_b, p->QKV, M, rows, 3 * D, round_up(3 * D, tn), D), st))) return rc;
        if (p->rope) {
            HIP_TRY(launch_rope_packed(dt, p->QKV, p->rope_cos, p->rope_sin, d_row0, d_toff, n, (long)rows - (long)n * Tp, half % 4 == 0, Tp, D, H, st));
            ++p->launches;
        }
        if (am && (rc = pack_attention_maps(p, at, il, n, st))) return rc;
        HIP_TRY(launch_attention_packed(dt, p->QKV, p->U, d_row0, d_qb0, n, qblocks, D, H, st)); ++p->launches;
        if ((rc = pack_gemm(p, EPI_BIAS_RESID, dense_gemm(p->U, w.proj_w, w.proj_b, p->X, M, rows, D, round_up(D, tn), D), st))) return rc;
        HIP_TRY(launch_layernorm(dt, p->X, D, w.ln2_w, w.ln2_b, p->U, D, rows, D, p->eps, st)); ++p->launches;
        if ((rc = pack_gemm(p, p->fc1_epi, dense_gemm(p->U, w.fc1_w, w.fc1_b, p->Hbuf, M, rows, p->F1, round_up(p->F1, tn), D), st))) return rc;
        if (p->glu) { HIP_TRY(launch_swiglu(dt, p->Hbuf, p->F1, p->Hg, p->F, rows, p->F, st)); ++p->launches; }
        if ((rc = pack_gemm(p, EPI_BIAS_RESID, dense_gemm(p->glu ? p->Hg : p->Hbuf, w.fc2_w, w.fc2_b, p->X, M, rows, D, round_up(D, tn), p->F), st))) return rc;
        // the dense head's operand: the final norm of every row of the pack as layer il stands, rounded to the operand type into the layer's column
        // slot of the compact rows [M][Dc] (the stand-alone LayerNorm: the rows a rectangular context's head reads, and the prefix rows, never used)
        if (dn && dn->selects(il)) {
            HIP_TRY(launch_layernorm(dt, p->X, D, ws.norm_w, ws.norm_b, dn->a[0].as<char>() + dn->col(il, D) * 2, dn->Dc, rows, D, p->eps, st));
            ++p->launches;
        }
        // the depth head's operand: the same rows raw, through the streaming conversion, or (VITX_DEPTH_NORM) through the final norm; the class rows
        // of a class half are gathered from them after the forward
        if (dp && dp->selects(il)) {
            void *y = dp->a[0].as<char>() + dp->col(il, D) * 2;
            if (dp->flags & VITX_DEPTH_NORM) HIP_TRY(launch_layernorm(dt, p->X, D, ws.norm_w, ws.norm_b, y, dp->Dc, rows, D, p->eps, st));
            else HIP_TRY(launch_depth_rows(dt, p->X, D, y, dp->Dc, rows, D, st));
            ++p->launches;
        }
    }
    // the class rows through the final norm (row0[i] is image i's class row), the head GEMM in f32, the class softmax
    HIP_TRY(launch_pool_rows(dt, p->X, d_row0, ws.norm_w, ws.norm_b, p->Z, n, Mh, D, p->eps, st)); ++p->launches;
    float *lg = d_logits ? d_logits : p->logits;
    const int ldl = d_logits ? p->C : p->C_pad;
    if ((rc = pack_gemm(p, EPI_BIAS_F32, dense_gemm(p->Z, ws.head_w, ws.head_b, lg, Mh, n, p->C, p->C_pad, D, ldl), st))) return rc;
    HIP_TRY(launch_softmax(dt, lg, d_probs, n, p->C, ldl, st)); ++p->launches;
    // features (vitx_pack_feat_enable): the f32 final norm of every row of the pack; vitx_pack_feat_read gathers the rows it was asked for
    if (p->feat_flags) { HIP_TRY(launch_layernorm_f32(p->X, ws.norm_w, ws.norm_b, p->feat.as<float>(), rows, D, p->eps, st)); ++p->launches; p->feat_n = n; }
    // the dense head: the logits of every row of the pack, then one label launch over the images' own output shapes (2 launches; the memset of
    // the operand's pad rows is not a kernel)
    if (dn) {
        const hipError_t e = head_dense_packed(HeadLaunch{*p->tune, dt, st, nullptr}, dn->a[0].p, dn->W.p, dn->bias.as<float>(), dn->acc[0].as<float>(), rows, dn->K, dn->Dc,
                                               p->tab + at.tile0(), p->tab + at.seg(), n, dn->last.tile0[n], dn->last.cells, (long)dn->last.pix0[n], dn->labels.as<uint8_t>(),
                                               dn->score ? dn->score.as<float>() : nullptr, dn->logits ? dn->logits.as<float>() : nullptr);
        if (e != hipSuccess) { set_error("vitx_pack_forward: the dense head: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
        p->launches += 2;
        dn->n = n;
    }
    // the depth head: the logits of every row of the pack, with a class half the gathered class rows and their offsets, then the fine planes and the
    // maps over the images' own shapes (3 launches, 5 with a class half)
    if (dp) {
        const bool cls = (bool)dp->Wc;
        const hipError_t e = head_depth_packed(HeadLaunch{*p->tune, dt, st, nullptr}, dp->a[0].p, dp->Wp.p, dp->zero.as<float>(), dp->acc[0].as<float>(), cls ? dp->ac[0].p : nullptr,
                                               dp->Wc.p, dp->bias.as<float>(), cls ? dp->o[0].as<float>() : nullptr, dp->bins.as<float>(), rows, dp->K, dp->Dc, d_row0,
                                               p->tab + at.ftile0(), p->tab + at.otile0(), p->tab + at.dseg(), n, dp->last.ftile0[n], dp->last.otile0[n], dp->last.cells, (long)dp->last.fine0[n],
                                               (long)dp->last.pix0[n], dp->lo, dp->hi, dp->fine.as<float>(), dp->depth.as<float>(), dp->logits ? dp->logits.as<float>() : nullptr,
                                               dp->off ? dp->off.as<float>() : nullptr);
        if (e != hipSuccess) { set_error("vitx_pack_forward: the depth head: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
        p->launches += cls ? 5 : 3;
        dp->n = n;
    }
    if (am) am->n = n;
    HIP_TRY(hipEventRecord(p->done, st));
    p->done_pending = true;
    return VITX_OK;
}

// What both host entry points do behind their upload to d_in: the forward on the context's stream, the results down, the stream drained
int host_forward(vitx_pack *p, PackCall &c, const void *d_in, const int32_t *shapes, int n, float *probs, float *logits) {
    if (const int rc = pack_forward(p, c, d_in, shapes, n, p->probs, logits ? p->logits_out : nullptr, p->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(probs, p->probs, (size_t)n * p->C * 4, hipMemcpyDeviceToHost, p->stream));
    if (logits) HIP_TRY(hipMemcpyAsync(logits, p->logits_out, (size_t)n * p->C * 4, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return VITX_OK;
}

}  // namespace

int pack_attn_args(const char *api, int L, uint64_t layer_mask, int flags, long max_sq_tokens) {
    if (flags & ~VITX_ATTN_ROLLOUT) { set_error("%s: unknown flags 0x%x", api, flags); return VITX_ERR_ARG; }
    if (L < 64 && (layer_mask >> L)) { set_error("%s: layer mask 0x%llx names layers beyond the model's %d", api, (unsigned long long)layer_mask, L); return VITX_ERR_ARG; }
    if ((flags & VITX_ATTN_ROLLOUT) && (max_sq_tokens < 1 || max_sq_tokens > 0x7fffffffL)) {
        set_error("%s: VITX_ATTN_ROLLOUT needs max_sq_tokens (the call's sum of N_i^2) in 1 .. 2^31 - 1, not %ld", api, max_sq_tokens);
        return VITX_ERR_ARG;
    }
    return VITX_OK;
}

extern "C" {

int vitx_pack_check(const vitx_model *m, const int32_t *shapes, int n, int max_tokens, int max_images, int32_t *row0) {
    return check_shapes("vitx_pack_check", m, shapes, n, max_tokens, max_images, row0);
}
int vitx_pack_distinct_grids(const vitx_model *m, const int32_t *shapes, int n) {
    if (!m || !shapes || n < 1 || m->hp.patch_size <= 0) return 0;
    return (int)distinct_grids(shapes, n, m->hp.patch_size).size();
}
int vitx_pack_dense_check(const vitx_model *m, const int32_t *shapes, const int32_t *out_shapes, int n, int K, long max_pixels, int64_t *pix0, int32_t *tile0) {
    // max_tokens / max_images: whatever holds the call -- their refusals are vitx_pack_check's
    if (const int rc = check_shapes("vitx_pack_dense_check", m, shapes, n, 0x7fffffff, n, nullptr)) return rc;
    PackDenseCall c;
    if (const int rc = check_dense("vitx_pack_dense_check", m, shapes, out_shapes, n, n, K, max_pixels, &c)) return rc;
    if (pix0) std::copy(c.pix0.begin(), c.pix0.end(), pix0);
    if (tile0) std::copy(c.tile0.begin(), c.tile0.end(), tile0);
    return VITX_OK;
}

int vitx_pack_depth_check(const vitx_model *m, const int32_t *shapes, const int32_t *out_shapes, int n, int K, int upsample, long max_pixels, int64_t *pix0, int64_t *fine0,
                          int32_t *ftile0, int32_t *otile0) {
    if (const int rc = check_shapes("vitx_pack_depth_check", m, shapes, n, 0x7fffffff, n, nullptr)) return rc;
    PackDepthCall c;
    if (const int rc = check_depth("vitx_pack_depth_check", m, shapes, out_shapes, n, n, K, upsample, max_pixels, &c)) return rc;
    if (pix0) std::copy(c.pix0.begin(), c.pix0.end(), pix0);
    if (fine0) std::copy(c.fine0.begin(), c.fine0.end(), fine0);
    if (ftile0) std::copy(c.ftile0.begin(), c.ftile0.end(), ftile0);
    if (otile0) std::copy(c.otile0.begin(), c.otile0.end(), otile0);
    return VITX_OK;
}

int vitx_pack_attn_check(const vitx_model *m, const int32_t *shapes, int n, uint64_t layer_mask, int flags, long max_sq_tokens, int32_t *rblk0, int32_t *sq0) {
    if (!m || !shapes) { set_error("vitx_pack_attn_check: NULL argument"); return VITX_ERR_ARG; }
    if (n < 1) { set_error("vitx_pack_attn_check: n = %d", n); return VITX_ERR_ARG; }
    // max_tokens / max_images: whatever holds the call -- their refusals are vitx_pack_check's
    std::vector<int32_t> row0((size_t)n + 1);
    if (const int rc = check_shapes("vitx_pack_attn_check", m, shapes, n, 0x7fffffff, n, row0.data())) return rc;
    if (const int rc = pack_attn_args("vitx_pack_attn_check", m->hp.num_hidden_layers, layer_mask, flags, max_sq_tokens)) return rc;
    PackRolloutCall c;
    if (flags & VITX_ATTN_ROLLOUT) {
        if (const int rc = check_attn("vitx_pack_attn_check", row0.data(), n, max_sq_tokens, &c)) return rc;
    } else {           // class maps alone refuse nothing per call; the tables are still the call's
        c.rblk0.resize((size_t)n + 1); c.sq0.resize((size_t)n + 1);
        if (!attn_pack_tables(row0.data(), n, c.rblk0.data(), c.sq0.data(), &c.n_max)) { set_error("vitx_pack_attn_check: the sum of N_i^2 leaves 31 bits"); return VITX_ERR_ARG; }
    }
    if (rblk0) std::copy(c.rblk0.begin(), c.rblk0.end(), rblk0);
    if (sq0) std::copy(c.sq0.begin(), c.sq0.end(), sq0);
    return VITX_OK;
}

int vitx_pack_forward_device(vitx_pack *p, const void *d_imgs, const int32_t *shapes, int n, void *d_probs, void *d_logits, void *stream) {
    if (!p || !d_imgs || !shapes || !d_probs) { set_error("vitx_pack_forward_device: NULL argument"); return VITX_ERR_ARG; }
    PackCall c;
    if (const int rc = check_call(p, d_imgs, shapes, n, &c)) return rc;
    return pack_forward(p, c, d_imgs, shapes, n, (float *)d_probs, (float *)d_logits, stream ? (hipStream_t)stream : p->stream);
}

int vitx_pack_forward(vitx_pack *p, const float *imgs, const int32_t *shapes, int n, float *probs, float *logits) {
    if (!p || !imgs || !shapes || !probs) { set_error("vitx_pack_forward: NULL argument"); return VITX_ERR_ARG; }
    PackCall c;
    if (const int rc = check_call(p, imgs, shapes, n, &c)) return rc;  // before the pixels go up
    if (c.u8.on) { set_error("vitx_pack_forward: u8 sources were declared for this call (vitx_pack_u8_sources): it takes vitx_pack_forward_device or vitx_pack_forward_u8"); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(p->device));
    if (!p->img) {       // the pixels of a full pack: max_tokens patches
        const size_t bytes = (size_t)p->max_tokens * p->P * p->P * 3 * 4;
        HIP_TRY(hipMalloc(&p->img.p, bytes));
        p->scratch_bytes += bytes;
    }
    size_t floats = 0;
    for (int i = 0; i < n; ++i) floats += (size_t)shapes[2 * i] * shapes[2 * i + 1] * 3;
    HIP_TRY(hipMemcpyAsync(p->img.p, imgs, floats * 4, hipMemcpyHostToDevice, p->stream));
    return host_forward(p, c, p->img.p, shapes, n, probs, logits);
}

// u8 sources: the host entry point -- vitx_pack_forward's shape on u8.  The declaration is made here and consumed by check_call, like any other.
int vitx_pack_forward_u8(vitx_pack *p, const uint8_t *srcs, const int32_t *src_shapes, const int32_t *shapes, int n, float *probs, float *logits) {
    if (!p || !srcs || !src_shapes || !shapes || !probs) { set_error("vitx_pack_forward_u8: NULL argument"); return VITX_ERR_ARG; }
    if (const int rc = vitx_pack_u8_sources(p, src_shapes, n)) return rc;
    PackCall c;
    if (const int rc = check_call(p, p->u8->src.p, shapes, n, &c)) return rc;        // before the sources go up
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(p->u8->src.p, srcs, (size_t)c.u8.src_bytes, hipMemcpyHostToDevice, p->stream));
    return host_forward(p, c, p->u8->src.p, shapes, n, probs, logits);
}

int vitx_pack_u8_check(const vitx_model *m, const vitx_preproc *pp, const int32_t *src_shapes, const int32_t *shapes, int n, size_t max_src_bytes, int64_t *src0,
                       int32_t *tile0, int *lds) {
    // max_tokens / max_images: whatever holds the call -- their refusals are vitx_pack_check's
    if (const int rc = check_shapes("vitx_pack_u8_check", m, shapes, n, 0x7fffffff, n, nullptr)) return rc;
    vitx_preproc own;
    if (!pp) { if (const int rc = vitx_model_preproc(m, &own)) return rc; pp = &own; }
    PackU8Call c;
    if (const int rc = check_u8("vitx_pack_u8_check", *pp, src_shapes, n, shapes, n, max_src_bytes, &c, src0)) return rc;
    if (tile0) std::copy(c.tile0.begin(), c.tile0.end(), tile0);
    if (lds) *lds = c.lds;
    return VITX_OK;
}

}  // extern "C"
