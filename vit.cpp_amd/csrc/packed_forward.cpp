// packed_forward.cpp -- the packed context and its forward (include/vitx.h "packed batches"): n images of different shapes, their tokens end
// to end in one residual stream, one forward.  The blocks are the image forward's row-wise launches through the same dispatchers (GEMMs,
// LayerNorm, activation, gate, pre-norm do not care where one image ends); new are the three launches that must know: the variable-length
// attention (attention_packed.hip), the rotary embeddings by a segment table (rope.hip) and the class-row gather (text_embed.hip).  The patch
// embedding is the rectangular context's kernel, one launch per run of consecutive images of one shape.  The one opt-in head is the dense head
// (vitx_pack_dense_set): the stand-alone LayerNorm and the head GEMM over all rows of the pack, then the label launch by its own segment table
// (dense_label.hip), one map per image at its own size.
// One stream, no sub-batch split, no hipGraph cache, no LayerNorm fusion, no class-token tail; block matrices are expanded at upload, as in
// the text context (text_forward.cpp).
#include <string.h>

#include <algorithm>
#include <cmath>
#include <new>

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
// check_shapes): the output shapes -- out_shapes [n_out][2], or the images' own -- against the grids and the buffers.  On success the call's
// tables: grids and outs [n][2], pix0 and tile0 [n + 1] (any may be NULL), *cells (dense_pack_tables).
int check_dense(const char *api, const vitx_model *m, const int32_t *shapes, const int32_t *out_shapes, int n_out, int n, int K, long max_pixels, int32_t *grids,
                int32_t *outs, int64_t *pix0, int32_t *tile0, int *cells) {
    if (K < 1) { set_error("%s: K = %d classes", api, K); return VITX_ERR_ARG; }
    if (K > kDenseMaxK) { set_error("%s: K = %d classes above %d (labels are bytes)", api, K, kDenseMaxK); return VITX_ERR_UNSUPPORTED; }
    if (max_pixels < 1) { set_error("%s: max_pixels = %ld", api, max_pixels); return VITX_ERR_ARG; }
    if (out_shapes && n_out != n) { set_error("%s: output shapes were given for %d images, the call has %d", api, n_out, n); return VITX_ERR_ARG; }
    const int P = m->hp.patch_size;
    std::vector<int32_t> g((size_t)2 * n), o((size_t)2 * n);
    std::vector<int64_t> px((size_t)n + 1);
    for (int i = 0; i < n; ++i) {
        const int gh = shapes[2 * i] / P, gw = shapes[2 * i + 1] / P;
        const int oh = out_shapes ? out_shapes[2 * i] : shapes[2 * i], ow = out_shapes ? out_shapes[2 * i + 1] : shapes[2 * i + 1];
        if (oh < gh || ow < gw || oh > kDenseMaxOut || ow > kDenseMaxOut) {
            set_error("%s: image %d: output %d x %d outside the patch grid %d x %d .. %d (upsampling only)", api, i, oh, ow, gh, gw, kDenseMaxOut);
            return VITX_ERR_ARG;
        }
        g[2 * i] = gh; g[2 * i + 1] = gw; o[2 * i] = oh; o[2 * i + 1] = ow;
    }
    if (!dense_pack_tables(g.data(), o.data(), n, px.data(), tile0, cells)) { set_error("%s: the call's outputs hold more than 2^31 - 1 tiles", api); return VITX_ERR_ARG; }
    if (px[n] > (int64_t)max_pixels) { set_error("%s: the call's outputs hold %lld pixels, above max_pixels = %ld", api, (long long)px[n], max_pixels); return VITX_ERR_ARG; }
    if (grids) std::copy(g.begin(), g.end(), grids);
    if (outs) std::copy(o.begin(), o.end(), outs);
    if (pix0) std::copy(px.begin(), px.end(), pix0);
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

PackGrid *find_grid(vitx_pack *p, int gh, int gw) {
    for (PackGrid &g : p->grids) if (g.gh == gh && g.gw == gw) return &g;
    return nullptr;
}

// Before a table is freed or overwritten: the last forward of this context, which may still read it on another stream, is waited for
int wait_done(vitx_pack *p) {
    if (p->done_pending) { HIP_TRY(hipEventSynchronize(p->done)); p->done_pending = false; }
    return VITX_OK;
}
void drop_grid(vitx_pack *p, size_t k) {
    PackGrid &g = p->grids[k];
    if (g.own) { (void)hipFree(g.pos); p->scratch_bytes -= ((size_t)g.gh * g.gw + 1) * p->D * 4; }
    p->grids.erase(p->grids.begin() + k);
}

// The tables of every grid the call names, built the first time a call names them: the position table by launch_pos_resample on the call's
// stream, the rotary table on the host (vitx_model_rope_table) and uploaded.  The cache holds max_grids grids; the least recently used grid
// the call does not name goes first.  A rotary table takes the next free piece of the arenas; when they are full the cache starts over.
int resolve_grids(vitx_pack *p, const std::vector<uint64_t> &want, hipStream_t st) {
    const int half = p->D / p->H / 2;
    ++p->tick;
    size_t missing = 0; long rope_need = 0;
    for (uint64_t k : want) {
        const int gh = (int)(k >> 32), gw = (int)(uint32_t)k;
        if (PackGrid *g = find_grid(p, gh, gw)) g->used = p->tick;
        else { ++missing; rope_need += (long)gh * gw * half; }
    }
    if (!missing) return VITX_OK;
    int rc;
    if (p->rope && p->rope_top + rope_need > p->rope_cap) {          // the arenas are full: every grid of the call is built again from their start
        if ((rc = wait_done(p))) return rc;
        while (!p->grids.empty()) drop_grid(p, p->grids.size() - 1);
        p->rope_top = 0;
    }
    while (p->grids.size() + missing > (size_t)p->max_grids) {       // (a call names at most max_grids grids: there is always one it does not name)
        size_t lru = p->grids.size();
        for (size_t k = 0; k < p->grids.size(); ++k)
            if (p->grids[k].used != p->tick && (lru == p->grids.size() || p->grids[k].used < p->grids[lru].used)) lru = k;
        if (lru == p->grids.size()) break;
        if ((rc = wait_done(p))) return rc;
        drop_grid(p, lru);
    }
    for (uint64_t k : want) {
        const int gh = (int)(k >> 32), gw = (int)(uint32_t)k;
        if (find_grid(p, gh, gw)) continue;
        PackGrid g;
        g.gh = gh; g.gw = gw; g.used = p->tick;
        if (gh == p->g_in && gw == p->g_in) g.pos = p->wset->pos;        // the file's own grid: the file's table, as in a context of the file's size
        else {
            const size_t bytes = ((size_t)gh * gw + 1) * p->D * 4;
            HIP_TRY(hipMalloc((void **)&g.pos, bytes));
            g.own = true; p->scratch_bytes += bytes;
            const hipError_t e = launch_pos_resample(p->wset->pos, p->g_in, p->g_in, p->D, gh, gw, p->pos_interp, g.pos, st);
            if (e != hipSuccess) { (void)hipFree(g.pos); p->scratch_bytes -= bytes; set_error("vitx_pack_forward: launch_pos_resample: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
            ++p->launches;
        }
        if (p->rope) {
            const size_t tab = (size_t)gh * gw * half;
            std::vector<float> h(2 * tab);
            rc = vitx_model_rope_table(p->model, gh, gw, h.data(), h.data() + tab);
            // a fresh piece of the arenas: nothing reads it yet, so the (synchronous) upload needs no ordering
            hipError_t e = rc ? hipSuccess : hipMemcpy(p->rope_cos + p->rope_top, h.data(), tab * 4, hipMemcpyHostToDevice);
            if (!rc && e == hipSuccess) e = hipMemcpy(p->rope_sin + p->rope_top, h.data() + tab, tab * 4, hipMemcpyHostToDevice);
            if (rc || e != hipSuccess) {
                if (g.own) { (void)hipFree(g.pos); p->scratch_bytes -= ((size_t)gh * gw + 1) * p->D * 4; }
                if (!rc) { set_error("vitx_pack_forward: rotary table upload: %s", hipGetErrorString(e)); rc = VITX_ERR_HIP; }
                return rc;
            }
            g.rope_off = p->rope_top; p->rope_top += (long)tab;
        }
        p->grids.push_back(g);
    }
    return VITX_OK;
}

int pack_gemm(vitx_pack *p, int epi, const GemmArgs &a, hipStream_t st) {
    HIP_TRY(launch_gemm(*p->tune, p->dtype, epi, a, st));
    ++p->launches;
    return VITX_OK;
}

// row0 (p->row0) and the grids are resolved; the segment tables go up in one copy, then the launches
int pack_forward(vitx_pack *p, const float *d_imgs, const int32_t *shapes, int n, float *d_probs, float *d_logits, hipStream_t st) {
    const WeightSet &ws = *p->wset;
    const int D = p->D, H = p->H, P = p->P, Tp = p->Tp, tm = p->tm, tn = p->tn, dt = p->dtype, cap = p->max_images, half = D / H / 2;
    const int rows = p->row0[n], M = round_up(rows, tm), Mh = round_up(n, tm);
    int rc;
    // staging: the previous call's upload may still be reading the buffer (this call only enqueues) -- wait for the upload, not for its forward
    if (p->uploaded_pending) { HIP_TRY(hipEventSynchronize(p->uploaded)); p->uploaded_pending = false; }
    int *h_row0 = p->host.data(), *h_qb0 = h_row0 + cap + 1, *h_toff = h_qb0 + cap + 1;
    long qblocks = 0;
    for (int i = 0; i < n; ++i) {
        h_row0[i] = p->row0[i]; h_qb0[i] = (int)qblocks;
        qblocks += (p->row0[i + 1] - p->row0[i] + 63) / 64;
        h_toff[i] = (int)find_grid(p, shapes[2 * i] / P, shapes[2 * i + 1] / P)->rope_off;
    }
    h_row0[n] = rows; h_qb0[n] = (int)qblocks;
    // the dense head's tables (pack_call checked and built them): image i's logit rows start behind its prefix rows
    PackDense *dn = p->dense.get();
    const size_t tile0_at = (size_t)3 * cap + 2, seg_at = tile0_at + cap + 1;        // ints into host / tab, there while a head is set
    if (dn) {
        int *h_tile0 = p->host.data() + tile0_at, *h_seg = p->host.data() + seg_at;
        std::vector<int32_t> lrow(n);
        for (int i = 0; i < n; ++i) lrow[i] = p->row0[i] + Tp;
        std::copy(dn->tile0.begin(), dn->tile0.end(), h_tile0);
        dense_pack_seg(dn->grids.data(), dn->outs.data(), lrow.data(), dn->pix0.data(), n, h_seg);
    }
    HIP_TRY(hipMemcpyAsync(p->tab, p->host.data(), p->host.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(p->uploaded, st));
    p->uploaded_pending = true;
    const int *d_row0 = p->tab, *d_qb0 = p->tab + cap + 1, *d_toff = d_qb0 + cap + 1;
    // patch embedding: one launch of the rectangular context's kernel per run of consecutive images of one shape, at the run's rows of X with the
    // position table of its grid -- the rows a rectangular context of that shape computes
    const float *px = d_imgs;
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
    }
    // the class rows through the final norm (row0[i] is image i's class row), the head GEMM in f32, the class softmax
    HIP_TRY(launch_pool_rows(dt, p->X, d_row0, ws.norm_w, ws.norm_b, p->Z, n, Mh, D, p->eps, st)); ++p->launches;
    float *lg = d_logits ? d_logits : p->logits;
    const int ldl = d_logits ? p->C : p->C_pad;
    if ((rc = pack_gemm(p, EPI_BIAS_F32, dense_gemm(p->Z, ws.head_w, ws.head_b, lg, Mh, n, p->C, p->C_pad, D, ldl), st))) return rc;
    HIP_TRY(launch_softmax(dt, lg, d_probs, n, p->C, ldl, st)); ++p->launches;
    // features (vitx_pack_feat_enable): the f32 final norm of every row of the pack; vitx_pack_feat_read gathers the rows it was asked for
    if (p->feat_flags) { HIP_TRY(launch_layernorm_f32(p->X, ws.norm_w, ws.norm_b, p->feat, rows, D, p->eps, st)); ++p->launches; p->feat_n = n; }
    // the dense head: the logits of every row of the pack, then one label launch over the images' own output shapes (2 launches; the memset of
    // the operand's pad rows is not a kernel)
    if (dn) {
        const hipError_t e = head_dense_packed(HeadLaunch{*p->tune, dt, st, nullptr}, dn->a[0].p, dn->W.p, dn->bias.as<float>(), dn->acc[0].as<float>(), rows, dn->K, dn->Dc,
                                               p->tab + tile0_at, p->tab + seg_at, n, dn->tile0[n], dn->cells, (long)dn->pix0[n], dn->labels.as<uint8_t>(),
                                               dn->score ? dn->score.as<float>() : nullptr, dn->logits ? dn->logits.as<float>() : nullptr);
        if (e != hipSuccess) { set_error("vitx_pack_forward: the dense head: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
        p->launches += 2;
        dn->n = n;
    }
    HIP_TRY(hipEventRecord(p->done, st));
    p->done_pending = true;
    return VITX_OK;
}

// Everything a call can be refused for comes before its first device call
int pack_call(vitx_pack *p, const void *d_imgs, const int32_t *shapes, int n, void *d_probs, void *d_logits, hipStream_t st) {
    int rc;
    PackDense *dn = p->dense.get();
    std::vector<int32_t> next_out;              // vitx_pack_dense_out: this call consumes the shapes, run or refused
    if (dn) next_out.swap(dn->next_out);
    if ((rc = check_shapes("vitx_pack_forward", p->model, shapes, n, p->max_tokens, p->max_images, p->chk.data()))) return rc;
    const std::vector<uint64_t> want = distinct_grids(shapes, n, p->P);
    if (want.size() > (size_t)p->max_grids) { set_error("vitx_pack_forward: the call names %d distinct grids, the table cache holds max_grids = %d", (int)want.size(), p->max_grids); return VITX_ERR_ARG; }
    if (dn) {       // into locals: a refused call leaves the tables of the last forward (vitx_pack_dense_read) alone
        std::vector<int32_t> g((size_t)2 * n), o((size_t)2 * n), t0((size_t)n + 1);
        std::vector<int64_t> px((size_t)n + 1);
        int cells = 0;
        if ((rc = check_dense("vitx_pack_forward", p->model, shapes, next_out.empty() ? nullptr : next_out.data(), (int)(next_out.size() / 2), n, dn->K, dn->max_pixels,
                              g.data(), o.data(), px.data(), t0.data(), &cells))) return rc;
        dn->grids.swap(g); dn->outs.swap(o); dn->pix0.swap(px); dn->tile0.swap(t0); dn->cells = cells; dn->n = 0;
    }
    HIP_TRY(hipSetDevice(p->device));
    p->row0 = p->chk; p->feat_n = 0;
    p->launches = p->pe_launches = 0;
    if ((rc = resolve_grids(p, want, st))) return rc;
    return pack_forward(p, (const float *)d_imgs, shapes, n, (float *)d_probs, (float *)d_logits, st);
}

}  // namespace

extern "C" {

int vitx_pack_check(const vitx_model *m, const int32_t *shapes, int n, int max_tokens, int max_images, int32_t *row0) {
    return check_shapes("vitx_pack_check", m, shapes, n, max_tokens, max_images, row0);
}
int vitx_pack_distinct_grids(const vitx_model *m, const int32_t *shapes, int n) {
    if (!m || !shapes || n < 1 || m->hp.patch_size <= 0) return 0;
    return (int)distinct_grids(shapes, n, m->hp.patch_size).size();
}

int vitx_pack_create(const vitx_model *m, int device, int max_tokens, int max_images, int dtype, const vitx_pack_options *opt, vitx_pack **out) {
    if (!m || !out || max_tokens <= 0 || max_images <= 0) { set_error("vitx_pack_create: invalid argument"); return VITX_ERR_ARG; }
    *out = nullptr;
    if (m->kind != VITX_KIND_IMAGE) { set_error("vitx_pack_create: a text-tower model takes a text context (vitx_text_create), not a packed context"); return VITX_ERR_ARG; }
    if (dtype == VITX_MXFP8) { set_error("vitx_pack_create: VITX_MXFP8 is not supported by packed contexts (VITX_F16 or VITX_BF16)"); return VITX_ERR_UNSUPPORTED; }
    if (dtype != VITX_F16 && dtype != VITX_BF16) { set_error("vitx_pack_create: unknown dtype %d", dtype); return VITX_ERR_ARG; }
    const int pos_interp = opt ? opt->pos_interp : VITX_POS_BICUBIC, max_grids = opt && opt->max_grids ? opt->max_grids : 32;
    if (pos_interp != VITX_POS_BICUBIC && pos_interp != VITX_POS_BICUBIC_AA) { set_error("vitx_pack_create: unknown pos_interp %d (0 bicubic, 1 bicubic with antialias)", pos_interp); return VITX_ERR_ARG; }
    if (max_grids < 1) { set_error("vitx_pack_create: max_grids %d is not positive", max_grids); return VITX_ERR_ARG; }
    // every refusal before the first device call: nothing is launched after one
    if (m->in_chans == 1) { set_error("vitx_pack_create: a ViTSTR (one-channel) model takes no packed context"); return VITX_ERR_UNSUPPORTED; }
    if (m->head_pool != VITX_POOL_CLS) { set_error("vitx_pack_create: packed contexts take the class-token head only, not the pooled (cls + mean) or the attention-pooling head"); return VITX_ERR_UNSUPPORTED; }
    const vitx_hparams &hp = m->hp;
    const int D = hp.hidden_size, H = hp.num_attention_heads, F1 = m->mlp_fc1_rows();
    if (!attention_packed_supports(D, H)) { set_error("vitx_pack_create: attention needs a head_dim that is a multiple of 8 up to 128 (this model: %d / %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    if (!layernorm_supports(D)) { set_error("vitx_pack_create: hidden_size %d has no LayerNorm instantiation", D); return VITX_ERR_UNSUPPORTED; }
    if (m->rope_kind && !rope_supports(D, H)) { set_error("vitx_pack_create: rotary position embeddings need an even head dim (D %d, H %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    if (hp.patch_size <= 0 || hp.img_size % hp.patch_size) { set_error("vitx_pack_create: the file's img_size %d is not a multiple of its patch size %d", hp.img_size, hp.patch_size); return VITX_ERR_UNSUPPORTED; }
    if ((long)max_tokens > (long)(0xf0000000u / ((size_t)std::max(F1, 3 * D) * 2)) / 256 * 256) { set_error("vitx_pack_create: max_tokens %d exceeds the kernels' 32-bit buffer window", max_tokens); return VITX_ERR_UNSUPPORTED; }
    const Tuning *tune = nullptr;
    int rc;
    if ((rc = open_device("vitx_pack_create", device, &tune))) return rc;
    std::unique_ptr<vitx_pack> p(new (std::nothrow) vitx_pack());
    if (!p) return VITX_ERR_NOMEM;
    p->model = m; p->device = device; p->dtype = dtype; p->tune = tune;
    p->D = D; p->L = hp.num_hidden_layers; p->H = H; p->C = hp.num_classes; p->C_pad = head_cols_pad(m); p->P = hp.patch_size;
    p->nreg = m->num_registers; p->Tp = 1 + p->nreg; p->g_in = hp.img_size / hp.patch_size; p->Kpe_pad = patch_k_pad(m);
    p->glu = m->glu_kind != VITX_GLU_NONE; p->F = m->mlp_hidden(); p->F1 = F1; p->rope = m->rope_kind != VITX_ROPE_NONE;
    p->fc1_epi = p->glu ? EPI_BIAS : act_epi(m->activation); p->eps = hp.eps;
    p->tm = gemm_tile_m(); p->tn = gemm_tile_n();
    p->max_tokens = max_tokens; p->max_images = max_images; p->max_grids = max_grids; p->pos_interp = pos_interp;
    // quantised block matrices are expanded at upload: block mode 0, as in the text context
    if ((rc = obtain_weights({m, device, dtype, false}, &p->wset, &p->weights_shared))) return rc;
    auto dmalloc = [&](void **q, size_t bytes) -> int {
        HIP_TRY(hipMalloc(q, bytes));
        p->allocs.push_back(*q); p->scratch_bytes += bytes;
        HIP_TRY(hipMemset(*q, 0, bytes));
        return VITX_OK;
    };
    const size_t Mp = (size_t)round_up(max_tokens, p->tm), Bp = (size_t)round_up(max_images, p->tm);
    p->host.assign((size_t)3 * max_images + 2, 0);
    p->row0.assign((size_t)max_images + 1, 0); p->chk = p->row0;
    if ((rc = dmalloc((void **)&p->tab, p->host.size() * 4))) return rc;
    if ((rc = dmalloc((void **)&p->X, Mp * D * 4))) return rc;
    if ((rc = dmalloc(&p->U, Mp * D * 2))) return rc;
    if ((rc = dmalloc(&p->QKV, Mp * 3 * D * 2))) return rc;
    if ((rc = dmalloc(&p->Hbuf, Mp * (size_t)F1 * 2))) return rc;
    if (p->glu && (rc = dmalloc(&p->Hg, Mp * (size_t)p->F * 2))) return rc;
    if ((rc = dmalloc(&p->Z, Bp * D * 2))) return rc;
    if ((rc = dmalloc((void **)&p->logits, Bp * (size_t)p->C_pad * 4))) return rc;
    if ((rc = dmalloc((void **)&p->probs, (size_t)max_images * p->C * 4))) return rc;
    if ((rc = dmalloc((void **)&p->logits_out, (size_t)max_images * p->C * 4))) return rc;
    if (p->rope) {       // a call's grids hold at most max_tokens patches; twice that, so that grids of earlier calls stay cached
        p->rope_cap = 2L * max_tokens * (D / H / 2);
        if ((rc = dmalloc((void **)&p->rope_cos, (size_t)p->rope_cap * 4))) return rc;
        if ((rc = dmalloc((void **)&p->rope_sin, (size_t)p->rope_cap * 4))) return rc;
    }
    HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&p->uploaded, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p->done, hipEventDisableTiming));
    HIP_TRY(hipDeviceSynchronize());
    *out = p.release();
    return VITX_OK;
}

void vitx_pack_free(vitx_pack *p) { delete p; }
int vitx_pack_shares_weights(const vitx_pack *p) { return p && p->weights_shared ? 1 : 0; }
size_t vitx_pack_scratch_bytes(const vitx_pack *p) { return p ? p->scratch_bytes : 0; }
int vitx_pack_launches(const vitx_pack *p, int *patch_embed) {
    if (!p) return 0;
    if (patch_embed) *patch_embed = p->pe_launches;
    return p->launches;
}

int vitx_pack_forward_device(vitx_pack *p, const void *d_imgs, const int32_t *shapes, int n, void *d_probs, void *d_logits, void *stream) {
    if (!p || !d_imgs || !shapes || !d_probs) { set_error("vitx_pack_forward_device: NULL argument"); return VITX_ERR_ARG; }
    return pack_call(p, d_imgs, shapes, n, d_probs, d_logits, stream ? (hipStream_t)stream : p->stream);
}

int vitx_pack_forward(vitx_pack *p, const float *imgs, const int32_t *shapes, int n, float *probs, float *logits) {
    if (!p || !imgs || !shapes || !probs) { set_error("vitx_pack_forward: NULL argument"); return VITX_ERR_ARG; }
    int rc;
    if ((rc = check_shapes("vitx_pack_forward", p->model, shapes, n, p->max_tokens, p->max_images, nullptr))) { if (p->dense) p->dense->next_out.clear(); return rc; }
    if (PackDense *dn = p->dense.get()) {       // the head's refusals too come before the pixels go up (pack_call makes the check again and keeps its tables)
        rc = check_dense("vitx_pack_forward", p->model, shapes, dn->next_out.empty() ? nullptr : dn->next_out.data(), (int)(dn->next_out.size() / 2), n, dn->K, dn->max_pixels,
                         nullptr, nullptr, nullptr, nullptr, nullptr);
        if (rc) { dn->next_out.clear(); return rc; }
    }
    HIP_TRY(hipSetDevice(p->device));
    if (!p->img) {       // the pixels of a full pack: max_tokens patches
        const size_t bytes = (size_t)p->max_tokens * p->P * p->P * 3 * 4;
        HIP_TRY(hipMalloc((void **)&p->img, bytes));
        p->scratch_bytes += bytes;
    }
    size_t floats = 0;
    for (int i = 0; i < n; ++i) floats += (size_t)shapes[2 * i] * shapes[2 * i + 1] * 3;
    HIP_TRY(hipMemcpyAsync(p->img, imgs, floats * 4, hipMemcpyHostToDevice, p->stream));
    if ((rc = pack_call(p, p->img, shapes, n, p->probs, logits ? p->logits_out : nullptr, p->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(probs, p->probs, (size_t)n * p->C * 4, hipMemcpyDeviceToHost, p->stream));
    if (logits) HIP_TRY(hipMemcpyAsync(logits, p->logits_out, (size_t)n * p->C * 4, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return VITX_OK;
}

int vitx_pack_feat_enable(vitx_pack *p, int flags) {
    if (!p || (flags & ~(VITX_FEAT_CLS | VITX_FEAT_TOKENS))) { set_error("vitx_pack_feat_enable: flags are VITX_FEAT_CLS | VITX_FEAT_TOKENS (0 = off)"); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(p->device));
    if (flags && !p->feat) {
        const size_t bytes = (size_t)p->max_tokens * p->D * 4;
        HIP_TRY(hipMalloc((void **)&p->feat, bytes));
        p->scratch_bytes += bytes;
    }
    p->feat_flags = flags; p->feat_n = 0;
    return VITX_OK;
}

// The last forward's final-norm rows, gathered on the host: cls [n][D] = row row0[i], tokens = rows row0[i] + T .. row0[i + 1] - 1, images end to end
int vitx_pack_feat_read(vitx_pack *p, float *cls, float *tokens) {
    if (!p || (!cls && !tokens)) { set_error("vitx_pack_feat_read: NULL argument"); return VITX_ERR_ARG; }
    if (!p->feat_flags || !p->feat_n) { set_error("vitx_pack_feat_read: no forward has run with features on since vitx_pack_feat_enable"); return VITX_ERR_ARG; }
    if ((cls && !(p->feat_flags & VITX_FEAT_CLS)) || (tokens && !(p->feat_flags & VITX_FEAT_TOKENS))) { set_error("vitx_pack_feat_read: an output was asked for that vitx_pack_feat_enable did not select"); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(p->device));
    if (p->done_pending) HIP_TRY(hipEventSynchronize(p->done));
    const int n = p->feat_n, D = p->D;
    const size_t rowb = (size_t)D * 4;
    for (int i = 0; i < n; ++i) {
        const float *src = p->feat + (size_t)p->row0[i] * D;
        if (cls) HIP_TRY(hipMemcpy(cls + (size_t)i * D, src, rowb, hipMemcpyDeviceToHost));
        if (tokens) {
            const size_t np = (size_t)(p->row0[i + 1] - p->row0[i] - p->Tp), at = (size_t)(p->row0[i] - i * p->Tp);
            HIP_TRY(hipMemcpy(tokens + at * D, src + (size_t)p->Tp * D, np * rowb, hipMemcpyDeviceToHost));
        }
    }
    return VITX_OK;
}

int vitx_pack_dense_check(const vitx_model *m, const int32_t *shapes, const int32_t *out_shapes, int n, int K, long max_pixels, int64_t *pix0, int32_t *tile0) {
    // max_tokens / max_images: whatever holds the call -- their refusals are vitx_pack_check's
    if (const int rc = check_shapes("vitx_pack_dense_check", m, shapes, n, 0x7fffffff, n, nullptr)) return rc;
    return check_dense("vitx_pack_dense_check", m, shapes, out_shapes, n, n, K, max_pixels, nullptr, nullptr, pix0, tile0, nullptr);
}

// The dense head of a packed context (include/vitx.h "packed batches").  Every argument check comes before the first device call; the head is
// built in a local and moved in, so a refused or failed set leaves the head that was set.
int vitx_pack_dense_set(vitx_pack *p, const float *W, const float *bias, int K, int Dc, uint64_t layer_mask, long max_pixels, int flags) {
    if (!p) { set_error("vitx_pack_dense_set: NULL context"); return VITX_ERR_ARG; }
    const bool off = !W && K == 0;
    uint64_t mask = layer_mask;
    const size_t Mp = (size_t)round_up(p->max_tokens, p->tm), Kpad = K > 0 ? (size_t)round_up(K, p->tn) : 0;
    if (!off) {
        if (!W) { set_error("vitx_pack_dense_set: NULL weights with K = %d", K); return VITX_ERR_ARG; }
        if (K < 1) { set_error("vitx_pack_dense_set: K = %d classes", K); return VITX_ERR_ARG; }
        if (flags & ~(VITX_DENSE_SCORE | VITX_DENSE_LOGITS)) { set_error("vitx_pack_dense_set: unknown flags 0x%x", flags); return VITX_ERR_ARG; }
        if (mask == 0) mask = 1ull << (p->L - 1);
        if (p->L < 64 && (mask >> p->L)) { set_error("vitx_pack_dense_set: layer mask selects a layer at or beyond L = %d", p->L); return VITX_ERR_ARG; }
        const int m = __builtin_popcountll(mask);
        if (m > 4) { set_error("vitx_pack_dense_set: %d layers selected, at most 4", m); return VITX_ERR_ARG; }
        if (Dc != m * p->D) { set_error("vitx_pack_dense_set: the head's width %d is not %d layers x D = %d", Dc, m, m * p->D); return VITX_ERR_ARG; }
        if (max_pixels < 1) { set_error("vitx_pack_dense_set: max_pixels = %ld", max_pixels); return VITX_ERR_ARG; }
        for (size_t i = 0, nb = (size_t)K * Dc; i < nb; ++i)
            if (!std::isfinite(W[i])) { set_error("vitx_pack_dense_set: weight [%zu][%zu] is not finite", i / Dc, i % Dc); return VITX_ERR_ARG; }
        if (bias) for (int k = 0; k < K; ++k)
            if (!std::isfinite(bias[k])) { set_error("vitx_pack_dense_set: bias [%d] is not finite", k); return VITX_ERR_ARG; }
        if (K > kDenseMaxK) { set_error("vitx_pack_dense_set: K = %d classes above %d (labels are bytes)", K, kDenseMaxK); return VITX_ERR_UNSUPPORTED; }
        if (Mp * Dc * 2 > 0xf0000000u || Mp * Kpad * 4 > 0xf0000000u) {
            set_error("vitx_pack_dense_set: the operand or logit rows of max_tokens = %d rows leave the GEMM's 32-bit byte window", p->max_tokens);
            return VITX_ERR_UNSUPPORTED;
        }
    }
    HIP_TRY(hipSetDevice(p->device));
    // nothing of this context is in flight while buffers and tables change hands
    if (p->uploaded_pending) { HIP_TRY(hipEventSynchronize(p->uploaded)); p->uploaded_pending = false; }
    if (const int rc = wait_done(p)) return rc;
    const size_t cap = (size_t)p->max_images, base_ints = 3 * cap + 2;
    // the segment tables with (ints > base_ints) or without the head's part behind them: a fresh zeroed buffer in place of the old one
    auto resize_tables = [&](size_t ints) -> int {
        if (p->host.size() == ints) return VITX_OK;
        int *t = nullptr;
        HIP_TRY(hipMalloc((void **)&t, ints * 4));
        if (const hipError_t e = hipMemset(t, 0, ints * 4); e != hipSuccess) { (void)hipFree(t); set_error("vitx_pack_dense_set: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
        std::replace(p->allocs.begin(), p->allocs.end(), (void *)p->tab, (void *)t);
        (void)hipFree(p->tab);
        p->scratch_bytes += ints * 4; p->scratch_bytes -= p->host.size() * 4;
        p->tab = t; p->host.assign(ints, 0);
        return VITX_OK;
    };
    if (off) {
        if (p->dense) { p->scratch_bytes -= p->dense->bytes; p->dense.reset(); }
        return resize_tables(base_ints);
    }
    auto dn = std::make_unique<PackDense>();
    dn->K = K; dn->Kpad = (int)Kpad; dn->Dc = Dc; dn->mask = mask; dn->flags = flags; dn->cap = p->max_images; dn->max_pixels = max_pixels;
    dn->a.resize(1); dn->acc.resize(1);
    dn->scratch = Mp * Dc * 2 + Mp * Kpad * 4;
    dn->bytes = dn->scratch + Kpad * Dc * 2 + Kpad * 4 + (size_t)max_pixels;
    bool ok = dn->W.alloc(Kpad * Dc * 2) && dn->bias.alloc(Kpad * 4) && dn->a[0].alloc(Mp * Dc * 2) && dn->acc[0].alloc(Mp * Kpad * 4) && dn->labels.alloc((size_t)max_pixels);
    if (ok && (flags & VITX_DENSE_SCORE)) { ok = dn->score.alloc((size_t)max_pixels * 4); dn->bytes += (size_t)max_pixels * 4; }
    if (ok && (flags & VITX_DENSE_LOGITS)) { ok = dn->logits.alloc((size_t)p->max_tokens * K * 4); dn->bytes += (size_t)p->max_tokens * K * 4; }
    if (!ok) { set_error("vitx_pack_dense_set: cannot allocate the buffers for %d classes, %ld pixels and %d token rows", K, max_pixels, p->max_tokens); return VITX_ERR_NOMEM; }
    // the head goes up rounded (RNE) to the operand type, zero rows beyond K; the operand rows start as zeros (a forward writes its rows and zeroes
    // the pad rows behind them)
    const std::vector<uint16_t> hw = operand_matrix_host(p->dtype, W, nullptr, K, Dc, (int)Kpad, Dc, 0, 0);
    HIP_TRY(hipMemcpy(dn->W.p, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dn->bias.p, 0, Kpad * 4));
    if (bias) HIP_TRY(hipMemcpy(dn->bias.p, bias, (size_t)K * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dn->a[0].p, 0, Mp * Dc * 2));
    HIP_TRY(hipDeviceSynchronize());
    if (const int rc = resize_tables(base_ints + cap + 1 + cap * kDenseSegInts)) return rc;
    if (p->dense) p->scratch_bytes -= p->dense->bytes;
    p->scratch_bytes += dn->bytes;
    p->dense = std::move(dn);
    return VITX_OK;
}

int vitx_pack_dense_out(vitx_pack *p, const int32_t *out_shapes, int n) {
    if (!p || !p->dense) { set_error("vitx_pack_dense_out: no dense head is set"); return VITX_ERR_ARG; }
    if (!out_shapes || n == 0) { p->dense->next_out.clear(); return VITX_OK; }
    if (n < 1 || n > p->max_images) { set_error("vitx_pack_dense_out: n = %d is outside 1 .. max_images = %d", n, p->max_images); return VITX_ERR_ARG; }
    p->dense->next_out.assign(out_shapes, out_shapes + (size_t)2 * n);
    return VITX_OK;
}

const void *vitx_pack_dense_device(const vitx_pack *p) { return p && p->dense ? p->dense->labels.p : nullptr; }
size_t vitx_pack_dense_scratch_bytes(const vitx_pack *p) { return p && p->dense ? p->dense->scratch : 0; }

// The last forward's maps, the images end to end, and the kept logits of its patch rows (row0[i] + T .. row0[i + 1] - 1 of the pack's rows)
int vitx_pack_dense_read(vitx_pack *p, uint8_t *labels, float *score, float *logits) {
    if (!p || !labels) { set_error("vitx_pack_dense_read: NULL argument"); return VITX_ERR_ARG; }
    const PackDense *dn = p->dense.get();
    const int n = dn ? dn->n : 0;
    if (n == 0) { set_error("vitx_pack_dense_read: no forward has run with a dense head set since vitx_pack_dense_set"); return VITX_ERR_ARG; }
    if (score && !dn->score) { set_error("vitx_pack_dense_read: the head was set without VITX_DENSE_SCORE"); return VITX_ERR_ARG; }
    if (logits && !dn->logits) { set_error("vitx_pack_dense_read: the head was set without VITX_DENSE_LOGITS"); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(p->device));
    if (p->done_pending) HIP_TRY(hipEventSynchronize(p->done));
    const size_t px = (size_t)dn->pix0[n];
    HIP_TRY(hipMemcpy(labels, dn->labels.p, px, hipMemcpyDeviceToHost));
    if (score) HIP_TRY(hipMemcpy(score, dn->score.p, px * 4, hipMemcpyDeviceToHost));
    if (logits) for (int i = 0; i < n; ++i) {
        const size_t np = (size_t)(p->row0[i + 1] - p->row0[i] - p->Tp), at = (size_t)(p->row0[i] - i * p->Tp);
        HIP_TRY(hipMemcpy(logits + at * dn->K, dn->logits.as<float>() + (size_t)(p->row0[i] + p->Tp) * dn->K, np * dn->K * 4, hipMemcpyDeviceToHost));
    }
    return VITX_OK;
}

}  // extern "C"
