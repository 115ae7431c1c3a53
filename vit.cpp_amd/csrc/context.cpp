// context.cpp -- creation of the execution context of the MI355X ViT engine: its configuration, the tables of its grid, scratch, streams.
// Replaces vit_state + the set-up half of vit_predict of the reference (vit.cpp:718-941, 1004-1040).  Differences by design: the batch is
// n images (the reference hard-wires 1, vit.cpp:747), weights live in HBM in the MFMA operand type (weights.cpp), all activation scratch is
// allocated once per context (the reference builds the graph twice and reallocates per call, vit.cpp:1009-1035), and the ~90 launches of a
// forward are enqueued on one HIP stream without host synchronisation (forward.cpp).
#include <stdlib.h>
#include <string.h>

#include <new>

#include "context.h"

namespace {

// vitx_ctx_create_ex / vitx_ctx_create_rect, step 1: the options (all zero = every default) and the geometry they ask for are validated, then the
// context is made and its fields are derived from them.  The first check that fails is the one reported; the device is opened behind those of the options.
// rect: the caller is vitx_ctx_create_rect and the geometry is rect_h x rect_w; otherwise it is the square of options.img_size (0: the file's).
int configure(const vitx_model *m, int device, int max_batch, int dtype, const vitx_ctx_options *opt_in, bool rect, int rect_h, int rect_w, vitx_ctx_options &opt, std::unique_ptr<vitx_ctx> &c) {
    if (opt_in) {
        if (opt_in->struct_size < 8 || opt_in->struct_size > (int)sizeof(vitx_ctx_options)) { set_error("vitx_ctx_create_ex: options.struct_size %d is not a size this library knows", opt_in->struct_size); return VITX_ERR_ARG; }
        memcpy(&opt, opt_in, (size_t)opt_in->struct_size);
        if (opt.streams < 0 || opt.streams > 4 || opt.q4_fused_rows < 0 || opt.split_first < 0 || (opt.last_layer_all_rows & ~1)) { set_error("vitx_ctx_create_ex: option out of range"); return VITX_ERR_ARG; }
    }
    // geometry of this context (vitx_ctx_options::img_size): checked before any device is touched
    if (opt.pos_interp != VITX_POS_BICUBIC && opt.pos_interp != VITX_POS_BICUBIC_AA) { set_error("vitx_ctx_create_ex: unknown pos_interp %d (0 bicubic, 1 bicubic with antialias)", opt.pos_interp); return VITX_ERR_ARG; }
    if (opt.img_size < 0 || (opt.img_size > 0 && (m->hp.patch_size <= 0 || opt.img_size % m->hp.patch_size))) {
        set_error("vitx_ctx_create_ex: img_size %d is not a positive multiple of the patch size %d", opt.img_size, m->hp.patch_size); return VITX_ERR_ARG;
    }
    if (rect) {
        if (opt.img_size != 0) { set_error("vitx_ctx_create_rect: options.img_size must be 0 (the shape is img_h x img_w; it is %d)", opt.img_size); return VITX_ERR_ARG; }
        if (m->hp.patch_size <= 0 || rect_h <= 0 || rect_w <= 0 || rect_h % m->hp.patch_size || rect_w % m->hp.patch_size) {
            set_error("vitx_ctx_create_rect: img_h %d and img_w %d must be positive multiples of the patch size %d", rect_h, rect_w, m->hp.patch_size); return VITX_ERR_ARG;
        }
    }
    const int img_size = opt.img_size > 0 ? opt.img_size : m->hp.img_size;
    const int img_h = rect ? rect_h : img_size, img_w = rect ? rect_w : img_size;
    const bool own_shape = img_h == m->hp.img_size && img_w == m->hp.img_size;      // the file's own geometry
    if (m->in_chans == 1 && (m->num_registers || m->head_pool != VITX_POOL_CLS)) { set_error("vitx_ctx_create_ex: a ViTSTR (one-channel) model takes neither register tokens nor a pooled or attention-pooling head"); return VITX_ERR_UNSUPPORTED; }
    if (dtype == VITX_MXFP8 && (m->num_registers || m->head_pool != VITX_POOL_CLS)) { set_error("vitx_ctx_create_ex: VITX_MXFP8 contexts do not take models with register tokens, the pooled head or the attention-pooling head"); return VITX_ERR_UNSUPPORTED; }
    if (m->head_pool == VITX_POOL_MAP && !own_shape) {
        set_error("vitx_ctx_create_ex: a model with the attention-pooling head stays at the file's img_size (%d): its position table has no class row and no resampling path yet", m->hp.img_size);
        return VITX_ERR_UNSUPPORTED;
    }
    if (m->rope_kind && dtype == VITX_MXFP8) { set_error("vitx_ctx_create_ex: VITX_MXFP8 contexts do not take models with rotary position embeddings"); return VITX_ERR_UNSUPPORTED; }
    if (m->rope_kind && m->in_chans == 1) { set_error("vitx_ctx_create_ex: a ViTSTR (one-channel) model takes no rotary position embeddings"); return VITX_ERR_UNSUPPORTED; }
    if (m->glu_kind && dtype == VITX_MXFP8) { set_error("vitx_ctx_create_ex: VITX_MXFP8 contexts do not take models with a gated MLP"); return VITX_ERR_UNSUPPORTED; }
    if (m->glu_kind && m->in_chans == 1) { set_error("vitx_ctx_create_ex: a ViTSTR (one-channel) model takes no gated MLP"); return VITX_ERR_UNSUPPORTED; }
    if (m->in_chans == 1 && (m->has_pre_norm || m->activation != VITX_ACT_GELU_TANH)) { set_error("vitx_ctx_create_ex: a ViTSTR (one-channel) model takes neither a pre-norm nor an activation other than tanh-GELU"); return VITX_ERR_UNSUPPORTED; }
    if (dtype == VITX_MXFP8 && m->activation != VITX_ACT_GELU_TANH) { set_error("vitx_ctx_create_ex: VITX_MXFP8 contexts evaluate tanh-GELU only (this model's activation: %d)", m->activation); return VITX_ERR_UNSUPPORTED; }
    if (m->in_chans == 1 && !own_shape) { set_error("vitx_ctx_create_ex: a ViTSTR context stays at the file's img_size (%d)", m->hp.img_size); return VITX_ERR_UNSUPPORTED; }
    const Tuning *tune = nullptr;
    if (int rc = open_device("vitx_ctx_create", device, &tune)) return rc;
    const vitx_hparams &hp = m->hp;
    if (hp.num_attention_heads <= 0 || hp.hidden_size % hp.num_attention_heads) { set_error("vitx_ctx_create: hidden_size %d is not a multiple of %d heads", hp.hidden_size, hp.num_attention_heads); return VITX_ERR_UNSUPPORTED; }
    if (hp.hidden_size % 64) { set_error("vitx_ctx_create: hidden_size must be a multiple of 64"); return VITX_ERR_UNSUPPORTED; }
    // (VITX_MXFP8 needs whole 32-element blocks per row: the multiple of 64 above already guarantees it, so no check of its own)
    static_assert(64 % kMxBlock == 0, "the hidden-size rule above must cover the MX block");
    c.reset(new (std::nothrow) vitx_ctx());
    if (!c) return VITX_ERR_NOMEM;
    c->model = m; c->hp = hp; c->device = device; c->max_batch = max_batch; c->tune = tune;
    c->mx = dtype == VITX_MXFP8; c->dtype = c->mx ? VITX_BF16 : dtype;      // everything but the MX GEMMs runs as in a VITX_BF16 context
    c->D = hp.hidden_size; c->L = hp.num_hidden_layers; c->H = hp.num_attention_heads; c->C = hp.num_classes; c->P = hp.patch_size;
    c->Sh = img_h; c->Sw = img_w; c->S = img_h == img_w ? img_h : 0;
    c->Cin = m->in_chans; c->R = m->in_chans == 1 ? VITX_VITSTR_SEQ_LEN : 1;
    c->glu = m->glu_kind != VITX_GLU_NONE; c->F = m->mlp_hidden(); c->F1 = m->mlp_fc1_rows();
    c->fc1_epi = c->glu ? EPI_BIAS : act_epi(m->activation);       // a gated MLP: the plain bias epilogue, the gate is a launch of its own
    c->nreg = m->num_registers; c->pool = m->head_pool == VITX_POOL_CLS_MEAN; c->map = m->head_pool == VITX_POOL_MAP;
    c->Tp = c->map ? 0 : 1 + c->nreg;
    if (c->map && c->H > kPoolMaxHeads) { set_error("vitx_ctx_create: the attention-pooling kernel takes at most %d heads (this model: %d)", kPoolMaxHeads, c->H); return VITX_ERR_UNSUPPORTED; }
    c->gh = c->Sh / c->P; c->gw = c->Sw / c->P;
    if ((long)c->gh * c->gw + c->Tp > 0x7fffffffl / 4) { set_error("vitx_ctx_create: %d x %d patches are more tokens than a context takes", c->gh, c->gw); return VITX_ERR_UNSUPPORTED; }
    c->N = c->gh * c->gw + c->Tp; c->Kpe = patch_k(m); c->Kpe_pad = patch_k_pad(m);
    if (c->N < c->R) { set_error("vitx_ctx_create: a ViTSTR head reads %d tokens, this model has %d (image %d x %d, patch_size %d)", c->R, c->N, c->Sh, c->Sw, c->P); return VITX_ERR_UNSUPPORTED; }
    c->tm = gemm_tile_m(); c->tn = gemm_tile_n();
    c->C_pad = head_cols_pad(m);
    // validate against what the kernels are actually instantiated for (a context that would fail on its first forward is refused here)
    if (!attention_supports(c->N, c->D, c->H)) {
        set_error("vitx_ctx_create: attention needs a head_dim that is a multiple of 8 up to 128 (this model: %d) and at least one token (%d tokens, image %d x %d, patch_size %d)", c->D / c->H, c->N, c->Sh, c->Sw, c->P);
        return VITX_ERR_UNSUPPORTED;
    }
    if (!layernorm_supports(c->D)) { set_error("vitx_ctx_create: hidden_size %d has no LayerNorm instantiation (64, 128, 192, 256, 320, 384, 448, 512, 576, 640, 768, 896, 1024, 1152, 1280, 1408, 1536, 1664, 2048)", c->D); return VITX_ERR_UNSUPPORTED; }
    c->split_first = opt.split_first;
    c->prec_attn = dtype == VITX_F16 && c->D == c->H * 64 && !opt.f16_fast_attention;
    c->quant_on_device = !opt.quant_on_host;
    // the pooled head averages every patch row of the last layer, the attention-pooling head attends over them: such a context runs exactly as one created with last_layer_all_rows = 1
    c->cls_tail = !opt.last_layer_all_rows && !c->pool && !c->map && c->R == 1 && attention_cls_supports(c->N, c->D, c->H);
    c->q4_fused_rows = opt.q4_fused_rows;
    c->graphs_on = opt.graph != 0;
    // fault injection for the parity tests: honoured only with the key in the upper half (VITX_LN_TEST_KEY | mode), so that no caller sets it by accident
    if (opt.ln_test) {
        if ((opt.ln_test & (int32_t)0xffff0000) != (int32_t)VITX_LN_TEST_KEY) { set_error("vitx_ctx_create_ex: ln_test is a test-only switch (it needs its key: include/vitx.h)"); return VITX_ERR_ARG; }
        c->ln_test = opt.ln_test & 0xffff;
        if (c->ln_test & ~7) { set_error("vitx_ctx_create_ex: ln_test mode %d has bits outside 1 | 2 | 4", c->ln_test); return VITX_ERR_ARG; }
        if ((c->ln_test & 3) == 3) c->ln_timeout = 5000;       // real time-outs in the test: 50 us (with or without bit 4; the kernel tests the bits one by one too)
    }
    // a captured launch would replay its epoch tag: no fusion under the graph cache; MX: every LayerNorm is its own launch (it writes MX)
    c->ln_fuse = !opt.no_ln_fusion && !opt.graph && !c->mx;
#ifdef VITX_LAB
    if (const char *e = getenv("VITX_SKIP")) c->skip = atoi(e);
#endif
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    return VITX_OK;
}

// Step 2: the scratch of one sub-batch slice; `internal`: a slice that runs on a stream of its own (every slice but the first of several)
int alloc_slice(vitx_ctx *c, vitx_ctx::Slice &sl, size_t hcols, bool internal) {
    const int D = c->D;
    int rc;
    sl.cap = c->pass_cap();     // every slice can hold a whole pass: the split point is chosen per call (split_batch)
    const size_t Mpad = (size_t)round_up(sl.cap * c->N, c->tm), Bpad = (size_t)round_up(sl.cap * c->R, c->tm);
    if ((rc = c->dmalloc((void **)&sl.X, Mpad * D * 4, true))) return rc;
    if ((rc = c->dmalloc(&sl.U, Mpad * D * 2, true))) return rc;
    if ((rc = c->dmalloc(&sl.U2, Mpad * D * 2, true))) return rc;
    if (D % 256 == 0 && D / 256 <= 4) {
        if ((rc = c->dmalloc((void **)&sl.ln_sync, (Mpad / 256) * (size_t)(D / 256) * 256 * 2 * sizeof(unsigned long long), true))) return rc;
        if ((rc = c->dmalloc((void **)&sl.ln_todo, (Mpad / 256 + 1) * sizeof(unsigned), true))) return rc;
        sl.ln_blocks = (int)(Mpad / 256);
    }
    if ((rc = c->dmalloc(&sl.QKV, Mpad * 3 * D * 2 * (c->prec_attn ? 2 : 1), true))) return rc;
    sl.qkv_lo_off = c->prec_attn ? (long)(Mpad * 3 * D) : 0;       // capacity; a forward places the lo plane right behind ITS rows (SliceForward)
    if ((rc = c->dmalloc(&sl.Hbuf, Mpad * hcols * 2, true))) return rc;
    if (c->glu && (rc = c->dmalloc(&sl.Hg, Mpad * (size_t)c->F * 2, true))) return rc;
    if ((rc = c->dmalloc(&sl.Z, Bpad * D * 2 * (c->pool ? 2 : 1), true))) return rc;
    if (c->mx) {
        const size_t kp = (size_t)mx_k_pad(D), kh = (size_t)mx_k_pad(c->F);
        if ((rc = c->dmalloc((void **)&sl.Umx, Mpad * kp * 33 / 32, true))) return rc;
        if ((rc = c->dmalloc((void **)&sl.U2mx, Mpad * kp * 33 / 32, true))) return rc;
        sl.Umx_s = sl.Umx + Mpad * kp; sl.U2mx_s = sl.U2mx + Mpad * kp;
        sl.Hmx = (uint8_t *)sl.Hbuf; sl.Hmx_s = sl.Hmx + Mpad * kh;             // Mpad * kh * 33 / 32 <= Mpad * F * 2 bytes of Hbuf
    }
    if ((c->cls_tail || c->map) && (rc = c->dmalloc((void **)&sl.Xc, Bpad * D * 4, true))) return rc;
    if (c->map && (rc = c->dmalloc(&sl.Mp, Bpad * c->H * D * 2, true))) return rc;
    if ((rc = c->dmalloc((void **)&sl.logits, Bpad * c->C_pad * 4, true))) return rc;
    // expansion scratch for quantised matrices: one buffer per matrix kind, shared by all layers (the largest layer decides)
    for (int k = 0; k < W_PER_LAYER; ++k) {
        size_t need = 0;
        for (const LayerW &w : c->wset->layers) if (w.q[k].blocks) need = std::max(need, (size_t)w.q[k].n_pad * w.q[k].K * 2);
        if (need && (rc = c->dmalloc(&sl.Wq[k], need, false))) return rc;
    }
    const QuantW &hq = c->wset->head_q;
    if (hq.blocks && (rc = c->dmalloc(&sl.Wq_head, (size_t)hq.n_pad * hq.K * 2, false))) return rc;
    if (internal) {
        // Slice 0 runs on the CALLER's stream, slices 1.. on internal HIGH-priority streams.  The runtime multiplexes all streams of one
        // priority onto a small pool of hardware queues (GPU_MAX_HW_QUEUES, 4 by default), round-robin in creation order; a hardware queue
        // executes its packets in order.  r02 gave slice 0 its own normal-priority stream: whenever that stream shared a hardware queue
        // with the caller's (torch's pool of streams, a second context in the process ...), step k + 1's slice-0 kernels queued up behind
        // the caller stream's wait for step k's slice 1, and the two sub-batches ran back to back -- measured r03: the 2nd and the 6th
        // context created in one process ran 11.8 instead of 9.9 ms per forward.  Pools are per priority: the caller's stream (normal,
        // unless the caller chose otherwise) and the internal ones (high, created back to back) can never share a queue.
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&sl.stream, hipStreamNonBlocking, greatest));
        HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    return VITX_OK;
}

}  // namespace

extern "C" {

int vitx_ctx_create(const vitx_model *m, int device, int max_batch, int dtype, vitx_ctx **out) { return vitx_ctx_create_ex(m, device, max_batch, dtype, nullptr, out); }

// One creation path for both entry points (rect: vitx_ctx_create_rect with img_h x img_w).  A rect call with img_h == img_w == S does what
// vitx_ctx_create_ex does with img_size = S: the same fields, the same launches.
static int ctx_create(const vitx_model *m, int device, int max_batch, int dtype, const vitx_ctx_options *opt_in, bool rect, int img_h, int img_w, vitx_ctx **out) {
    if (!m || !out || max_batch <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16 && dtype != VITX_MXFP8)) { set_error("vitx_ctx_create: invalid argument"); return VITX_ERR_ARG; }
    *out = nullptr;
    if (m->kind != VITX_KIND_IMAGE) { set_error("vitx_ctx_create: a text-tower model takes a text context (vitx_text_create), not an image context"); return VITX_ERR_ARG; }
    vitx_ctx_options opt{};                   // all zero = every default
    std::unique_ptr<vitx_ctx> c;
    int rc;
    if ((rc = configure(m, device, max_batch, dtype, opt_in, rect, img_h, img_w, opt, c))) return rc;
    if ((rc = obtain_weights({m, device, dtype, c->quant_on_device}, &c->wset, &c->weights_shared))) return rc;
    const vitx_hparams &hp = m->hp;
    const int D = c->D;
    // the position table of THIS context: the set's (the file's) at the file's size, else resampled on the device into scratch the context owns
    c->pos = c->wset->pos;
    const int g_in = hp.img_size / hp.patch_size;
    if (c->gh != g_in || c->gw != g_in) {
        if ((rc = c->dmalloc((void **)&c->pos_own, ((size_t)c->gh * c->gw + 1) * D * 4, false))) return rc;      // (never a VITX_POOL_MAP model: configure refuses it)
        HIP_TRY(launch_pos_resample(c->wset->pos, g_in, g_in, D, c->gh, c->gw, opt.pos_interp, c->pos_own, c->stream));
        c->pos = c->pos_own;                 // (the hipDeviceSynchronize at the end of the creation covers the launch)
    }
    // rotary position embeddings: the table of THIS context's grid, built on the host in double and uploaded once (cos, then sin)
    if (m->rope_kind) {
        const size_t tab = (size_t)c->gh * c->gw * (D / c->H / 2);
        std::vector<float> h(2 * tab);
        if ((rc = vitx_model_rope_table(m, c->gh, c->gw, h.data(), h.data() + tab))) return rc;
        if ((rc = c->dmalloc((void **)&c->rope_cos, 2 * tab * 4, false))) return rc;
        c->rope_sin = c->rope_cos + tab;
        HIP_TRY(hipMemcpy(c->rope_cos, h.data(), 2 * tab * 4, hipMemcpyHostToDevice));
    }

    // sub-batch slices (vitx_ctx_options::streams; 1 = single stream).  Small contexts stay single-slice.
    int ns = opt.streams > 0 ? opt.streams : 2;      // (configure: 0 .. 4)
    if (max_batch < 8 * ns) ns = 1;
    c->nslices = ns;
    c->slices.resize(ns);
    const size_t hcols = std::max<size_t>((size_t)c->F1, (size_t)c->Kpe_pad);
    {
        // The kernels address every activation buffer with 32-bit BYTE offsets (buffer instructions): a sub-batch must keep its largest buffer --
        // the MLP hidden tensor, or the two QKV planes of the F16 parity mode -- below 0xf0000000 bytes (ViT-B: 3326 images per sub-batch, 2217 in
        // parity mode).  Batches beyond one such window run as several passes through the same scratch (vitx_forward_device), so max_batch
        // itself is only bounded by memory.  r04: the guards used to sit in the individual launchers only, and a 10 000-image batch computed garbage.
        const size_t row_bytes = std::max<size_t>(hcols * 2, (size_t)3 * D * 2 * (c->prec_attn ? 2 : 1));
        const size_t rows = (size_t)0xf0000000u / row_bytes / 256 * 256;
        const long per_slice = (long)(rows / c->N);
        if (per_slice < 1) { set_error("vitx_ctx_create: a single image exceeds the kernels' 32-bit buffer window (%d tokens x %d)", c->N, D); return VITX_ERR_UNSUPPORTED; }
        c->call_limit = (int)std::min<long>((long)max_batch, per_slice);          // whatever the split of a pass, no sub-batch exceeds the window
    }
    for (int i = 0; i < ns; ++i) if ((rc = alloc_slice(c.get(), c->slices[i], hcols, ns > 1 && i > 0))) return rc;
    if (ns > 1) HIP_TRY(hipEventCreateWithFlags(&c->fork, hipEventDisableTiming));
    HIP_TRY(hipHostMalloc((void **)&c->ln_fb_host, sizeof(unsigned) * 4, hipHostMallocDefault));
    for (int i = 0; i < 4; ++i) c->ln_fb_host[i] = 0;
    if ((rc = c->dmalloc((void **)&c->img, (size_t)max_batch * c->img_floats() * 4, false))) return rc;
    if ((rc = c->dmalloc((void **)&c->probs, (size_t)max_batch * c->R * c->C * 4, true))) return rc;
    if ((rc = c->dmalloc((void **)&c->logits_all, (size_t)max_batch * c->R * c->C * 4, true))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    *out = c.release();
    return VITX_OK;
}

int vitx_ctx_create_ex(const vitx_model *m, int device, int max_batch, int dtype, const vitx_ctx_options *opt_in, vitx_ctx **out) {
    return ctx_create(m, device, max_batch, dtype, opt_in, false, 0, 0, out);
}
int vitx_ctx_create_rect(const vitx_model *m, int device, int max_batch, int dtype, const vitx_ctx_options *opt_in, int img_h, int img_w, vitx_ctx **out) {
    return ctx_create(m, device, max_batch, dtype, opt_in, true, img_h, img_w, out);
}

void vitx_ctx_free(vitx_ctx *c) { delete c; }
int vitx_ctx_max_batch(const vitx_ctx *c) { return c ? c->max_batch : 0; }
int vitx_ctx_img_size(const vitx_ctx *c) { return c ? c->S : 0; }
int vitx_ctx_img_shape(const vitx_ctx *c, int *img_h, int *img_w) {
    if (!c || !img_h || !img_w) { set_error("vitx_ctx_img_shape: NULL argument"); return VITX_ERR_ARG; }
    *img_h = c->Sh; *img_w = c->Sw;
    return VITX_OK;
}
int vitx_ctx_grid(const vitx_ctx *c, int *gh, int *gw) {
    if (!c || !gh || !gw) { set_error("vitx_ctx_grid: NULL argument"); return VITX_ERR_ARG; }
    *gh = c->gh; *gw = c->gw;
    return VITX_OK;
}
int vitx_ctx_tokens(const vitx_ctx *c) { return c ? c->N : 0; }
int vitx_ctx_registers(const vitx_ctx *c) { return c ? c->nreg : 0; }
int vitx_ctx_out_rows(const vitx_ctx *c) { return c ? c->R : 0; }
size_t vitx_ctx_weight_bytes(const vitx_ctx *c) { return c ? c->wset->weight_bytes : 0; }
int vitx_ctx_shares_weights(const vitx_ctx *c) { return c && c->weights_shared ? 1 : 0; }

}  // extern "C"
