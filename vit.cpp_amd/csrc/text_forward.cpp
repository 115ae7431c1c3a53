// text_forward.cpp -- the text context and its forward (include/vitx.h "the text tower"): token ids in, projected text embeddings out.
// The blocks are the image forward's launches through the same dispatchers; new are the token-embedding front, the short-sequence
// attention with an optional causal mask (attention_text.hip) and the pooling of one row per prompt (text_embed.hip).
// One stream, no sub-batch split, no hipGraph cache, no LayerNorm fusion.  Quantised block matrices are expanded once at upload
// (quant_on_device = false): the just-in-time expansion of the image forward exists for ITS memory budget -- hundreds of images of
// activations beside the weights -- and a text tower's batch of short prompts has no such pressure.
#include <string.h>

#include <new>

#include "text_context.h"
#include "weights.h"

namespace {

int text_gemm(const vitx_text *t, const Tuning &tune, int epi, const GemmArgs &a, hipStream_t st) {
    HIP_TRY(launch_gemm(tune, t->dtype, epi, a, st));
    return VITX_OK;
}

// The checked ids and their pooled positions into the staging buffer [max_prompts pooled positions | n * T ids].  Everything that can be refused is
// refused (vitx_text_check_ids: host only) before the first device call; only then does the call wait for the previous call's upload, which may
// still be reading the buffer (vitx_text_embed_device only enqueues) -- for the upload, not for its forward.
int stage_ids(vitx_text *t, const int32_t *ids, int n) {
    t->pooled_host.resize((size_t)n);
    const int rc = vitx_text_check_ids(t->model, ids, n, t->pooled_host.data());
    if (rc) return rc;
    if (t->uploaded_pending) { HIP_TRY(hipSetDevice(t->device)); HIP_TRY(hipEventSynchronize(t->uploaded)); t->uploaded_pending = false; }
    memcpy(t->host.data(), t->pooled_host.data(), (size_t)n * 4);
    memcpy(t->host.data() + t->max_prompts, ids, (size_t)n * t->T * 4);
    return VITX_OK;
}

int text_forward(vitx_text *t, int n, int flags, float *d_out, hipStream_t st) {
    const WeightSet &ws = *t->wset;
    const int T = t->T, D = t->D, H = t->H, tn = t->tn, tm = t->tm, dtype = t->dtype;
    const int rows = n * T, M = round_up(rows, tm), Mh = round_up(n, tm);
    int rc;
    // pooled positions and ids: ONE upload of the staging buffer's front (the ids sit at their fixed place behind max_prompts positions)
    HIP_TRY(hipMemcpyAsync(t->pooled, t->host.data(), ((size_t)t->max_prompts + rows) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(t->uploaded, st));
    t->uploaded_pending = true;
    HIP_TRY(launch_text_embed(ws.tok_f16, ws.tok, ws.pos, t->ids, t->X, n, T, D, st));
    for (const LayerW &w : ws.layers) {
        HIP_TRY(launch_layernorm(dtype, t->X, D, w.ln1_w, w.ln1_b, t->U, D, rows, D, t->eps, st));
        if ((rc = text_gemm(t, t->tune_qkv, EPI_BIAS, dense_gemm(t->U, w.qkv_w, w.qkv_b, t->QKV, M, rows, 3 * D, round_up(3 * D, tn), D), st))) return rc;
        HIP_TRY(launch_attention_text(dtype, t->QKV, t->U, n, T, D, H, t->causal, st));
        if ((rc = text_gemm(t, t->tune_proj, EPI_BIAS_RESID, dense_gemm(t->U, w.proj_w, w.proj_b, t->X, M, rows, D, round_up(D, tn), D), st))) return rc;
        HIP_TRY(launch_layernorm(dtype, t->X, D, w.ln2_w, w.ln2_b, t->U, D, rows, D, t->eps, st));
        if ((rc = text_gemm(t, t->tune_fc1, t->fc1_epi, dense_gemm(t->U, w.fc1_w, w.fc1_b, t->Hbuf, M, rows, 4 * D, round_up(4 * D, tn), D), st))) return rc;
        if ((rc = text_gemm(t, t->tune_fc2, EPI_BIAS_RESID, dense_gemm(t->Hbuf, w.fc2_w, w.fc2_b, t->X, M, rows, D, round_up(D, tn), 4 * D), st))) return rc;
    }
    HIP_TRY(launch_text_pool(dtype, t->X, t->pooled, ws.norm_w, ws.norm_b, t->Z, n, Mh, T, D, t->eps, st));
    // VITX_TEXT_L2: the head writes the scratch rows and zs_embed_kernel's f32 instantiation (zeroshot.hip: THE sum-of-squares rule) writes the output
    float *e = (flags & VITX_TEXT_L2) ? t->raw : d_out;
    if ((rc = text_gemm(t, t->tune_head, EPI_BIAS_F32, dense_gemm(t->Z, ws.head_w, ws.head_b, e, Mh, n, t->E, t->E_pad, D, t->E), st))) return rc;
    if (flags & VITX_TEXT_L2) HIP_TRY(launch_zs_embed_f32(t->raw, t->E, d_out, n, t->E, st));
    return VITX_OK;
}

int check_call(const vitx_text *t, const int32_t *ids, int n, int flags, const void *out) {
    if (!t || !ids || !out) { set_error("vitx_text_embed: NULL argument"); return VITX_ERR_ARG; }
    if (n < 1 || n > t->max_prompts) { set_error("vitx_text_embed: n = %d is outside 1 .. max_prompts = %d", n, t->max_prompts); return VITX_ERR_ARG; }
    if (flags & ~VITX_TEXT_L2) { set_error("vitx_text_embed: unknown flags 0x%x (0 or VITX_TEXT_L2)", flags); return VITX_ERR_ARG; }
    return VITX_OK;
}

}  // namespace

extern "C" {

int vitx_text_create(const vitx_model *m, int device, int max_prompts, int dtype, vitx_text **out) {
    if (!m || !out || max_prompts <= 0) { set_error("vitx_text_create: invalid argument"); return VITX_ERR_ARG; }
    *out = nullptr;
    if (m->kind != VITX_KIND_TEXT) { set_error("vitx_text_create: an image model takes an image context (vitx_ctx_create), not a text context"); return VITX_ERR_ARG; }
    if (dtype == VITX_MXFP8) { set_error("vitx_text_create: VITX_MXFP8 is not supported by text contexts (VITX_F16 or VITX_BF16)"); return VITX_ERR_UNSUPPORTED; }
    if (dtype != VITX_F16 && dtype != VITX_BF16) { set_error("vitx_text_create: unknown dtype %d", dtype); return VITX_ERR_ARG; }
    const vitx_hparams &hp = m->hp;
    const int D = hp.hidden_size, H = hp.num_attention_heads, T = hp.img_size, E = hp.num_classes;
    // every shape check before the first device call: nothing is launched after a refusal
    if (T > VITX_TEXT_MAX_TOKENS) { set_error("vitx_text_create: context length %d exceeds the %d tokens the text attention takes", T, VITX_TEXT_MAX_TOKENS); return VITX_ERR_UNSUPPORTED; }
    if (!attention_text_supports(T, D, H)) { set_error("vitx_text_create: attention needs a head_dim that is a multiple of 8 up to 128 (this model: %d / %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    if (!layernorm_supports(D)) { set_error("vitx_text_create: hidden_size %d has no LayerNorm instantiation", D); return VITX_ERR_UNSUPPORTED; }
    if (E % 64) { set_error("vitx_text_create: embedding width %d is not a multiple of 64", E); return VITX_ERR_UNSUPPORTED; }
    if ((long)max_prompts * T > (long)(0xf0000000u / ((size_t)4 * D * 2)) / 256 * 256) { set_error("vitx_text_create: max_prompts %d x %d tokens exceed the kernels' 32-bit buffer window", max_prompts, T); return VITX_ERR_UNSUPPORTED; }
    const Tuning *tune = nullptr;
    int rc;
    if ((rc = open_device("vitx_text_create", device, &tune))) return rc;
    std::unique_ptr<vitx_text> t(new (std::nothrow) vitx_text());
    if (!t) return VITX_ERR_NOMEM;
    t->model = m; t->device = device; t->dtype = dtype; t->tune = tune;
    t->D = D; t->L = hp.num_hidden_layers; t->H = H;
    t->tm = gemm_tile_m(); t->tn = gemm_tile_n();
    t->V = m->vocab; t->T = T; t->E = E; t->E_pad = head_cols_pad(m); t->causal = m->causal; t->eos = m->eos; t->max_prompts = max_prompts;
    t->fc1_epi = act_epi(m->activation); t->eps = hp.eps;
    const int Mcap = round_up(max_prompts * T, t->tm), Bcap = round_up(max_prompts, t->tm), tn = t->tn;
    struct { Tuning *tune; int M, N, K; } pins[] = {{&t->tune_qkv, Mcap, 3 * D, D}, {&t->tune_proj, Mcap, D, D}, {&t->tune_fc1, Mcap, 4 * D, D}, {&t->tune_fc2, Mcap, D, 4 * D}, {&t->tune_head, Bcap, E, D}};
    for (auto &p : pins) {
        *p.tune = *tune;
        // the dispatcher's own rule between its two ring tilings (gemm_ring_cfg, gemm.hip), at the rows of a full batch: never the wide persistent
        // kernels, whose choice depends on the row count of a call
        p.tune->gemm_cfg = gemm_ring_cfg(*tune, dense_gemm(nullptr, nullptr, nullptr, nullptr, p.M, p.M, p.N, round_up(p.N, tn), p.K));
        if (!p.tune->gemm_cfg) { set_error("vitx_text_create: no GEMM tiling for %d x %d x %d", p.M, p.N, p.K); return VITX_ERR_UNSUPPORTED; }
    }
    // quantised block matrices are expanded at upload (the comment at the top): block mode 0
    if ((rc = obtain_weights({m, device, dtype, false}, &t->wset, &t->weights_shared))) return rc;
    auto dmalloc = [&](void **p, size_t bytes) -> int {
        HIP_TRY(hipMalloc(p, bytes));
        t->allocs.push_back(*p);
        HIP_TRY(hipMemset(*p, 0, bytes));
        return VITX_OK;
    };
    const size_t Mp = (size_t)Mcap, Bp = (size_t)Bcap;
    t->host.assign((size_t)max_prompts * T + max_prompts, 0);
    if ((rc = dmalloc((void **)&t->pooled, t->host.size() * 4))) return rc;
    t->ids = t->pooled + max_prompts;
    if ((rc = dmalloc((void **)&t->X, Mp * D * 4))) return rc;
    if ((rc = dmalloc(&t->U, Mp * D * 2))) return rc;
    if ((rc = dmalloc(&t->QKV, Mp * 3 * D * 2))) return rc;
    if ((rc = dmalloc(&t->Hbuf, Mp * 4 * D * 2))) return rc;
    if ((rc = dmalloc(&t->Z, Bp * D * 2))) return rc;
    if ((rc = dmalloc((void **)&t->out, Bp * (size_t)E * 4))) return rc;
    if ((rc = dmalloc((void **)&t->raw, Bp * (size_t)E * 4))) return rc;
    HIP_TRY(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&t->uploaded, hipEventDisableTiming));
    HIP_TRY(hipDeviceSynchronize());
    *out = t.release();
    return VITX_OK;
}

// Host only: what vitx_text_embed refuses about its ids, and where it pools
int vitx_text_check_ids(const vitx_model *m, const int32_t *ids, int n, int32_t *pooled) {
    if (!m || !ids || n < 1 || m->kind != VITX_KIND_TEXT) { set_error("vitx_text_check_ids: a text-tower model, ids and n >= 1 are needed"); return VITX_ERR_ARG; }
    const int T = m->hp.img_size, V = m->vocab, eos = m->eos;
    for (int i = 0; i < n; ++i) {
        int at = eos < 0 ? T - 1 : -1;
        for (int k = 0; k < T; ++k) {
            const int id = ids[(size_t)i * T + k];
            if (id < 0 || id >= V) { set_error("vitx_text_embed: prompt %d, position %d: token id %d is outside 0 .. %d", i, k, id, V - 1); return VITX_ERR_ARG; }
            if (at < 0 && id == eos) at = k;
        }
        if (at < 0) { set_error("vitx_text_embed: prompt %d holds no EOS token (id %d): the model pools at the first one", i, eos); return VITX_ERR_ARG; }
        if (pooled) pooled[i] = at;
    }
    return VITX_OK;
}

void vitx_text_free(vitx_text *t) { delete t; }
int vitx_text_shares_weights(const vitx_text *t) { return t && t->weights_shared ? 1 : 0; }

int vitx_text_embed_device(vitx_text *t, const int32_t *ids, int n, int flags, void *d_out, void *stream) {
    int rc = check_call(t, ids, n, flags, d_out);
    if (rc) return rc;
    if ((rc = stage_ids(t, ids, n))) return rc;
    HIP_TRY(hipSetDevice(t->device));
    return text_forward(t, n, flags, (float *)d_out, (hipStream_t)stream);
}

int vitx_text_embed(vitx_text *t, const int32_t *ids, int n, int flags, float *out) {
    int rc = check_call(t, ids, n, flags, out);
    if (rc) return rc;
    if ((rc = stage_ids(t, ids, n))) return rc;
    HIP_TRY(hipSetDevice(t->device));
    if ((rc = text_forward(t, n, flags, t->out, t->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(out, t->out, (size_t)n * t->E * 4, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    return VITX_OK;
}

}  // extern "C"
