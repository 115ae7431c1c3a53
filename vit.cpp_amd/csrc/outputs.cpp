// outputs.cpp -- what a context gives besides probabilities: the per-kernel profile, the residual-stream trace, attention maps, features,
// and the diagnostics counters.  All opt-in; the forward (forward.cpp) launches nothing for an output that is off.
#include <cmath>
#include <utility>

#include "context.h"
#include "depth_bins.h"

// Synchronise and copy the n x fpi floats of an opt-in output to the host, or say why not.  `api`: "vitx_attn" / "vitx_feat"; n: the images
// of the last forward made with the output on (0: it is off, or no forward since <api>_enable)
static int read_output(vitx_ctx *c, const char *api, const char *what, int n, int fpi, const float *buf, float *out, size_t n_floats) {
    if (!out) return VITX_ERR_ARG;
    if (n == 0) { set_error("%s_read: no forward has run with %s on since %s_enable", api, what, api); return VITX_ERR_ARG; }
    const size_t need = (size_t)n * fpi;
    if (n_floats < need) { set_error("%s_read: buffer too small (%zu floats needed for %d images)", api, need, n); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, buf, need * 4, hipMemcpyDeviceToHost));
    return VITX_OK;
}

extern "C" {

int vitx_profile_enable(vitx_ctx *c, int on) {
    if (!c) return VITX_ERR_ARG;
    HIP_TRY(hipSetDevice(c->device));
    c->prof_on = on != 0; c->recs.clear(); c->ev_used = 0;
    if (on) {       // time origin for the busy-interval union (kernels of concurrent slices overlap)
        if (!c->prof_base) HIP_TRY(hipEventCreate(&c->prof_base));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipEventRecord(c->prof_base, c->stream));
        HIP_TRY(hipEventSynchronize(c->prof_base));
    }
    return VITX_OK;
}

// What the HIP-event bracket of vitx_profile_enable adds to ONE launch: 32 x [record, 20 us kernel that stamps its own first and last
// wall-clock reading, record] queued back to back on the context's stream like a profiled forward; the median of
// (event interval - the kernel's own interval).  bench.py subtracts it from every launch of the profiled step (r04: the bracket read
// 5.3-5.5 us above the device's dispatch stamps for every kernel class, so `roofline.achieved` was 4-13 % low).
int vitx_profile_bracket_us(vitx_ctx *c, double *bracket_us) {
    if (!c || !bracket_us) return VITX_ERR_ARG;
    HIP_TRY(hipSetDevice(c->device));
    constexpr int NB = 32;
    long long *d_st = nullptr; hipEvent_t ev[2 * NB];
    HIP_TRY(hipMalloc((void **)&d_st, sizeof(long long) * 2 * NB));
    const DevMem d_st_own(d_st);
    int made = 0; hipError_t e = hipSuccess;
    while (made < 2 * NB) { if ((e = hipEventCreate(&ev[made])) != hipSuccess) break; ++made; }      // `made` counts the handles that exist
    // nothing else of this device may be in flight (another slice stream's forward would stretch the brackets): the whole device, not only c->stream
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (int i = 0; i < NB && e == hipSuccess; ++i) {
        e = hipEventRecord(ev[2 * i], c->stream);
        if (e == hipSuccess) e = launch_spin_stamp(20, d_st + 2 * i, c->stream);
        if (e == hipSuccess) e = hipEventRecord(ev[2 * i + 1], c->stream);
    }
    long long h_st[2 * NB];
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(h_st, d_st, sizeof h_st, hipMemcpyDeviceToHost);
    std::vector<double> over;
    for (int i = 0; i < NB && e == hipSuccess; ++i) {
        float ms = 0.0f;
        e = hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]);
        over.push_back((double)ms * 1e3 - (double)(h_st[2 * i + 1] - h_st[2 * i]) * 0.01);
    }
    for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]);
    if (e != hipSuccess) { set_error("vitx_profile_bracket_us: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
    std::sort(over.begin(), over.end());
    *bracket_us = over[over.size() / 2];
    return VITX_OK;
}

int vitx_profile_read(vitx_ctx *c, vitx_prof_entry *out, int max_entries, int *n_entries) {
    if (!c || !out || !n_entries) return VITX_ERR_ARG;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    vitx_prof_entry acc[PC_COUNT];
    std::vector<std::pair<float, float>> iv[PC_COUNT];
    for (int i = 0; i < PC_COUNT; ++i) acc[i] = vitx_prof_entry{kProfNames[i], 0, 0.0, 0.0, 0.0, 0.0};
    for (const auto &r : c->recs) {
        float ms = 0.0f, ta = 0.0f, tb = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        if (c->prof_base) { HIP_TRY(hipEventElapsedTime(&ta, c->prof_base, r.a)); HIP_TRY(hipEventElapsedTime(&tb, c->prof_base, r.b)); iv[r.cls].push_back({ta, tb}); }
        acc[r.cls].launches++; acc[r.cls].total_ms += ms; acc[r.cls].flops += r.flops; acc[r.cls].bytes += r.bytes;
    }
    for (int i = 0; i < PC_COUNT; ++i) {        // union of this class's [start, stop] intervals over all streams
        std::sort(iv[i].begin(), iv[i].end());
        double busy = 0.0; float cur_a = 0, cur_b = -1;
        for (auto &p : iv[i]) {
            if (cur_b < cur_a || p.first > cur_b) { if (cur_b >= cur_a) busy += cur_b - cur_a; cur_a = p.first; cur_b = p.second; }
            else cur_b = std::max(cur_b, p.second);
        }
        if (cur_b >= cur_a && !iv[i].empty()) busy += cur_b - cur_a;
        acc[i].busy_ms = iv[i].empty() ? acc[i].total_ms : busy;
    }
    int k = 0;
    for (int i = 0; i < PC_COUNT && k < max_entries; ++i) if (acc[i].launches) out[k++] = acc[i];
    *n_entries = k;
    c->recs.clear(); c->ev_used = 0;
    return VITX_OK;
}

int vitx_ctx_stream_retries(const vitx_ctx *c) { return c ? c->stream_retries : -1; }
long long vitx_ctx_graph_launches(const vitx_ctx *c) { return c ? c->graph_launches : -1; }
int vitx_ctx_ln_fusion_active(const vitx_ctx *c) { return c ? ((c->ln_fuse && !c->slices.empty() && c->slices[0].ln_sync && c->tune->n_xcd == 8) ? 1 : (c->ln_fuse_disabled ? -1 : 0)) : 0; }
long long vitx_ctx_ln_fallbacks(vitx_ctx *c) {
    if (!c) return -1;
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    long long total = 0;
    for (auto &sl : c->slices) {
        if (!sl.ln_todo) continue;
        unsigned v = 0;
        if (hipMemcpy(&v, sl.ln_todo + sl.ln_blocks, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        total += v;
    }
    return total;
}

int vitx_trace_enable(vitx_ctx *c, const int32_t *image_ids, int n) {
    if (!c || n < 0 || (n > 0 && !image_ids)) return VITX_ERR_ARG;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    if (c->trace_buf) { (void)hipFree(c->trace_buf); c->trace_buf = nullptr; }
    c->trace_ids.assign(image_ids, image_ids + n);
    for (int id : c->trace_ids) if (id < 0 || id >= c->max_batch) { c->trace_ids.clear(); set_error("vitx_trace_enable: image id %d outside 0..%d", id, c->max_batch - 1); return VITX_ERR_ARG; }
    if (n) HIP_TRY(hipMalloc((void **)&c->trace_buf, (size_t)(c->L + 1) * n * c->N * c->D * 4));
    return VITX_OK;
}
int vitx_trace_read(vitx_ctx *c, float *out, size_t n_floats) {
    if (!c || !out) return VITX_ERR_ARG;
    const size_t need = (size_t)(c->L + 1) * c->trace_ids.size() * c->N * c->D;
    if (!c->trace_buf || n_floats < need) { set_error("vitx_trace_read: trace not enabled or buffer too small (%zu floats needed)", need); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, c->trace_buf, need * 4, hipMemcpyDeviceToHost));
    return VITX_OK;
}

int vitx_attn_enable(vitx_ctx *c, uint64_t layer_mask, int flags) {
    if (!c) return VITX_ERR_ARG;
    if (flags & ~VITX_ATTN_ROLLOUT) { set_error("vitx_attn_enable: unknown flags 0x%x", flags); return VITX_ERR_ARG; }
    if (c->L < 64 && (layer_mask >> c->L)) { set_error("vitx_attn_enable: layer mask 0x%llx names layers beyond the model's %d", (unsigned long long)layer_mask, c->L); return VITX_ERR_ARG; }
    const bool on = layer_mask != 0 || flags != 0, rollout = (flags & VITX_ATTN_ROLLOUT) != 0;
    if (on && c->R != 1) { set_error("vitx_attn_enable: attention maps are not available for ViTSTR contexts"); return VITX_ERR_UNSUPPORTED; }
    if (on && c->map) { set_error("vitx_attn_enable: the maps are defined by the class-token row, and a model with the attention-pooling head has no class token"); return VITX_ERR_UNSUPPORTED; }
    if (on && !attention_map_supports(c->N, c->D, c->H)) { set_error("vitx_attn_enable: head_dim %d is not covered by the map kernels", c->D / c->H); return VITX_ERR_UNSUPPORTED; }
    if (rollout && !attention_mean_supports(c->N, c->D, c->H)) { set_error("vitx_attn_enable: rollout keeps two N x N matrices per image and takes at most %d tokens (this model: %d)", kAttnMeanMaxTokens, c->N); return VITX_ERR_UNSUPPORTED; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());          // no forward in flight writes the buffers about to be freed
    c->attn_free();
    c->attn_mask = 0; c->attn_flags = 0; c->attn_fpi = 0; c->attn_cap = 0; c->attn_n = 0;
    if (!on) return VITX_OK;
    const int cap = c->pass_cap(), N = c->N, H = c->H;
    const int fpi = layer_slot(layer_mask, c->L) * H * N + (rollout ? N : 0);
    auto alloc = [&](float **p, size_t floats) { if (hipMalloc((void **)p, floats * 4) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; } return true; };
    bool ok = alloc(&c->attn_out, (size_t)cap * fpi);
    if (ok && rollout) ok = alloc(&c->attn_roll[0], (size_t)cap * N * N) && alloc(&c->attn_roll[1], (size_t)cap * N * N);
    if (ok && rollout && !((layer_mask >> (c->L - 1)) & 1)) ok = alloc(&c->attn_cls_last, (size_t)cap * H * N);
    if (!ok) { c->attn_free(); set_error("vitx_attn_enable: cannot allocate the map buffers for %d images", cap); return VITX_ERR_NOMEM; }
    c->attn_mask = layer_mask; c->attn_flags = flags; c->attn_fpi = fpi; c->attn_cap = cap;
    return VITX_OK;
}
int vitx_attn_floats(const vitx_ctx *c) { return c ? c->attn_fpi : 0; }
int vitx_attn_images(const vitx_ctx *c) { return c ? c->attn_n : 0; }
int vitx_attn_read(vitx_ctx *c, float *out, size_t n_floats) {
    return c ? read_output(c, "vitx_attn", "attention maps", c->attn_on() ? c->attn_n : 0, c->attn_fpi, c->attn_out, out, n_floats) : VITX_ERR_ARG;
}

int vitx_feat_enable(vitx_ctx *c, int flags, uint64_t layer_mask) {
    if (!c) return VITX_ERR_ARG;
    constexpr int kinds = VITX_FEAT_CLS | VITX_FEAT_MEAN | VITX_FEAT_TOKENS;
    if (flags & ~(kinds | VITX_FEAT_L2)) { set_error("vitx_feat_enable: unknown flags 0x%x", flags); return VITX_ERR_ARG; }
    if (flags && !(flags & kinds)) { set_error("vitx_feat_enable: VITX_FEAT_L2 modifies VITX_FEAT_CLS / VITX_FEAT_MEAN and selects nothing on its own"); return VITX_ERR_ARG; }
    if (c->L < 64 && (layer_mask >> c->L)) { set_error("vitx_feat_enable: layer mask 0x%llx names layers beyond the model's %d", (unsigned long long)layer_mask, c->L); return VITX_ERR_ARG; }
    if (flags && c->R != 1) { set_error("vitx_feat_enable: features are not available for ViTSTR contexts"); return VITX_ERR_UNSUPPORTED; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());          // no forward in flight writes the buffer about to be freed
    c->feat_free();
    c->feat_flags = 0; c->feat_mask = 0; c->feat_fpi = 0; c->feat_cap = 0; c->feat_n = 0;
    if (!flags) return VITX_OK;
    if (!layer_mask) layer_mask = 1ull << (c->L - 1);
    if (c->map && (flags & VITX_FEAT_CLS) && layer_mask != 1ull << (c->L - 1)) {
        set_error("vitx_feat_enable: VITX_FEAT_CLS of a model with the attention-pooling head is the pooled embedding: it exists for the last layer only (mask 0x%llx)", (unsigned long long)layer_mask);
        return VITX_ERR_ARG;
    }
    c->feat_flags = flags;                    // feat_layer_floats() reads it
    const int cap = c->pass_cap();
    const size_t fpi = (size_t)layer_slot(layer_mask, c->L) * c->feat_layer_floats();
    if (fpi > 0x7fffffff || hipMalloc((void **)&c->feat_out, (size_t)cap * fpi * 4) != hipSuccess) {
        (void)hipGetLastError(); c->feat_out = nullptr; c->feat_flags = 0;
        set_error("vitx_feat_enable: cannot allocate the feature buffer for %d images of %zu floats", cap, fpi);
        return VITX_ERR_NOMEM;
    }
    c->feat_mask = layer_mask; c->feat_fpi = (int)fpi; c->feat_cap = cap;
    return VITX_OK;
}
int vitx_feat_floats(const vitx_ctx *c) { return c ? c->feat_fpi : 0; }
int vitx_feat_images(const vitx_ctx *c) { return c ? c->feat_n : 0; }
const void *vitx_feat_device(const vitx_ctx *c) { return c ? c->feat_out : nullptr; }
int vitx_feat_read(vitx_ctx *c, float *out, size_t n_floats) {
    return c ? read_output(c, "vitx_feat", "features", c->feat_on() ? c->feat_n : 0, c->feat_fpi, c->feat_out, out, n_floats) : VITX_ERR_ARG;
}

// Zero-shot classification: the bank of a context (include/vitx.h).  Every argument check comes before the first device call.
int vitx_zeroshot_set(vitx_ctx *c, const float *bank, int K, int E, int kind, float scale, float bias) {
    if (!c) return VITX_ERR_ARG;
    const bool off = !bank && K == 0;
    if (!off) {
        if (!bank) { set_error("vitx_zeroshot_set: NULL bank with K = %d", K); return VITX_ERR_ARG; }
        if (K < 1) { set_error("vitx_zeroshot_set: K = %d (a bank has at least one class; NULL and 0 turn it off)", K); return VITX_ERR_ARG; }
        if (kind != VITX_ZS_SOFTMAX && kind != VITX_ZS_SIGMOID) { set_error("vitx_zeroshot_set: unknown kind %d (0 softmax, 1 sigmoid)", kind); return VITX_ERR_ARG; }
        if (!std::isfinite(scale) || !std::isfinite(bias)) { set_error("vitx_zeroshot_set: scale and bias must be finite"); return VITX_ERR_ARG; }
        if (c->R != 1) { set_error("vitx_zeroshot_set: zero-shot classification is not available for ViTSTR contexts"); return VITX_ERR_UNSUPPORTED; }
        if (E != c->zs_width()) { set_error("vitx_zeroshot_set: the bank's width %d is not this context's embedding width %d (%s)", E, c->zs_width(), c->map ? "the pooled embedding: hidden_size" : "the head's rows: num_classes"); return VITX_ERR_ARG; }
        if (E % 64) { set_error("vitx_zeroshot_set: the embedding width %d is not a multiple of 64 (the GEMMs' K step)", E); return VITX_ERR_UNSUPPORTED; }
        if (K > vitx_zeroshot_max_classes(E)) { set_error("vitx_zeroshot_set: %d classes of width %d exceed the bank GEMM's 32-bit window (at most %d)", K, E, vitx_zeroshot_max_classes(E)); return VITX_ERR_UNSUPPORTED; }
        for (size_t i = 0, nb = (size_t)K * E; i < nb; ++i)
            if (!std::isfinite(bank[i])) { set_error("vitx_zeroshot_set: bank entry [%zu][%zu] is not finite", i / E, i % E); return VITX_ERR_ARG; }
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());          // no forward in flight reads or writes the buffers about to be freed
    c->zs_free();
    if (off) return VITX_OK;
    const int Kpad = round_up(K, c->tn), cap = c->pass_cap();
    const size_t rows = (size_t)round_up(cap, c->tm);
    const std::vector<uint16_t> hb = operand_matrix_host(c->dtype, bank, nullptr, K, E, Kpad, E, 0, 0);
    auto alloc = [](void **p, size_t bytes) { if (hipMalloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; } return true; };
    bool ok = alloc(&c->zs_bank, hb.size() * 2) && alloc((void **)&c->zs_zero, (size_t)Kpad * 4) && alloc((void **)&c->zs_out, (size_t)cap * 2 * K * 4);
    c->zs_a.assign(c->nslices, nullptr); c->zs_acc.assign(c->nslices, nullptr);
    for (int i = 0; ok && i < c->nslices; ++i) ok = alloc(&c->zs_a[i], rows * E * 2) && alloc((void **)&c->zs_acc[i], rows * Kpad * 4);
    if (!ok) { c->zs_free(); set_error("vitx_zeroshot_set: cannot allocate the buffers for %d classes and %d images", K, cap); return VITX_ERR_NOMEM; }
    hipError_t e = hipMemcpy(c->zs_bank, hb.data(), hb.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(c->zs_zero, 0, (size_t)Kpad * 4);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { c->zs_free(); set_error("vitx_zeroshot_set: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
    c->zs_K = K; c->zs_Kpad = Kpad; c->zs_kind = kind; c->zs_scale = scale; c->zs_bias = bias; c->zs_cap = cap;
    return VITX_OK;
}
int vitx_zeroshot_classes(const vitx_ctx *c) { return c ? c->zs_K : 0; }
int vitx_zeroshot_images(const vitx_ctx *c) { return c ? c->zs_n : 0; }
const void *vitx_zeroshot_device(const vitx_ctx *c) { return c ? c->zs_out : nullptr; }
int vitx_zeroshot_read(vitx_ctx *c, float *probs, float *logits, size_t n_floats_each) {
    if (!c || !probs) return VITX_ERR_ARG;
    const int n = c->zs_on() ? c->zs_n : 0, K = c->zs_K;
    if (n == 0) { set_error("vitx_zeroshot_read: no forward has run with a bank set since vitx_zeroshot_set"); return VITX_ERR_ARG; }
    const size_t need = (size_t)n * K;
    if (n_floats_each < need) { set_error("vitx_zeroshot_read: buffer too small (%zu floats needed for %d images of %d classes)", need, n, K); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy2D(probs, (size_t)K * 4, c->zs_out, (size_t)2 * K * 4, (size_t)K * 4, n, hipMemcpyDeviceToHost));
    if (logits) HIP_TRY(hipMemcpy2D(logits, (size_t)K * 4, c->zs_out + K, (size_t)2 * K * 4, (size_t)K * 4, n, hipMemcpyDeviceToHost));
    return VITX_OK;
}

// Nearest neighbours: the gallery of a context (include/vitx.h).  Every argument check comes before the first device call.
int vitx_nn_width(const vitx_ctx *c, int source) { return c ? c->nn_width(source) : 0; }
int vitx_nn_set(vitx_ctx *c, const float *gallery, long G, int E, int k, int source, const int32_t *labels, int n_labels, float temperature) {
    if (!c) return VITX_ERR_ARG;
    const bool off = !gallery && G == 0;
    if (!off) {
        if (!gallery) { set_error("vitx_nn_set: NULL gallery with G = %ld", G); return VITX_ERR_ARG; }
        if (source != VITX_NN_LOGITS && source != VITX_NN_EMBED) { set_error("vitx_nn_set: unknown source %d (0 logits, 1 embed)", source); return VITX_ERR_ARG; }
        if (k < 1 || k > G) { set_error("vitx_nn_set: k = %d outside 1 .. G = %ld", k, G); return VITX_ERR_ARG; }
        if (labels && n_labels < 1) { set_error("vitx_nn_set: labels with n_labels = %d", n_labels); return VITX_ERR_ARG; }
        if (labels && !(std::isfinite(temperature) && temperature > 0.0f)) { set_error("vitx_nn_set: the vote's temperature must be finite and positive"); return VITX_ERR_ARG; }
        if (c->R != 1) { set_error("vitx_nn_set: nearest neighbours are not available for ViTSTR contexts"); return VITX_ERR_UNSUPPORTED; }
        if (E != c->nn_width(source)) { set_error("vitx_nn_set: the gallery's width %d is not this context's width %d of source %d", E, c->nn_width(source), source); return VITX_ERR_ARG; }
        if (k > kNnMaxK) { set_error("vitx_nn_set: k = %d above %d", k, kNnMaxK); return VITX_ERR_UNSUPPORTED; }
        if (E % 64) { set_error("vitx_nn_set: the embedding width %d is not a multiple of 64 (the GEMMs' K step)", E); return VITX_ERR_UNSUPPORTED; }
        if (G >= 0x7fffffffL - 127) { set_error("vitx_nn_set: %ld gallery rows: indices are 31 bits (at most 2^31 - 129 rows)", G); return VITX_ERR_UNSUPPORTED; }
        if ((size_t)round_up(c->pass_cap(), c->tm) * vitx_ctx::kNnChunk * 4 > 0xf0000000u) {       // the chunk GEMM addresses its output inside a 32-bit byte window
            set_error("vitx_nn_set: the score scratch of %d images exceeds the chunk GEMM's 32-bit window (at most %d images per pass)", c->pass_cap(), (int)(0xf0000000u / 4 / vitx_ctx::kNnChunk / c->tm * c->tm));
            return VITX_ERR_UNSUPPORTED;
        }
        for (size_t i = 0, nb = (size_t)G * E; i < nb; ++i)
            if (!std::isfinite(gallery[i])) { set_error("vitx_nn_set: gallery entry [%zu][%zu] is not finite", i / E, i % E); return VITX_ERR_ARG; }
        if (labels) for (long g = 0; g < G; ++g)
            if (labels[g] < 0 || labels[g] >= n_labels) { set_error("vitx_nn_set: label %d of gallery row %ld outside 0 .. %d", labels[g], g, n_labels - 1); return VITX_ERR_ARG; }
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());          // no forward in flight reads or writes the buffers about to be freed
    c->nn_free();
    if (off) return VITX_OK;
    constexpr int Gc = vitx_ctx::kNnChunk;
    const long Gpad = (G + c->tn - 1) / c->tn * c->tn;
    const int cap = c->pass_cap();
    const size_t rows = (size_t)round_up(cap, c->tm), state_bytes = nn_state_bytes((int)rows, k);
    auto alloc = [](void **p, size_t bytes) { if (hipMalloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; } return true; };
    bool ok = alloc(&c->nn_gallery, (size_t)Gpad * E * 2) && alloc((void **)&c->nn_zero, (size_t)Gc * 4) && alloc((void **)&c->nn_out, (size_t)cap * k * 8);
    if (ok && labels) ok = alloc((void **)&c->nn_labels, (size_t)G * 4) && alloc((void **)&c->nn_vote, (size_t)cap * n_labels * 4);
    c->nn_a.assign(c->nslices, nullptr); c->nn_acc.assign(c->nslices, nullptr); c->nn_state.assign(c->nslices, nullptr);
    for (int i = 0; ok && i < c->nslices; ++i) ok = alloc(&c->nn_a[i], rows * E * 2) && alloc((void **)&c->nn_acc[i], rows * Gc * 4) && alloc(&c->nn_state[i], state_bytes);
    if (!ok) { c->nn_free(); set_error("vitx_nn_set: cannot allocate the buffers for %ld gallery rows and %d images", G, cap); return VITX_ERR_NOMEM; }
    // the gallery goes up in blocks of rows, rounded (RNE) to the operand type; the zero rows beyond G come from the memset
    hipError_t e = hipMemset(c->nn_gallery, 0, (size_t)Gpad * E * 2);
    if (e == hipSuccess) e = hipMemset(c->nn_zero, 0, (size_t)Gc * 4);
    for (long g0 = 0; g0 < G && e == hipSuccess; g0 += 65536) {
        const int nr = (int)std::min<long>(65536, G - g0);
        const std::vector<uint16_t> hb = operand_matrix_host(c->dtype, gallery + (size_t)g0 * E, nullptr, nr, E, nr, E, 0, 0);
        e = hipMemcpy((char *)c->nn_gallery + (size_t)g0 * E * 2, hb.data(), hb.size() * 2, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && labels) e = hipMemcpy(c->nn_labels, labels, (size_t)G * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { c->nn_free(); set_error("vitx_nn_set: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
    c->nn_G = G; c->nn_Gpad = Gpad; c->nn_k = k; c->nn_source = source; c->nn_E = E; c->nn_nlabels = labels ? n_labels : 0; c->nn_T = labels ? temperature : 0.0f; c->nn_cap = cap;
    c->nn_scratch = (size_t)c->nslices * (rows * Gc * 4 + state_bytes);
    return VITX_OK;
}
long vitx_nn_rows(const vitx_ctx *c) { return c ? c->nn_G : 0; }
int vitx_nn_k(const vitx_ctx *c) { return c ? c->nn_k : 0; }
int vitx_nn_labels(const vitx_ctx *c) { return c ? c->nn_nlabels : 0; }
int vitx_nn_images(const vitx_ctx *c) { return c ? c->nn_n : 0; }
const void *vitx_nn_device(const vitx_ctx *c) { return c ? c->nn_out : nullptr; }
size_t vitx_nn_scratch_bytes(const vitx_ctx *c) { return c ? c->nn_scratch : 0; }
int vitx_nn_read(vitx_ctx *c, int32_t *idx, float *score, float *vote) {
    if (!c || !idx || !score) return VITX_ERR_ARG;
    const int n = c->nn_on() ? c->nn_n : 0, k = c->nn_k;
    if (n == 0) { set_error("vitx_nn_read: no forward has run with a gallery set since vitx_nn_set"); return VITX_ERR_ARG; }
    if (vote && !c->nn_nlabels) { set_error("vitx_nn_read: the gallery has no labels: there is no vote"); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy2D(score, 4, c->nn_out, 8, 4, (size_t)n * k, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy2D(idx, 4, c->nn_out + 1, 8, 4, (size_t)n * k, hipMemcpyDeviceToHost));
    if (vote) HIP_TRY(hipMemcpy(vote, c->nn_vote, (size_t)n * c->nn_nlabels * 4, hipMemcpyDeviceToHost));
    return VITX_OK;
}

// The dense head of a context (include/vitx.h "dense prediction").  Every argument check comes before the first device call.
int vitx_dense_set(vitx_ctx *c, const float *W, const float *bias, int K, int Dc, uint64_t layer_mask, int out_h, int out_w, int flags) {
    if (!c) return VITX_ERR_ARG;
    const bool off = !W && K == 0;
    uint64_t mask = layer_mask;
    int m = 0, oh = out_h, ow = out_w;
    if (!off) {
        if (!W) { set_error("vitx_dense_set: NULL weights with K = %d", K); return VITX_ERR_ARG; }
        if (K < 1) { set_error("vitx_dense_set: K = %d classes", K); return VITX_ERR_ARG; }
        if (flags & ~(VITX_DENSE_SCORE | VITX_DENSE_LOGITS)) { set_error("vitx_dense_set: unknown flags 0x%x", flags); return VITX_ERR_ARG; }
        if (mask == 0) mask = 1ull << (c->L - 1);
        if (c->L < 64 && (mask >> c->L)) { set_error("vitx_dense_set: layer mask selects a layer at or beyond L = %d", c->L); return VITX_ERR_ARG; }
        m = __builtin_popcountll(mask);
        if (m > 4) { set_error("vitx_dense_set: %d layers selected, at most 4", m); return VITX_ERR_ARG; }
        if (Dc != m * c->D) { set_error("vitx_dense_set: the head's width %d is not %d layers x D = %d", Dc, m, m * c->D); return VITX_ERR_ARG; }
        if (out_h < 0 || out_w < 0 || ((out_h == 0) != (out_w == 0))) { set_error("vitx_dense_set: output shape %d x %d (0 x 0: the context's image shape)", out_h, out_w); return VITX_ERR_ARG; }
        if (out_h == 0) { oh = c->Sh; ow = c->Sw; }
        for (size_t i = 0, nb = (size_t)K * Dc; i < nb; ++i)
            if (!std::isfinite(W[i])) { set_error("vitx_dense_set: weight [%zu][%zu] is not finite", i / Dc, i % Dc); return VITX_ERR_ARG; }
        if (bias) for (int k = 0; k < K; ++k)
            if (!std::isfinite(bias[k])) { set_error("vitx_dense_set: bias [%d] is not finite", k); return VITX_ERR_ARG; }
        if (K > kDenseMaxK) { set_error("vitx_dense_set: K = %d classes above %d (labels are bytes)", K, kDenseMaxK); return VITX_ERR_UNSUPPORTED; }
        if (c->R != 1) { set_error("vitx_dense_set: the dense head is not available for ViTSTR contexts"); return VITX_ERR_UNSUPPORTED; }
        if (oh < c->gh || ow < c->gw || oh > kDenseMaxOut || ow > kDenseMaxOut) {
            set_error("vitx_dense_set: output %d x %d outside the patch grid %d x %d .. %d (upsampling only)", oh, ow, c->gh, c->gw, kDenseMaxOut);
            return VITX_ERR_UNSUPPORTED;
        }
        const size_t rows = (size_t)c->pass_cap() * c->gh * c->gw;
        if (rows * Dc * 2 > 0xf0000000u || rows * round_up(K, c->tn) * 4 > 0xf0000000u || c->pass_cap() > 65535) {
            set_error("vitx_dense_set: the operand or logit rows of a pass of %d images leave the GEMM's 32-bit byte window", c->pass_cap());
            return VITX_ERR_UNSUPPORTED;
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());          // no forward in flight reads or writes the buffers about to be freed
    c->dense_free();
    if (off) return VITX_OK;
    const int Kpad = round_up(K, c->tn), cap = c->pass_cap(), Np = c->gh * c->gw;
    const size_t px = (size_t)oh * ow;
    auto alloc = [](void **p, size_t bytes) { if (hipMalloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; } return true; };
    bool ok = alloc(&c->dn_W, (size_t)Kpad * Dc * 2) && alloc((void **)&c->dn_bias, (size_t)Kpad * 4) && alloc((void **)&c->dn_labels, (size_t)cap * px);
    if (ok && (flags & VITX_DENSE_SCORE)) ok = alloc((void **)&c->dn_score, (size_t)cap * px * 4);
    if (ok && (flags & VITX_DENSE_LOGITS)) ok = alloc((void **)&c->dn_logits, (size_t)cap * Np * K * 4);
    c->dn_a.assign(c->nslices, nullptr); c->dn_acc.assign(c->nslices, nullptr);
    size_t scratch = 0;
    hipError_t e = hipSuccess;
    for (int i = 0; ok && i < c->nslices; ++i) {
        const size_t rows = (size_t)round_up(std::min(c->slices[i].cap, cap) * Np, c->tm);
        ok = alloc(&c->dn_a[i], rows * Dc * 2) && alloc((void **)&c->dn_acc[i], rows * Kpad * 4);
        if (ok) e = hipMemset(c->dn_a[i], 0, rows * Dc * 2);
        if (e != hipSuccess) break;
        scratch += rows * Dc * 2 + rows * Kpad * 4;
    }
    if (!ok) { c->dense_free(); set_error("vitx_dense_set: cannot allocate the buffers for %d classes, %d x %d labels and %d images", K, oh, ow, cap); return VITX_ERR_NOMEM; }
    // the head goes up rounded (RNE) to the operand type; the zero rows beyond K come from operand_matrix_host, the zero biases from the memset
    if (e == hipSuccess) {
        const std::vector<uint16_t> hw = operand_matrix_host(c->dtype, W, nullptr, K, Dc, Kpad, Dc, 0, 0);
        e = hipMemcpy(c->dn_W, hw.data(), hw.size() * 2, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemset(c->dn_bias, 0, (size_t)Kpad * 4);
    if (e == hipSuccess && bias) e = hipMemcpy(c->dn_bias, bias, (size_t)K * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { c->dense_free(); set_error("vitx_dense_set: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
    c->dn_K = K; c->dn_Kpad = Kpad; c->dn_Dc = Dc; c->dn_mask = mask; c->dn_oh = oh; c->dn_ow = ow; c->dn_flags = flags; c->dn_cap = cap; c->dn_scratch = scratch;
    return VITX_OK;
}
int vitx_dense_classes(const vitx_ctx *c) { return c ? c->dn_K : 0; }
int vitx_dense_shape(const vitx_ctx *c, int *out_h, int *out_w) {
    if (!c) return VITX_ERR_ARG;
    if (out_h) *out_h = c->dn_oh;
    if (out_w) *out_w = c->dn_ow;
    return VITX_OK;
}
int vitx_dense_images(const vitx_ctx *c) { return c ? c->dn_n : 0; }
const void *vitx_dense_device(const vitx_ctx *c) { return c ? c->dn_labels : nullptr; }
size_t vitx_dense_scratch_bytes(const vitx_ctx *c) { return c ? c->dn_scratch : 0; }
int vitx_dense_read(vitx_ctx *c, uint8_t *labels, float *score, float *logits) {
    if (!c || !labels) return VITX_ERR_ARG;
    const int n = c->dense_on() ? c->dn_n : 0;
    if (n == 0) { set_error("vitx_dense_read: no forward has run with a dense head set since vitx_dense_set"); return VITX_ERR_ARG; }
    if (score && !c->dn_score) { set_error("vitx_dense_read: the head was set without VITX_DENSE_SCORE"); return VITX_ERR_ARG; }
    if (logits && !c->dn_logits) { set_error("vitx_dense_read: the head was set without VITX_DENSE_LOGITS"); return VITX_ERR_ARG; }
    const size_t px = (size_t)c->dn_oh * c->dn_ow;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(labels, c->dn_labels, (size_t)n * px, hipMemcpyDeviceToHost));
    if (score) HIP_TRY(hipMemcpy(score, c->dn_score, (size_t)n * px * 4, hipMemcpyDeviceToHost));
    if (logits) HIP_TRY(hipMemcpy(logits, c->dn_logits, (size_t)n * c->gh * c->gw * c->dn_K * 4, hipMemcpyDeviceToHost));
    return VITX_OK;
}

// The depth head of a context (include/vitx.h "depth estimation").  Every argument check comes before the first device call.
int vitx_depth_set(vitx_ctx *c, const float *Wp, const float *Wc, const float *bias, const float *bins, int K, int Dc, uint64_t layer_mask, int upsample,
                   float min_depth, float max_depth, int out_h, int out_w, int flags) {
    if (!c) return VITX_ERR_ARG;
    const bool off = !Wp && K == 0;
    uint64_t mask = layer_mask;
    int m = 0, oh = out_h, ow = out_w;
    const int fh = upsample * c->gh, fw = upsample * c->gw;
    if (!off) {
        if (!Wp || !bins) { set_error("vitx_depth_set: NULL weights or bins with K = %d", K); return VITX_ERR_ARG; }
        if (K < 1) { set_error("vitx_depth_set: K = %d bins", K); return VITX_ERR_ARG; }
        if (flags & ~(VITX_DEPTH_NORM | VITX_DEPTH_LOGITS | VITX_DEPTH_FINE)) { set_error("vitx_depth_set: unknown flags 0x%x", flags); return VITX_ERR_ARG; }
        if (mask == 0) mask = 1ull << (c->L - 1);
        if (c->L < 64 && (mask >> c->L)) { set_error("vitx_depth_set: layer mask selects a layer at or beyond L = %d", c->L); return VITX_ERR_ARG; }
        m = __builtin_popcountll(mask);
        if (m > 4) { set_error("vitx_depth_set: %d layers selected, at most 4", m); return VITX_ERR_ARG; }
        if (Dc != m * c->D) { set_error("vitx_depth_set: the head's width %d is not %d layers x D = %d", Dc, m, m * c->D); return VITX_ERR_ARG; }
        if (out_h < 0 || out_w < 0 || ((out_h == 0) != (out_w == 0))) { set_error("vitx_depth_set: output shape %d x %d (0 x 0: the context's image shape)", out_h, out_w); return VITX_ERR_ARG; }
        if (out_h == 0) { oh = c->Sh; ow = c->Sw; }
        if (!std::isfinite(min_depth) || !std::isfinite(max_depth) || min_depth > max_depth) { set_error("vitx_depth_set: the depth range %g .. %g must be finite and ordered", (double)min_depth, (double)max_depth); return VITX_ERR_ARG; }
        for (const float *W : {Wp, Wc})
            if (W) for (size_t i = 0, nb = (size_t)K * Dc; i < nb; ++i)
                if (!std::isfinite(W[i])) { set_error("vitx_depth_set: %s weight [%zu][%zu] is not finite", W == Wp ? "patch" : "class", i / Dc, i % Dc); return VITX_ERR_ARG; }
        for (int k = 0; k < K; ++k) {
            if (bias && !std::isfinite(bias[k])) { set_error("vitx_depth_set: bias [%d] is not finite", k); return VITX_ERR_ARG; }
            if (!std::isfinite(bins[k]) || !(bins[k] > 0.0f)) { set_error("vitx_depth_set: bin [%d] = %g is not a finite positive depth", k, (double)bins[k]); return VITX_ERR_ARG; }
        }
        if (K > kDepthMaxK) { set_error("vitx_depth_set: K = %d bins above %d", K, kDepthMaxK); return VITX_ERR_UNSUPPORTED; }
        if (upsample != 1 && upsample != 2 && upsample != 4) { set_error("vitx_depth_set: upsample = %d, not 1, 2 or 4", upsample); return VITX_ERR_UNSUPPORTED; }
        if (c->R != 1) { set_error("vitx_depth_set: the depth head is not available for ViTSTR contexts"); return VITX_ERR_UNSUPPORTED; }
        if (Wc && c->map) { set_error("vitx_depth_set: a class half on a context without a class token (VITX_POOL_MAP)"); return VITX_ERR_UNSUPPORTED; }
        if (oh < fh || ow < fw || oh > kDepthMaxOut || ow > kDepthMaxOut) {
            set_error("vitx_depth_set: output %d x %d outside the fine plane %d x %d .. %d (upsampling only)", oh, ow, fh, fw, kDepthMaxOut);
            return VITX_ERR_UNSUPPORTED;
        }
        const size_t rows = (size_t)c->pass_cap() * c->gh * c->gw;
        if (rows * Dc * 2 > 0xf0000000u || rows * round_up(K, c->tn) * 4 > 0xf0000000u || c->pass_cap() > 65535) {
            set_error("vitx_depth_set: the operand or logit rows of a pass of %d images leave the GEMM's 32-bit byte window", c->pass_cap());
            return VITX_ERR_UNSUPPORTED;
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());          // no forward in flight reads or writes the buffers about to be freed
    c->depth_free();
    if (off) return VITX_OK;
    const int Kpad = round_up(K, c->tn), cap = c->pass_cap(), Np = c->gh * c->gw;
    const size_t px = (size_t)oh * ow, fpx = (size_t)fh * fw;
    auto alloc = [](void **p, size_t bytes) { if (hipMalloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; } return true; };
    bool ok = alloc(&c->dp_Wp, (size_t)Kpad * Dc * 2) && (!Wc || alloc(&c->dp_Wc, (size_t)Kpad * Dc * 2)) && alloc((void **)&c->dp_bias, (size_t)Kpad * 4) &&
              alloc((void **)&c->dp_zero, (size_t)Kpad * 4) && alloc((void **)&c->dp_bins, (size_t)Kpad * 4) && alloc((void **)&c->dp_depth, (size_t)cap * px * 4) &&
              alloc((void **)&c->dp_fine, (size_t)cap * fpx * 4);
    if (ok && (flags & VITX_DEPTH_LOGITS)) ok = alloc((void **)&c->dp_logits, (size_t)cap * Np * K * 4) && (!Wc || alloc((void **)&c->dp_off, (size_t)cap * K * 4));
    c->dp_a.assign(c->nslices, nullptr); c->dp_acc.assign(c->nslices, nullptr); c->dp_ac.assign(c->nslices, nullptr); c->dp_o.assign(c->nslices, nullptr);
    size_t scratch = 0;
    hipError_t e = hipSuccess;
    for (int i = 0; ok && i < c->nslices; ++i) {
        const int imgs = std::min(c->slices[i].cap, cap);
        const size_t rows = (size_t)round_up(imgs * Np, c->tm), crows = (size_t)round_up(imgs, c->tm);
        ok = alloc(&c->dp_a[i], rows * Dc * 2) && alloc((void **)&c->dp_acc[i], rows * Kpad * 4);
        if (ok) e = hipMemset(c->dp_a[i], 0, rows * Dc * 2);
        scratch += rows * Dc * 2 + rows * Kpad * 4;
        if (ok && Wc && e == hipSuccess) {
            ok = alloc(&c->dp_ac[i], crows * Dc * 2) && alloc((void **)&c->dp_o[i], crows * Kpad * 4);
            if (ok) e = hipMemset(c->dp_ac[i], 0, crows * Dc * 2);
            scratch += crows * Dc * 2 + crows * Kpad * 4;
        }
        if (e != hipSuccess) break;
    }
    if (!ok) { c->depth_free(); set_error("vitx_depth_set: cannot allocate the buffers for %d bins, %d x %d maps and %d images", K, oh, ow, cap); return VITX_ERR_NOMEM; }
    // the halves go up rounded (RNE) to the operand type; the zero rows beyond K come from operand_matrix_host, the zero biases from the memset
    for (int h = 0; h < 2 && e == hipSuccess; ++h) {
        if (h && !Wc) break;
        const std::vector<uint16_t> hw = operand_matrix_host(c->dtype, h ? Wc : Wp, nullptr, K, Dc, Kpad, Dc, 0, 0);
        e = hipMemcpy(h ? c->dp_Wc : c->dp_Wp, hw.data(), hw.size() * 2, hipMemcpyHostToDevice);
    }
    for (float *p : {c->dp_bias, c->dp_zero, c->dp_bins}) if (e == hipSuccess) e = hipMemset(p, 0, (size_t)Kpad * 4);
    if (e == hipSuccess && bias) e = hipMemcpy(c->dp_bias, bias, (size_t)K * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->dp_bins, bins, (size_t)K * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { c->depth_free(); set_error("vitx_depth_set: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
    c->dp_bias_host.assign(K, 0.0f);
    if (bias) std::copy(bias, bias + K, c->dp_bias_host.begin());
    c->dp_K = K; c->dp_Kpad = Kpad; c->dp_Dc = Dc; c->dp_mask = mask; c->dp_u = upsample; c->dp_oh = oh; c->dp_ow = ow; c->dp_lo = min_depth; c->dp_hi = max_depth;
    c->dp_flags = flags; c->dp_cap = cap; c->dp_scratch = scratch;
    return VITX_OK;
}
int vitx_depth_bins(const vitx_ctx *c) { return c ? c->dp_K : 0; }
int vitx_depth_shape(const vitx_ctx *c, int *out_h, int *out_w, int *fine_h, int *fine_w) {
    if (!c) return VITX_ERR_ARG;
    if (out_h) *out_h = c->dp_oh;
    if (out_w) *out_w = c->dp_ow;
    if (fine_h) *fine_h = c->dp_u * c->gh;
    if (fine_w) *fine_w = c->dp_u * c->gw;
    return VITX_OK;
}
int vitx_depth_images(const vitx_ctx *c) { return c ? c->dp_n : 0; }
const void *vitx_depth_device(const vitx_ctx *c) { return c ? c->dp_depth : nullptr; }
size_t vitx_depth_scratch_bytes(const vitx_ctx *c) { return c ? c->dp_scratch : 0; }
int vitx_depth_read(vitx_ctx *c, float *depth, float *fine, float *logits, float *offsets) {
    if (!c || !depth) return VITX_ERR_ARG;
    const int n = c->depth_on() ? c->dp_n : 0, K = c->dp_K;
    if (n == 0) { set_error("vitx_depth_read: no forward has run with a depth head set since vitx_depth_set"); return VITX_ERR_ARG; }
    if (fine && !(c->dp_flags & VITX_DEPTH_FINE)) { set_error("vitx_depth_read: the head was set without VITX_DEPTH_FINE"); return VITX_ERR_ARG; }
    if ((logits || offsets) && !c->dp_logits) { set_error("vitx_depth_read: the head was set without VITX_DEPTH_LOGITS"); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(depth, c->dp_depth, (size_t)n * c->dp_oh * c->dp_ow * 4, hipMemcpyDeviceToHost));
    if (fine) HIP_TRY(hipMemcpy(fine, c->dp_fine, (size_t)n * c->dp_u * c->gh * c->dp_u * c->gw * 4, hipMemcpyDeviceToHost));
    if (logits) HIP_TRY(hipMemcpy(logits, c->dp_logits, (size_t)n * c->gh * c->gw * K * 4, hipMemcpyDeviceToHost));
    if (offsets && c->dp_off) HIP_TRY(hipMemcpy(offsets, c->dp_off, (size_t)n * K * 4, hipMemcpyDeviceToHost));
    if (offsets && !c->dp_off) for (int i = 0; i < n; ++i) std::copy(c->dp_bias_host.begin(), c->dp_bias_host.end(), offsets + (size_t)i * K);
    return VITX_OK;
}

}  // extern "C"
