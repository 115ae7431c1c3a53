// outputs.cpp -- what a context gives besides probabilities: the per-kernel profile, the residual-stream trace, attention maps, features,
// the zero-shot bank, the gallery, the dense and the depth head (their state: heads.h), and the diagnostics counters.  All opt-in; the forward
// (forward.cpp) launches nothing for an output that is off.
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

// How every vitx_*_enable / vitx_*_set goes: its argument checks (before the first device call: a refused call leaves the output that was set in
// place); quiesce(); the old object dropped, so that its buffers are free before the new ones are asked for; the new object built in a local, and
// moved into the context only when every allocation and upload succeeded -- any earlier return frees the local and leaves the output off.
// quiesce: the context's device is current and no forward in flight reads or writes the buffers about to be freed
static int quiesce(vitx_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    return VITX_OK;
}
static int hip_failed(const char *api, hipError_t e) {
    set_error("%s: %s", api, hipGetErrorString(e));
    return VITX_ERR_HIP;
}

// What vitx_dense_set and vitx_depth_set (`api`) share beyond the checks of the head itself (heads.h: patch_head_mask and its kin).  The argument
// checks come in two pieces because each head's own checks sit between them:
// patch_head_shape: the output shape (0 x 0: the context's image shape)
static int patch_head_shape(const vitx_ctx *c, const char *api, int *oh, int *ow) {
    if (*oh < 0 || *ow < 0 || ((*oh == 0) != (*ow == 0))) { set_error("%s: output shape %d x %d (0 x 0: the context's image shape)", api, *oh, *ow); return VITX_ERR_ARG; }
    if (*oh == 0) { *oh = c->Sh; *ow = c->Sw; }
    return VITX_OK;
}
// patch_head_window: the operand and logit rows of a pass lie inside the 32-bit byte window the GEMM addresses
static int patch_head_window(const vitx_ctx *c, const char *api, int K, int Dc) {
    const size_t rows = (size_t)c->pass_cap() * c->gh * c->gw;
    if (rows * Dc * 2 > 0xf0000000u || rows * round_up(K, c->tn) * 4 > 0xf0000000u || c->pass_cap() > 65535) {
        set_error("%s: the operand or logit rows of a pass of %d images leave the GEMM's 32-bit byte window", api, c->pass_cap());
        return VITX_ERR_UNSUPPORTED;
    }
    return VITX_OK;
}
static void patch_head_init(const vitx_ctx *c, PatchHead *h, int K, int Dc, uint64_t mask, int oh, int ow, int flags) {
    h->K = K; h->Kpad = round_up(K, c->tn); h->Dc = Dc; h->mask = mask; h->oh = oh; h->ow = ow; h->flags = flags; h->cap = c->pass_cap();
    h->last_all_rows = (mask >> (c->L - 1)) & 1;       // a selected last layer needs every row of it (as VITX_FEAT_TOKENS of the last layer does)
}
// patch_head_scratch: the per-slice operand rows -- zero-filled once: a forward writes the real rows of its batch and zeroes the pad rows behind
// them -- and patch logits, counted into h->scratch.  false: the device has no room; *e: the zero fill failed
static bool patch_head_scratch(const vitx_ctx *c, PatchHead *h, hipError_t *e) {
    h->a.resize(c->nslices); h->acc.resize(c->nslices);
    for (int i = 0; i < c->nslices && *e == hipSuccess; ++i) {
        const size_t rows = (size_t)round_up(std::min(c->slices[i].cap, h->cap) * c->gh * c->gw, c->tm);
        if (!h->a[i].alloc(rows * h->Dc * 2) || !h->acc[i].alloc(rows * h->Kpad * 4)) return false;
        *e = hipMemset(h->a[i].p, 0, rows * h->Dc * 2);
        h->scratch += rows * h->Dc * 2 + rows * h->Kpad * 4;
    }
    return true;
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
    if (const int rc = quiesce(c)) return rc;
    c->attn.reset();
    if (!on) return VITX_OK;
    auto am = std::make_unique<AttnMaps>();
    const size_t cap = c->pass_cap(), N = c->N, H = c->H;
    am->mask = layer_mask; am->flags = flags; am->cap = (int)cap;
    am->fpi = layer_slot(layer_mask, c->L) * c->H * c->N + (rollout ? c->N : 0);
    bool ok = am->out.alloc(cap * am->fpi * 4);
    if (ok && rollout) ok = am->roll[0].alloc(cap * N * N * 4) && am->roll[1].alloc(cap * N * N * 4);
    if (ok && rollout && !((layer_mask >> (c->L - 1)) & 1)) ok = am->cls_last.alloc(cap * H * N * 4);
    if (!ok) { set_error("vitx_attn_enable: cannot allocate the map buffers for %d images", am->cap); return VITX_ERR_NOMEM; }
    c->attn = std::move(am);
    return VITX_OK;
}
int vitx_attn_floats(const vitx_ctx *c) { return c && c->attn ? c->attn->fpi : 0; }
int vitx_attn_images(const vitx_ctx *c) { return c && c->attn ? c->attn->n : 0; }
int vitx_attn_read(vitx_ctx *c, float *out, size_t n_floats) {
    if (!c) return VITX_ERR_ARG;
    const AttnMaps *a = c->attn.get();
    return read_output(c, "vitx_attn", "attention maps", a ? a->n : 0, a ? a->fpi : 0, a ? a->out.as<float>() : nullptr, out, n_floats);
}

int vitx_feat_enable(vitx_ctx *c, int flags, uint64_t layer_mask) {
    if (!c) return VITX_ERR_ARG;
    constexpr int kinds = VITX_FEAT_CLS | VITX_FEAT_MEAN | VITX_FEAT_TOKENS;
    if (flags & ~(kinds | VITX_FEAT_L2)) { set_error("vitx_feat_enable: unknown flags 0x%x", flags); return VITX_ERR_ARG; }
    if (flags && !(flags & kinds)) { set_error("vitx_feat_enable: VITX_FEAT_L2 modifies VITX_FEAT_CLS / VITX_FEAT_MEAN and selects nothing on its own"); return VITX_ERR_ARG; }
    if (c->L < 64 && (layer_mask >> c->L)) { set_error("vitx_feat_enable: layer mask 0x%llx names layers beyond the model's %d", (unsigned long long)layer_mask, c->L); return VITX_ERR_ARG; }
    if (flags && c->R != 1) { set_error("vitx_feat_enable: features are not available for ViTSTR contexts"); return VITX_ERR_UNSUPPORTED; }
    if (const int rc = quiesce(c)) return rc;
    c->feat.reset();
    if (!flags) return VITX_OK;
    if (!layer_mask) layer_mask = 1ull << (c->L - 1);
    if (c->map && (flags & VITX_FEAT_CLS) && layer_mask != 1ull << (c->L - 1)) {      // the one refusal that comes after the free: the features are off now
        set_error("vitx_feat_enable: VITX_FEAT_CLS of a model with the attention-pooling head is the pooled embedding: it exists for the last layer only (mask 0x%llx)", (unsigned long long)layer_mask);
        return VITX_ERR_ARG;
    }
    auto ft = std::make_unique<Features>(flags, layer_mask, c->D, c->N - c->Tp, c->L);
    ft->cap = c->pass_cap();
    const size_t fpi = (size_t)layer_slot(layer_mask, c->L) * ft->layer_floats();
    if (fpi > 0x7fffffff || !ft->out.alloc((size_t)ft->cap * fpi * 4)) {
        set_error("vitx_feat_enable: cannot allocate the feature buffer for %d images of %zu floats", ft->cap, fpi);
        return VITX_ERR_NOMEM;
    }
    ft->fpi = (int)fpi;
    c->feat = std::move(ft);
    return VITX_OK;
}
int vitx_feat_floats(const vitx_ctx *c) { return c && c->feat ? c->feat->fpi : 0; }
int vitx_feat_images(const vitx_ctx *c) { return c && c->feat ? c->feat->n : 0; }
const void *vitx_feat_device(const vitx_ctx *c) { return c && c->feat ? c->feat->out.p : nullptr; }
int vitx_feat_read(vitx_ctx *c, float *out, size_t n_floats) {
    if (!c) return VITX_ERR_ARG;
    const Features *f = c->feat.get();
    return read_output(c, "vitx_feat", "features", f ? f->n : 0, f ? f->fpi : 0, f ? f->out.as<float>() : nullptr, out, n_floats);
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
    if (const int rc = quiesce(c)) return rc;
    c->zs.reset();
    if (off) return VITX_OK;
    auto zs = std::make_unique<ZeroShot>();
    zs->K = K; zs->Kpad = round_up(K, c->tn); zs->E = E; zs->kind = kind; zs->scale = scale; zs->bias = bias; zs->cap = c->pass_cap();
    const size_t Kpad = zs->Kpad, rows = (size_t)round_up(zs->cap, c->tm);
    const std::vector<uint16_t> hb = operand_matrix_host(c->dtype, bank, nullptr, K, E, zs->Kpad, E, 0, 0);
    bool ok = zs->bank.alloc(hb.size() * 2) && zs->zero.alloc(Kpad * 4) && zs->out.alloc((size_t)zs->cap * 2 * K * 4);
    zs->a.resize(c->nslices); zs->acc.resize(c->nslices);
    for (int i = 0; ok && i < c->nslices; ++i) ok = zs->a[i].alloc(rows * E * 2) && zs->acc[i].alloc(rows * Kpad * 4);
    if (!ok) { set_error("vitx_zeroshot_set: cannot allocate the buffers for %d classes and %d images", K, zs->cap); return VITX_ERR_NOMEM; }
    hipError_t e = hipMemcpy(zs->bank.p, hb.data(), hb.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(zs->zero.p, 0, Kpad * 4);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_failed("vitx_zeroshot_set", e);
    c->zs = std::move(zs);
    return VITX_OK;
}
int vitx_zeroshot_classes(const vitx_ctx *c) { return c && c->zs ? c->zs->K : 0; }
int vitx_zeroshot_images(const vitx_ctx *c) { return c && c->zs ? c->zs->n : 0; }
const void *vitx_zeroshot_device(const vitx_ctx *c) { return c && c->zs ? c->zs->out.p : nullptr; }
int vitx_zeroshot_read(vitx_ctx *c, float *probs, float *logits, size_t n_floats_each) {
    if (!c || !probs) return VITX_ERR_ARG;
    const ZeroShot *zs = c->zs.get();
    const int n = zs ? zs->n : 0;
    if (n == 0) { set_error("vitx_zeroshot_read: no forward has run with a bank set since vitx_zeroshot_set"); return VITX_ERR_ARG; }
    const int K = zs->K;
    const size_t need = (size_t)n * K;
    if (n_floats_each < need) { set_error("vitx_zeroshot_read: buffer too small (%zu floats needed for %d images of %d classes)", need, n, K); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy2D(probs, (size_t)K * 4, zs->out.p, (size_t)2 * K * 4, (size_t)K * 4, n, hipMemcpyDeviceToHost));
    if (logits) HIP_TRY(hipMemcpy2D(logits, (size_t)K * 4, zs->out.as<float>() + K, (size_t)2 * K * 4, (size_t)K * 4, n, hipMemcpyDeviceToHost));
    return VITX_OK;
}

// Nearest neighbours: the gallery of a context (include/vitx.h).  Every argument check comes before the first device call.
int vitx_nn_width(const vitx_ctx *c, int source) { return c ? c->nn_width(source) : 0; }
int vitx_nn_set(vitx_ctx *c, const float *gallery, long G, int E, int k, int source, const int32_t *labels, int n_labels, float temperature) {
    if (!c) return VITX_ERR_ARG;
    constexpr int Gc = Gallery::kChunk;
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
        if ((size_t)round_up(c->pass_cap(), c->tm) * Gc * 4 > 0xf0000000u) {       // the chunk GEMM addresses its output inside a 32-bit byte window
            set_error("vitx_nn_set: the score scratch of %d images exceeds the chunk GEMM's 32-bit window (at most %d images per pass)", c->pass_cap(), (int)(0xf0000000u / 4 / Gc / c->tm * c->tm));
            return VITX_ERR_UNSUPPORTED;
        }
        for (size_t i = 0, nb = (size_t)G * E; i < nb; ++i)
            if (!std::isfinite(gallery[i])) { set_error("vitx_nn_set: gallery entry [%zu][%zu] is not finite", i / E, i % E); return VITX_ERR_ARG; }
        if (labels) for (long g = 0; g < G; ++g)
            if (labels[g] < 0 || labels[g] >= n_labels) { set_error("vitx_nn_set: label %d of gallery row %ld outside 0 .. %d", labels[g], g, n_labels - 1); return VITX_ERR_ARG; }
    }
    if (const int rc = quiesce(c)) return rc;
    c->nn.reset();
    if (off) return VITX_OK;
    auto nn = std::make_unique<Gallery>();
    nn->G = G; nn->Gpad = (G + c->tn - 1) / c->tn * c->tn; nn->k = k; nn->source = source; nn->E = E; nn->cap = c->pass_cap();
    nn->nlabels = labels ? n_labels : 0; nn->T = labels ? temperature : 0.0f;
    const size_t gallery_bytes = (size_t)nn->Gpad * E * 2, rows = (size_t)round_up(nn->cap, c->tm), state_bytes = nn_state_bytes((int)rows, k);
    bool ok = nn->gallery.alloc(gallery_bytes) && nn->zero.alloc((size_t)Gc * 4) && nn->out.alloc((size_t)nn->cap * k * 8);
    if (ok && labels) ok = nn->labels.alloc((size_t)G * 4) && nn->vote.alloc((size_t)nn->cap * n_labels * 4);
    nn->a.resize(c->nslices); nn->acc.resize(c->nslices); nn->state.resize(c->nslices);
    for (int i = 0; ok && i < c->nslices; ++i) ok = nn->a[i].alloc(rows * E * 2) && nn->acc[i].alloc(rows * Gc * 4) && nn->state[i].alloc(state_bytes);
    if (!ok) { set_error("vitx_nn_set: cannot allocate the buffers for %ld gallery rows and %d images", G, nn->cap); return VITX_ERR_NOMEM; }
    nn->scratch = (size_t)c->nslices * (rows * Gc * 4 + state_bytes);
    // the gallery goes up in blocks of rows, rounded (RNE) to the operand type; the zero rows beyond G come from the memset
    hipError_t e = hipMemset(nn->gallery.p, 0, gallery_bytes);
    if (e == hipSuccess) e = hipMemset(nn->zero.p, 0, (size_t)Gc * 4);
    for (long g0 = 0; g0 < G && e == hipSuccess; g0 += 65536) {
        const int nr = (int)std::min<long>(65536, G - g0);
        const std::vector<uint16_t> hb = operand_matrix_host(c->dtype, gallery + (size_t)g0 * E, nullptr, nr, E, nr, E, 0, 0);
        e = hipMemcpy(nn->gallery.as<char>() + (size_t)g0 * E * 2, hb.data(), hb.size() * 2, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && labels) e = hipMemcpy(nn->labels.p, labels, (size_t)G * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_failed("vitx_nn_set", e);
    c->nn = std::move(nn);
    return VITX_OK;
}
long vitx_nn_rows(const vitx_ctx *c) { return c && c->nn ? c->nn->G : 0; }
int vitx_nn_k(const vitx_ctx *c) { return c && c->nn ? c->nn->k : 0; }
int vitx_nn_labels(const vitx_ctx *c) { return c && c->nn ? c->nn->nlabels : 0; }
int vitx_nn_images(const vitx_ctx *c) { return c && c->nn ? c->nn->n : 0; }
const void *vitx_nn_device(const vitx_ctx *c) { return c && c->nn ? c->nn->out.p : nullptr; }
size_t vitx_nn_scratch_bytes(const vitx_ctx *c) { return c && c->nn ? c->nn->scratch : 0; }
int vitx_nn_read(vitx_ctx *c, int32_t *idx, float *score, float *vote) {
    if (!c || !idx || !score) return VITX_ERR_ARG;
    const Gallery *nn = c->nn.get();
    const int n = nn ? nn->n : 0;
    if (n == 0) { set_error("vitx_nn_read: no forward has run with a gallery set since vitx_nn_set"); return VITX_ERR_ARG; }
    if (vote && !nn->nlabels) { set_error("vitx_nn_read: the gallery has no labels: there is no vote"); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy2D(score, 4, nn->out.p, 8, 4, (size_t)n * nn->k, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy2D(idx, 4, nn->out.as<float>() + 1, 8, 4, (size_t)n * nn->k, hipMemcpyDeviceToHost));
    if (vote) HIP_TRY(hipMemcpy(vote, nn->vote.p, (size_t)n * nn->nlabels * 4, hipMemcpyDeviceToHost));
    return VITX_OK;
}

// The dense head of a context (include/vitx.h "dense prediction").  Every argument check comes before the first device call.
int vitx_dense_set(vitx_ctx *c, const float *W, const float *bias, int K, int Dc, uint64_t layer_mask, int out_h, int out_w, int flags) {
    if (!c) return VITX_ERR_ARG;
    const bool off = !W && K == 0;
    uint64_t mask = layer_mask;
    int oh = out_h, ow = out_w;
    if (!off) {
        if (const int rc = dense_head_args("vitx_dense_set", W, K, Dc, flags, c->L, c->D, &mask)) return rc;
        if (const int rc = patch_head_shape(c, "vitx_dense_set", &oh, &ow)) return rc;
        if (const int rc = dense_head_values("vitx_dense_set", W, bias, K, Dc)) return rc;
        if (c->R != 1) { set_error("vitx_dense_set: the dense head is not available for ViTSTR contexts"); return VITX_ERR_UNSUPPORTED; }
        if (oh < c->gh || ow < c->gw || oh > kDenseMaxOut || ow > kDenseMaxOut) {
            set_error("vitx_dense_set: output %d x %d outside the patch grid %d x %d .. %d (upsampling only)", oh, ow, c->gh, c->gw, kDenseMaxOut);
            return VITX_ERR_UNSUPPORTED;
        }
        if (const int rc = patch_head_window(c, "vitx_dense_set", K, Dc)) return rc;
    }
    if (const int rc = quiesce(c)) return rc;
    c->dense.reset();
    if (off) return VITX_OK;
    auto dn = std::make_unique<DenseHead>();
    patch_head_init(c, dn.get(), K, Dc, mask, oh, ow, flags);
    const size_t Kpad = dn->Kpad, cap = dn->cap, px = (size_t)oh * ow, Np = (size_t)c->gh * c->gw;
    bool ok = dn->W.alloc(Kpad * Dc * 2) && dn->bias.alloc(Kpad * 4) && dn->labels.alloc(cap * px);
    if (ok && (flags & VITX_DENSE_SCORE)) ok = dn->score.alloc(cap * px * 4);
    if (ok && (flags & VITX_DENSE_LOGITS)) ok = dn->logits.alloc(cap * Np * K * 4);
    hipError_t e = hipSuccess;
    if (!ok || !patch_head_scratch(c, dn.get(), &e)) { set_error("vitx_dense_set: cannot allocate the buffers for %d classes, %d x %d labels and %d images", K, oh, ow, dn->cap); return VITX_ERR_NOMEM; }
    // the head goes up rounded (RNE) to the operand type; the zero rows beyond K come from operand_matrix_host, the zero biases from the memset
    if (e == hipSuccess) e = dense_head_upload(*dn, c->dtype, W, bias);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_failed("vitx_dense_set", e);
    c->dense = std::move(dn);
    return VITX_OK;
}
int vitx_dense_classes(const vitx_ctx *c) { return c && c->dense ? c->dense->K : 0; }
int vitx_dense_shape(const vitx_ctx *c, int *out_h, int *out_w) {
    if (!c) return VITX_ERR_ARG;
    if (out_h) *out_h = c->dense ? c->dense->oh : 0;
    if (out_w) *out_w = c->dense ? c->dense->ow : 0;
    return VITX_OK;
}
int vitx_dense_images(const vitx_ctx *c) { return c && c->dense ? c->dense->n : 0; }
const void *vitx_dense_device(const vitx_ctx *c) { return c && c->dense ? c->dense->labels.p : nullptr; }
size_t vitx_dense_scratch_bytes(const vitx_ctx *c) { return c && c->dense ? c->dense->scratch : 0; }
int vitx_dense_read(vitx_ctx *c, uint8_t *labels, float *score, float *logits) {
    if (!c || !labels) return VITX_ERR_ARG;
    const DenseHead *dn = c->dense.get();
    const int n = dn ? dn->n : 0;
    if (n == 0) { set_error("vitx_dense_read: no forward has run with a dense head set since vitx_dense_set"); return VITX_ERR_ARG; }
    if (score && !dn->score) { set_error("vitx_dense_read: the head was set without VITX_DENSE_SCORE"); return VITX_ERR_ARG; }
    if (logits && !dn->logits) { set_error("vitx_dense_read: the head was set without VITX_DENSE_LOGITS"); return VITX_ERR_ARG; }
    const size_t px = (size_t)dn->oh * dn->ow;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(labels, dn->labels.p, (size_t)n * px, hipMemcpyDeviceToHost));
    if (score) HIP_TRY(hipMemcpy(score, dn->score.p, (size_t)n * px * 4, hipMemcpyDeviceToHost));
    if (logits) HIP_TRY(hipMemcpy(logits, dn->logits.p, (size_t)n * c->gh * c->gw * dn->K * 4, hipMemcpyDeviceToHost));
    return VITX_OK;
}

// The depth head of a context (include/vitx.h "depth estimation").  Every argument check comes before the first device call.
int vitx_depth_set(vitx_ctx *c, const float *Wp, const float *Wc, const float *bias, const float *bins, int K, int Dc, uint64_t layer_mask, int upsample,
                   float min_depth, float max_depth, int out_h, int out_w, int flags) {
    if (!c) return VITX_ERR_ARG;
    const bool off = !Wp && K == 0;
    uint64_t mask = layer_mask;
    int oh = out_h, ow = out_w;
    const int fh = upsample * c->gh, fw = upsample * c->gw;
    if (!off) {
        if (const int rc = depth_head_args("vitx_depth_set", Wp, bins, K, Dc, flags, c->L, c->D, &mask)) return rc;
        if (const int rc = patch_head_shape(c, "vitx_depth_set", &oh, &ow)) return rc;
        if (const int rc = depth_head_values("vitx_depth_set", Wp, Wc, bias, bins, K, Dc, min_depth, max_depth, upsample)) return rc;
        if (c->R != 1) { set_error("vitx_depth_set: the depth head is not available for ViTSTR contexts"); return VITX_ERR_UNSUPPORTED; }
        if (Wc && c->map) { set_error("vitx_depth_set: a class half on a context without a class token (VITX_POOL_MAP)"); return VITX_ERR_UNSUPPORTED; }
        if (oh < fh || ow < fw || oh > kDepthMaxOut || ow > kDepthMaxOut) {
            set_error("vitx_depth_set: output %d x %d outside the fine plane %d x %d .. %d (upsampling only)", oh, ow, fh, fw, kDepthMaxOut);
            return VITX_ERR_UNSUPPORTED;
        }
        if (const int rc = patch_head_window(c, "vitx_depth_set", K, Dc)) return rc;
    }
    if (const int rc = quiesce(c)) return rc;
    c->depth.reset();
    if (off) return VITX_OK;
    auto dp = std::make_unique<DepthHead>();
    patch_head_init(c, dp.get(), K, Dc, mask, oh, ow, flags);
    dp->u = upsample; dp->lo = min_depth; dp->hi = max_depth;
    dp->bias_host.assign(K, 0.0f);
    if (bias) std::copy(bias, bias + K, dp->bias_host.begin());
    const size_t Kpad = dp->Kpad, cap = dp->cap, px = (size_t)oh * ow, fpx = (size_t)fh * fw, Np = (size_t)c->gh * c->gw;
    bool ok = dp->Wp.alloc(Kpad * Dc * 2) && (!Wc || dp->Wc.alloc(Kpad * Dc * 2)) && dp->bias.alloc(Kpad * 4) && dp->zero.alloc(Kpad * 4) && dp->bins.alloc(Kpad * 4) &&
              dp->depth.alloc(cap * px * 4) && dp->fine.alloc(cap * fpx * 4);
    if (ok && (flags & VITX_DEPTH_LOGITS)) ok = dp->logits.alloc(cap * Np * K * 4) && (!Wc || dp->off.alloc(cap * K * 4));
    hipError_t e = hipSuccess;
    ok = ok && patch_head_scratch(c, dp.get(), &e);
    if (Wc) {        // the class rows and the offsets, per slice: zero-filled once like the patch rows
        dp->ac.resize(c->nslices); dp->o.resize(c->nslices);
        for (int i = 0; ok && e == hipSuccess && i < c->nslices; ++i) {
            const size_t crows = (size_t)round_up(std::min(c->slices[i].cap, dp->cap), c->tm);
            ok = dp->ac[i].alloc(crows * Dc * 2) && dp->o[i].alloc(crows * Kpad * 4);
            if (ok) e = hipMemset(dp->ac[i].p, 0, crows * Dc * 2);
            dp->scratch += crows * Dc * 2 + crows * Kpad * 4;
        }
    }
    if (!ok) { set_error("vitx_depth_set: cannot allocate the buffers for %d bins, %d x %d maps and %d images", K, oh, ow, dp->cap); return VITX_ERR_NOMEM; }
    if (e == hipSuccess) e = depth_head_upload(*dp, c->dtype, Wp, Wc, bias, bins);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_failed("vitx_depth_set", e);
    c->depth = std::move(dp);
    return VITX_OK;
}
int vitx_depth_bins(const vitx_ctx *c) { return c && c->depth ? c->depth->K : 0; }
int vitx_depth_shape(const vitx_ctx *c, int *out_h, int *out_w, int *fine_h, int *fine_w) {
    if (!c) return VITX_ERR_ARG;
    const DepthHead *dp = c->depth.get();
    if (out_h) *out_h = dp ? dp->oh : 0;
    if (out_w) *out_w = dp ? dp->ow : 0;
    if (fine_h) *fine_h = dp ? dp->u * c->gh : 0;
    if (fine_w) *fine_w = dp ? dp->u * c->gw : 0;
    return VITX_OK;
}
int vitx_depth_images(const vitx_ctx *c) { return c && c->depth ? c->depth->n : 0; }
const void *vitx_depth_device(const vitx_ctx *c) { return c && c->depth ? c->depth->depth.p : nullptr; }
size_t vitx_depth_scratch_bytes(const vitx_ctx *c) { return c && c->depth ? c->depth->scratch : 0; }
int vitx_depth_read(vitx_ctx *c, float *depth, float *fine, float *logits, float *offsets) {
    if (!c || !depth) return VITX_ERR_ARG;
    const DepthHead *dp = c->depth.get();
    const int n = dp ? dp->n : 0;
    if (n == 0) { set_error("vitx_depth_read: no forward has run with a depth head set since vitx_depth_set"); return VITX_ERR_ARG; }
    if (fine && !(dp->flags & VITX_DEPTH_FINE)) { set_error("vitx_depth_read: the head was set without VITX_DEPTH_FINE"); return VITX_ERR_ARG; }
    if ((logits || offsets) && !dp->logits) { set_error("vitx_depth_read: the head was set without VITX_DEPTH_LOGITS"); return VITX_ERR_ARG; }
    const int K = dp->K;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(depth, dp->depth.p, (size_t)n * dp->oh * dp->ow * 4, hipMemcpyDeviceToHost));
    if (fine) HIP_TRY(hipMemcpy(fine, dp->fine.p, (size_t)n * dp->u * c->gh * dp->u * c->gw * 4, hipMemcpyDeviceToHost));
    if (logits) HIP_TRY(hipMemcpy(logits, dp->logits.p, (size_t)n * c->gh * c->gw * K * 4, hipMemcpyDeviceToHost));
    if (offsets && dp->off) HIP_TRY(hipMemcpy(offsets, dp->off.p, (size_t)n * K * 4, hipMemcpyDeviceToHost));
    if (offsets && !dp->off) for (int i = 0; i < n; ++i) std::copy(dp->bias_host.begin(), dp->bias_host.end(), offsets + (size_t)i * K);
    return VITX_OK;
}

}  // extern "C"

