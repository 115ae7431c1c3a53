// vit_api.cpp -- the reference's C++ entry points on top of the C ABI (see ../vit.h).
#include "../vit.h"

#include <stdio.h>
#include <stdlib.h>

vit_model::~vit_model() { vitx_model_free(handle); }
vit_state::~vit_state() { vitx_ctx_free(ctx); vitx_pack_free(pack); }
vit_text_state::~vit_text_state() { vitx_text_free(ctx); }

// vit.cpp:109-127 -- false + message on stderr when the file cannot be read or decoded
bool load_image_from_file(const std::string &fname, image_u8 &img) {
    uint8_t *data = nullptr; int nx = 0, ny = 0;
    if (vitx_image_load(fname.c_str(), &data, &nx, &ny) != VITX_OK) {
        fprintf(stderr, "%s: failed to load '%s'\n", __func__, fname.c_str());
        return false;
    }
    img.nx = nx; img.ny = ny;
    img.data.assign(data, data + (size_t)nx * ny * 3);
    vitx_image_free(data);
    return true;
}

// vit.cpp:308-712 -- false + message on stderr for any error
bool vit_model_load(const std::string &fname, vit_model &model) {
    printf("%s: loading model from '%s' - please wait\n", __func__, fname.c_str());
    vitx_model *h = nullptr;
    const int rc = vitx_model_load(fname.c_str(), &h);
    if (rc != VITX_OK) { fprintf(stderr, "%s: %s\n", __func__, vitx_last_error()); return false; }
    vitx_model_free(model.handle);
    model.handle = h;
    vitx_hparams hp;
    vitx_model_hparams(h, &hp);
    vit_hparams &o = model.hparams;
    o.hidden_size = hp.hidden_size; o.num_hidden_layers = hp.num_hidden_layers; o.num_attention_heads = hp.num_attention_heads;
    o.num_classes = hp.num_classes; o.patch_size = hp.patch_size; o.img_size = hp.img_size; o.ftype = hp.ftype; o.eps = hp.eps;
    o.id2label.clear();
    for (int i = 0; i < hp.num_classes; ++i) { const char *l = vitx_model_label(h, i); if (l) o.id2label[i] = l; }
    printf("%s: hidden_size            = %d\n", __func__, o.hidden_size);
    printf("%s: num_hidden_layers      = %d\n", __func__, o.num_hidden_layers);
    printf("%s: num_attention_heads    = %d\n", __func__, o.num_attention_heads);
    printf("%s: patch_size             = %d\n", __func__, o.patch_size);
    printf("%s: img_size               = %d\n", __func__, o.img_size);
    printf("%s: num_classes            = %d\n", __func__, o.num_classes);
    printf("%s: ftype                  = %d\n", __func__, o.ftype);
    return true;
}

// vit.cpp:289-305 -- false only for an unknown interpolation mode
bool vit_image_preprocess(const image_u8 &img, image_f32 &res, const vit_hparams &params) {
    int interp;
    if (params.interpolation == "bilinear") interp = VITX_BILINEAR;
    else if (params.interpolation == "bicubic") interp = VITX_BICUBIC;
    else { printf("Interpolation mode '%s' is not supported; returning 'false'...", params.interpolation.c_str()); return false; }
    const int S = params.n_img_size();
    res.nx = S; res.ny = S;
    res.data.resize((size_t)3 * S * S);
    return vitx_preprocess_u8(img.data.data(), img.nx, img.ny, S, interp, res.data.data()) == VITX_OK;
}

// No counterpart in the reference: the file's own preprocessing (vitx_model_preproc), at the file's size or at another one
bool vit_image_preprocess_model(const image_u8 &img, image_f32 &res, const vit_model &model, int img_size) {
    vitx_preproc pp;
    if (!model.handle || vitx_model_preproc(model.handle, &pp) != VITX_OK) { fprintf(stderr, "%s: no model is loaded\n", __func__); return false; }
    if (img_size > 0 && img_size != model.hparams.img_size && vitx_preproc_at_size(&pp, img_size, &pp) != VITX_OK) { fprintf(stderr, "%s: %s\n", __func__, vitx_last_error()); return false; }
    const int S = pp.crop ? pp.crop : pp.resize_a;
    res.nx = S; res.ny = S;
    res.data.resize((size_t)3 * S * S);
    if (vitx_preprocess_ex(&pp, img.data.data(), img.nx, img.ny, res.data.data()) != VITX_OK) { fprintf(stderr, "%s: %s\n", __func__, vitx_last_error()); return false; }
    return true;
}

// No counterpart in the reference: the whole image stretched to w x h for a rectangular state (vitx_preprocess_rect)
bool vit_image_preprocess_rect(const image_u8 &img, image_f32 &res, const vit_model &model, int w, int h) {
    vitx_preproc pp;
    if (!model.handle || vitx_model_preproc(model.handle, &pp) != VITX_OK) { fprintf(stderr, "%s: no model is loaded\n", __func__); return false; }
    if (pp.filter != VITX_PP_PIL_BILINEAR && pp.filter != VITX_PP_PIL_BICUBIC) pp.filter = VITX_PP_PIL_BICUBIC;
    if (w <= 0 || h <= 0) { fprintf(stderr, "%s: the shape %d x %d is not positive\n", __func__, w, h); return false; }
    res.nx = w; res.ny = h;
    res.data.resize((size_t)3 * w * h);
    if (vitx_preprocess_rect(&pp, img.data.data(), img.nx, img.ny, w, h, res.data.data()) != VITX_OK) { fprintf(stderr, "%s: %s\n", __func__, vitx_last_error()); return false; }
    return true;
}

// The reference's vit_state carries no weights and can be reused with any model; ours caches a context that does, so the cache
// is keyed on the unique id of the parsed model it was built from (vit_model_load frees and replaces that handle on every call),
// and on everything else of the state the context was created from: geometry, pos_interp, device and dtype.
// The input side a state's context takes: vit_state::img_size, or the file's when that is 0
static int state_img_size(const vit_model &model, const vit_state &state) { return state.img_size > 0 ? state.img_size : model.hparams.img_size; }

// ... and the shape: img_h x img_w of a rectangular state, the square of state_img_size otherwise.  false (and a message): img_h / img_w half set, or set beside img_size
static bool state_shape(const vit_model &model, const vit_state &state, int &h, int &w, const char *who) {
    const bool rect = state.img_h != 0 || state.img_w != 0;
    if (rect && (state.img_h <= 0 || state.img_w <= 0 || state.img_size != 0)) {
        fprintf(stderr, "%s: vit_state::img_h and img_w are set together, with img_size == 0 (img_h %d, img_w %d, img_size %d)\n", who, state.img_h, state.img_w, state.img_size);
        return false;
    }
    h = rect ? state.img_h : state_img_size(model, state);
    w = rect ? state.img_w : h;
    return true;
}
// n images of the state's shape?  -1 or the index of the first that is not
static int first_bad_image(const image_f32 *imgs, int n, int h, int w) {
    for (int i = 0; i < n; ++i) if (imgs[i].nx != w || imgs[i].ny != h || imgs[i].data.size() != (size_t)3 * h * w) return i;
    return -1;
}

static int ensure_ctx(const vit_model &model, vit_state &state, int n) {
    int Sh = 0, Sw = 0, ch = -1, cw = -1;
    if (!state_shape(model, state, Sh, Sw, __func__)) return VITX_ERR_ARG;
    const bool rect = state.img_h != 0;
    if (state.ctx) (void)vitx_ctx_img_shape(state.ctx, &ch, &cw);
    const bool own = Sh == model.hparams.img_size && Sw == model.hparams.img_size;
    const bool same_geometry = state.ctx && ch == Sh && cw == Sw && (own || state.ctx_pos_interp == state.pos_interp);
    if (same_geometry && state.ctx_model_uid == vitx_model_uid(model.handle) && state.ctx_device == state.device && state.ctx_dtype == state.dtype &&
        vitx_ctx_max_batch(state.ctx) >= n) return VITX_OK;
    vitx_ctx_free(state.ctx); state.ctx = nullptr; state.ctx_model_uid = 0;
    state.max_batch = std::max(state.max_batch, n);
    vitx_ctx_options opt{};
    opt.struct_size = (int32_t)sizeof(opt); opt.img_size = state.img_size; opt.pos_interp = state.pos_interp;
    const int rc = rect ? vitx_ctx_create_rect(model.handle, state.device, state.max_batch, state.dtype, &opt, Sh, Sw, &state.ctx)
                        : vitx_ctx_create_ex(model.handle, state.device, state.max_batch, state.dtype, &opt, &state.ctx);
    if (rc == VITX_OK) { state.ctx_model_uid = vitx_model_uid(model.handle); state.ctx_pos_interp = state.pos_interp; state.ctx_device = state.device; state.ctx_dtype = state.dtype; }
    return rc;
}

int vit_predict_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, const vit_params &params,
                      std::vector<std::vector<std::pair<float, int>>> &predictions, bool print) {
    predictions.clear();
    if (!model.handle || !imgs || n <= 0) { fprintf(stderr, "%s: invalid argument\n", __func__); return 1; }
    if (vitx_model_seq_len(model.handle) > 0) { fprintf(stderr, "%s: this is a ViTSTR model (one-channel patch kernel): use vitstr_predict\n", __func__); return 1; }
    const int C = model.hparams.num_classes;
    int Sh = 0, Sw = 0;
    if (!state_shape(model, state, Sh, Sw, __func__)) return 1;
    const size_t img_floats = (size_t)3 * Sh * Sw;
    if (const int i = first_bad_image(imgs, n, Sh, Sw); i >= 0) {                                  // GGML_ASSERT at vit.cpp:757
        fprintf(stderr, "%s: image %d is %dx%d, this state expects %dx%d\n", __func__, i, imgs[i].nx, imgs[i].ny, Sw, Sh);
        abort();
    }
    if (ensure_ctx(model, state, n) != VITX_OK) { fprintf(stderr, "%s: failed to encode image: %s\n", __func__, vitx_last_error()); return 1; }
    std::vector<float> batch;
    const float *src = imgs[0].data.data();
    if (n > 1) {
        batch.resize((size_t)n * img_floats);
        for (int i = 0; i < n; ++i) std::copy(imgs[i].data.begin(), imgs[i].data.end(), batch.begin() + (size_t)i * img_floats);
        src = batch.data();
    }
    state.prediction.resize((size_t)n * C);
    if (vitx_forward(state.ctx, src, n, state.prediction.data(), nullptr) != VITX_OK) {
        fprintf(stderr, "%s: failed to encode image: %s\n", __func__, vitx_last_error());
        return 1;
    }
    predictions.resize(n);
    for (int b = 0; b < n; ++b) {
        auto &p = predictions[b];
        p.reserve(C);
        for (int i = 0; i < C; ++i) p.push_back(std::make_pair(state.prediction[(size_t)b * C + i], i));      // vit.cpp:1047-1050
        std::sort(p.begin(), p.end(), [](const std::pair<float, int> &a, const std::pair<float, int> &b2) { return a.first > b2.first; });   // vit.cpp:1053-1057
        if (print) {
            fprintf(stderr, "\n");
            for (int i = 0; i < params.topk && i < (int)p.size(); ++i)                                        // vit.cpp:1062-1067
                printf(" > %s : %.2f\n", model.hparams.id2label.at(p[i].second).c_str(), p[i].first);
        }
    }
    return 0;
}

// No counterpart in the reference: images of different shapes in one forward of a packed context (include/vitx.h "packed batches")
int vit_pack_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, std::vector<std::vector<std::pair<float, int>>> &predictions) {
    predictions.clear();
    if (!model.handle || !imgs || n <= 0) { fprintf(stderr, "%s: invalid argument\n", __func__); return 1; }
    std::vector<int32_t> shapes((size_t)2 * n), row0((size_t)n + 1);
    size_t floats = 0;
    for (int i = 0; i < n; ++i) {
        if (imgs[i].nx <= 0 || imgs[i].ny <= 0 || imgs[i].data.size() != (size_t)3 * imgs[i].nx * imgs[i].ny) { fprintf(stderr, "%s: image %d does not hold nx * ny * 3 floats\n", __func__, i); return 1; }
        shapes[2 * i] = imgs[i].ny; shapes[2 * i + 1] = imgs[i].nx;
        floats += imgs[i].data.size();
    }
    if (vitx_pack_check(model.handle, shapes.data(), n, 0x7fffffff, n, row0.data()) != VITX_OK) { fprintf(stderr, "%s: %s\n", __func__, vitx_last_error()); return 1; }
    const bool fits = state.pack && state.pack_model_uid == vitx_model_uid(model.handle) && state.pack_tokens >= row0[n] && state.pack_images >= n &&
                      state.pack_dtype == state.dtype && state.pack_pos_interp == state.pos_interp && state.pack_device == state.device;
    if (!fits) {
        vitx_pack_free(state.pack); state.pack = nullptr;
        vitx_pack_options opt{};
        opt.pos_interp = state.pos_interp;
        state.pack_tokens = std::max(state.pack_tokens, (int)row0[n]); state.pack_images = std::max(state.pack_images, n);
        if (vitx_pack_create(model.handle, state.device, state.pack_tokens, state.pack_images, state.dtype, &opt, &state.pack) != VITX_OK) {
            fprintf(stderr, "%s: failed to create the packed context: %s\n", __func__, vitx_last_error());
            state.pack_tokens = state.pack_images = 0;
            return 1;
        }
        state.pack_model_uid = vitx_model_uid(model.handle); state.pack_dtype = state.dtype; state.pack_pos_interp = state.pos_interp; state.pack_device = state.device;
    }
    std::vector<float> pixels;
    pixels.reserve(floats);
    for (int i = 0; i < n; ++i) pixels.insert(pixels.end(), imgs[i].data.begin(), imgs[i].data.end());
    const int C = model.hparams.num_classes;
    state.prediction.resize((size_t)n * C);
    if (vitx_pack_forward(state.pack, pixels.data(), shapes.data(), n, state.prediction.data(), nullptr) != VITX_OK) { fprintf(stderr, "%s: failed to encode the pack: %s\n", __func__, vitx_last_error()); return 1; }
    predictions.resize(n);
    for (int b = 0; b < n; ++b) {
        auto &p = predictions[b];
        p.reserve(C);
        for (int i = 0; i < C; ++i) p.push_back(std::make_pair(state.prediction[(size_t)b * C + i], i));
        std::sort(p.begin(), p.end(), [](const std::pair<float, int> &a, const std::pair<float, int> &b2) { return a.first > b2.first; });
    }
    return 0;
}

// No counterpart in the reference (its forward ends in the class probabilities): the last layer's final-norm features of n images
int vit_embed_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, int flags, std::vector<std::vector<float>> &out) {
    out.clear();
    if (!model.handle || !imgs || n <= 0 || !flags) { fprintf(stderr, "%s: invalid argument\n", __func__); return 1; }
    if (vitx_model_seq_len(model.handle) > 0) { fprintf(stderr, "%s: this is a ViTSTR model: it has no image embedding\n", __func__); return 1; }
    const int C = model.hparams.num_classes;
    int Sh = 0, Sw = 0;
    if (!state_shape(model, state, Sh, Sw, __func__)) return 1;
    const size_t img_floats = (size_t)3 * Sh * Sw;
    if (const int i = first_bad_image(imgs, n, Sh, Sw); i >= 0) {
        fprintf(stderr, "%s: image %d is %dx%d, this state expects %dx%d\n", __func__, i, imgs[i].nx, imgs[i].ny, Sw, Sh);
        return 1;
    }
    if (ensure_ctx(model, state, n) != VITX_OK) { fprintf(stderr, "%s: failed to create the context: %s\n", __func__, vitx_last_error()); return 1; }
    if (vitx_feat_enable(state.ctx, flags, 0) != VITX_OK) { fprintf(stderr, "%s: %s\n", __func__, vitx_last_error()); return 1; }
    std::vector<float> batch((size_t)n * img_floats);
    for (int i = 0; i < n; ++i) std::copy(imgs[i].data.begin(), imgs[i].data.end(), batch.begin() + (size_t)i * img_floats);
    state.prediction.resize((size_t)n * C);
    const size_t fpi = (size_t)vitx_feat_floats(state.ctx);
    std::vector<float> all((size_t)n * fpi);
    const bool ok = vitx_forward(state.ctx, batch.data(), n, state.prediction.data(), nullptr) == VITX_OK && vitx_feat_read(state.ctx, all.data(), all.size()) == VITX_OK;
    if (!ok) fprintf(stderr, "%s: failed to encode image: %s\n", __func__, vitx_last_error());
    (void)vitx_feat_enable(state.ctx, 0, 0);
    if (!ok) return 1;
    out.resize(n);
    for (int i = 0; i < n; ++i) out[i].assign(all.begin() + (size_t)i * fpi, all.begin() + (size_t)(i + 1) * fpi);
    return 0;
}

int vit_embed(const vit_model &model, vit_state &state, const image_f32 &img1, int flags, std::vector<float> &out) {
    std::vector<std::vector<float>> all;
    const int rc = vit_embed_batch(model, state, &img1, 1, flags, all);
    out.clear();
    if (rc == 0) out = std::move(all[0]);
    return rc;
}

// No counterpart in the reference: zero-shot classification of n images against a bank of class (text) embeddings (include/vitx.h)
int vit_zeroshot_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, const vit_zeroshot_bank &bank, std::vector<std::vector<std::pair<float, int>>> &out, int topk) {
    out.clear();
    if (!model.handle || !imgs || n <= 0 || bank.K <= 0 || bank.E <= 0 || bank.embeds.size() != (size_t)bank.K * bank.E) { fprintf(stderr, "%s: invalid argument\n", __func__); return 1; }
    if (vitx_model_seq_len(model.handle) > 0) { fprintf(stderr, "%s: this is a ViTSTR model: it has no image embedding\n", __func__); return 1; }
    const int C = model.hparams.num_classes, K = bank.K;
    int Sh = 0, Sw = 0;
    if (!state_shape(model, state, Sh, Sw, __func__)) return 1;
    const size_t img_floats = (size_t)3 * Sh * Sw;
    if (const int i = first_bad_image(imgs, n, Sh, Sw); i >= 0) {
        fprintf(stderr, "%s: image %d is %dx%d, this state expects %dx%d\n", __func__, i, imgs[i].nx, imgs[i].ny, Sw, Sh);
        return 1;
    }
    if (ensure_ctx(model, state, n) != VITX_OK) { fprintf(stderr, "%s: failed to create the context: %s\n", __func__, vitx_last_error()); return 1; }
    if (vitx_zeroshot_set(state.ctx, bank.embeds.data(), K, bank.E, bank.kind, bank.scale, bank.bias) != VITX_OK) { fprintf(stderr, "%s: %s\n", __func__, vitx_last_error()); return 1; }
    std::vector<float> batch((size_t)n * img_floats);
    for (int i = 0; i < n; ++i) std::copy(imgs[i].data.begin(), imgs[i].data.end(), batch.begin() + (size_t)i * img_floats);
    state.prediction.resize((size_t)n * C);
    std::vector<float> probs((size_t)n * K);
    const bool ok = vitx_forward(state.ctx, batch.data(), n, state.prediction.data(), nullptr) == VITX_OK && vitx_zeroshot_read(state.ctx, probs.data(), nullptr, probs.size()) == VITX_OK;
    if (!ok) fprintf(stderr, "%s: failed to encode image: %s\n", __func__, vitx_last_error());
    (void)vitx_zeroshot_set(state.ctx, nullptr, 0, 0, 0, 0.0f, 0.0f);
    if (!ok) return 1;
    const int k = std::min(topk > 0 ? topk : K, K);
    std::vector<int32_t> idx(k); std::vector<float> pr(k);
    out.resize(n);
    for (int i = 0; i < n; ++i) {
        if (vitx_topk(probs.data() + (size_t)i * K, K, k, idx.data(), pr.data()) != VITX_OK) { fprintf(stderr, "%s: %s\n", __func__, vitx_last_error()); out.clear(); return 1; }
        for (int j = 0; j < k; ++j) out[i].push_back(std::make_pair(pr[j], (int)idx[j]));
    }
    return 0;
}

// No counterpart in the reference: the nearest gallery rows of n images, and the vote of their labels (include/vitx.h "nearest neighbours in a gallery")
int vit_nn_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, const vit_nn_gallery &g, std::vector<vit_nn_result> &out) {
    out.clear();
    const bool voting = !g.labels.empty();
    if (!model.handle || !imgs || n <= 0 || g.G <= 0 || g.E <= 0 || g.embeds.size() != (size_t)g.G * g.E || (voting && g.labels.size() != (size_t)g.G)) { fprintf(stderr, "%s: invalid argument\n", __func__); return 1; }
    if (vitx_model_seq_len(model.handle) > 0) { fprintf(stderr, "%s: this is a ViTSTR model: it has no image embedding\n", __func__); return 1; }
    const int C = model.hparams.num_classes, k = g.k;
    int Sh = 0, Sw = 0;
    if (!state_shape(model, state, Sh, Sw, __func__)) return 1;
    const size_t img_floats = (size_t)3 * Sh * Sw;
    if (const int i = first_bad_image(imgs, n, Sh, Sw); i >= 0) {
        fprintf(stderr, "%s: image %d is %dx%d, this state expects %dx%d\n", __func__, i, imgs[i].nx, imgs[i].ny, Sw, Sh);
        return 1;
    }
    if (ensure_ctx(model, state, n) != VITX_OK) { fprintf(stderr, "%s: failed to create the context: %s\n", __func__, vitx_last_error()); return 1; }
    if (vitx_nn_set(state.ctx, g.embeds.data(), g.G, g.E, k, g.source, voting ? g.labels.data() : nullptr, g.n_labels, g.temperature) != VITX_OK) { fprintf(stderr, "%s: %s\n", __func__, vitx_last_error()); return 1; }
    std::vector<float> batch((size_t)n * img_floats);
    for (int i = 0; i < n; ++i) std::copy(imgs[i].data.begin(), imgs[i].data.end(), batch.begin() + (size_t)i * img_floats);
    state.prediction.resize((size_t)n * C);
    std::vector<int32_t> idx((size_t)n * k); std::vector<float> score((size_t)n * k), vote(voting ? (size_t)n * g.n_labels : 0);
    const bool ok = vitx_forward(state.ctx, batch.data(), n, state.prediction.data(), nullptr) == VITX_OK &&
                    vitx_nn_read(state.ctx, idx.data(), score.data(), voting ? vote.data() : nullptr) == VITX_OK;
    if (!ok) fprintf(stderr, "%s: failed to encode image: %s\n", __func__, vitx_last_error());
    (void)vitx_nn_set(state.ctx, nullptr, 0, 0, 0, 0, nullptr, 0, 0.0f);
    if (!ok) return 1;
    out.resize(n);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < k; ++j) out[i].neighbours.push_back(std::make_pair(score[(size_t)i * k + j], (int)idx[(size_t)i * k + j]));
        if (voting) out[i].vote.assign(vote.begin() + (size_t)i * g.n_labels, vote.begin() + (size_t)(i + 1) * g.n_labels);
    }
    return 0;
}

// No counterpart in the reference: a class label for every pixel of n images (include/vitx.h "dense prediction")
int vit_dense_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, const vit_dense_head &head, std::vector<vit_dense_result> &out) {
    out.clear();
    if (!model.handle || !imgs || n <= 0 || head.K <= 0 || head.Dc <= 0 || head.weight.size() != (size_t)head.K * head.Dc || (!head.bias.empty() && head.bias.size() != (size_t)head.K)) { fprintf(stderr, "%s: invalid argument\n", __func__); return 1; }
    if (vitx_model_seq_len(model.handle) > 0) { fprintf(stderr, "%s: this is a ViTSTR model: it has no dense head\n", __func__); return 1; }
    uint64_t mask = 0;
    for (const int l : head.layers) {
        if (l < 0 || l >= 64) { fprintf(stderr, "%s: layer %d outside 0 .. 63\n", __func__, l); return 1; }
        mask |= 1ull << l;
    }
    const int C = model.hparams.num_classes;
    int Sh = 0, Sw = 0;
    if (!state_shape(model, state, Sh, Sw, __func__)) return 1;
    const size_t img_floats = (size_t)3 * Sh * Sw;
    if (const int i = first_bad_image(imgs, n, Sh, Sw); i >= 0) {
        fprintf(stderr, "%s: image %d is %dx%d, this state expects %dx%d\n", __func__, i, imgs[i].nx, imgs[i].ny, Sw, Sh);
        return 1;
    }
    if (ensure_ctx(model, state, n) != VITX_OK) { fprintf(stderr, "%s: failed to create the context: %s\n", __func__, vitx_last_error()); return 1; }
    if (vitx_dense_set(state.ctx, head.weight.data(), head.bias.empty() ? nullptr : head.bias.data(), head.K, head.Dc, mask, head.out_h, head.out_w,
                       head.want_score ? VITX_DENSE_SCORE : 0) != VITX_OK) { fprintf(stderr, "%s: %s\n", __func__, vitx_last_error()); return 1; }
    int oh = 0, ow = 0;
    (void)vitx_dense_shape(state.ctx, &oh, &ow);
    const size_t px = (size_t)oh * ow;
    std::vector<float> batch((size_t)n * img_floats);
    for (int i = 0; i < n; ++i) std::copy(imgs[i].data.begin(), imgs[i].data.end(), batch.begin() + (size_t)i * img_floats);
    state.prediction.resize((size_t)n * C);
    std::vector<uint8_t> labels((size_t)n * px); std::vector<float> score(head.want_score ? (size_t)n * px : 0);
    const bool ok = vitx_forward(state.ctx, batch.data(), n, state.prediction.data(), nullptr) == VITX_OK &&
                    vitx_dense_read(state.ctx, labels.data(), head.want_score ? score.data() : nullptr, nullptr) == VITX_OK;
    if (!ok) fprintf(stderr, "%s: failed to encode image: %s\n", __func__, vitx_last_error());
    (void)vitx_dense_set(state.ctx, nullptr, nullptr, 0, 0, 0, 0, 0, 0);
    if (!ok) return 1;
    out.resize(n);
    for (int i = 0; i < n; ++i) {
        out[i].h = oh; out[i].w = ow;
        out[i].labels.assign(labels.begin() + (size_t)i * px, labels.begin() + (size_t)(i + 1) * px);
        if (head.want_score) out[i].score.assign(score.begin() + (size_t)i * px, score.begin() + (size_t)(i + 1) * px);
    }
    return 0;
}

// No counterpart in the reference: a depth for every pixel of n images (include/vitx.h "depth estimation")
int vit_depth_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, const vit_depth_head &head, std::vector<vit_depth_result> &out) {
    out.clear();
    const size_t wsz = (size_t)std::max(head.K, 0) * std::max(head.Dc, 0);
    if (!model.handle || !imgs || n <= 0 || head.K <= 0 || head.Dc <= 0 || head.wp.size() != wsz || (!head.wc.empty() && head.wc.size() != wsz) ||
        (!head.bias.empty() && head.bias.size() != (size_t)head.K) || head.bins.size() != (size_t)head.K) { fprintf(stderr, "%s: invalid argument\n", __func__); return 1; }
    if (vitx_model_seq_len(model.handle) > 0) { fprintf(stderr, "%s: this is a ViTSTR model: it has no depth head\n", __func__); return 1; }
    uint64_t mask = 0;
    for (const int l : head.layers) {
        if (l < 0 || l >= 64) { fprintf(stderr, "%s: layer %d outside 0 .. 63\n", __func__, l); return 1; }
        mask |= 1ull << l;
    }
    const int C = model.hparams.num_classes;
    int Sh = 0, Sw = 0;
    if (!state_shape(model, state, Sh, Sw, __func__)) return 1;
    const size_t img_floats = (size_t)3 * Sh * Sw;
    if (const int i = first_bad_image(imgs, n, Sh, Sw); i >= 0) {
        fprintf(stderr, "%s: image %d is %dx%d, this state expects %dx%d\n", __func__, i, imgs[i].nx, imgs[i].ny, Sw, Sh);
        return 1;
    }
    if (ensure_ctx(model, state, n) != VITX_OK) { fprintf(stderr, "%s: failed to create the context: %s\n", __func__, vitx_last_error()); return 1; }
    if (vitx_depth_set(state.ctx, head.wp.data(), head.wc.empty() ? nullptr : head.wc.data(), head.bias.empty() ? nullptr : head.bias.data(), head.bins.data(), head.K, head.Dc,
                       mask, head.upsample, head.min_depth, head.max_depth, head.out_h, head.out_w, head.norm ? VITX_DEPTH_NORM : 0) != VITX_OK) {
        fprintf(stderr, "%s: %s\n", __func__, vitx_last_error());
        return 1;
    }
    int oh = 0, ow = 0;
    (void)vitx_depth_shape(state.ctx, &oh, &ow, nullptr, nullptr);
    const size_t px = (size_t)oh * ow;
    std::vector<float> batch((size_t)n * img_floats);
    for (int i = 0; i < n; ++i) std::copy(imgs[i].data.begin(), imgs[i].data.end(), batch.begin() + (size_t)i * img_floats);
    state.prediction.resize((size_t)n * C);
    std::vector<float> depth((size_t)n * px);
    const bool ok = vitx_forward(state.ctx, batch.data(), n, state.prediction.data(), nullptr) == VITX_OK &&
                    vitx_depth_read(state.ctx, depth.data(), nullptr, nullptr, nullptr) == VITX_OK;
    if (!ok) fprintf(stderr, "%s: failed to encode image: %s\n", __func__, vitx_last_error());
    (void)vitx_depth_set(state.ctx, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0.0f, 0.0f, 0, 0, 0);
    if (!ok) return 1;
    out.resize(n);
    for (int i = 0; i < n; ++i) {
        out[i].h = oh; out[i].w = ow;
        out[i].depth.assign(depth.begin() + (size_t)i * px, depth.begin() + (size_t)(i + 1) * px);
    }
    return 0;
}

// No counterpart in the reference: the text embeddings of n tokenised prompts (include/vitx.h "the text tower")
int vit_text_embed_batch(const vit_model &model, vit_text_state &state, const int32_t *ids, int n, int flags, std::vector<std::vector<float>> &out) {
    out.clear();
    if (!model.handle || !ids || n <= 0) { fprintf(stderr, "%s: invalid argument\n", __func__); return 1; }
    if (vitx_model_kind(model.handle) != VITX_KIND_TEXT) { fprintf(stderr, "%s: this is an image model: it has no text tower\n", __func__); return 1; }
    if (!state.ctx || state.ctx_model_uid != vitx_model_uid(model.handle) || state.ctx_device != state.device || state.ctx_dtype != state.dtype || state.max_prompts < n) {
        vitx_text_free(state.ctx); state.ctx = nullptr; state.ctx_model_uid = 0;
        state.max_prompts = std::max(state.max_prompts, n);
        if (vitx_text_create(model.handle, state.device, state.max_prompts, state.dtype, &state.ctx) != VITX_OK) { fprintf(stderr, "%s: failed to create the context: %s\n", __func__, vitx_last_error()); return 1; }
        state.ctx_model_uid = vitx_model_uid(model.handle); state.ctx_device = state.device; state.ctx_dtype = state.dtype;
    }
    const int E = model.hparams.num_classes;
    std::vector<float> flat((size_t)n * E);
    if (vitx_text_embed(state.ctx, ids, n, flags, flat.data()) != VITX_OK) { fprintf(stderr, "%s: %s\n", __func__, vitx_last_error()); return 1; }
    out.resize(n);
    for (int i = 0; i < n; ++i) out[i].assign(flat.begin() + (size_t)i * E, flat.begin() + (size_t)(i + 1) * E);
    return 0;
}

// extensions/vitstr.cpp/vitstr.cpp:135-201
bool vitstr_image_preprocess(const image_u8 &img, image_f32 &res, const vit_hparams &params) {
    const int S = params.n_img_size();
    res.nx = S; res.ny = S;
    res.data.resize((size_t)S * S);
    return vitx_preprocess_vitstr_u8(img.data.data(), img.nx, img.ny, S, res.data.data()) == VITX_OK;
}

// extensions/vitstr.cpp/vitstr.cpp:970-1061 -- 0 ok / 1 failure
int vitstr_predict(const vit_model &model, vit_state &state, const image_f32 img1, const vit_params &params, std::string &text, double &score) {
    (void)params;
    text.clear(); score = 0.0;
    if (!model.handle) { fprintf(stderr, "%s: invalid argument\n", __func__); return 1; }
    const int R = vitx_model_seq_len(model.handle), S = model.hparams.img_size, C = model.hparams.num_classes;
    if (R <= 0) { fprintf(stderr, "%s: not a ViTSTR model (the patch kernel has 3 input channels): use vit_predict\n", __func__); return 1; }
    if (img1.nx != S || img1.ny != S || img1.data.size() != (size_t)S * S) { fprintf(stderr, "%s: image is %dx%d, model expects %dx%d grey\n", __func__, img1.nx, img1.ny, S, S); abort(); }
    if (ensure_ctx(model, state, 1) != VITX_OK) { fprintf(stderr, "%s: failed to encode image: %s\n", __func__, vitx_last_error()); return 1; }
    state.prediction.resize((size_t)R * C);
    if (vitx_forward(state.ctx, img1.data.data(), 1, state.prediction.data(), nullptr) != VITX_OK) {
        fprintf(stderr, "%s: failed to encode image: %s\n", __func__, vitx_last_error());
        return 1;
    }
    std::vector<int32_t> ids((size_t)R);
    int n_ids = 0;
    if (vitx_vitstr_decode(state.prediction.data(), R, C, ids.data(), &n_ids, &score) != VITX_OK) return 1;
    printf("------------------ \n");                                              // vitstr.cpp:1024
    for (int i = 0; i < n_ids; ++i) { const std::string &ch = model.hparams.id2label.at(ids[i]); printf("%s", ch.c_str()); text += ch; }   // :1050
    printf("\n");
    printf("score : %.2f \n", score);
    printf("------------------ \n");
    return 0;
}

// vit.cpp:1004-1075 -- 0 ok / 1 failure; prints the top-k lines like the reference does
int vit_predict(const vit_model &model, vit_state &state, const image_f32 img1, const vit_params &params,
                std::vector<std::pair<float, int>> &predictions) {
    std::vector<std::vector<std::pair<float, int>>> all;
    const int rc = vit_predict_batch(model, state, &img1, 1, params, all, /*print=*/true);
    predictions.clear();
    if (rc == 0) predictions = std::move(all[0]);
    return rc;
}

void print_usage(int argc, char **argv, const vit_params &params) {                                      // vit.cpp:943-956
    (void)argc;
    fprintf(stderr, "usage: %s [options]\n", argv[0]);
    fprintf(stderr, "\n");
    fprintf(stderr, "options:\n");
    fprintf(stderr, "  -h, --help              show this help message and exit\n");
    fprintf(stderr, "  -m FNAME, --model       model path (default: %s)\n", params.model.c_str());
    fprintf(stderr, "  -i FNAME, --inp         input file (default: %s)\n", params.fname_inp.c_str());
    fprintf(stderr, "  -t N, --threads         number of threads to use during computation (default: %d)\n", params.n_threads);
    fprintf(stderr, "  -k N, --topk            top k classes to print (default: %d)\n", params.topk);
    fprintf(stderr, "  -s SEED, --seed         RNG seed (default: -1)\n");
    fprintf(stderr, "  -e FLOAT, --epsilon     epsilon constant in Layer Norm layers (default: %f)\n", params.eps);
    fprintf(stderr, "\n");
}

bool vit_params_parse(int argc, char **argv, vit_params &params) {                                       // vit.cpp:958-1002
    for (int i = 1; i < argc; i++) {
        const std::string arg = argv[i];
        const bool has_val = i + 1 < argc;
        if ((arg == "-s" || arg == "--seed") && has_val) params.seed = std::stoi(argv[++i]);
        else if ((arg == "-t" || arg == "--threads") && has_val) params.n_threads = std::stoi(argv[++i]);
        else if ((arg == "-m" || arg == "--model") && has_val) params.model = argv[++i];
        else if ((arg == "-i" || arg == "--inp") && has_val) params.fname_inp = argv[++i];
        else if ((arg == "-k" || arg == "--topk") && has_val) params.topk = std::stoi(argv[++i]);
        else if ((arg == "-e" || arg == "--epsilon") && has_val) params.eps = std::stof(argv[++i]);
        else if (arg == "-h" || arg == "--help") { print_usage(argc, argv, params); exit(0); }
        else { fprintf(stderr, "error: unknown argument: %s\n", arg.c_str()); print_usage(argc, argv, params); exit(0); }
    }
    return true;
}
