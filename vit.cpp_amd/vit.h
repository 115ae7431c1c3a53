// vit.h -- C++ drop-in mirror of the reference's public API for the forward path.
//
// Same entry-point names, argument meaning and error behaviour as
// /root/reference/vit.h:115-124, re-declared so the reference's callers (main.cpp:57-98, tests/benchmark.cpp:57-122) build
// against libvitx.so once their ggml lines are removed (main.cpp:82-91 creates state.ctx / state.prediction by hand and :110
// frees model.ctx -- ggml objects this engine does not have; examples/vit_main.cpp is main.cpp without them):
//   * vit_model / vit_state keep their names but hold opaque engine handles instead of
//     ggml_tensor* / ggml_context* (the reference's fields are ggml internals);
//   * vit_predict still fills `predictions` with all (prob, class) pairs sorted
//     descending and prints the top-k lines to stdout (vit.cpp:1043-1067);
//   * vit_predict_batch is NEW (the reference has no batched call): n images per launch;
//   * vit_embed / vit_embed_batch are NEW (the reference returns class probabilities only): the image embedding;
//   * vit_zeroshot_batch is NEW: zero-shot classes of a CLIP / SigLIP file against a bank of text embeddings;
//   * vit_nn_batch is NEW: the nearest rows of a gallery of embeddings, and the weighted k-NN vote of their labels;
//   * vit_dense_batch is NEW: a linear head over the patch tokens, a class label for every pixel.
// Everything below is a thin wrapper over the C ABI in include/vitx.h.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../include/vitx.h"

struct vit_hparams {                      // vit.h:20-37
    int32_t hidden_size = 768;
    int32_t num_hidden_layers = 12;
    int32_t num_attention_heads = 12;
    int32_t num_classes = 1000;
    int32_t patch_size = 8;
    int32_t img_size = 224;
    int32_t ftype = 1;
    float eps = 1e-6f;
    std::string interpolation = "bicubic";
    std::map<int, std::string> id2label;

    int32_t n_enc_head_dim() const { return hidden_size / num_attention_heads; }   // vit.cpp:30-33
    int32_t n_img_size() const { return img_size; }                                // vit.cpp:35-38
    int32_t n_patch_size() const { return patch_size; }                            // vit.cpp:40-43
    int32_t n_img_embd() const { return img_size / patch_size; }                   // vit.cpp:45-48
};

struct vit_model {                        // vit.h:82-89 (tensor handles replaced by the engine's)
    vit_hparams hparams;
    vitx_model *handle = nullptr;         // parsed weight file (host)
    vit_model() = default;
    vit_model(const vit_model &) = delete;
    vit_model &operator=(const vit_model &) = delete;
    ~vit_model();
};

struct vit_state {                        // vit.h:72-80: per-caller mutable scratch
    vitx_ctx *ctx = nullptr;              // created lazily by vit_predict on `device`
    uint64_t ctx_model_uid = 0;           // vitx_model_uid of the parsed file `ctx` holds the weights of: a state reused with another (or a
                                          // reloaded) vit_model gets a fresh context instead of silently running the old weights.  An id,
                                          // not the pointer: `vit_model m; vit_model_load(f, m);` in a loop usually re-allocates the same address
    int device = 0;                       // the HIP device `ctx` and `pack` live on.  device and dtype may be changed between calls: a cached context that was
                                          // created with other values is replaced on the next call (ctx_device / ctx_dtype, pack_device / pack_dtype hold what
                                          // each was created with); a device that does not exist makes that call return 1
    int max_batch = 1;                    // capacity of ctx; grown on demand by vit_predict_batch
    int dtype = VITX_F16;                 // MFMA operand type (VITX_F16 reproduces the reference's rounding); VITX_MXFP8: experimental, slower than bf16
    int ctx_device = 0, ctx_dtype = 0;    // the device and dtype `ctx` was created with
    int img_size = 0;                     // 0 = the file's; else the side of the images THIS state takes (a positive multiple of the patch size): the context
                                          // runs on the file's position table resampled to that grid (vitx_ctx_options::img_size).  vit_predict, vit_predict_batch
                                          // and vit_embed_batch check their images against this size; preprocess to it by passing vit_image_preprocess a copy of
                                          // the hparams with img_size set.  Changing it (or pos_interp) replaces the context on the next call.  Not for ViTSTR.
    int img_h = 0, img_w = 0;             // both 0, or both set with img_size == 0: THIS state takes img_h x img_w images (positive multiples of the patch size) in a
                                          // rectangular context (vitx_ctx_create_rect; include/vitx.h "rectangular contexts"): res.nx == img_w, res.ny == img_h, as
                                          // vit_image_preprocess_rect emits.  Changing them replaces the context on the next call, as img_size does.  Not for ViTSTR.
    int pos_interp = VITX_POS_BICUBIC;    // enum vitx_pos_interp: which bicubic convention resamples the table (include/vitx.h)
    int ctx_pos_interp = 0;               // the pos_interp `ctx` was created with
    std::vector<float> prediction;        // class probabilities of the last call ([n][num_classes])
    vitx_pack *pack = nullptr;            // the packed context of vit_pack_batch, created lazily on `device` with `dtype` and `pos_interp`; grown on demand
    uint64_t pack_model_uid = 0;
    int pack_tokens = 0, pack_images = 0, pack_dtype = 0, pack_pos_interp = 0, pack_device = 0;      // what `pack` was created with
    vit_state() = default;
    vit_state(const vit_state &) = delete;
    vit_state &operator=(const vit_state &) = delete;
    ~vit_state();
};

struct image_u8 { int nx; int ny; std::vector<uint8_t> data; };     // vit.h:91-96
struct image_f32 { int nx; int ny; std::vector<float> data; };      // vit.h:98-103

struct vit_params {                       // vit.h:105-113
    int32_t seed = -1;
    int32_t n_threads = std::min(4, (int32_t)std::thread::hardware_concurrency());   // unused: the GPU does the work
    int32_t topk = 5;
    std::string model = "../ggml-model-f16.gguf";
    std::string fname_inp = "../assets/tench.jpg";
    float eps = 1e-6f;                    // parsed but unused by the forward, as in the reference (vit.cpp:984-987 vs 808)
};

bool load_image_from_file(const std::string &fname, image_u8 &img);                                    // vit.h:118 (stbi_load replaced by csrc/image_decode.cpp)
bool vit_model_load(const std::string &fname, vit_model &model);                                       // vit.h:120
// resizes to params.img_size, whatever it is: for a state at another size than the file's, pass a copy of model.hparams with img_size = state.img_size
bool vit_image_preprocess(const image_u8 &img, image_f32 &res, const vit_hparams &params);            // vit.h:119
// NEW, no counterpart in the reference: the preprocessing the MODEL FILE describes (include/vitx.h "each model's own preprocessing": CLIP's and
// DINOv2's shortest-edge resize + centre crop, HuggingFace ViT's stretch, each with Pillow's filter and the publisher's mean / std).  A file
// without a description gets vit_image_preprocess with bicubic interpolation: the reference's own files are preprocessed as always.
// img_size 0 = the file's; else the side of the images a state with that vit_state::img_size takes (vitx_preproc_at_size).
bool vit_image_preprocess_model(const image_u8 &img, image_f32 &res, const vit_model &model, int img_size = 0);
// NEW: the whole image stretched to w x h for a state with img_w = w, img_h = h (vitx_preprocess_rect): the file's PIL filter, mean and std, no crop; a file
// without a description, or with the reference's filter, takes Pillow bicubic with its default mean / std.
bool vit_image_preprocess_rect(const image_u8 &img, image_f32 &res, const vit_model &model, int w, int h);
int vit_predict(const vit_model &model, vit_state &state, const image_f32 img1, const vit_params &params,
                std::vector<std::pair<float, int>> &predictions);                                      // vit.h:122
int vit_predict_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, const vit_params &params,
                      std::vector<std::vector<std::pair<float, int>>> &predictions, bool print = false);
// NEW, no counterpart in the reference: n preprocessed images, each of its OWN shape (vit_image_preprocess_rect at any w x h that are multiples of the
// patch size), in ONE forward of a packed context (include/vitx.h "packed batches"; VITX_F16 is plain fp16 there).  predictions[i] = image i's class
// probabilities, sorted as vit_predict_batch sorts them; state.prediction holds them unsorted.  An image's result does not depend on the others.
// state.img_size / img_h / img_w are not consulted.  0 ok / 1 failure.
int vit_pack_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, std::vector<std::vector<std::pair<float, int>>> &predictions);
// NEW, no counterpart in the reference: the embeddings of n preprocessed images -- the f32 final-norm features of the last layer
// (include/vitx.h, "image embeddings and token features").  flags = VITX_FEAT_CLS, VITX_FEAT_MEAN, VITX_FEAT_TOKENS, optionally | VITX_FEAT_L2;
// out[i] = image i's floats in the order [cls D][mean D][tokens (N-T) * D] (the selected parts; T = 1 + the model's register tokens, 0 for a model with the attention-pooling head, whose cls part is the pooled embedding).  state.prediction holds the class
// probabilities of the same forward; the features are switched off again before returning.  0 ok / 1 failure.
int vit_embed_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, int flags, std::vector<std::vector<float>> &out);
int vit_embed(const vit_model &model, vit_state &state, const image_f32 &img1, int flags, std::vector<float> &out);
// NEW, no counterpart in the reference: zero-shot classification (include/vitx.h "zero-shot classification").  A bank = K unit-length class
// (text) embeddings of width E -- the model's embedding width: num_classes of a CLIP file (its head is the visual projection), hidden_size of a
// SigLIP file -- with the publisher's kind, scale = exp(logit_scale) and bias (convert.py zeroshot_bank computes all of it from a transformers model).
struct vit_zeroshot_bank {
    std::vector<float> embeds;            // [K][E], rows of unit length (the engine does not renormalise them)
    int K = 0, E = 0;
    int kind = VITX_ZS_SOFTMAX;           // VITX_ZS_SOFTMAX (CLIP) or VITX_ZS_SIGMOID (SigLIP)
    float scale = 1.0f, bias = 0.0f;
    std::vector<std::string> labels;      // K names, or empty
};
// out[i] = image i's topk (probability, class) pairs in vitx_topk's order (topk <= 0 or > K: all K).  The bank is set for this call and switched off again before
// returning; state.prediction holds the file's own class "probabilities" of the same forward.  0 ok / 1 failure.
int vit_zeroshot_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, const vit_zeroshot_bank &bank,
                       std::vector<std::vector<std::pair<float, int>>> &out, int topk = 5);
// NEW, no counterpart in the reference: nearest neighbours in a gallery of embeddings (include/vitx.h "nearest neighbours in a gallery") -- retrieval,
// and with labels the temperature-weighted k-NN vote a headless DINOv2 / DINOv3 backbone is evaluated with.
struct vit_nn_gallery {
    std::vector<float> embeds;            // [G][E], rows of unit length (the engine does not renormalise them); E = vitx_nn_width of `source`
    long G = 0;
    int E = 0, k = 5;
    int source = VITX_NN_EMBED;           // VITX_NN_EMBED (the head's operand row) or VITX_NN_LOGITS (the logits row: image_embeds of a CLIP file)
    std::vector<int32_t> labels;          // G labels in [0, n_labels), or empty: no vote
    int n_labels = 0;
    float temperature = 0.07f;
};
struct vit_nn_result {
    std::vector<std::pair<float, int>> neighbours;   // k (score, gallery row) pairs, best first
    std::vector<float> vote;                         // n_labels weights that sum to 1, or empty
};
// out[i] = image i's result.  The gallery is set for this call and switched off again before returning; state.prediction holds the file's own class
// probabilities of the same forward.  0 ok / 1 failure.
int vit_nn_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, const vit_nn_gallery &gallery, std::vector<vit_nn_result> &out);
// NEW, no counterpart in the reference: dense prediction (include/vitx.h "dense prediction") -- a linear head over the final-norm patch tokens of up to
// four layers (the form DINOv2's segmentation heads are published in; convert.py --dense-head-in writes one from an mmseg checkpoint).
struct vit_dense_head {
    std::vector<float> weight;            // [K][Dc], Dc = layers.size() * hidden_size
    std::vector<float> bias;              // K, or empty: zeros
    int K = 0, Dc = 0;
    std::vector<int> layers;              // the layers whose tokens are concatenated, ascending; empty: the last layer
    int out_h = 0, out_w = 0;             // the label map's shape; 0 x 0: the state's image shape
    bool want_score = false;              // also the winner's resampled logit per pixel
    std::vector<std::string> names;       // K names, or empty
};
struct vit_dense_result {
    int h = 0, w = 0;
    std::vector<uint8_t> labels;          // [h][w]
    std::vector<float> score;             // [h][w], or empty
};
// out[i] = image i's label map.  The head is set for this call and switched off again before returning; state.prediction holds the file's own class
// probabilities of the same forward.  0 ok / 1 failure.
int vit_dense_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, const vit_dense_head &head, std::vector<vit_dense_result> &out);
// NEW, no counterpart in the reference: depth estimation (include/vitx.h "depth estimation") -- a binned linear head over the patch and class tokens of
// up to four layers (the form DINOv2's linear depth heads are published in; convert.py --depth-head-in writes one from a checkpoint).
struct vit_depth_head {
    std::vector<float> wp;                // [K][Dc] over the patch tokens, Dc = layers.size() * hidden_size
    std::vector<float> wc;                // [K][Dc] over the class tokens, or empty: no class half
    std::vector<float> bias;              // K, or empty: zeros
    std::vector<float> bins;              // K bin centres, all > 0
    int K = 0, Dc = 0;
    std::vector<int> layers;              // the layers whose tokens are concatenated, ascending; empty: the last layer
    int upsample = 4;                     // 1, 2 or 4: the bins are reduced on a grid this many times finer than the patch grid
    float min_depth = 0.001f, max_depth = 10.0f;
    bool norm = false;                    // the head reads final-norm tokens, not the raw residual stream
    int out_h = 0, out_w = 0;             // the depth map's shape; 0 x 0: the state's image shape
};
struct vit_depth_result {
    int h = 0, w = 0;
    std::vector<float> depth;             // [h][w]
};
// out[i] = image i's depth map.  The head is set for this call and switched off again before returning; state.prediction holds the file's own class
// probabilities of the same forward.  0 ok / 1 failure.
int vit_depth_batch(const vit_model &model, vit_state &state, const image_f32 *imgs, int n, const vit_depth_head &head, std::vector<vit_depth_result> &out);
// NEW, no counterpart in the reference: the text tower of a CLIP / SigLIP checkpoint (include/vitx.h "the text tower").  `model` is a text-tower
// file (vitx_model_kind == VITX_KIND_TEXT; hparams.img_size is its context length T, hparams.num_classes its embedding width E).  ids: n
// tokenised prompts [n][T] -- there is no tokenizer in the engine; out[i] = prompt i's E floats; flags 0 or VITX_TEXT_L2.  0 ok / 1 failure.
struct vit_text_state {                   // per-caller mutable scratch of the text tower, the analogue of vit_state
    vitx_text *ctx = nullptr;             // created lazily on `device`, grown on demand
    uint64_t ctx_model_uid = 0;
    int device = 0;                       // device and dtype may be changed between calls, as in vit_state: the context is then replaced on the next call
    int max_prompts = 1;
    int dtype = VITX_F16;                 // VITX_F16 or VITX_BF16
    int ctx_device = 0, ctx_dtype = 0;    // the device and dtype `ctx` was created with
    vit_text_state() = default;
    vit_text_state(const vit_text_state &) = delete;
    vit_text_state &operator=(const vit_text_state &) = delete;
    ~vit_text_state();
};
int vit_text_embed_batch(const vit_model &model, vit_text_state &state, const int32_t *ids, int n, int flags, std::vector<std::vector<float>> &out);
// ---- the ViTSTR scene-text extension (extensions/vitstr.cpp).  It is a separate program in the reference that re-uses the names
// vit_image_preprocess / vit_predict with different bodies (vitstr.h:115-119); here both programs live in one library, so the
// extension's two functions carry a vitstr_ prefix.  vit_model_load is shared: a file whose patch kernel has ONE input channel is
// a ViTSTR model (vitstr.cpp:482).
bool vitstr_image_preprocess(const image_u8 &img, image_f32 &res, const vit_hparams &params);         // vitstr.cpp:135-201: grey, [img_size][img_size]
// vitstr.cpp:970-1061: forward + greedy decode; prints the text and "score : x.xx" framed by dashed lines exactly like the
// extension, and also returns them.  state.prediction = [25][num_classes] probabilities.
int vitstr_predict(const vit_model &model, vit_state &state, const image_f32 img1, const vit_params &params, std::string &text, double &score);
void print_usage(int argc, char **argv, const vit_params &params);                                     // vit.h:123
bool vit_params_parse(int argc, char **argv, vit_params &params);                                      // vit.h:124
