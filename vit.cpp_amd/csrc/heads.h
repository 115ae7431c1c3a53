// heads.h -- the opt-in outputs of an execution context (attention maps, features, the zero-shot bank, the gallery, the dense and the depth
// head): one struct each, owning its parameters and its device memory, held by vitx_ctx (context.h) through a pointer -- null means off,
// dropping the object frees everything.  outputs.cpp builds them, forward.cpp reads them.  Below them: the launch sequences of the four heads
// (heads.cpp), on plain pointers, as the forward and the vitx_op_* entry points (ops.cpp) both run them, and the part of setting a patch head that an
// image context and a packed context share.  Internal; needs no context.
#pragma once
#include <type_traits>
#include <vector>

#include "weights.h"

struct vitx_ctx;

namespace vitx {

// selected layers of an output's layer mask below layer il: the slot of il's block in the per-image layout; il = L: their number
inline int layer_slot(uint64_t mask, int il) { return __builtin_popcountll(il < 64 ? mask & ((1ull << il) - 1) : mask); }

// One device allocation: owns its pointer and frees it on every way out.  Move-only.
struct DevMem {
    void *p = nullptr;
    DevMem() = default;
    explicit DevMem(void *p_) : p(p_) {}
    DevMem(DevMem &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevMem &operator=(DevMem &&o) noexcept { if (this != &o) { (void)hipFree(p); p = o.p; o.p = nullptr; } return *this; }
    ~DevMem() { (void)hipFree(p); }
    // false, with the HIP error cleared and p == nullptr, when the device has no room
    bool alloc(size_t bytes) {
        (void)hipFree(p); p = nullptr;
        if (hipMalloc(&p, bytes) == hipSuccess) return true;
        (void)hipGetLastError(); p = nullptr;
        return false;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
    explicit operator bool() const { return p != nullptr; }
};
static_assert(!std::is_copy_constructible<DevMem>::value && !std::is_copy_assignable<DevMem>::value, "two owners would free the pointer twice");

// What the forward asks of every opt-in output, whichever it is (vitx_ctx::each_output)
struct Output {
    const char *one_pass;        // "<the output> take(s)": vitx_forward_device's "... one pass (at most %d images)"
    bool last_all_rows = false;  // the output reads every row of the last layer: no class-rows-only tail while it is set (as while the trace is on)
    int cap = 0;                 // images the buffers hold (= the images one pass takes)
    int n = 0;                   // images of the last forward made with the output set (0: none since it was set)
    explicit Output(const char *phrase) : one_pass(phrase) {}
};

// attention maps (vitx_attn_enable)
struct AttnMaps : Output {
    AttnMaps() : Output("attention maps take") {}
    uint64_t mask = 0;
    int flags = 0;
    int fpi = 0;                 // floats per image: popcount(mask) * H * N (+ N with VITX_ATTN_ROLLOUT)
    DevMem out;                  // [cap][fpi] f32: per image the selected layers' [H][N] class-token maps in ascending order, then the rollout row [N]
    DevMem roll[2];              // rollout: [cap][N][N] f32 x 2, A^_l written into one, the product R_l in place of it (ping-pong)
    DevMem cls_last;             // rollout without the last layer in the mask: its class-token maps [cap][H][N] f32
};

// embeddings and token features (vitx_feat_enable)
struct Features : Output {
    Features(int flags_, uint64_t mask_, int D_, int patches_, int L) : Output("features take"), flags(flags_), mask(mask_), D(D_), patches(patches_) {
        // MEAN or TOKENS of the last layer need every row of it
        last_all_rows = (flags & (VITX_FEAT_MEAN | VITX_FEAT_TOKENS)) && ((mask >> (L - 1)) & 1);
    }
    int flags;                   // VITX_FEAT_*, never 0
    uint64_t mask;               // selected layers, never 0: "the last layer" is resolved at vitx_feat_enable
    int D, patches;              // the context's hidden size and patch rows per image (N - Tp)
    int fpi = 0;                 // floats per image: popcount(mask) * layer_floats()
    DevMem out;                  // [cap][fpi] f32: per image the selected layers in ascending order, each [cls D][mean D][tokens patches x D] (selected parts only)
    int layer_floats() const { return D * ((flags & VITX_FEAT_CLS ? 1 : 0) + (flags & VITX_FEAT_MEAN ? 1 : 0) + (flags & VITX_FEAT_TOKENS ? patches : 0)); }
    bool selects(int il) const { return (mask >> il) & 1; }
    // the slots of layer il in image first_img's block of `out` (nullptr: not selected), in the layout's order cls, mean, tokens
    void slots(int first_img, int il, float **o_cls, float **o_mean, float **o_tok) const {
        float *o = out.as<float>() + (size_t)first_img * fpi + (size_t)layer_slot(mask, il) * layer_floats();
        *o_cls = *o_mean = *o_tok = nullptr;
        if (flags & VITX_FEAT_CLS) { *o_cls = o; o += D; }
        if (flags & VITX_FEAT_MEAN) { *o_mean = o; o += D; }
        if (flags & VITX_FEAT_TOKENS) *o_tok = o;
    }
};

// zero-shot classification (vitx_zeroshot_set)
struct ZeroShot : Output {
    ZeroShot() : Output("zero-shot classification takes") {}
    int K = 0, Kpad = 0;         // classes of the bank; its rows on the device (K rounded up to the GEMM's column tile, zero rows beyond K)
    int E = 0;                   // the embedding width (vitx_ctx::zs_width)
    int kind = 0;                // enum vitx_zs_kind
    float scale = 1.0f, bias = 0.0f;
    DevMem bank;                 // [Kpad][E] operand type
    DevMem zero;                 // [Kpad] f32 zeros: the bank GEMM's bias
    DevMem out;                  // [cap][2][K] f32: per image the probabilities, then the logits
    std::vector<DevMem> a;       // per slice: [round_up(cap, tm)][E] operand type, the normalised embeddings (the GEMM's A rows)
    std::vector<DevMem> acc;     // per slice: [round_up(cap, tm)][Kpad] f32, the GEMM's output
};

// nearest neighbours in a gallery (vitx_nn_set)
struct Gallery : Output {
    Gallery() : Output("nearest neighbours take") {}
    static constexpr int kChunk = 32768;   // Gc: gallery rows one chunk GEMM scores (a multiple of the GEMM's column tile; tools/nn_cost.py sweeps it)
    long G = 0, Gpad = 0;        // rows of the gallery; its rows on the device (G rounded up to the column tile, zero rows beyond G)
    int k = 0, source = 0, E = 0;
    int nlabels = 0;             // 0: no labels, no vote
    float T = 0.0f;
    DevMem gallery;              // [Gpad][E] operand type
    DevMem labels;               // [G] i32
    DevMem zero;                 // [kChunk] f32 zeros: the chunk GEMMs' bias
    DevMem out;                  // [cap][k] {f32 score, i32 index}
    DevMem vote;                 // [cap][nlabels] f32
    std::vector<DevMem> a;       // per slice: [round_up(cap, tm)][E] operand type, the normalised queries (the GEMMs' A rows)
    std::vector<DevMem> acc;     // per slice: [round_up(cap, tm)][kChunk] f32, one chunk's scores
    std::vector<DevMem> state;   // per slice: the running top-k (nn_state_bytes)
    size_t scratch = 0;          // bytes of acc + state over all slices
};

// What the dense and the depth head share: a linear map over the patch rows of up to four layers, K columns per patch
struct PatchHead : Output {
    using Output::Output;
    int K = 0, Kpad = 0;         // columns of the head; its rows on the device (K rounded up to the GEMM's column tile, zero rows beyond K)
    int Dc = 0;                  // the operand's width: popcount(mask) * D
    uint64_t mask = 0;           // selected layers, never 0: "the last layer" is resolved at the set call
    int oh = 0, ow = 0;          // the output map's shape
    int flags = 0;               // VITX_DENSE_* / VITX_DEPTH_*
    std::vector<DevMem> a;       // per slice: [round_up(slice cap * gh * gw, tm)][Dc] operand type, the patch GEMM's A rows
    std::vector<DevMem> acc;     // per slice: [the same rows][Kpad] f32, the patch logits
    size_t scratch = 0;          // bytes of the per-slice buffers over all slices
    bool selects(int il) const { return (mask >> il) & 1; }
    // the operand rows' columns of layer il, in elements of the operand type
    size_t col(int il, int D) const { return (size_t)layer_slot(mask, il) * D; }
};

// the dense head (vitx_dense_set)
struct DenseHead : PatchHead {
    DenseHead() : PatchHead("the dense head takes") {}
    DevMem W;                    // [Kpad][Dc] operand type
    DevMem bias;                 // [Kpad] f32, zeros beyond K
    DevMem labels;               // [cap][oh][ow] u8
    DevMem score;                // VITX_DENSE_SCORE: [cap][oh][ow] f32
    DevMem logits;               // VITX_DENSE_LOGITS: [cap][gh * gw][K] f32, the patch logits kept for vitx_dense_read
};

// What the checks of a packed forward call give it while a dense head is set (packed_forward.cpp check_dense; kernels.h dense_pack_tables)
struct PackDenseCall {
    std::vector<int32_t> grids, outs;    // [n][2] each, the patch grids and the output shapes
    std::vector<int64_t> pix0;   // [n + 1], the running pixel count of the outputs
    std::vector<int32_t> tile0;  // [n + 1], the running tile count of the label launch
    int cells = 0;               // the widest tile window
};

// the dense head of a packed context (vitx_pack_dense_set): the same linear map over ALL rows of the pack -- a[0] [round_up(max_tokens, tm)][Dc],
// acc[0] the same rows x Kpad, the prefix rows computed and never used -- and one label map per image at its own size, the maps end to end
struct PackDense : DenseHead {
    long max_pixels = 0;         // elements of labels (and score); logits: [max_tokens][K], every row of the pack
    size_t bytes = 0;            // device bytes of everything above: what the head adds to vitx_pack_scratch_bytes
    std::vector<int32_t> next_out;       // vitx_pack_dense_out: the output shapes [n][2] of the next forward (empty: the images' own shapes)
    PackDenseCall last;          // of the last call that passed its checks with the head set
};

// the depth head (vitx_depth_set)
struct DepthHead : PatchHead {
    DepthHead() : PatchHead("the depth head takes") {}
    int u = 0;                   // the fine plane is u gh x u gw
    float lo = 0.0f, hi = 0.0f;  // the clamp
    DevMem Wp;                   // [Kpad][Dc] operand type: the patch half
    DevMem Wc;                   // the class half, or empty: the offsets are the bias then, and no class rows are written
    DevMem bias;                 // [Kpad] f32, zeros beyond K: the class GEMM's bias, or every image's offsets
    DevMem zero;                 // [Kpad] f32 zeros: the patch GEMM's bias
    DevMem bins;                 // [Kpad] f32 bin centres
    std::vector<float> bias_host;        // [K]: what vitx_depth_read returns as offsets of a head without a class half
    DevMem depth;                // [cap][oh][ow] f32
    DevMem fine;                 // [cap][u gh][u gw] f32: the resize reads it; vitx_depth_read returns it under VITX_DEPTH_FINE
    DevMem logits;               // VITX_DEPTH_LOGITS: [cap][gh * gw][K] f32, the patch logits kept for vitx_depth_read
    DevMem off;                  // VITX_DEPTH_LOGITS with a class half: [cap][K] f32, the offsets kept
    std::vector<DevMem> ac;      // per slice, class half only: [round_up(slice cap, tm)][Dc] operand type, the class rows
    std::vector<DevMem> o;       // per slice, class half only: [round_up(slice cap, tm)][Kpad] f32, the offsets
};

// The same while a depth head is set (check_depth; kernels.h depth_pack_tables)
struct PackDepthCall {
    std::vector<int32_t> grids, outs;    // [n][2] each, the patch grids and the depth maps' shapes
    std::vector<int64_t> pix0, fine0;    // [n + 1] each, the running pixel counts of the maps and of the fine planes
    std::vector<int32_t> ftile0, otile0; // [n + 1] each, the running tile counts of the fine and the resize launch
    int cells = 0;               // the widest fine-tile window
};

// the depth head of a packed context (vitx_pack_depth_set): the same two linear maps over ALL rows of the pack -- a[0] [round_up(max_tokens, tm)][Dc],
// acc[0] the same rows x Kpad, the prefix rows computed and never used; with a class half ac[0] [round_up(max_images, tm)][Dc], the class rows gathered
// from a[0], and o[0] their offsets -- and one fine plane and one depth map per image at its own size, planes and maps end to end
struct PackDepth : DepthHead {
    long max_pixels = 0;         // floats of depth; fine: u^2 max_tokens floats; logits: [max_tokens][K], every row of the pack; off: [max_images][K]
    size_t bytes = 0;            // device bytes of everything above: what the head adds to vitx_pack_scratch_bytes
    std::vector<int32_t> next_out;       // vitx_pack_depth_out: the output shapes [n][2] of the next forward (empty: the images' own shapes)
    PackDepthCall last;          // of the last call that passed its checks with the head set
};

// ---- the launch sequences of the four heads (heads.cpp) --------------------------------------------------------------------------------
// Each only enqueues on `st`, on the caller's buffers: every pointer is a device pointer, rows are padded to the GEMMs' row tile
// (gemm_tile_m) and the columns of a head to their column tile (gemm_tile_n) as the struct comments above say.  `prof` != nullptr: every launch
// is recorded in that context's profile (ProfScope, context.h) while its profile is on.
struct HeadLaunch { const Tuning &tune; int dtype; hipStream_t st; vitx_ctx *prof; };

// One GEMM launch's algorithmic work as the profile counts it: M rows of A [.][K], W [N][K] (q4: kept as q4_0 blocks), the output of `epi`
// (+ the residual it reads, the second plane of EPI_BIAS_HILO, ln: the normalised rows a LayerNorm-fusing launch also stores)
inline void gemm_work(int epi, int M, int N, int K, bool q4, bool ln, double *flops, double *bytes) {
    const int esz = epi_out_bytes(epi);
    *bytes = (double)M * K * 2 + (double)N * K * (q4 ? 0.5625 : 2.0) + (double)M * N * esz;
    if (epi == EPI_BIAS_RESID) *bytes += (double)M * N * 4;
    if (epi == EPI_BIAS_HILO) *bytes += (double)M * N * esz;        // the second plane
    if (ln) *bytes += (double)M * N * 2;
    *flops = 2.0 * M * (double)N * K;
}

// Zero-shot classification: z = n f32 embedding rows (row stride ldz floats) -> unit rows in the operand type (a), the bank GEMM through the
// dispatcher with the zero bias (acc), then logits and probabilities (rows out_stride floats apart).  3 launches.
hipError_t head_zeroshot(const HeadLaunch &l, const float *z, long ldz, void *a, const void *bank, const float *zero, float *acc, float *probs, float *logits,
                         long out_stride, int n, int K, int E, int kind, float scale, float bias);
// Nearest neighbours: the n query rows z -- f32, or (z_is_operand) operand-type rows; row stride ldz elements -- become unit rows in the operand type
// (zero-shot's rule); then the gallery passes by in chunks of `chunk` rows, each one dispatcher GEMM into the score scratch acc (its own base pointer
// into the gallery: only a chunk has to fit the GEMM's operand window) and one selection launch that merges the chunk's real columns into the running
// state; the last launch writes the k best (and, with labels, the vote).  2 ceil(G / chunk) + 2 launches.
hipError_t head_nearest(const HeadLaunch &l, const void *z, long ldz, bool z_is_operand, void *a, const void *gallery, const float *zero, float *acc, void *state,
                        long G, int E, int k, int chunk, const int *labels, int nlabels, float T, void *pairs, float *vote, int n);
// One linear map over compact operand rows, the step both patch heads (and the depth head's class half) are made of: the pad rows of a zeroed,
// acc [round_up(rows, tile)][Kpad] = a . W^T + bias through the dispatcher, and (keep != nullptr) the K real columns copied to keep [rows][K]
hipError_t head_linear(const HeadLaunch &l, int pc, void *a, const void *W, const float *bias, float *acc, int rows, int K, int Dc, float *keep);
// The dense head after its operand rows are written: the patch logits (head_linear), then the label kernel
hipError_t head_dense(const HeadLaunch &l, void *a, const void *W, const float *bias, float *acc, int n, int gh, int gw, int K, int Dc, int oh, int ow,
                      uint8_t *labels, float *score, float *keep);
// The dense head of a pack after its operand rows are written: the logits of all `rows` rows of the pack (head_linear; keep: [rows][K]), then the
// packed label kernel on the device tables tile0 / seg (kernels.h dense_pack_tables, dense_pack_seg).  2 launches.
hipError_t head_dense_packed(const HeadLaunch &l, void *a, const void *W, const float *bias, float *acc, int rows, int K, int Dc, const int *tile0, const int *seg,
                             int n, int tiles, int cells, long pixels, uint8_t *labels, float *score, float *keep);
// The depth head after its operand rows are written: the patch logits with the zero bias, with a class half (Wc) the offsets from the class rows ac
// with the head's bias (without: the bias is every image's offsets), the fine plane, the depth map
hipError_t head_depth(const HeadLaunch &l, void *a, const void *Wp, const float *zero, float *acc, void *ac, const void *Wc, const float *bias, float *o,
                      const float *bins, int n, int gh, int gw, int K, int Dc, int u, int oh, int ow, float lo, float hi, float *fine, float *depth,
                      float *keep, float *keep_off);

// The depth head of a pack after its operand rows are written: the patch logits of all `rows` rows of the pack with the zero bias (head_linear; keep:
// [rows][K]); with a class half the class rows gathered from a by row0 (device, [n]) into ac and their offsets with the head's bias (keep_off: [n][K]);
// then the packed fine and resize kernels on the device tables ftile0 / otile0 / seg (kernels.h depth_pack_tables, depth_pack_seg; seg's offset rows
// are 0 .. n - 1).  3 launches, 5 with a class half.
hipError_t head_depth_packed(const HeadLaunch &l, void *a, const void *Wp, const float *zero, float *acc, void *ac, const void *Wc, const float *bias, float *o,
                             const float *bins, int rows, int K, int Dc, const int *row0, const int *ftile0, const int *otile0, const int *seg, int n, int ftiles,
                             int otiles, int cells, long fine_px, long pixels, float lo, float hi, float *fine, float *depth, float *keep, float *keep_off);

// the argument checks vitx_op_depth_fine / vitx_op_depth_resize / vitx_op_depth (ops.cpp) share with vitx_depth_host (depth_host.cpp): none needs a device
int depth_fine_args(const char *name, const void *logits, long ld, const void *bins, int n, int gh, int gw, int K, int u, const void *fine);
int depth_resize_args(const char *name, const void *fine, int n, int fh, int fw, int out_h, int out_w, float lo, float hi, const void *out);

// ---- what setting a patch head takes, whichever context it serves (heads.cpp) -----------------------------------------------------------
// The argument checks need no device and put `api` in front of every refusal.  They come in pieces because each context's and each head's own
// checks sit between them (outputs.cpp: vitx_dense_set, vitx_depth_set; packed_outputs.cpp: vitx_pack_dense_set, vitx_pack_depth_set).
// patch_head_mask: the layer mask of a head on a model of L layers of width D (0: the last layer), at most 4 layers, Dc = layers x D
int patch_head_mask(const char *api, int L, int D, int Dc, uint64_t *mask);
// dense_head_args: the weights are there, K >= 1, known flags, then patch_head_mask
int dense_head_args(const char *api, const float *W, int K, int Dc, int flags, int L, int D, uint64_t *mask);
// dense_head_values: W [K][Dc] and bias [K] (or NULL) are finite, K is at most kDenseMaxK
int dense_head_values(const char *api, const float *W, const float *bias, int K, int Dc);
// depth_head_args: the weights and bins are there, K >= 1, known flags, then patch_head_mask
int depth_head_args(const char *api, const float *Wp, const float *bins, int K, int Dc, int flags, int L, int D, uint64_t *mask);
// depth_head_values: the depth range is finite and ordered, Wp and Wc [K][Dc] and bias [K] (each but Wp or NULL) are finite, the bins finite and positive,
// K is at most kDepthMaxK, upsample is 1, 2 or 4
int depth_head_values(const char *api, const float *Wp, const float *Wc, const float *bias, const float *bins, int K, int Dc, float min_depth, float max_depth, int upsample);
// The parameters of a depth head whose K, Kpad and Dc are set and whose Wp, Wc (with a class half), bias, zero and bins are allocated, onto the device:
// the halves through upload_operand, bias / zero / bins zero-filled, then `bias` [K] (or NULL) and `bins` [K] copied
hipError_t depth_head_upload(const DepthHead &dp, int dtype, const float *Wp, const float *Wc, const float *bias, const float *bins);
// W [K][Dc] f32 -> dst [Kpad][Dc], rounded (RNE) to the operand type, zero rows beyond K
hipError_t upload_operand(int dtype, const DevMem &dst, const float *W, int K, int Kpad, int Dc);
// The parameters of a dense head whose K, Kpad and Dc are set, onto the device: W through upload_operand, bias zero-filled, then `bias` [K] (or NULL) copied
hipError_t dense_head_upload(const DenseHead &dn, int dtype, const float *W, const float *bias);

}  // namespace vitx
