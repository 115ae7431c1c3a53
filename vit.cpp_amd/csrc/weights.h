// weights.h -- the device copies of a loaded model's weights (struct WeightSet) and their upload (weights.cpp).  Everything an upload needs follows
// from the model, the device, the requested dtype and the block mode (struct WeightSpec): image contexts (context.cpp) and text contexts
// (text_forward.cpp) obtain their set through the same call.  Internal, like context.h and text_context.h, which both include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <vector>

#include "kernels.h"
#include "model_file.h"
#include "mxfp8.h"

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e__ = (expr);                                                                           \
        if (e__ != hipSuccess) { set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); return VITX_ERR_HIP; } \
    } while (0)

namespace vitx {

// A weight matrix kept in the file's block form on the device (quant.hip): `blocks` = N rows of K/32 blocks in the file's byte
// layout -- except q4_0, which is split into a nibble plane (`blocks`, 16 B per block, rows padded to n_pad) and an f16 scale
// plane (`scales`) so both the dequant kernel and the fused small-batch GEMM read aligned 16-byte pieces.  Same bits, same size.
struct QuantW {
    void *blocks = nullptr; uint16_t *scales = nullptr;
    int type = 0, N = 0, K = 0, n_pad = 0;
};
enum { W_QKV = 0, W_PROJ, W_FC1, W_FC2, W_PER_LAYER };
// A weight matrix of a VITX_MXFP8 context (mxfp8.h): elements [n_pad][k_pad] e4m3 and scales [n_pad][k_pad / 32], encoded on the host at upload
struct MxW {
    uint8_t *q = nullptr, *s = nullptr;
    int N = 0, K = 0, n_pad = 0, k_pad = 0;
};
struct LayerW {
    float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *qkv_b, *proj_b, *fc1_b, *fc2_b;
    void *qkv_w, *proj_w, *fc1_w, *fc2_w;      // expanded operand-type matrices; nullptr where the blocks stay quantised (q[]) or are MX (mx[])
    QuantW q[W_PER_LAYER];
    MxW mx[W_PER_LAYER];                       // VITX_MXFP8: qkv, fc1 and fc2 (proj stays bf16)
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// The padded extents that the upload lays matrices out with and a context sizes its scratch and GEMMs by: THE definitions, for both
inline int head_cols_pad(const vitx_model *m) { return round_up(m->hp.num_classes, gemm_tile_n()); }      // C_pad: rows of head.weight (text: E_pad)
inline int patch_k(const vitx_model *m) { return m->in_chans * m->hp.patch_size * m->hp.patch_size; }     // Kpe: K of the patch-embedding GEMM
inline int patch_k_pad(const vitx_model *m) { return round_up(patch_k(m), 64); }                          // Kpe_pad
// [Nrows][K] -> operand type, rows padded to n_pad, cols to k_pad (zeros): f32 `f` rounded once (RNE), or -- `bits` != nullptr -- operand-type rows
// forwarded bit-exact.  patch_P > 0: a patch-embedding kernel [D][Cin * P * P], its K axis permuted to the image's memory order (patch_embed.hip)
std::vector<uint16_t> operand_matrix_host(int dtype, const float *f, const uint16_t *bits, int Nrows, int K, int n_pad, int k_pad, int patch_P, int patch_Cin);

// One set per (loaded model, device, requested dtype, block mode), shared by every context that asks for it (e.g. the two contexts of
// INTEGRATION.md's "two forwards in flight"): uploaded by the first, freed with the last
struct WeightSet {
    const int device;
    explicit WeightSet(int device_) : device(device_) {}
    std::vector<void *> allocs;
    float *pre_w = nullptr, *pre_b = nullptr;      // pre_norm.* (nullptr without them): LayerNorm of the token rows in front of layer 0
    float *cls = nullptr, *reg = nullptr, *pos = nullptr, *pe_b = nullptr, *norm_w = nullptr, *norm_b = nullptr, *head_b = nullptr;
    void *pe_w = nullptr, *head_w = nullptr;
    QuantW head_q;
    void *tok = nullptr;             // a text tower's token table [V][D] as filed: f16 (tok_f16) or f32
    bool tok_f16 = false;
    // VITX_POOL_MAP (attn_pool.*): u [H][D] f32 (the folded probe, vitx_model_pool_query); the V half of kv.weight / kv.bias, padded by 128 rows so that
    // every head's [d][D] block can be read as a whole column tile; proj, norm, fc1, fc2 like a block's
    float *map_u = nullptr, *map_v_b = nullptr, *map_proj_b = nullptr, *map_ln_w = nullptr, *map_ln_b = nullptr, *map_fc1_b = nullptr, *map_fc2_b = nullptr;
    void *map_v_w = nullptr, *map_proj_w = nullptr, *map_fc1_w = nullptr, *map_fc2_w = nullptr;
    std::vector<LayerW> layers;
    size_t weight_bytes = 0;         // device bytes held by weight matrices (vitx_ctx_weight_bytes)
    int alloc(void **p, size_t bytes) {
        HIP_TRY(hipMalloc(p, bytes ? bytes : 16));
        allocs.push_back(*p);
        return VITX_OK;
    }
    ~WeightSet() {       // may run on any thread (the last context of the set): leave the caller's current device as it was
        int cur = -1; (void)hipGetDevice(&cur);
        (void)hipSetDevice(device); for (void *p : allocs) (void)hipFree(p);
        if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
    }
};

// dtype: as the caller requested it (VITX_F16 / VITX_BF16 / VITX_MXFP8: the key tells MXFP8 from BF16); quant_on_device: block types stay blocks
struct WeightSpec { const vitx_model *model; int device; int dtype; bool quant_on_device; };
// The set of `spec`, found in the registry (*shared = true) or uploaded.  On an error *out may hold a partly uploaded set: dropping it frees it
int obtain_weights(const WeightSpec &spec, std::shared_ptr<WeightSet> *out, bool *shared);

// What both kinds of context do first with their device: make it current and bring its kernels up.  `api`: the name the error messages start with
int open_device(const char *api, int device, const Tuning **tune);

}  // namespace vitx
