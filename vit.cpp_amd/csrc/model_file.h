// model_file.h -- host-side parse of the reference's legacy-ggml ".gguf" weight file.
// Replaces the file half of vit_model_load (/root/reference/vit.cpp:308-712).
#pragma once
#include <stdint.h>
#include <map>
#include <string>
#include <vector>

#include "../../include/vitx.h"

namespace vitx {

enum { T_F32 = 0, T_F16 = 1, T_Q4_0 = 2, T_Q4_1 = 3, T_Q5_0 = 6, T_Q5_1 = 7, T_Q8_0 = 8 };
int type_block_bytes(int t);   // 0 for unknown
int type_block_elems(int t);

struct HostTensor {
    std::string name;
    int32_t type = 0;
    int32_t n_dims = 0;
    int64_t ne[4] = {1, 1, 1, 1};
    std::vector<uint8_t> raw;
    int64_t nelements() const { return ne[0] * ne[1] * ne[2] * ne[3]; }
    // exact decode to f32 (f16 widening / block dequantisation, ggml dequantize_row_*)
    void decode_f32(float *out) const;
};

}  // namespace vitx

struct vitx_model {
    vitx_hparams hp;
    uint64_t uid = 0;                                 // unique per successful vitx_model_load in this process (never reused: an address can be)
    int in_chans = 3;                                 // 1 = ViTSTR file (grey input, sequence head), from the patch kernel's shape
    int num_registers = 0;                            // R of an optional `reg_token` [1][R][D]: tokens between the class token and the patches
    int head_pool = VITX_POOL_CLS;                    // VITX_POOL_CLS_MEAN: head.weight is [C][2 D], over concat(cls, mean of the patch tokens);
                                                      // VITX_POOL_MAP: the thirteen attn_pool.* tensors, no cls_token, pos_embed of g^2 rows
    int activation = VITX_ACT_GELU_TANH;              // MLP activation, from an optional `arch` [4] = {activation, eps, 0, 0}; hp.eps carries its eps
    bool has_pre_norm = false;                        // `pre_norm.weight` / `pre_norm.bias` [D]: LayerNorm of every token row in front of layer 0
    int rope_kind = VITX_ROPE_NONE;                   // `rope` [4] = {kind, theta, 0, 0}: rotary position embeddings on q and k of the patch tokens (include/vitx.h)
    float rope_theta = 0.0f;
    int glu_kind = VITX_GLU_NONE;                     // `glu` [4] = {kind, F, 0, 0}: a gated MLP (include/vitx.h "gated MLP"); fc1 is then [2 F][D], fc2 [D][F]
    int glu_width = 0;                                // F, the MLP hidden width of such a file (fc2's K); 0 without `glu`: the width is 4 D
    int mlp_hidden() const { return glu_kind ? glu_width : 4 * hp.hidden_size; }          // F: fc2's K
    int mlp_fc1_rows() const { return glu_kind ? 2 * glu_width : 4 * hp.hidden_size; }    // F1: fc1's N
    bool has_preproc = false;                         // `preproc` [16]: the model's own preprocessing (include/vitx.h); without it `preproc` is the reference default
    vitx_preproc preproc;
    // a text-tower file (patch_size == 0; include/vitx.h "the text tower"): hp.img_size = T, hp.num_classes = E
    int kind = VITX_KIND_IMAGE;
    int vocab = 0;                                    // V, token_embed.weight's row count
    int causal = 0;                                   // arch[2]
    int eos = -1;                                     // arch[3] - 1: the EOS token id whose first position is pooled; -1: the last position
    bool has_zs = false;                              // `zs` [4] = {kind, scale, bias, 0}
    int zs_kind = 0;
    float zs_scale = 1.0f, zs_bias = 0.0f;
    std::map<int, std::string> id2label;
    std::vector<vitx::HostTensor> tensors;            // file order
    std::map<std::string, int> index;                 // name -> position
    const vitx::HostTensor *find(const std::string &n) const {
        auto it = index.find(n);
        return it == index.end() ? nullptr : &tensors[it->second];
    }
};

namespace vitx {
void set_error(const char *fmt, ...);
float f16_bits_to_f32(uint16_t h);
uint16_t f32_to_f16_bits(float f);     // round-to-nearest-even
uint16_t f32_to_bf16_bits(float f);    // round-to-nearest-even
// the `preproc` tensor (preprocess.cpp): the reference default at img_size; description <-> the 16 f32 slots (pp_from_slots: nullptr = fine,
// else what is wrong with the slots or the description)
vitx_preproc pp_default(int img_size);
void pp_to_slots(const vitx_preproc &p, float slots[16]);
const char *pp_from_slots(const float slots[16], vitx_preproc &p);
}  // namespace vitx
