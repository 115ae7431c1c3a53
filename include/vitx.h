/*
 * vitx.h -- C ABI of the MI355X-native ViT forward engine (libvitx.so).
 *
 * This is the drop-in boundary for the forward path of staghado/vit.cpp.  The
 * reference exposes three C++ entry points (vit.h:119-122):
 *     bool vit_model_load(const std::string&, vit_model&);                      vit.h:120
 *     bool vit_image_preprocess(const image_u8&, image_f32&, const vit_hparams&); vit.h:119
 *     int  vit_predict(const vit_model&, vit_state&, const image_f32,
 *                      const vit_params&, std::vector<std::pair<float,int>>&);  vit.h:122
 * The C++ mirror of those signatures lives in vit.cpp_amd/vit.h and is a thin
 * wrapper over the functions below (plain pointers and sizes, int status codes,
 * caller-owned output buffers, no exceptions across the ABI).  INTEGRATION.md
 * shows the binding a maintainer of the reference would add.
 *
 * Threading: a vitx_model is immutable after load and may be shared; a vitx_ctx
 * is per (thread, GPU) mutable scratch -- the analogue of vit_state (vit.h:72-80).
 */
#ifndef VITX_H
#define VITX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vitx_model vitx_model;
typedef struct vitx_ctx vitx_ctx;

enum vitx_status {
    VITX_OK = 0,
    VITX_ERR_IO = 1,          /* cannot open / short read                         (vit.cpp:312-317) */
    VITX_ERR_FORMAT = 2,      /* bad magic, unknown tensor, wrong shape or size   (vit.cpp:320-328, 618-685, 697-701) */
    VITX_ERR_ARG = 3,         /* NULL pointer, batch > max_batch, wrong image size (vit.cpp:757) */
    VITX_ERR_HIP = 4,         /* a HIP runtime call or kernel launch failed */
    VITX_ERR_UNSUPPORTED = 5, /* model shape the kernels do not cover */
    VITX_ERR_NOMEM = 6
};

/* Arithmetic type of the MFMA operands (accumulation, LayerNorm, softmax and the
 * residual stream are always f32).  F16 reproduces the reference's rounding points
 * (ggml rounds mul_mat activations to fp16); BF16 is the mode BASELINE.json names. */
enum vitx_dtype { VITX_F16 = 0, VITX_BF16 = 1, VITX_MXFP8 = 2 };

/* VITX_MXFP8 is EXPERIMENTAL: measured slower than VITX_BF16 on MI355X; VITX_BF16 stays the mode to use.
 * VITX_MXFP8 (vitx_ctx_create, vitx_ctx_create_ex, vitx_group_create, vit_state.dtype; the vitx_op_* entry points above VITX_MXFP8
 * take dtype 0 or 1 only -- MX has its own, below):
 *   qkv, fc1 and fc2 of every layer (the class-row tail of the last layer included) multiply MX operands, A and W, on the block-scaled
 *   MFMA.  Everything else is what a VITX_BF16 context computes: patch embedding, attention (on the bf16 q, k, v the qkv GEMM writes),
 *   proj + residual (its A operand comes from the attention kernels), the LayerNorm statistics, final norm, head, softmax and the f32
 *   residual stream.  LayerNorm fusion is off (vitx_ctx_ln_fusion_active returns 0): each LayerNorm is its own launch and writes MX.
 *   Hidden sizes that are not a multiple of 32: VITX_ERR_UNSUPPORTED at context creation (every context already requires a multiple of 64).
 * Block encoding: a block is 32 consecutive K elements of one row; elements are OCP e4m3fn (not fnuz); one E8M0 scale byte s per block;
 * a block decodes to q_i * 2^(s - 127).  For a block x in f32:
 *   a = max |x_i|; a == 0: s = 127 and every q_i = 0.  Otherwise a = m * 2^E with m in [1, 2), exact from the bits (f32 subnormals
 *   included); e = E - 8 if m <= 1.75, else E - 7 -- the smallest e with a * 2^-e <= 448; e is clamped to at least -127; s = e + 127;
 *   q_i = RNE_e4m3(x_i * 2^-e).  Nothing saturates or overflows; small values go to subnormals or zero by round-to-nearest-even.
 *   This deliberately differs from the OCP MX rule e = floor(log2 a) - 8, which clips the block maximum (1.75 * 2^8 = 448 is the
 *   largest e4m3 value, so blocks with m > 1.75 would saturate).
 * Stored layout: elements [rows][K_pad] bytes, scales [rows][K_pad / 32] bytes, K_pad = K rounded up to 128 (the MFMA's K step);
 * padding = zero elements with scale 127, written by the producers.
 * Rounding points: norm1 and norm2 outputs are encoded from the f32 LayerNorm value (the value a VITX_BF16 context rounds to bf16); the
 * fc1 output is encoded from f32 gelu_tanh(acc + bias) (ditto); the weights are encoded once at upload on the host from the file's f32
 * decode (vitx_model_tensor_f32), whatever the file type; the qkv output is bf16 and fc2 adds into the f32 residual stream. */

/* Interpolation of vit_image_preprocess (vit_hparams::interpolation, vit.h:30). */
enum vitx_interp { VITX_BICUBIC = 0, VITX_BILINEAR = 1 };

/* Mirrors vit_hparams (vit.h:20-37); eps is the LayerNorm epsilon of every norm of the model: 1e-6 unless the file carries an `arch` tensor
 * ("activation, epsilon and pre-norm" below). */
typedef struct vitx_hparams {
    int32_t hidden_size;
    int32_t num_hidden_layers;
    int32_t num_attention_heads;
    int32_t num_classes;
    int32_t patch_size;
    int32_t img_size;
    int32_t ftype;
    float eps;
} vitx_hparams;

const char *vitx_status_str(int status);
/* Thread-local description of the last error raised on this thread ("" if none). */
const char *vitx_last_error(void);

/* ---- model file (replaces vit_model_load, vit.cpp:308-712) ------------------ */
/* Parses the legacy-ggml ".gguf" file into host memory; validates magic, names,
 * shapes and byte sizes exactly where the reference does.  No GPU is touched. */
int vitx_model_load(const char *path, vitx_model **out);
void vitx_model_free(vitx_model *m);
/* Unique id of this load within the process (> 0; 0 for NULL).  A context cache must key on this, not on the pointer: a freed model's
 * address is routinely handed to the next vitx_model_load. */
uint64_t vitx_model_uid(const vitx_model *m);
int vitx_model_hparams(const vitx_model *m, vitx_hparams *out);
int vitx_model_num_labels(const vitx_model *m);
/* id2label lookup (vit.cpp:1065 uses .at(idx)); NULL when the id has no label. */
const char *vitx_model_label(const vitx_model *m, int class_id);
/* 3 for a ViT classifier file; 1 for a ViTSTR scene-text file (extensions/vitstr.cpp: the patch kernel is [P, P, 1, D],
 * vitstr.cpp:482).  vitx_model_seq_len: 0 for a classifier (one probability row per image: the cls token), 25 for ViTSTR
 * (the head reads tokens 0..24 of every image, vitstr.cpp:864-904: 25 probability rows per image). */
#define VITX_VITSTR_SEQ_LEN 25
int vitx_model_in_channels(const vitx_model *m);
int vitx_model_seq_len(const vitx_model *m);
/* ---- register tokens and the pooled head (DINOv2-class models) ---------------
 * Two optional extensions of the file, recognised by tensor name and shape; magic and the seven hparams are unchanged:
 *   `reg_token`   f32 [1][R][D], R >= 1 (ggml dims [D, R, 1]), written directly after cls_token: R learned register tokens that sit between
 *                 the class token and the patches and receive NO position embedding.  The file then holds 4 + 12 L + 4 + 1 tensors.
 *   `head.weight` of [C][2 D] instead of [C][D]: the DINOv2 linear head over concat(cls, mean of the patch tokens) of the final norm.
 * Any other type or shape of reg_token, or a head.weight whose rows are neither D nor 2 D long: VITX_ERR_FORMAT.  The reference's vit_model_load
 * cannot read a file with either extension (unknown tensor / wrong shape, vit.cpp:618-641) -- the models it cannot run are the only ones that
 * need them; files without them load and run exactly as before, bit for bit.
 * Token layout of an image, T = 1 + R prefix tokens, N = g^2 + T (vitx_ctx_tokens):
 *   row 0            cls_token + pos_embed[0]
 *   rows 1 .. R      reg_token[r]                      (no position embedding)
 *   rows T .. N-1    patch p + pos_embed[1 + p]        (raster order)
 * pos_embed keeps its [1 + g^2][D] shape (and is resampled as before: registers are untouched).  Token 0 is the class token everywhere; the
 * trace and the attention maps cover all N tokens (map index 0 = cls, 1 .. R = registers, T .. = patches); MEAN and TOKENS features cover the
 * patch rows T .. N-1 only -- registers are not exposed as features (DINOv2 discards them).
 * VITX_POOL_CLS_MEAN: the head GEMM's operand is Z[i] = RNE(F[0]) ‖ RNE(mean over t = T .. N-1 of F[t]), [2 D] in the operand type, F = the f32
 * final-norm rows defined under "image embeddings and token features", the mean in VITX_FEAT_MEAN's fixed order -- so with VITX_FEAT_CLS |
 * VITX_FEAT_MEAN on for the last layer (no VITX_FEAT_L2), RNE(feature) == the head operand bit for bit.  Such a context evaluates every row of
 * the last layer: it behaves exactly as, and is bit-identical to, one created with last_layer_all_rows = 1.  A class-token head with registers
 * keeps the class-rows-only last layer.  ViTSTR (one-channel) files with either extension, and VITX_MXFP8 contexts of such files, are
 * VITX_ERR_UNSUPPORTED at context creation.
 * LayerScale needs no slot: the converter folds it into attn.proj / mlp.fc2 (convert.py). */
enum vitx_head_pool { VITX_POOL_CLS = 0, VITX_POOL_CLS_MEAN = 1, VITX_POOL_MAP = 2 };
int vitx_model_num_registers(const vitx_model *m);   /* R; 0 without reg_token (and for NULL) */
int vitx_model_head_pool(const vitx_model *m);       /* enum vitx_head_pool, from head.weight's shape and the presence of attn_pool.* */
/* ---- no class token and the attention-pooling head (SigLIP-class models) --------
 * One more optional extension, recognised by the presence of the thirteen `attn_pool.*` tensors (timm's AttentionPoolLatent names; transformers'
 * SiglipMultiheadAttentionPoolingHead), written after norm.bias and before head.*: VITX_POOL_MAP.
 *   attn_pool.latent [1][1][D] f32; attn_pool.q.weight [D][D], .q.bias [D]; attn_pool.kv.weight [2 D][D], .kv.bias [2 D] (K rows first, then V);
 *   attn_pool.proj.weight [D][D], .proj.bias [D]; attn_pool.norm.weight, .norm.bias [D]; attn_pool.mlp.fc1.weight [4 D][D], .fc1.bias [4 D];
 *   attn_pool.mlp.fc2.weight [D][4 D], .fc2.bias [D].  Vectors are f32, matrices f32 or f16: they are never block-quantised (vitx_quantize_file
 *   copies all thirteen through byte for byte).
 * Such a file has NO cls_token and no reg_token, and its pos_embed is [1][g^2][D]: it holds 3 + 12 L + 2 + 13 + 2 tensors.  VITX_ERR_FORMAT:
 * attn_pool.* together with a class or register token (or a [C][2 D] head); a missing class token without attn_pool.*; a partial set, a wrong
 * shape or type, a duplicate; a pos_embed whose row count does not fit.  head.weight stays [C][D], over the pooled embedding e.
 * Token layout: an image is its g^2 patch rows, patch t + pos_embed[t]; N = g^2, T = vitx_model_num_prefix = 0.
 * Textbook definition, F[t] = the f32 final-norm row of token t (the F of "image embeddings and token features", unrounded), d = D / H:
 *   q = Wq latent + bq;  k_t = Wk F[t] + bk;  v_t = Wv F[t] + bv;  per head h: p_h = softmax_t(q_h . k_{t,h} / sqrt(d)), o_h = sum_t p_{h,t} v_{t,h};
 *   a = Wproj o + bproj;  e = a + fc2(act(fc1(LN(a)))) with the file's activation and eps.  e [D] is the pooled embedding.
 * What the engine evaluates (identical in exact arithmetic):
 *   at context creation, on the host, in double from vitx_model_tensor_f32's decode: u_h = Wk_h^T q_h / sqrt(d), stored as f32 [H][D]
 *     (vitx_model_pool_query returns it).  q_h . bk_h is constant over t and cancels in the softmax: kv.bias's K half never reaches the device;
 *   the pooling kernel (attention_pool.hip): s_{h,t} = u_h . F[t], p_h = softmax_t(s_h), M_h = sum_t p_{h,t} F[t], all in f32, M is [n][H][D];
 *   o_h = Wv_h RNE(M_h) + bv_h (RNE to the operand type, as every GEMM operand is rounded; uses sum_t p = 1): H launches of the short-M GEMM,
 *     head h reads M[:, h, :] and writes columns h d .. (h + 1) d;
 *   proj (a stays f32), LayerNorm, fc1 + activation, fc2 + residual on n rows through the GEMM dispatcher and the LayerNorm launcher; e stays f32;
 *   the head GEMM's operand is RNE(e).
 * A VITX_POOL_MAP context evaluates every row of the last layer, exactly as a VITX_POOL_CLS_MEAN context does.  Features: VITX_FEAT_CLS is the
 * f32 pooled embedding e (the last layer only: any other layer in the mask is VITX_ERR_ARG; RNE(e) equals the head operand bit for bit);
 * VITX_FEAT_MEAN and VITX_FEAT_TOKENS cover all N rows; VITX_FEAT_L2 applies as before.
 * VITX_ERR_UNSUPPORTED: ViTSTR files with the extension and VITX_MXFP8 contexts of such files (at context creation); vitx_attn_enable on such a
 * context (the maps are defined by the class-token row, which does not exist); a context at another img_size than the file's and
 * vitx_model_resize_file of such a file (the g^2-row position table has no resampling path yet). */
int vitx_model_num_prefix(const vitx_model *m);      /* tokens in front of the patches: 0 for a VITX_POOL_MAP file, 1 + R otherwise (0 for NULL) */
/* u [H][D] f32 of a VITX_POOL_MAP file (above); host only.  VITX_ERR_ARG for NULL or a file without the head. */
int vitx_model_pool_query(const vitx_model *m, float *out /* [H][D] */);
/* ---- activation, epsilon and pre-norm (HuggingFace ViT, timm, DINOv2, CLIP) ----
 * Two more optional extensions of the file, recognised by tensor name and shape; magic and the seven hparams are unchanged:
 *   `arch`         f32 [4] = {activation, eps, 0, 0}.  activation: enum vitx_activation, the function between mlp.fc1 and mlp.fc2
 *                  (0 ggml's tanh-GELU, 1 the erf GELU x Phi(x) of nn.GELU, 2 QuickGELU x sigmoid(1.702 x)); eps: the epsilon of EVERY LayerNorm of
 *                  the model, a finite f32 > 0, reported as vitx_hparams::eps.  Slots 2 and 3 are reserved and must be 0.  Without `arch` a file
 *                  means {0, 1e-6}: the reference's arithmetic, which is what such files have always run as.  The converter writes it first.
 *   `pre_norm.weight`, `pre_norm.bias`   f32 [D], both or neither: a LayerNorm (the model's eps) of every token row -- class and register rows
 *                  included -- after the patch embedding and before layer 0: CLIP's pre_layrnorm.  Written directly after pos_embed.
 * Any other type, shape or activation code, an eps that is not finite and positive, a non-zero reserved slot, a duplicate, or one pre_norm tensor
 * without the other: VITX_ERR_FORMAT.  The loader takes them anywhere in the file; vitx_quantize_file and vitx_model_resize_file copy them
 * through byte for byte.  The reference's vit_model_load cannot read a file with either (unknown tensor, vit.cpp:618-622); files without them load
 * and run exactly as before, bit for bit.
 * Rounding points of the activation are those of tanh-GELU for all three: VITX_F16 rounds the argument and the result to fp16 (ggml's fp16
 * tables: ggml_gelu, ggml_gelu_quick), VITX_BF16 rounds only the stored value.
 * With a pre-norm, stage 0 of the residual-stream trace is the stream that ENTERS layer 0, i.e. after the pre-norm.
 * A CLIP file's head is the bias-free visual projection: its logits are CLIP's image_embeds (L2-normalise them on the host, or
 * give the context a bank of text embeddings: "zero-shot classification" below), its "probabilities" mean nothing.
 * ViTSTR (one-channel) files with a pre-norm or an activation other than tanh-GELU, and VITX_MXFP8 contexts of a file whose activation is not
 * tanh-GELU, are VITX_ERR_UNSUPPORTED at context creation (eps and the pre-norm do work under VITX_MXFP8). */
enum vitx_activation { VITX_ACT_GELU_TANH = 0, VITX_ACT_GELU_ERF = 1, VITX_ACT_QUICK_GELU = 2 };
int vitx_model_activation(const vitx_model *m);      /* enum vitx_activation; 0 without `arch` (and for NULL) */
int vitx_model_has_pre_norm(const vitx_model *m);    /* 1 when the file carries pre_norm.weight / pre_norm.bias */
/* ---- each model's own preprocessing (CLIP, DINOv2, HuggingFace ViT, timm) ----
 * How the publisher's image processor turns a decoded u8 RGB image into the model's input: resize (stretch, or shortest edge with the aspect
 * kept), an optional square centre crop, mean / std.  The PIL filters are Pillow's Image.resize on u8 -- separable, antialiased, fixed-point
 * coefficients, u8 between the passes -- and are matched BIT FOR BIT, on the host and on the device (arithmetic below); the REF filters are the
 * reference's vit_image_preprocess (vitx_preprocess_u8), which is what a file without a description has always meant.
 *   SHORTEST_EDGE: the short side becomes resize_a, the long side (int)((double)(resize_a * long_src) / (double)short_src) -- truncated, as
 *     transformers and torchvision do (500 x 375 at 224 -> 298 x 224); the width is the short side when nx <= ny.
 *   Output: crop x crop, or resize_a x resize_b when crop == 0.  The outputs of a description are square: STRETCH without a crop needs resize_a == resize_b, and
 *     SHORTEST_EDGE needs a crop (vitx_preprocess_rect, "rectangular contexts" below, stretches to any out_w x out_h).
 *   Crop offset per axis, d = resized - crop: d / 2 for even d; odd d: (d - 1) / 2 with crop_round 0 (transformers' floor), d / 2.0 rounded half
 *     to even with crop_round 1 (torchvision CenterCrop).
 *   VITX_ERR_ARG: a crop larger than either resized side of the given source (padding is not offered), non-positive sizes (or any side above
 *     16384, a source side above 2^20), resize_b != 0 with SHORTEST_EDGE, a REF filter with anything but STRETCH and no crop, a non-square
 *     output, a mean255 that is not finite or a std255 that is not finite and positive, an unknown enum value.
 * Arithmetic of the PIL filters (csrc/preproc_resample.h: ONE definition for host and device; no FMA contraction).  Per axis, in = source
 * length, out = resized length, everything up to k_j in double:
 *   scale = (double)in / out;  fs = max(scale, 1.0);  support = S0 * fs (S0: bilinear 1.0, bicubic 2.0);  ss = 1.0 / fs
 *   target index o:  center = (o + 0.5) * scale;  first = max((int)(center - support + 0.5), 0);
 *     n = min((int)(center + support + 0.5), in) - first   (truncating casts);   w_j = f((j + first - center + 0.5) * ss), j = 0 .. n-1
 *     f bilinear: |x| < 1 ? 1 - |x| : 0;   f bicubic (a = -0.5): |x| < 1: ((a+2)|x| - (a+3))|x||x| + 1;  |x| < 2: (((|x|-5)|x| + 8)|x| - 4) a;  else 0
 *     ww = ((w_0 + w_1) + w_2) + ...;  ww != 0: w_j = w_j / ww;   k_j = w_j < 0 ? (int)(-0.5 + w_j * 4194304.0) : (int)(0.5 + w_j * 4194304.0)
 *   Per pixel and channel, int32: acc = 2^21 + sum_j px_j * k_j;  q = clamp(acc >> 22, 0, 255) (arithmetic shift).
 *   The horizontal pass runs first, over the source rows the vertical taps need, into a u8 intermediate; then the vertical pass.  An axis with
 *   in == out is skipped.  The crop window is a slice of the result: only its rows and columns are computed.
 *   out = ((float)q - mean255[c]) / std255[c] in f32 with IEEE division, HWC -- the form of the reference's normalisation.
 * File extension `preproc`: f32 [16] = {resize_mode, resize_a, resize_b, filter, crop, crop_round, mean255 r g b, std255 r g b, 0, 0, 0, 0}; the
 * integers are stored exactly, the four reserved slots must be 0.  Any other type or shape, a duplicate, an invalid description, an output side
 * other than hparams.img_size, or the tensor in a one-channel (ViTSTR) file: VITX_ERR_FORMAT.  The loader takes it anywhere in the file (the
 * converter writes it directly after `arch`); vitx_quantize_file copies it through byte for byte; vitx_model_resize_file writes the
 * vitx_preproc_at_size values.  The reference's vit_model_load cannot read such a file; files without it load, preprocess and run as before.
 *   vitx_model_preproc      the file's description; without the tensor the reference default {STRETCH, img_size, img_size, REF_BICUBIC, 0, 0,
 *                           the ImageNet mean255 / std255 of vitx_preprocess_u8}.  f32(255.0 * m) of the ImageNet mean / std equals those six
 *                           literals bit for bit, so a DINOv2 file normalises exactly as vitx_preprocess_u8 does.
 *   vitx_model_has_preproc  1 when the file carries the tensor.
 *   vitx_preproc_at_size    the description for a context at another img_size -- THIS LIBRARY'S convention (publishers define one size only):
 *                           crop' = img_size when a crop is set; every resize side becomes (2 * side * img_size + old) / (2 * old) in integers,
 *                           old = the old output side: the crop fraction is kept, rounded to nearest.  in == out is allowed.
 *   vitx_preprocess_ex      host: hwc u8 [ny][nx][3] -> out f32 [S][S][3], S = the output side; rows are split over host threads.  With a REF
 *                           filter it runs vitx_preprocess_u8's code with the description's mean / std: the default description gives its bits.
 *   vitx_preprocess_ex_device   the same for n images of one source size on device pointers, bit for bit; ONE launch, no scratch, only
 *                           enqueues on `stream`.  A workgroup owns a 32 x 8 tile of one image's output window and keeps its coefficients, a
 *                           staged source row per wave and the u8 intermediate of its tile in LDS, so the LDS need grows with the down-scale
 *                           factor: about 96 * (8 * scale_y + 2 * support_y) + 12 * (32 * scale_x + 2 * support_x) + 4 * (32 * taps_x + 8 * taps_y)
 *                           bytes, at most 64 KiB (a 4032 x 3024 source at shortest edge 256 needs about 26 KiB; a bicubic stretch of 8 x 576 to 8 x 8
 *                           is the limit).  Beyond it: VITX_ERR_UNSUPPORTED before any launch; the host path has no bound.
 *   vitx_preprocess_ex_device_supports   1 / 0 for that bound (0 also for an invalid description or source); no device call. */
enum vitx_pp_filter { VITX_PP_REF_BICUBIC = 0, VITX_PP_REF_BILINEAR = 1,   /* the reference's (vitx_preprocess_u8's two) */
                      VITX_PP_PIL_BILINEAR = 2, VITX_PP_PIL_BICUBIC = 3 }; /* Pillow Image.resize on u8 */
enum vitx_pp_resize { VITX_PP_STRETCH = 0, VITX_PP_SHORTEST_EDGE = 1 };
typedef struct vitx_preproc {
    int32_t resize_mode;   /* STRETCH: to resize_a (width) x resize_b (height); SHORTEST_EDGE: short edge = resize_a, resize_b = 0 */
    int32_t resize_a, resize_b;
    int32_t filter;
    int32_t crop;          /* side of the square centre crop; 0 = none */
    int32_t crop_round;    /* offset = d/2 for even d = resized - crop; odd d: 0 = floor (transformers), 1 = round half to even (torchvision CenterCrop) */
    float mean255[3], std255[3];   /* the f32 values the arithmetic uses: out = ((float)q - mean255[c]) / std255[c] */
} vitx_preproc;
int vitx_model_preproc(const vitx_model *m, vitx_preproc *out);
int vitx_model_has_preproc(const vitx_model *m);
int vitx_preproc_at_size(const vitx_preproc *in, int img_size, vitx_preproc *out);
int vitx_preprocess_ex(const vitx_preproc *pp, const uint8_t *hwc, int nx, int ny, float *out_hwc);          /* out: [S][S][3] */
int vitx_preprocess_ex_device(const vitx_preproc *pp, const void *d_hwc, int n, int nx, int ny, void *d_out_hwc, void *stream);
int vitx_preprocess_ex_device_supports(const vitx_preproc *pp, int nx, int ny);   /* 1 / 0, no device call */
int vitx_model_num_tensors(const vitx_model *m);
/* Name, file type code (0 f32,1 f16,2 q4_0,3 q4_1,6 q5_0,7 q5_1,8 q8_0), ggml-order dims. */
int vitx_model_tensor_info(const vitx_model *m, int index, const char **name, int32_t *type, int64_t ne[4], size_t *nbytes);
/* Decodes tensor `index` to f32 into out (n_elements floats).  Host only. */
int vitx_model_tensor_f32(const vitx_model *m, int index, float *out, size_t n_elements);

/* Re-encodes an f16/f32 model file with its 2-D "*weight" tensors in block format `ftype`
 * (2 q4_0, 3 q4_1, 6 q5_0, 7 q5_1, 8 q8_0), byte-identical to what the reference's offline
 * `quantize` tool writes (quantize.cpp:34-353: header ftype, label order, which tensors, block
 * encoders).  Host only.  VITX_ERR_ARG for another ftype, VITX_ERR_FORMAT if already quantised.
 * Files with the extensions above pass through: reg_token is copied, a [C][2 D] head is quantised like any 2-D "*weight", the thirteen
 * attn_pool.* tensors are copied byte for byte (the selection over the reference's own tensors stays the reference's). */
int vitx_quantize_file(const char *path_in, const char *path_out, int ftype);

/* ---- image files (replaces load_image_from_file = stbi_load(..., 3), vit.cpp:109-127) ---- */
/* Decodes a JPEG (baseline or progressive Huffman, 8-bit, gray or YCbCr), a non-interlaced PNG or a binary PPM into tightly
 * packed RGB u8 [ny][nx][3], top row first -- what stbi_load(fname, &nx, &ny, &nc, 3) hands the reference.  *out_rgb is
 * malloc'ed; release it with vitx_image_free.  VITX_ERR_IO if the file cannot be read, VITX_ERR_FORMAT if it cannot be decoded. */
int vitx_image_load(const char *path, uint8_t **out_rgb, int *nx, int *ny);
int vitx_image_decode(const uint8_t *bytes, size_t n_bytes, uint8_t **out_rgb, int *nx, int *ny);
void vitx_image_free(uint8_t *rgb);

/* ---- preprocess (replaces vit_image_preprocess, vit.cpp:289-305) ------------ */
/* u8 HWC RGB [ny][nx][3] -> f32 HWC [img_size][img_size][3], resized without
 * crop/antialias, rounded to u8, ImageNet mean/std normalised (vit.cpp:130-287). */
int vitx_preprocess_u8(const uint8_t *hwc, int nx, int ny, int img_size, int interp, float *out_hwc);

/* The same on the GPU for n images of one source size: d_hwc u8 [n][ny][nx][3] -> d_out f32
 * [n][img_size][img_size][3], both device pointers; only enqueues on `stream`.  Bit-identical
 * to vitx_preprocess_u8 (same operations in the same order, IEEE division, no FMA contraction). */
int vitx_preprocess_u8_device(const void *d_hwc, int n, int nx, int ny, int img_size, int interp, void *d_out_hwc, void *stream);

/* ViTSTR (extensions/vitstr.cpp) front and back end.  vitx_preprocess_vitstr_u8 replaces that extension's vit_image_preprocess
 * (vitstr.cpp:135-201): RGB u8 HWC -> grey (PIL weights, truncated to u8) -> direct linear resize to img_size^2 -> [-1, 1]; out is
 * ONE channel [img_size][img_size] f32 (nx, ny >= 2).  vitx_vitstr_decode replaces the greedy decode of its vit_predict
 * (vitstr.cpp:1025-1051) on one image's [seq_len][num_classes] probabilities: ids gets the classes of the characters (at most
 * seq_len - 1), *score the product of their probabilities; position 0 is skipped, class 1 ("[s]") ends the text. */
int vitx_preprocess_vitstr_u8(const uint8_t *hwc, int nx, int ny, int img_size, float *out_hw);
int vitx_vitstr_decode(const float *probs, int seq_len, int num_classes, int32_t *ids, int *n_ids, double *score);

/* ---- execution context (replaces vit_state + the per-call graph build) ------ */
/* Uploads the weights to `device` in `dtype` and allocates all activation scratch
 * for up to max_batch images once (the reference reallocates per call, vit.cpp:1009-1035).
 * Contexts for >= 16 images cut every batch into 2 contiguous sub-batches that run on two
 * internal HIP streams; the cut is placed where the GEMM tile counts of both parts fill whole
 * rounds of CUs (110 + 146 for 256 ViT-B images on 256 CUs).
 * Results do not depend on the split: images are independent in every kernel.
 * A non-finite value (NaN, Inf) in one image stays in that image's outputs: its batch neighbours keep the bits of a batch without it.
 * The library reads NO environment variable: everything tunable is in vitx_ctx_options. */
int vitx_ctx_create(const vitx_model *m, int device, int max_batch, int dtype, vitx_ctx **out);
/* Options of a context; every field 0 = the default.  Set struct_size = sizeof(vitx_ctx_options) (lets the struct grow).
 * They change HOW the forward is scheduled or where weights live, not what it computes -- except f16_fast_attention and last_layer_all_rows, which
 * select between two evaluations of the same graph that differ within the operand type's rounding (see the fields). */
typedef struct vitx_ctx_options {
    int32_t struct_size;
    int32_t streams;          /* sub-batch streams, 1..4 (default 2; contexts for fewer than 8 images per stream use 1) */
    int32_t graph;            /* 1: cache the single-stream (small-batch) forward as a hipGraph, captured the second time a call repeats */
    int32_t quant_on_host;    /* 1: expand block-quantised tensors once at upload (16 bits per weight in HBM) instead of keeping the blocks */
    int32_t q4_fused_rows;    /* q4_0 GEMMs with at most this many rows expand the blocks inside the GEMM's LDS-fill path (default 0 = never) */
    int32_t split_first;      /* with 2 streams: images of the first sub-batch (default 0 = the tile-round model decides) */
    int32_t no_ln_fusion;     /* 1: every LayerNorm runs as its own kernel (default: norm2 / the next norm1 ride in the proj / fc2 GEMMs) */
    int32_t ln_test;          /* parity tests only, honoured only as VITX_LN_TEST_KEY | mode (anything else is refused): mode 1 = every fifth tile of a LayerNorm-fusing GEMM behaves as if a peer had timed out, 3 = and withholds its
                                 statistics (real 50 us time-outs): the consumer-side fix-up must then give the same bits; | 4 = the forced fall-backs count against the
                                 fall-back budget (without it a test context keeps fusing whatever the count) */
    int32_t f16_fast_attention; /* VITX_F16 contexts: 1 = q, k, v rounded to fp16 for the attention products (the r03 behaviour: one QKV plane, the fast
                                 attention kernels) instead of the parity mode's f32-grade products (two fp16 planes, three MFMAs per product) */
    int32_t last_layer_all_rows; /* 1 = the last encoder layer computes every token row, as the reference graph does (vit.cpp:805-900 for il = L - 1).
                                 Default 0: past its qkv projection the last layer of a classifier carries only the class-token row of each image -- the only
                                 row vit.cpp:910-911 reads, and no other row can reach it (rows meet only through k and v inside the attention).  The
                                 probabilities are equal within the operand type's rounding (measured on 256 images: 1.1e-3 bf16, 3.0e-4 F16, top-1 equal), not
                                 bit for bit; 0.76 of one layer's work is not done (ViT-B: 6.3 % of the forward's flops).  ViTSTR contexts and contexts with a
                                 residual-stream trace always compute every row. */
    int32_t img_size;         /* 0 = the file's; else the side of the square input of THIS context, a positive multiple of patch_size: the context runs
                                 [n][img_size][img_size][3] images on (img_size / patch_size)^2 + 1 (+ the model's registers) tokens with the file's position table resampled on the
                                 device at creation (vitx_pos_embed_resample below).  Equal to the file's: today's context bit for bit, nothing is launched.
                                 Not a positive multiple of the patch size: VITX_ERR_ARG; a ViTSTR file at a size other than its own: VITX_ERR_UNSUPPORTED. */
    int32_t pos_interp;       /* enum vitx_pos_interp; used only when img_size differs from the file's (an unknown value is VITX_ERR_ARG in any case) */
} vitx_ctx_options;
#define VITX_LN_TEST_KEY 0x7e570000
int vitx_ctx_create_ex(const vitx_model *m, int device, int max_batch, int dtype, const vitx_ctx_options *options, vitx_ctx **out);
void vitx_ctx_free(vitx_ctx *c);
int vitx_ctx_max_batch(const vitx_ctx *c);
/* The geometry of THIS context (vitx_ctx_options::img_size): what vitx_forward expects is [n][img_size][img_size][3] (ViTSTR: one plane), and
 * N = (img_size / patch_size)^2 + 1 + R tokens (R = vitx_ctx_registers, the model's register tokens) size the trace and the attention maps;
 * the token features have N - 1 - R rows.  0 for NULL. */
int vitx_ctx_img_size(const vitx_ctx *c);      /* 0 also for a non-square context of vitx_ctx_create_rect (vitx_ctx_img_shape) */
int vitx_ctx_tokens(const vitx_ctx *c);
int vitx_ctx_registers(const vitx_ctx *c);
/* Probability rows per image that vitx_forward / vitx_forward_device write: 1 for a classifier ([n][num_classes]), 25 for a ViTSTR
 * file ([n][25][num_classes], row t = token t of the image; decode with vitx_vitstr_decode).  Images are then ONE grey channel:
 * [img_size][img_size] f32, as vitx_preprocess_vitstr_u8 emits. */
int vitx_ctx_out_rows(const vitx_ctx *c);
/* How a forward of n images is cut into contiguous sub-batches (one per internal stream): images[i] = size of sub-batch i, in image
 * order; returns the number of sub-batches (1 when the batch runs on one stream), 0 on a bad argument.  Results never depend on the
 * cut; the parity tests use it to pick the images on either side of every stream boundary.  A batch beyond the kernels' 32-bit buffer window
 * (ViT-B: 3326 images, 2217 in the F16 parity mode) runs as several passes through the same scratch: the cut reported is the first pass's. */
int vitx_ctx_split(const vitx_ctx *c, int n, int32_t *images, int max_parts);

/* Forward pass (replaces vit_encode_image + the compute half of vit_predict,
 * vit.cpp:718-941, 1028-1040) on n <= max_batch images.
 *   imgs_hwc : n x [img_size][img_size][3] f32, as vit_image_preprocess emits
 *   probs    : n x num_classes f32 class probabilities (state.prediction)
 *   logits   : optional (may be NULL), pre-softmax
 * vitx_forward takes host pointers (copies in/out and synchronises);
 * vitx_forward_device takes device pointers and only enqueues on `stream`
 * (a hipStream_t, NULL = the context's own stream).  One exception: the FIRST multi-stream forward of a context (>= 16 images)
 * synchronises the host once for ~0.2 ms while it measures whether its internal sub-batch stream really runs beside the caller's
 * stream (vitx_ctx_stream_retries); every later call, on this or any other caller stream, only enqueues. */
int vitx_forward(vitx_ctx *c, const float *imgs_hwc, int n, float *probs, float *logits);
int vitx_forward_device(vitx_ctx *c, const void *d_imgs_hwc, int n, void *d_probs, void *d_logits, void *stream);
int vitx_ctx_synchronize(vitx_ctx *c);

/* ---- contexts at another image size: the position table is resampled ------------ */
/* The file stores pos_embed for ONE grid, [1 + g^2][D] with g = img_size / patch_size (row 0 = class token, then the grid in raster order, x
 * fastest).  A context created with vitx_ctx_options::img_size keeps the model's weight matrices (contexts of one loaded model at different
 * sizes share ONE device copy: vitx_ctx_shares_weights, vitx_ctx_weight_bytes unchanged) and owns a table resampled to its own grid, computed
 * by the device kernel at creation from the f32 table already uploaded; the file's table is left as it is.  vitx_group_* has no options argument:
 * a group stays at the file's size.  Contexts of vitx_ctx_create_ex are square, those of
 * vitx_ctx_create_rect ("rectangular contexts" below) take any img_h x img_w; a size per call on one context is not offered.
 * Two conventions are in use and differ by 1e-3 .. 5e-2 on a trained table, so both are offered, each equal to CPU torch:
 *   VITX_POS_BICUBIC     torch.nn.functional.interpolate(mode="bicubic", align_corners=False, antialias=False) -- HuggingFace
 *                        interpolate_pos_encoding, DINO: cubic convolution with A = -0.75 on 4 x 4 taps, border indices clamped;
 *   VITX_POS_BICUBIC_AA  the same call with antialias=True -- timm resample_abs_pos_embed: separable, a = -0.5, the support widened by
 *                        max(in / out, 1), taps outside the grid dropped and the remaining weights normalised to sum 1.
 * Arithmetic, f32 throughout, the same operations in the same order on host and device with no FMA contraction, so both give the same bits.
 * Per axis (in source cells, out target cells, target index o), scale = (float)in / (float)out:
 *   BICUBIC     x = scale * ((float)o + 0.5f) - 0.5f; i0 = floorf(x); t = x - i0; taps i0 - 1 .. i0 + 2 clamped to [0, in - 1] with
 *               w0 = ((A u - 5A) u + 8A) u - 4A at u = t + 1;  w1 = ((A + 2) t - (A + 3)) t t + 1;  w2 = the w1 form at 1 - t;  w3 = the w0 form at 2 - t;
 *   BICUBIC_AA  support = scale >= 1 ? 2 scale : 2; inv = scale >= 1 ? 1 / scale : 1; center = scale * ((float)o + 0.5f);
 *               first = max((int)(center - support + 0.5f), 0); n = min((int)(center + support + 0.5f), in) - first (truncating casts);
 *               f_j = k(((float)(first + j) - center + 0.5f) * inv) with k(x) = ((a + 2)|x| - (a + 3))|x||x| + 1 for |x| < 1,
 *               (((|x| - 5)|x| + 8)|x| - 4) a for |x| < 2, else 0;  total = ((f_0 + f_1) + f_2) + ...;  w_j = f_j / total.
 * Per output cell and channel (horizontal first, then vertical, every sum from the first tap on):
 *   h_i = ((v(y_i, x_0) wx_0 + v(y_i, x_1) wx_1) + v(y_i, x_2) wx_2) + ...;   out = ((h_0 wy_0 + h_1 wy_1) + h_2 wy_2) + ...
 * Row 0 is copied bit for bit; equal grids are an exact copy in both conventions.  Grids may be rectangular in these two entry points.
 * NULL pointers, non-positive sizes, an unknown interp or a table of 2^31 floats or more: VITX_ERR_ARG.
 *   vitx_pos_embed_resample     host: pos f32 [1 + gy_in * gx_in][D] -> out f32 [1 + gy_out * gx_out][D];
 *   vitx_op_pos_embed_resample  the gfx950 kernel on device pointers, same arguments and bits; only enqueues on `stream`;
 *   vitx_model_resize_file      writes path_out = path_in with hparams.img_size = img_size and pos_embed resampled on the host; every other byte of
 *                               the file is copied through (quantised files included: pos_embed is always f32).  The result is an ordinary model
 *                               file: this library, the oracle and the reference's own vit_model_load read it (a file with reg_token or the
 *                               pooled head stays one only this library reads; reg_token is copied, pos_embed keeps 1 + g^2 rows; a `preproc` tensor is
 *                               rewritten with its vitx_preproc_at_size values).  img_size not a positive multiple
 *                               of the patch size, an unknown interp or path_out == path_in: VITX_ERR_ARG; a ViTSTR file at another size than its
 *                               own: VITX_ERR_UNSUPPORTED; an unreadable input: VITX_ERR_IO. */
enum vitx_pos_interp { VITX_POS_BICUBIC = 0, VITX_POS_BICUBIC_AA = 1 };
int vitx_pos_embed_resample(const float *pos, int gy_in, int gx_in, int D, int gy_out, int gx_out, int interp, float *out);
int vitx_op_pos_embed_resample(const void *d_pos, int gy_in, int gx_in, int D, int gy_out, int gx_out, int interp, void *d_out, void *stream);
int vitx_model_resize_file(const char *path_in, const char *path_out, int img_size, int interp);

/* ---- rectangular contexts: images of any height and width --------------------------- */
/* vitx_ctx_create_rect makes a context for [n][img_h][img_w][Cin] f32 HWC images: img_h and img_w positive multiples of patch_size (anything else:
 * VITX_ERR_ARG, before any device is touched), gh = img_h / patch_size, gw = img_w / patch_size, N = gh * gw + prefix tokens (vitx_ctx_tokens).  Patches
 * are in raster order, x fastest; the token features have gh * gw rows in that order, attention maps and rollout N columns, the trace N rows.
 *   Position table: the file's, resampled by the device kernel from (g_in, g_in) to (gh, gw) whenever the grids differ -- vitx_op_pos_embed_resample with
 *   its rectangular arguments, which is F.interpolate(size=(gh, gw), mode="bicubic", align_corners=False) for VITX_POS_BICUBIC (HuggingFace
 *   interpolate_pos_encoding); options->pos_interp as in a square context.  A file with `rope` builds vitx_model_rope_table(m, gh, gw, ..).
 *   `options` may be NULL; options->img_size must be 0 (VITX_ERR_ARG otherwise: the shape is the two arguments).  Every other option, quantised files,
 *   VITX_MXFP8 where a square context takes it, vitx_attn_enable, vitx_feat_enable, vitx_zeroshot_set, the trace and batches beyond the 32-bit buffer
 *   window work by the rules of a square context at another img_size.
 *   img_h == img_w == S is the context vitx_ctx_create_ex makes with img_size = S: the same launches, the same bits; at the file's own size nothing is
 *   resampled and the weight set is shared (vitx_ctx_shares_weights).
 *   A ViTSTR file, or a file with the attention-pooling head, at any shape other than the file's own: VITX_ERR_UNSUPPORTED.  vitx_group_* and
 *   vitx_model_resize_file stay square (the file format has one img_size).
 *   vitx_ctx_img_shape  img_h, img_w of any context;  vitx_ctx_grid  gh, gw of any context (VITX_ERR_ARG for NULL).
 *   vitx_ctx_img_size   the side of a square context and 0 for a non-square one: a caller that sizes S * S buffers fails loudly.
 * Preprocessing to a rectangle (the arithmetic is "each model's own preprocessing" above, per axis with in = nx, out = out_w and in = ny, out = out_h):
 *   vitx_rect_shape     the aspect-preserving shape, in integers: short_side a positive multiple of patch; with s = min(nx, ny), l = max(nx, ny):
 *                       long = ((int64)short_side * l / s) / patch * patch, capped at max_long when max_long != 0 (a multiple of patch, at least
 *                       short_side); the width is the short side when nx <= ny.  500 x 375, patch 16, short 224 -> 288 x 224 (an 18 x 14 grid).
 *                       Anything else, or a long side above 16384: VITX_ERR_ARG.
 *   vitx_preprocess_rect   host: the source stretched to out_w x out_h with the description's filter, mean255 and std255; no crop: resize_* and crop are
 *                       ignored, but the description must be valid.  out f32 [out_h][out_w][3].  out_w == out_h == S equals vitx_preprocess_ex with
 *                       {STRETCH, S, S, filter, 0, 0} bit for bit.  A REF filter: VITX_ERR_UNSUPPORTED (the reference's resize is defined for squares
 *                       only); sides outside 1 .. 16384 (source: 1 .. 2^20): VITX_ERR_ARG.
 *   vitx_preprocess_rect_device   the same for n images of one source size on device pointers, bit for bit: ONE launch of the PIL kernel with a
 *                       rectangular output window, the LDS bound of vitx_preprocess_ex_device (VITX_ERR_UNSUPPORTED beyond it, before any launch).
 *   vitx_preprocess_rect_device_supports   1 / 0 for that bound (0 also for an invalid description, a REF filter or bad sizes); no device call. */
int vitx_ctx_create_rect(const vitx_model *m, int device, int max_batch, int dtype, const vitx_ctx_options *options /* may be NULL; options->img_size must be 0 */,
                         int img_h, int img_w, vitx_ctx **out);
int vitx_ctx_img_shape(const vitx_ctx *c, int *img_h, int *img_w);
int vitx_ctx_grid(const vitx_ctx *c, int *gh, int *gw);
int vitx_rect_shape(int nx, int ny, int patch, int short_side, int max_long, int *out_w, int *out_h);
int vitx_preprocess_rect(const vitx_preproc *pp, const uint8_t *hwc, int nx, int ny, int out_w, int out_h, float *out_hwc);
int vitx_preprocess_rect_device(const vitx_preproc *pp, const void *d_hwc, int n, int nx, int ny, int out_w, int out_h, void *d_out_hwc, void *stream);
int vitx_preprocess_rect_device_supports(const vitx_preproc *pp, int nx, int ny, int out_w, int out_h);

/* ---- rotary position embeddings (DINOv3-class models) ---------------------------- */
/* A file may carry `rope`, f32 [4] = {kind, theta, 0, 0}: the position signal is then a rotation of q and k of the patch tokens in every layer, a
 * function of the grid and not a table.  kind 1 (VITX_ROPE_DINOV3_AXIAL, the only one) is DINOv3's: normalised patch-centre coordinates, half-split
 * rotation, prefix tokens (class token, registers) not rotated; theta is the base (100 for the published models).  The loader refuses
 * (VITX_ERR_FORMAT) any other kind, a theta that is not finite and positive, non-zero reserved slots, a head dim that is no multiple of 4, `rope` in
 * a text-tower file and `rope` together with attn_pool.*.  Such a file still carries a pos_embed of 1 + g^2 rows, ALL ZERO: the patch embedding, the
 * resampler and vitx_model_resize_file stay as they are (a resampled zero table is a zero table), at the price of 0.6 MB in a ViT-B file.
 * vitx_quantize_file and vitx_model_resize_file copy `rope` byte for byte.  A file without `rope` loads, runs and hashes exactly as before.
 * The table (host, double, once per context), hd = head dim, outputs [gh * gw][hd / 2], row-major over (y, x):
 *   cy = 2 (y + 0.5) / gh - 1, cx = 2 (x + 0.5) / gw - 1;  inv_j = theta^(-4 j / hd) for j < hd / 4;
 *   angle of column j < hd / 4: 2 pi cy inv_j;  of column hd / 4 + j: 2 pi cx inv_j;  cos / sin rounded once to f32.
 * (HuggingFace tiles these hd / 2 angles twice: columns j and j + hd / 2 of a head share one cos / sin.)  Grids may be rectangular here, as in the two
 * resampler entry points, and a rectangular context (vitx_ctx_create_rect) uses that.  A context of such a file builds the table for ITS grid (vitx_ctx_options::img_size,
 * or gh x gw of a rectangular context) at creation and
 * keeps it with the context, not in the shared weight set; so a context at another img_size is exact.  pos_interp is validated but has no effect.
 * The rotation (rope.hip), in place on the qkv GEMM's output, after that GEMM and before everything that reads q or k (attention, the class-row tail,
 * attention maps and rollout): for token t >= T (patch p = t - T), s in {q, k}, head h, j < hd / 2, a = element h hd + j, b = element h hd + hd / 2 + j,
 *   a' = a cos[p][j] - b sin[p][j];  b' = b cos[p][j] + a sin[p][j]
 * each product rounded to f32, then the sum (no FMA), the result rounded RNE to the operand type: bf16, one fp16 plane (f16_fast_attention), or the
 * parity mode's two fp16 planes (read as f32(hi) + f32(lo) / 2048, split again as the qkv GEMM splits: hi = RNE(v), lo = RNE((v - hi) 2048)).
 * v columns, prefix rows and rows beyond n_img * N keep their bits; every element has one writer, so the bits do not depend on the batch.
 * VITX_MXFP8 contexts of such a file: VITX_ERR_UNSUPPORTED at creation.  ViTSTR does not apply.  A context of a file without `rope` launches and
 * allocates nothing new.
 *   vitx_model_rope        1 and *kind / *theta (either may be NULL) for a file with `rope`, 0 without (and for NULL)
 *   vitx_model_rope_table  cos, sin f32 [gh * gw][hd / 2]; VITX_ERR_ARG for NULL, a file without `rope` or a non-positive grid
 *   vitx_op_rope           the gfx950 kernel on device pointers: d_qkv [n_img * N][3 D] of `dtype` (VITX_F16 / VITX_BF16), lo_off != 0: the lo plane that
 *                          many ELEMENTS behind (VITX_F16 only, a multiple of 8, at least n_img * N * 3 * D), d_cos / d_sin f32 [N - prefix][hd / 2].
 *                          Every check comes before the launch: NULL, non-positive sizes, prefix outside 0 .. N, a bad lo plane, both planes beyond
 *                          0xf0000000 bytes: VITX_ERR_ARG; D no multiple of H or an odd head dim: VITX_ERR_UNSUPPORTED.  Only enqueues on `stream`. */
enum vitx_rope_kind { VITX_ROPE_NONE = 0, VITX_ROPE_DINOV3_AXIAL = 1 };
int vitx_model_rope(const vitx_model *m, int *kind, float *theta);
int vitx_model_rope_table(const vitx_model *m, int gh, int gw, float *cos_out, float *sin_out);
int vitx_op_rope(int dtype, void *d_qkv, long lo_off, const void *d_cos, const void *d_sin, int n_img, int N, int prefix, int D, int H, void *stream);

/* ---- gated MLP (DINOv2 ViT-g/14, DINOv3 ViT-H+) ---------------------------------- */
/* A file may carry `glu`, f32 [4] = {kind, F, 0, 0}: the MLP of every block is then fc2( act(gate(x)) . up(x) ) with hidden width F instead of
 * fc2( act(fc1(x)) ) with hidden width 4 D.  kind 1 (VITX_GLU_SWIGLU, the only one): h = silu(gate) . up, silu(g) = g / (1 + exp(-g)).  With it every
 * blocks.i.mlp.fc1.weight is [2 F][D] -- rows 0 .. F-1 the gate projection, rows F .. 2F-1 the up projection: cat(gate_proj, up_proj), the order of
 * HuggingFace's weights_in.chunk(2) --, mlp.fc1.bias is [2 F] and mlp.fc2.weight is [D][F].  F is fc2's K: it must be a whole number, at least 64 and a
 * multiple of 64 -- the rule every GEMM family puts on K (the ring kernels step K in pairs of 32-deep slots, gemm_ring_supports; the ping-pong kernel
 * takes multiples of 128 and leaves the others to the ring), the same rule context creation puts on hidden_size.
 * The loader refuses (VITX_ERR_FORMAT) any other kind, such an F, non-zero reserved slots, a second `glu`, `glu` in a text-tower file and `glu`
 * together with attn_pool.*.  `glu` stands IN FRONT of the first blocks.* record (the loader sizes the records from the expected shapes as it reads;
 * the converter writes it directly after `arch` / `rope`); behind one it is VITX_ERR_FORMAT.  The activation slot of such a file's `arch` is carried
 * and not applied in the blocks.  vitx_quantize_file and vitx_model_resize_file copy `glu` byte for byte; fc1 and fc2 quantise like any matrix.
 * A file without `glu` loads, runs and hashes exactly as before.
 * The forward of such a file: fc1 with the plain bias epilogue into [rows][2 F], one launch of the gate kernel (swiglu.hip) into a compact [rows][F],
 * fc2 from that -- so fc2 sees lda == K and keeps whatever kernel family and LayerNorm fusion any other model's fc2 gets.  The class-rows-only last
 * layer takes the same three steps on the class rows.  The gate kernel widens g and u to f32, evaluates the sigmoid and both products in f32 and
 * rounds the product once (RNE) to the operand type.  Only STORED values are rounded, in both operand types: the fc1 output and the product.  The
 * reference has no gated MLP, so the F16 parity mode has no ggml rounding point (the fp16 activation table's argument) to honour here.  The result is
 * finite for every finite operand pair with a finite product: a large negative g gives -0, a large positive g gives g u.
 * VITX_MXFP8 contexts and ViTSTR (one-channel) contexts of such a file: VITX_ERR_UNSUPPORTED at creation.  A context of a file without `glu`
 * allocates and launches nothing new.
 *   vitx_model_glu   1 and *kind / *width (either may be NULL) for a file with `glu`, 0 without (and for NULL)
 *   vitx_op_swiglu   the gfx950 kernel on device pointers: d_in [rows][ld_in] of `dtype` (VITX_F16 / VITX_BF16), gate in columns 0 .. F-1, up in
 *                    F .. 2F-1; d_out [rows][ld_out], written in columns 0 .. F-1 and nowhere else.  Every check comes before the launch:
 *                    NULL, non-positive sizes, another dtype, F % 8, a leading dimension that is no multiple of 8, ld_in < 2 F, ld_out < F, a
 *                    pointer off a 16-byte boundary: VITX_ERR_ARG.  Only enqueues on `stream`. */
enum vitx_glu_kind { VITX_GLU_NONE = 0, VITX_GLU_SWIGLU = 1 };
int vitx_model_glu(const vitx_model *m, int *kind, int *width);
int vitx_op_swiglu(int dtype, const void *d_in, long ld_in, void *d_out, long ld_out, long rows, int F, void *stream);

/* ---- several GPUs in one process (north_star: batch shards + one RCCL gather) -- */
/* One context (replicated weights) and one PERSISTENT host thread per listed device (created here, parked between calls).  Images are
 * cut into contiguous shards, run concurrently, and the results are all-gathered with ONE ncclAllGather over RCCL.
 * The reference has no counterpart (single image, single device: vit.cpp:747).
 *   vitx_group_out_floats     floats per image in `probs`: num_classes, or 25 * num_classes for a ViTSTR file
 *   vitx_group_forward        n host images (f32 HWC, as vit_image_preprocess emits; ViTSTR: one grey plane each); the first n % n_devices
 *                             devices take one extra image; `probs` receives n x out_floats in image order
 *   vitx_group_forward_device the shards are ALREADY on their devices: d_imgs[r] = n_local[r] preprocessed images on devices[r]
 *                             (0 <= n_local[r] <= max_batch_per_device; NULL allowed where n_local[r] == 0).  Nothing crosses PCIe.
 *                             Afterwards EVERY device holds the gathered result of all shards -- vitx_group_result(g, r) is device r's
 *                             copy, vitx_group_result_rows() = n_max = the largest shard:
 *                               topk == 0: [n_devices][n_max][out_floats] f32 probabilities (rows beyond a shard's n_local are zero)
 *                               topk  > 0: [n_devices][n_max][rows_per_image][topk] pairs {f32 probability, i32 class}, descending,
 *                                          ties by the lower class (topk <= 16): 8 k bytes per row on the links instead of 4 num_classes
 *                             Synchronous (returns when every device's stream has finished). */
typedef struct vitx_group vitx_group;
int vitx_group_create(const vitx_model *m, const int *devices, int n_devices, int max_batch_per_device, int dtype, vitx_group **out);
void vitx_group_free(vitx_group *g);
int vitx_group_num_devices(const vitx_group *g);
int vitx_group_out_floats(const vitx_group *g);
int vitx_group_forward(vitx_group *g, const float *imgs_hwc, int n, float *probs);
int vitx_group_forward_device(vitx_group *g, const void *const *d_imgs, const int *n_local, int topk);
const void *vitx_group_result(const vitx_group *g, int device_index);
int vitx_group_result_rows(const vitx_group *g);

/* Sorted top-k of one probability row (vit.cpp:1043-1057: descending by prob, ties by the lower class; +0 and -0 tie).  Entries that are
 * NaN come after every other entry, by class: every index returned lies in [0, num_classes) and none repeats, whatever the row holds. */
int vitx_topk(const float *probs, int num_classes, int k, int32_t *out_idx, float *out_prob);

/* ---- measurement ------------------------------------------------------------ */
/* When enabled, every kernel launch of vitx_forward_device is bracketed by HIP
 * events on the launch stream and the sub-batches run back to back on that one
 * stream (exclusive per-kernel durations); vitx_profile_read() synchronises, folds
 * the event pairs into per-kernel-class totals and clears the pool. */
#define VITX_PROF_MAX_CLASSES 24
typedef struct vitx_prof_entry {
    const char *name;     /* kernel class, e.g. "gemm_fc1_gelu" */
    int32_t launches;
    double total_ms;
    double flops;         /* algorithmic 2*M*N*K summed over the launches (0 for non-GEMM classes) */
    double bytes;         /* algorithmic HBM bytes summed over the launches */
    double busy_ms;       /* wall time during which >= 1 launch of this class was running (union over the
                             context's concurrent sub-batch streams); == total_ms on a single stream */
} vitx_prof_entry;
/* Matrix-pipe probe: back-to-back v_mfma_f32_16x16x32 (the instruction of the GEMM kernels) on register operands on every CU for ~target_ms (no LDS, no memory);
 * dtype VITX_MXFP8: v_mfma_scale_f32_16x16x128_f8f6f4 on e4m3 operands with unit scales (the ceiling of the MX GEMMs).
 * fill 0 = zero operands, 1 = constant, 2 = uniform random in [-1, 1).  Returns TFLOP/s and the shader clock the device actually ran
 * at.  MI355X is power-capped on random operands (bf16 ~1830 of the nominal 2517 TFLOP/s): the roofline bench.py reports carries
 * this measured ceiling next to the nominal peak. */
int vitx_probe_mfma(int device, int dtype, int fill, double target_ms, double *tflops, double *clock_mhz);
int vitx_profile_enable(vitx_ctx *c, int on);
int vitx_profile_read(vitx_ctx *c, vitx_prof_entry *out, int max_entries, int *n_entries);
/* What one HIP-event bracket adds to a launch's duration, in microseconds (median of 32 brackets around a 20 us kernel that stamps its own
 * duration, queued back to back on the context's stream): vitx_profile_read() reports RAW event intervals; a caller that wants device-side
 * kernel durations subtracts launches x this (bench.py does, and says so in its line). */
int vitx_profile_bracket_us(vitx_ctx *c, double *bracket_us);

/* ---- single-kernel entry points (device pointers; used by the parity tests) - */
/* y[M][N] (dtype) = LayerNorm(x[M][D] f32) * w + b, eps inside the sqrt (vit.cpp:808-812). */
int vitx_op_layernorm(int dtype, const void *d_x, const void *d_w, const void *d_b, void *d_y, int M, int D, float eps, void *stream);
/* The same LayerNorm with the result left in f32, not rounded: y[M][D] f32 = ((x - mean) * rstd) * w + b, the value vitx_op_layernorm rounds (same
 * statistics, same operation order, every hidden size it covers).  d_y == d_x (in place) is allowed.  This is the pre-norm launch of a file
 * with pre_norm.*.  Only enqueues on `stream`; argument errors as vitx_op_layernorm. */
int vitx_op_layernorm_f32(const void *d_x, const void *d_w, const void *d_b, void *d_y, int M, int D, float eps, void *stream);
/* C = A[M][K] . W[N][K]^T with a fused epilogue; A, W in `dtype`.
 *   epi 0: out dtype  = acc + bias                  (vit.cpp:820-821)
 *   epi 1: out dtype  = gelu_tanh(acc + bias)       (vit.cpp:889-893)
 *   epi 6: out dtype  = gelu_erf(acc + bias)        (x Phi(x): VITX_ACT_GELU_ERF)   } the rounding points of epi 1: F16 rounds the argument
 *   epi 7: out dtype  = quick_gelu(acc + bias)      (x sigmoid(1.702 x): VITX_ACT_QUICK_GELU) } and the result, BF16 the result only
 *   epi 2: out f32    = (acc + bias) + out  in place (vit.cpp:868-873, 896-900)
 *   epi 3: out f32    = acc + bias                  (vit.cpp:927-928)
 *   epi 5: out dtype  = TWO planes of acc + bias: hi = round(v) at out[m][n], lo = round((v - hi) * 2048) at out[M * N + m * N + n]
 *                      (the parity mode's f32-grade q, k, v; vitx_op_gemm_ex only; `out` holds 2 * M * N elements)
 * M must be a multiple of 128 rows allocated; N, K multiples of 64. */
int vitx_op_gemm(int dtype, int epi, const void *d_a, const void *d_w, const void *d_bias, void *d_out, int M, int N, int K, void *stream);
/* The same with an explicit kernel family, so every production GEMM variant can be checked against a numeric reference:
 *   kernel 0 = automatic (what the forward would pick for this shape), 1 = ping-pong persistent 256x256 kernel (gemm_pp.hip),
 *   945 / 445 = ring kernels with 256x256 tiles (persistent / one workgroup per tile), 245 = 128x256, 122 = skinny 64x128,
 *   2 = the automatic choice with the tail split forced on (rows of a partial round re-tiled 128x256 in a second launch).
 * Adds epi 4 (patch embedding, vit.cpp:772-797): out f32 [M + M/tpi + 1 rows] : row m -> row m + m/tpi + 1, + d_pos[(m % tpi) + 1][n];
 * d_pos is [tpi + 1][N] f32 and is ignored by the other epilogues.  M_real <= M rows are stored (M is the padded row count).
 * d_w and d_bias must hold N rounded up to a multiple of 256 rows (zeros beyond N).
 * VITX_ERR_UNSUPPORTED when the chosen kernel cannot tile the shape. */
int vitx_op_gemm_ex(int dtype, int epi, int kernel, const void *d_a, const void *d_w, const void *d_bias, void *d_out, const void *d_pos,
                    int M, int M_real, int N, int K, int tpi, void *stream);
/* The residual GEMM with the LayerNorm that follows it computed in its epilogue (what proj + norm2 and fc2 + the next norm1 run as at
 * large batches): d_x f32 [M][N] += A . W^T + bias in place, d_y (dtype) [M][N] = ((x - mean) / sqrt(var + eps)) * ln_w + ln_b of the
 * updated rows.  M % 256 == 0, N in {256, 512, 768, 1024}, K % 128 == 0, at least 128 tiles of 256 x 256 (VITX_ERR_UNSUPPORTED otherwise).
 * test: 0; 1 = every fifth tile behaves as if a peer workgroup had timed out; 3 = and really withholds its statistics (its peers time out
 * after timeout_us microseconds) -- the fix-up launch must then produce the same bits.  Synchronous.  *fallbacks = tiles left to the fix-up. */
int vitx_op_gemm_ln(int dtype, const void *d_a, const void *d_w, const void *d_bias, void *d_x, const void *d_ln_w, const void *d_ln_b, void *d_y,
                    int M, int N, int K, float eps, int test, int timeout_us, int *fallbacks, void *stream);
/* Block-quantised weights on the device (reference: ggml keeps q4_0 ... q8_0 tensors in block form through compute,
 * vit.cpp:384-414, 645-678).  A context built from a quantised file keeps the blocks in HBM (vitx_ctx_weight_bytes reports the
 * footprint; vitx_ctx_options::quant_on_host expands once on the host instead) and expands them on the device:
 *   vitx_op_dequant : out[n_pad][K] (dtype) = expansion of N rows of K/32 blocks of type `qtype` (2 q4_0, 3 q4_1, 6 q5_0, 7 q5_1,
 *                     8 q8_0) laid out as in the file -- except q4_0: d_blocks = nibble plane [N][K/32][16 bytes],
 *                     d_scales = f16 block scales [N][K/32] (d_scales is ignored for the other types); rows N..n_pad are zeros.
 *                     Values are the reference's dequantize_row_* results rounded once (nearest-even) to dtype.
 *   vitx_op_gemm_q4 : C = A[M][K] . dequant(W)^T with the q4_0 blocks expanded in the GEMM's LDS-fill path; d_qs / d_scales as
 *                     above but with N rounded up to 128 rows (zero scales in the pad rows), epi 0..3, 6 and 7 as vitx_op_gemm. */
int vitx_op_dequant(int dtype, int qtype, const void *d_blocks, const void *d_scales, void *d_out, int N, int n_pad, int K, void *stream);
/* The same for njobs = 1..4 matrices of one block type in ONE launch, as the forward expands the qkv, proj, fc1 and fc2 matrices of a
 * layer (launch_dequant, quant.hip): job j takes d_blocks[j], d_scales[j] (d_scales may be NULL for every type but q4_0), d_out[j],
 * N[j], n_pad[j], K[j] under the rules above.  The arrays live on the host; the destinations must not overlap. */
int vitx_op_dequant_jobs(int dtype, int qtype, int njobs, const void *const *d_blocks, const void *const *d_scales, void *const *d_out,
                         const int *N, const int *n_pad, const int *K, void *stream);
int vitx_op_gemm_q4(int dtype, int epi, const void *d_a, const void *d_qs, const void *d_scales, const void *d_bias, void *d_out,
                    int M, int M_real, int N, int K, void *stream);
/* Device bytes held by the context's weight matrices (blocks for quantised tensors, 16-bit operands otherwise). */
size_t vitx_ctx_weight_bytes(const vitx_ctx *c);
/* Contexts of the same loaded model on the same device, with the same operand type and quantisation mode, share ONE device copy of the
 * weights (uploaded by the first, freed with the last: e.g. the two contexts that keep two forwards in flight).
 * 1 when this context attached to a copy that was already there, 0 when it uploaded it. */
int vitx_ctx_shares_weights(const vitx_ctx *c);
/* Diagnostic: GEMM tiles whose fused LayerNorm was left to the fix-up launch since the context was created (a peer workgroup did not
 * publish its row statistics in time -- possible when two such GEMMs on the context's two streams hold each other's CUs; results are
 * the same bits either way).  Synchronises the device.  -1 on error. */
long long vitx_ctx_ln_fallbacks(vitx_ctx *c);
/* Diagnostic: internal sub-batch streams the context re-created because a 40 us probe showed them serialised with the caller's stream
 * (the runtime's stream -> hardware-queue mapping depends on the other streams alive in the process).  0 in a fresh process. */
int vitx_ctx_stream_retries(const vitx_ctx *c);
/* Diagnostic: forwards this context enqueued by launching a cached hipGraph (vitx_ctx_options::graph) since it was created; -1 for NULL. */
long long vitx_ctx_graph_launches(const vitx_ctx *c);
/* 1 = norm2 / the next norm1 are computed in the proj / fc2 GEMMs' epilogues where the shape allows it (the default on an 8-XCD device); 0 = every
 * LayerNorm is its own launch (option no_ln_fusion, graph cache, a device that does not report 8 XCDs); -1 = the context switched the fusion off
 * itself because more than 8 tiles per forward (averaged over 16 forwards) had to fall back -- peers' CUs held by other work; it tries the fused
 * path again after a cool-down of 256 forwards (doubled on every further trip, at most 65536).  Same bits in all cases. */
int vitx_ctx_ln_fusion_active(const vitx_ctx *c);
/* out[n_img*N][D] (dtype) = softmax(q k^T / sqrt(64)) v per head from qkv[n_img*N][3D] (vit.cpp:826-866). */
int vitx_op_attention(int dtype, const void *d_qkv, void *d_out, int n_img, int N, int D, int H, void *stream);
/* kernel 0 = automatic, 1 = single-pass kernel (N <= 224, 257-288 or 577-608 tokens only),
 * 3 = pipelined two-pass kernel (any N; LDS-DMA double buffering, transposed LDS reads), 4 = persistent single-pass kernel (193..224
 * tokens: one workgroup per CU walks the (image, head) items, the next item's K/V land by LDS-DMA while the current one is computed).
 * F16: kernels 1 and 3 give bit-identical results (both apply the fp16 exp table relative to the TRUE row maximum).  BF16: they do not --
 * kernel 3 keeps a RUNNING maximum and rounds its numerators at another scale (equal within the numerators' bf16 rounding, 4e-3 relative in
 * the tests), and the automatic choice switches from kernel 1 / 4 to kernel 3 above 288 tokens: a bf16 result depends on the kernel family
 * the token count selects, not on the batch.  Kernel 4 issues v_mfma_f32_16x16x32 instead of 32x32x16 (same products, another accumulation
 * grouping: equal within f32 summation noise).
 * kernel 5 = streaming two-pass kernel (attention_stream.hip; any N, head dim 64: v_mfma_f32_16x16x32, 64-key chunks through a 3-slot LDS-DMA ring). */
int vitx_op_attention_ex(int dtype, int kernel, const void *d_qkv, void *d_out, int n_img, int N, int D, int H, void *stream);
/* Token 0 of every image only -- the one attention row the last layer of a classifier needs (vit.cpp:910-911): d_out [n_img][D] (dtype),
 * softmax(q_0 k^T / sqrt(head_dim)) v per head with f32 products and the same numerator rounding as the kernels above.  lo_off != 0: d_qkv is
 * the hi plane of the F16 parity mode and the lo plane lies lo_off elements behind it (multiple of 8; VITX_F16 only).  head_dim 8, 16, 32, 64, 128. */
int vitx_op_attention_cls(int dtype, const void *d_qkv, long lo_off, void *d_out, int n_img, int N, int D, int H, void *stream);
/* The F16 parity mode's attention on f32 q, k, v (the reference multiplies f32 operands, vit.cpp:848,858): d_qkv_f32 [n_img * N][3 D] f32 is
 * split into hi / lo fp16 planes (what the QKV GEMM's epi 5 emits) and every product is hi.hi + (hi.lo + lo.hi) / 2048.  d_out [n_img * N][D]
 * fp16.  Head dim 64.  TEST-ONLY entry point: it allocates and frees its own scratch and synchronises `stream` on every call. */
int vitx_op_attention_f32(const float *d_qkv_f32, void *d_out, int n_img, int N, int D, int H, void *stream);
/* The same kernel on planes that are already split (the output of vitx_op_gemm_ex epi 5): d_hi [n_img * N][3 D] fp16, the lo plane lo_off
 * ELEMENTS behind it (a multiple of 4, at least n_img * N * 3 D, both planes below 0xf0000000 bytes).  Only enqueues on `stream`. */
int vitx_op_attention_planes(const void *d_hi, long lo_off, void *d_out, int n_img, int N, int D, int H, void *stream);
/* probs[rows][cols] = softmax(logits[rows][ld]) over num_classes with the reference's fp16 exp rounding (vit.cpp:931); ld >= cols. */
int vitx_op_softmax(const void *d_logits, void *d_probs, int rows, int cols, int ld, void *stream);
/* The same with the rounding type of the exp explicit (VITX_F16 = the reference's LUT semantics, VITX_BF16 = the bf16 engine). */
int vitx_op_softmax_dt(int dtype, const void *d_logits, void *d_probs, int rows, int cols, int ld, void *stream);
/* The device-side top-k of vitx_group_forward_device (topk_kernel, softmax_topk.hip): d_pairs[rows][k] = {f32 probability, i32 class} of
 * d_probs[rows][cols] f32 in the order of vitx_topk; 0 < k <= cols.  Only enqueues on `stream`. */
int vitx_op_topk(const void *d_probs, int rows, int cols, int k, void *d_pairs, void *stream);

/* ---- residual-stream trace (parity localisation) ------------------------------ */
/* After vitx_trace_enable(ctx, ids, n) every forward also copies the f32 residual stream X of images ids[0..n) -- after the
 * patch embedding and after each encoder layer -- into a device buffer; vitx_trace_read() synchronises and returns it as
 * [L + 1][n][tokens][hidden] f32 (vit.cpp:797 and :900: the tensor `cur` carries between blocks).  n = 0 disables.
 * A traced context evaluates EVERY row of the last layer (as with last_layer_all_rows = 1): its probabilities are those of the whole graph and
 * can differ from the same context's untraced forward by the operand type's rounding (bf16 about 1e-3). */
int vitx_trace_enable(vitx_ctx *c, const int32_t *image_ids, int n);
int vitx_trace_read(vitx_ctx *c, float *out, size_t n_floats);

/* ---- attention maps and attention rollout (what the model looked at) --------- */
/* Opt-in outputs of the forward, for classifier contexts.  Notation for one image, layer l, head h, N tokens, hd = D / H:
 *   q, k  = the f32 values of the operands the context holds after that layer's qkv projection: the bf16 values (VITX_BF16); the fp16 values
 *           (VITX_F16 with f16_fast_attention, and every VITX_F16 context whose head dim is not 64: it has no parity mode); hi + lo * 2^-11 of
 *           the two planes of the F16 parity mode (VITX_F16, head dim 64, the default);
 *   s[i][j] = (q_i . k_j) / sqrt(hd) in f32;   A_h[i][j] = expf(s[i][j] - max_j s[i]) / sum_j (...)  with f32 expf.
 * The maps are f32 softmaxes of the context's own q, k -- NOT the numerators that multiply v (those use the reference's fp16 exp table or the
 * kernels' rounded numerators).
 *   class-token map of layer l:  A_h[0][0..N) for every head; index 0 is the class token itself, 1..N-1 the patches in raster order
 *     (a model with R register tokens: N includes them, 1..R are the registers, 1 + R.. the patches).
 *   rollout (Abnar & Zuidema 2020):  A^_l = 0.5 mean_h A_h + 0.5 I,  R = A^_(L-1) ... A^_0,  output = row 0 of R (length N; rows of R sum to 1).
 *     The last factor only ever needs row 0 of A^_(L-1), which is built from that layer's class-token maps -- so it is available when the last
 *     layer carries only the class rows (the default; see last_layer_all_rows) and gives the same bits with last_layer_all_rows = 1.
 * vitx_attn_enable(ctx, layer_mask, flags): bit l of layer_mask selects layer l's class-token maps, VITX_ATTN_ROLLOUT adds the rollout row;
 *   mask 0 and flags 0 = off (frees the buffers).  Buffers are sized for max_batch images and allocated here (VITX_ERR_NOMEM when that fails);
 *   rollout keeps two N x N f32 matrices per image and is VITX_ERR_UNSUPPORTED above 1024 tokens.  Mask bits at or beyond L: VITX_ERR_ARG.
 *   ViTSTR contexts: VITX_ERR_UNSUPPORTED.  Synchronises the device.
 * While maps are on, a forward of more than one pass (vitx_ctx_split) is VITX_ERR_ARG, and forwards do not use the hipGraph cache (as with the
 * trace); maps are written only by forwards made while they are on.  Turning them off launches nothing and allocates nothing: the forward
 * is the one without maps (probabilities and logits are the same bits with maps on and off).
 * vitx_attn_floats: floats per image = popcount(mask) * H * N + (rollout ? N : 0).  Layout per image: the selected layers in ascending order,
 *   each [H][N], then the rollout row [N].
 * vitx_attn_read: synchronises and copies the maps of the last forward's n images ([n][vitx_attn_floats] f32); VITX_ERR_ARG before any
 *   forward with maps on or when n_floats is too small.  vitx_attn_images: that n (0 before any forward with maps on since vitx_attn_enable).
 * vitx_op_attention_map: the kernels on their own (device pointers; only enqueues): d_cls [n_img][H][N] class-token maps, d_mean
 *   [n_img][N][N] mean_h A_h (N <= 1024); either may be NULL.  d_qkv [n_img * N][3 D] as the qkv projection writes it; lo_off != 0: the lo
 *   plane of the F16 parity mode lies lo_off elements behind (VITX_F16 only, a multiple of 8, at least n_img * N * 3 D).  head_dim: any
 *   multiple of 8 up to 128.
 * The three rollout kernels on their own (device pointers, f32 matrices; only enqueue; every check comes before the launch; N <= 1024, above
 * it VITX_ERR_UNSUPPORTED; a null pointer or n_img, N, H <= 0: VITX_ERR_ARG):
 *   vitx_op_rollout_factor: d_out [n_img][N][N] = A^ = 0.5 mean_h A_h + 0.5 I of d_qkv (arguments and checks of vitx_op_attention_map).  An
 *     entry is float(0.5) * m + float(0.5) * [i == j] in f32 with no contraction, m the entry vitx_op_attention_map's d_mean holds.
 *   vitx_op_rollout_step: d_a [n_img][N][N] <- d_a . d_r per image, in place over d_a (the forward's R_l = A^_l R_(l-1), f32 products and
 *     sums in an unspecified order).  d_r [n_img][N][N] is only read; ranges of d_a and d_r that overlap are VITX_ERR_ARG.
 *   vitx_op_rollout_row: d_out[b * out_stride + k] = sum_j w_j d_r[b][j][k] for k < N, with w_j = 0.5 mean_h d_cls[b * cls_stride + h * N + j]
 *     + 0.5 [j == 0] (row 0 of the last factor from that layer's class-token maps; the head sum in ascending h, times float(1 / H)); d_r NULL
 *     (a one-layer model): d_out = w.  Strides in floats; cls_stride < H * N or out_stride < N: VITX_ERR_ARG.  Nothing is written beyond
 *     the N floats of each output row. */
#define VITX_ATTN_ROLLOUT 1
int vitx_attn_enable(vitx_ctx *c, uint64_t layer_mask, int flags);
int vitx_attn_floats(const vitx_ctx *c);
int vitx_attn_images(const vitx_ctx *c);
int vitx_attn_read(vitx_ctx *c, float *out, size_t n_floats);
int vitx_op_attention_map(int dtype, const void *d_qkv, long lo_off, void *d_cls, void *d_mean, int n_img, int N, int D, int H, void *stream);
int vitx_op_rollout_factor(int dtype, const void *d_qkv, long lo_off, void *d_out, int n_img, int N, int D, int H, void *stream);
int vitx_op_rollout_step(void *d_a, const void *d_r, int n_img, int N, void *stream);
int vitx_op_rollout_row(const void *d_cls, long cls_stride, const void *d_r, void *d_out, long out_stride, int n_img, int N, int H, void *stream);

/* ---- image embeddings and token features (what retrieval, probes and dense heads read) --------- */
/* Opt-in outputs of the forward, for classifier contexts of every operand type (the residual stream is f32 in all of them).
 * For one image, a selected layer l, N tokens, hidden size D:
 *   X_l = the f32 residual stream after encoder layer l -- the tensor vitx_trace_read returns as stage l + 1 (vit.cpp:900);
 *   F_l = ((X_l - mean) * rstd) * norm.weight + norm.bias per row, in f32, with the model's FINAL norm (vit.cpp:915-919), eps inside the
 *         square root, the engine's own statistics (by 256-column tiles for D in {256, 512, 768, 1024}, over the whole row otherwise) and
 *         the operation order of its LayerNorm kernels.  F_l is NOT rounded to the operand type.
 *   For l = L - 1, row 0 of F_l is exactly the value the forward rounds (to nearest even) into the operand of the head GEMM: the embedding
 *   is what the classifier saw.  For l < L - 1 it is the "intermediate layer, norm applied" convention (DINO get_intermediate_layers(norm=True)).
 * Outputs (flags of vitx_feat_enable):
 *   VITX_FEAT_CLS     F_l[0], [D];
 *   VITX_FEAT_MEAN    (sum over t = T .. N-1 of F_l[t]) / (N - T), [D]: global average pooling over the patch tokens; the class token and the
 *                     register tokens are excluded (T = 1 + vitx_ctx_registers: 1 for a model without registers);
 *   VITX_FEAT_TOKENS  F_l[T .. N-1], [N-T][D], patches in raster order;
 *   VITX_FEAT_L2      modifier: the CLS and MEAN vectors are divided by their Euclidean norm (sum of squares and square root in f32; an
 *                     all-zero vector stays zero).  Tokens are never normalised.  Alone it is VITX_ERR_ARG.
 * Layout per image: the selected layers in ascending order; per layer [cls D], then [mean D], then [tokens (N-T) * D], only the selected parts.
 *   vitx_feat_floats = popcount(layers) * (D * [CLS] + D * [MEAN] + (N-T) * D * [TOKENS]).
 * Determinism: the pooled sum has a fixed order (one workgroup per image and layer, no atomics).  An image's feature bits do not depend on
 *   its batch, its position in the batch, the sub-batch cut or the number of streams -- the invariant the probabilities keep.
 * vitx_feat_enable(ctx, flags, layer_mask): bit l of layer_mask selects layer l; layer_mask 0 = the last layer only; flags 0 = off (frees
 *   the buffer).  The buffer is sized for the images one pass takes and allocated here (VITX_ERR_NOMEM when that fails).  Mask bits at or
 *   beyond L, unknown flags, VITX_FEAT_L2 alone: VITX_ERR_ARG.  ViTSTR contexts: VITX_ERR_UNSUPPORTED.  Synchronises the device.
 * The last layer:
 *   CLS only: the last layer still carries only the class rows (the default; see last_layer_all_rows): probabilities and logits are the same
 *     bits as with features off.
 *   MEAN or TOKENS of the last layer: while enabled, the context evaluates EVERY row of the last layer (as with last_layer_all_rows = 1): its
 *     probabilities are those of the whole graph and can differ from the same context's forward without features by the operand type's
 *     rounding (bf16 about 1e-3).  They are the bits of a last_layer_all_rows = 1 context.
 *   Intermediate layers never change the forward.
 * While features are on, a forward of more than one pass (vitx_ctx_split) is VITX_ERR_ARG, and forwards do not use the hipGraph cache (as
 *   with the trace and the maps); profiling reports the launches as class "features".  With features off nothing is launched or allocated.
 * vitx_feat_read: synchronises and copies the features of the last forward's n images ([n][vitx_feat_floats] f32); VITX_ERR_ARG before any
 *   forward with features on or when n_floats is too small.  vitx_feat_images: that n (0 before any such forward since vitx_feat_enable).
 * vitx_feat_device: the device buffer itself ([capacity][vitx_feat_floats] f32; NULL while off) for callers that stay on the GPU.  It is
 *   written by the forward's streams: work that reads it is ordered after the caller's stream, like d_probs.
 * vitx_op_features: the kernel on its own (device pointers; only enqueues).  Row t of image i is read at d_x + i * img_stride + t * row_stride
 *   (floats; the compact class rows of a class-rows-only last layer are N = 1, img_stride = D); d_w, d_b [D]; image i's outputs go to
 *   d_cls / d_mean / d_tokens + i * out_img_stride.  Any output may be NULL (at least one is not); row 0 is read only for d_cls, rows 1 .. N-1
 *   only for d_mean / d_tokens.  NULL inputs, n_img or N < 1, N == 1 with d_mean or d_tokens, pointers not 16-byte aligned or strides not
 *   multiples of 4 floats: VITX_ERR_ARG; a hidden size without a LayerNorm instantiation: VITX_ERR_UNSUPPORTED (both before any device call).
 * vitx_op_features_ex: the same with `first` = T, the first patch row (1 <= first <= N; vitx_op_features is first = 1): d_mean / d_tokens cover rows
 *   first .. N-1 ([N - first][D]), rows 1 .. first-1 are never read.  d_z != NULL: also the pooled head's operand (VITX_POOL_CLS_MEAN),
 *   d_z[i] = RNE(F[0]) ‖ RNE(mean) as [2 D] elements of `dtype` (VITX_F16 / VITX_BF16), rounded before any l2 -- the launch the forward of a
 *   pooled-head context makes (one launch serves the features and the head; profiling class "head_pool" when no feature of the last layer is on).
 * vitx_op_patch_embed: the forward's patch-embedding kernel on its own.  TEST ONLY: it allocates, uploads and synchronises.  d_img f32
 *   [n_img][S][S][Cin]; d_w f32 [D][Cin * P * P] in the file's (channel-major) order -- rounded to `dtype`, permuted and padded inside as the
 *   context does at upload; d_bias [D], d_pos [1 + (S/P)^2][D], d_cls [D], d_reg [R][D] (NULL when R == 0), all f32; d_X f32
 *   [n_img * ((S/P)^2 + 1 + R)][D] receives the token rows in the layout above and nothing beyond them.
 * vitx_op_features_ex also takes first = 0 (a model without prefix tokens: VITX_POOL_MAP): d_mean / d_tokens cover rows 0 .. N-1; d_cls and d_z
 *   are then VITX_ERR_ARG (there is no class row).  vitx_op_patch_embed takes d_cls == NULL with R == 0: no prefix row is written, patch t
 *   takes d_pos[t] (d_pos [(S/P)^2][D]) and d_X is [n_img * (S/P)^2][D].
 * vitx_op_attention_pool: the pooling kernel of a VITX_POOL_MAP head on its own (device pointers; only enqueues).  Row t of image i is read at
 *   d_x + i * img_stride + t * row_stride (floats); d_ln_w, d_ln_b [D] and eps are the final norm; d_u [H][D] f32; d_M [n_img][H][D] f32 receives
 *   M_h; d_p (may be NULL) [n_img][H][N] f32 receives p_h.  Every width of the LayerNorm table, 1 <= H <= 32, any N >= 1.  No atomics: an image's
 *   M is a function of its own rows, N, D and H only -- the same bits at any batch size and position.  NULL inputs, n_img, N < 1, H outside
 *   1 .. 32, pointers not 16-byte aligned or strides not multiples of 4 floats: VITX_ERR_ARG; a width without an instantiation: VITX_ERR_UNSUPPORTED. */
#define VITX_FEAT_CLS 1
#define VITX_FEAT_MEAN 2
#define VITX_FEAT_TOKENS 4
#define VITX_FEAT_L2 8
int vitx_feat_enable(vitx_ctx *c, int flags, uint64_t layer_mask);
int vitx_feat_floats(const vitx_ctx *c);
int vitx_feat_images(const vitx_ctx *c);
int vitx_feat_read(vitx_ctx *c, float *out, size_t n_floats);
const void *vitx_feat_device(const vitx_ctx *c);
int vitx_op_features(const void *d_x, long row_stride, long img_stride, const void *d_w, const void *d_b,
                     void *d_cls, void *d_mean, void *d_tokens, long out_img_stride,
                     int n_img, int N, int D, float eps, int l2, void *stream);
int vitx_op_features_ex(const void *d_x, long row_stride, long img_stride, const void *d_w, const void *d_b,
                        void *d_cls, void *d_mean, void *d_tokens, long out_img_stride,
                        int n_img, int N, int first, int D, float eps, int l2, void *d_z, int dtype, void *stream);
int vitx_op_patch_embed_rect(int dtype, const void *d_img /* [n][img_h][img_w][Cin] */, const void *d_w, const void *d_bias, const void *d_pos, const void *d_cls,
                             const void *d_reg, int R, int n_img, int img_h, int img_w, int P, int Cin, int D, void *d_X);   /* the same kernel on rectangular images (null stream) */
int vitx_op_patch_embed(int dtype, const void *d_img, const void *d_w, const void *d_bias, const void *d_pos, const void *d_cls, const void *d_reg, int R,
                        void *d_X, int n_img, int S, int P, int Cin, int D, void *stream);
int vitx_op_attention_pool(const void *d_x, long row_stride, long img_stride, const void *d_ln_w, const void *d_ln_b, float eps, const void *d_u, void *d_M,
                           void *d_p /* [n_img][H][N] or NULL */, int n_img, int N, int D, int H, void *stream);

/* ---- zero-shot classification (CLIP, SigLIP): a bank of class embeddings --------- */
/* An opt-in output of the forward, in the manner of the maps and the features.  A context is given a BANK: K unit-length class (text) embeddings
 * of width E, a kind, a scale and a bias; every forward then also writes [n][K] zero-shot logits and probabilities.  Nothing else the forward
 * writes changes (probabilities and logits are the same bits with a bank set and without); with no bank nothing is launched or allocated.
 * For one image, z = its f32 embedding of width E:
 *   a VITX_POOL_MAP context:          z = the pooled embedding e [D], the value VITX_FEAT_CLS returns (unnormalised); E = D = hidden_size;
 *   every other classifier context:   z = the f32 logits row [C] of the head GEMM -- image_embeds for a CLIP file; E = C = num_classes.  It is the row
 *                                     the caller gets in `logits`, computed whether or not the caller passes d_logits.
 * Per image:
 *   ss = sum z_i^2 in f32, in a fixed order that depends on E only; nrm = sqrtf(ss), IEEE.
 *   a_i = RNE_dtype(z_i / nrm), IEEE division; an all-zero z gives a = 0.  (VITX_FEAT_L2's rule.  The two are separate device functions: that
 *     one follows the LayerNorm tables' column ownership and exists for their widths only, this one takes any E that is a multiple of 64.)
 *   dtype = the context's operand type; a VITX_MXFP8 context uses bf16 here, as its head does.
 *   c_k = sum_i a_i * RNE_dtype(t_{k,i}), f32 accumulation on the MFMA: the bank GEMM is the head's GEMM dispatcher, so the forward's shape gets the
 *     family the dispatcher chooses.  t = the bank row as given: the engine does NOT renormalise it.
 *   l_k = c_k * scale + bias in f32: one multiply, one add, no contraction.
 *   VITX_ZS_SOFTMAX (CLIP):  p_k = expf(l_k - max_j l_j) / sum_j expf(l_j - max_j l_j), f32 expf, over the K real classes only (the sum: per thread of
 *     a 256-thread workgroup over k = t, t + 256, ... ascending, a butterfly over each wave's lanes, then the four waves in order).
 *   VITX_ZS_SIGMOID (SigLIP): p_k = 1 / (1 + expf(-l_k)), evaluated as written for l_k <= 0 and as 1 - 1 / (1 + expf(l_k)) for l_k > 0 -- the
 *     same function; the second form keeps the bits just below 1 that the first loses when 1 + expf(-l_k) rounds to 1 (16.7 < l_k < 17.3).
 *   scale = the multiplier itself, exp(logit_scale) of both publishers; it must be finite.
 * Determinism: an image's outputs are a function of its own z and the bank only -- the same bits at any batch size, position in the batch,
 *   sub-batch cut and stream count.
 * vitx_zeroshot_set(ctx, bank, K, E, kind, scale, bias): bank = host [K][E] f32.  Uploads it rounded (RNE) to the operand type and padded with
 *   zero rows to the GEMM's column tile (128), allocates the operand rows and the accumulator scratch of every sub-batch slice and the output
 *   buffer for the images one pass takes, synchronises the device.  Setting a bank again replaces it (new prompts need no new context);
 *   bank NULL and K 0 turn the output off and free the buffers.
 *   VITX_ERR_ARG: NULL bank with K > 0, K < 1 otherwise, E different from the context's embedding width, an unknown kind, a scale, bias or bank
 *     entry that is not finite.  VITX_ERR_UNSUPPORTED: a ViTSTR context; E not a multiple of 64 (the GEMMs' K step); K above
 *     vitx_zeroshot_max_classes(E) = the multiple of 128 below 0xf0000000 / (2 E): the padded bank must lie inside the 32-bit byte window the
 *     GEMM kernels address their operands with (E 512: 3 932 160 classes; the score kernel itself takes any K).  VITX_ERR_NOMEM: an allocation
 *     fails (the bank is then off).  All but the last are raised before any device call.
 * While a bank is set, a forward of more than one pass (vitx_ctx_split) is VITX_ERR_ARG, and forwards do not use the hipGraph cache (as with the
 *   maps and the features); profiling reports the three launches per sub-batch as class "zeroshot".
 * vitx_zeroshot_classes: K (0 while off).  vitx_zeroshot_images: the images of the last forward made with a bank set (0 before any since
 *   vitx_zeroshot_set).  vitx_zeroshot_read: synchronises and copies that forward's probabilities [n][K] and, unless NULL, logits [n][K];
 *   VITX_ERR_ARG before any such forward or when n_floats_each < n * K.
 * vitx_zeroshot_device: the device buffer itself, [capacity][2][K] f32 -- per image the probabilities, then the logits (NULL while off).  It is
 *   written by the forward's streams: work that reads it is ordered after the caller's stream, like d_probs.
 * vitx_group_* has no bank: a group computes probabilities only.
 * vitx_op_zeroshot: the three launches on their own (device pointers; only enqueues).  Row i of z is read at d_z + i * z_stride floats (z_stride
 *   >= E, a multiple of 4); d_bank [K_pad][E] in `dtype`, K_pad = K rounded up to 128, zero rows beyond K; d_a_scratch [n_pad][E] in `dtype`
 *   and d_acc_scratch [n_pad + 1][K_pad] f32 with n_pad = n rounded up to 256 (the last row becomes the GEMM's zero bias; pad rows of a are
 *   written as zeros, pad rows and columns of acc are neither written nor read); d_probs, d_logits [n][K] f32.  dtype VITX_F16 or VITX_BF16.
 *   NULL pointers, n, K, E < 1, an unknown kind, a scale or bias that is not finite, a bad z_stride, d_z, d_bank or scratch not 16-byte
 *   aligned: VITX_ERR_ARG; E not a multiple of 64 or K above vitx_zeroshot_max_classes(E): VITX_ERR_UNSUPPORTED (all before any device call). */
enum vitx_zs_kind { VITX_ZS_SOFTMAX = 0, VITX_ZS_SIGMOID = 1 };
int vitx_zeroshot_set(vitx_ctx *c, const float *bank /* host [K][E] f32 */, int K, int E, int kind, float scale, float bias);  /* bank NULL && K == 0: off, frees */
int vitx_zeroshot_classes(const vitx_ctx *c);        /* K; 0 while off */
int vitx_zeroshot_images(const vitx_ctx *c);
int vitx_zeroshot_read(vitx_ctx *c, float *probs /* [n][K] */, float *logits /* [n][K] or NULL */, size_t n_floats_each);
const void *vitx_zeroshot_device(const vitx_ctx *c); /* [capacity][2][K] f32: probs then logits per image; NULL while off */
int vitx_zeroshot_max_classes(int E);                /* the bound on K for width E (0 for an E that is not a positive multiple of 64) */
int vitx_op_zeroshot(int dtype, const void *d_z, long z_stride, const void *d_bank /* dtype, [K_pad][E], zero rows beyond K */,
                     void *d_a_scratch, void *d_acc_scratch, void *d_probs, void *d_logits, int n, int K, int E, int kind, float scale, float bias, void *stream);

/* ---- nearest neighbours in a gallery: device retrieval and weighted k-NN --------- */
/* An opt-in output of the forward, in the manner of the maps, the features and the bank.  A context is given a GALLERY: G embeddings of width E
 * (and, optionally, a label per row); every forward then also writes, per image, the k gallery rows with the best scores and -- with labels -- the
 * temperature-weighted vote of their labels (the DINO k-NN protocol: k = 20, T = 0.07).  Nothing else the forward writes changes; with no gallery
 * nothing is launched or allocated.  The gallery is walked in chunks: the scratch does not grow with G, and G is not bound by the GEMMs' 32-bit
 * operand window (only one chunk of it is).  For one image:
 *   source embedding z, width E = vitx_nn_width(ctx, source), a multiple of 64 (the GEMMs' K step):
 *     VITX_NN_LOGITS  the f32 logits row of the head GEMM, the z of the zero-shot path of a context without the attention-pooling head; E = C
 *                     (image_embeds of a CLIP file).
 *     VITX_NN_EMBED   the head GEMM's own operand row Z[i] widened to f32: RNE of the final-norm class embedding (class-token head, E = D), RNE(e) of
 *                     the pooled embedding (VITX_POOL_MAP, E = D), RNE(cls) ‖ RNE(patch mean) (VITX_POOL_CLS_MEAN, E = 2 D) -- the values the
 *                     "RNE(feature) == the head operand" rules above pin.  Z exists in every classifier forward: this source costs no feature pass
 *                     and leaves the class-rows-only last layer alone.  It is what a backbone converted without a head is searched by.
 *   query operand  a = RNE_dtype(z / sqrtf(ss)): the zero-shot rule unchanged (the same kernel text: the same sum-of-squares order, an all-zero row
 *     stays zero, a VITX_MXFP8 context uses bf16).
 *   gallery        host [G][E] f32 rows, uploaded RNE to the operand type, padded with zero rows to a multiple of 128.  The engine does NOT
 *     renormalise them (as for the bank); every entry must be finite.  labels: [G] i32 in [0, n_labels), or NULL.
 *   scores         s_g = sum_i a_i * t_{g,i}, f32 accumulation on the MFMA, through the head's GEMM dispatcher with a zero bias, one GEMM per chunk of
 *     Gc = 32768 gallery rows, each with its own base pointer into the gallery.  The bits of s_g depend on the image's a and on row g only.
 *   selection      the k best of the G scores in vitx_topk's total order: score descending, then gallery index ascending; +0 and -0 tie; NaN last, by
 *     index.  1 <= k <= 64, k <= G.  Output idx[k] i32 and score[k] f32, best first.  The result is a function of the G scores alone: not of the
 *     chunk size, nor of how a chunk is cut among wavefronts.  A score is returned as its place in the order names it: either zero as +0, any NaN as
 *     the quiet NaN 0x7fc00000, every other value bit for bit.  Pad rows of the gallery never reach the selection.
 *   vote (labels only)  T > 0 finite; w_j = expf((score_j - score_0) / T), f32 subtract, IEEE division; W = sum_j w_j serially over rank j = 0 .. k-1;
 *     vote[c] = (sum of w_j over the ranks j with label[idx_j] == c, serially in rank order) / W: a row of n_labels f32.  One writer per element.
 * Determinism: an image's outputs are the same bits at any batch size, position in the batch, sub-batch cut and stream count; the forward's
 *   probabilities and logits are the same bits with a gallery set and without; a bank and a gallery may both be set, neither changes the other.
 * vitx_nn_set: uploads the gallery (and labels), allocates per sub-batch slice the operand rows, one chunk's score scratch and the running top-k
 *   state -- none of them depends on G (vitx_nn_scratch_bytes) -- and the output buffers for the images one pass takes; synchronises the device.
 *   Setting again replaces the gallery; gallery NULL and G 0 turn the output off and free everything.
 *   VITX_ERR_ARG: NULL gallery with G > 0; an unknown source; k < 1 or k > G; E different from vitx_nn_width; a gallery entry that is not finite; a
 *     label outside [0, n_labels); labels with n_labels < 1 or with a temperature that is not finite and positive.  VITX_ERR_UNSUPPORTED: k > 64; E
 *     not a multiple of 64; a ViTSTR context; G >= 2^31 - 128; a context whose pass takes more than 30720 images (one chunk's score rows must lie
 *     inside the GEMM's 32-bit byte window).  VITX_ERR_NOMEM: an allocation fails (the gallery is then off).  All but the last
 *     are raised before any device call.
 * While a gallery is set, a forward of more than one pass is VITX_ERR_ARG and forwards do not use the hipGraph cache; profiling reports the
 *   2 ceil(G / Gc) + 2 launches per sub-batch (the operand rows, per chunk the GEMM and the selection, the final merge) as class "nn".
 * vitx_nn_read: synchronises and copies the last such forward's idx [n][k], score [n][k] and, unless NULL, vote [n][n_labels]; VITX_ERR_ARG before
 *   any such forward, or for a vote without labels.  vitx_nn_device: the device buffer, [capacity][k] {f32 score, i32 index} pairs (the layout
 *   vitx_op_topk writes), NULL while off.  vitx_group_* has no gallery.
 * The kernels on their own (device pointers; only enqueue):
 *   vitx_op_nn_select: merges columns 0 .. cols of d_scores [n][ld] f32 (column j = gallery row base_index + j; columns cols .. ld are never read)
 *     into d_state (vitx_op_nn_state_bytes(n, k) bytes, 8-byte aligned); first != 0: the state is initialised by this launch, not read.
 *   vitx_op_nn_finish: d_state -> d_pairs [n][k] and, d_labels != NULL, d_vote [n][n_labels]; d_labels must cover every index in the state.
 *   vitx_op_nn: the forward's launches without the vote.  Row i of z at d_z + i * z_stride elements: f32 (z_is_operand 0) or `dtype` (1); z_stride
 *     >= E, a multiple of 4.  d_gallery [G_pad][E] in `dtype`, G_pad = G rounded up to 128, zero rows beyond G; d_a_scratch [n_pad][E] `dtype`,
 *     d_acc_scratch [n_pad + 1][chunk] f32 with n_pad = n rounded up to 256 (the last row becomes the zero bias).
 *     VITX_ERR_ARG: NULL or misaligned (16 bytes) pointers, n, G, E < 1, k < 1 or k > G, a bad z_stride, chunk not a positive multiple of 128;
 *     VITX_ERR_UNSUPPORTED: k > 64, E not a multiple of 64, G >= 2^31 - 128, a chunk beyond the GEMM's operand window. */
enum vitx_nn_source { VITX_NN_LOGITS = 0, VITX_NN_EMBED = 1 };
int vitx_nn_width(const vitx_ctx *c, int source);     /* E of that source for this context; 0 for NULL / an unknown source */
int vitx_nn_set(vitx_ctx *c, const float *gallery /* host [G][E] */, long G, int E, int k, int source,
                const int32_t *labels /* [G] or NULL */, int n_labels, float temperature);   /* gallery NULL && G == 0: off, frees */
long vitx_nn_rows(const vitx_ctx *c);                 /* G; 0 while off */
int vitx_nn_k(const vitx_ctx *c);
int vitx_nn_labels(const vitx_ctx *c);                /* n_labels; 0 without labels */
int vitx_nn_images(const vitx_ctx *c);
int vitx_nn_read(vitx_ctx *c, int32_t *idx /* [n][k] */, float *score /* [n][k] */, float *vote /* [n][n_labels] or NULL */);
const void *vitx_nn_device(const vitx_ctx *c);        /* [capacity][k] {f32 score, i32 index}; NULL while off */
size_t vitx_nn_scratch_bytes(const vitx_ctx *c);      /* device bytes of score scratch + running state over all slices; 0 while off */
int vitx_op_nn_select(const void *d_scores /* [n][ld] f32 */, long ld, int n, int cols, long base_index, void *d_state, int k, int first, void *stream);
int vitx_op_nn_finish(const void *d_state, int n, int k, const void *d_labels, int n_labels, float temperature, void *d_pairs, void *d_vote, void *stream);
size_t vitx_op_nn_state_bytes(int n, int k);
int vitx_op_nn(int dtype, const void *d_z, long z_stride, int z_is_operand, int n, const void *d_gallery /* dtype [G_pad][E] */, long G, int E, int k, int chunk,
               void *d_a_scratch, void *d_acc_scratch /* [n_pad + 1][chunk] */, void *d_state, void *d_pairs, void *stream);

/* ---- dense prediction: a linear head over the patch tokens, label maps on the device --------- */
/* An opt-in output of the forward, in the manner of the bank and the gallery, with one result per PIXEL.  A context is given a linear HEAD over its
 * patch tokens (the form DINOv2's segmentation heads are published in: a 1 x 1 convolution over the final-norm tokens of the last layer, or of four
 * layers concatenated); every forward then also writes, per image, an [out_h][out_w] u8 label map and -- optionally -- the winner's score and the
 * patch-level logits.  Nothing else the forward writes changes; with no head nothing is launched or allocated.  For one image with grid gh x gw,
 * Np = gh gw patches, first patch row T, and the selected layers l_1 < ... < l_m (1 <= m <= 4; mask 0 = the last layer):
 *   operand      A[t] = RNE_dtype(F_{l_1}[T + t]) ‖ ... ‖ RNE_dtype(F_{l_m}[T + t]), width Dc = m D; F_l is the F_l of the features section above (the
 *     final norm applied, the engine's own statistics): RNE of the VITX_FEAT_TOKENS feature of the same forward, bit for bit.  Written by the stand-alone
 *     LayerNorm as each selected layer finishes, into compact rows [n Np][Dc] of the sub-batch (zero rows up to the GEMM's row tile).  dtype = the
 *     context's operand type; a VITX_MXFP8 context uses bf16, as its head does.  A selected last layer makes the context evaluate EVERY row of the last
 *     layer while the head is set (the rule of VITX_FEAT_TOKENS, with its consequence: probabilities and logits are those of a last_layer_all_rows = 1
 *     context, bit for bit).
 *   patch logits c[t][k] = bias_k + sum_i A[t][i] RNE_dtype(W[k][i]), f32 accumulation on the MFMA, through the head's GEMM dispatcher into [M_pad][K_pad]
 *     f32; K_pad = K rounded up to 128, weight rows beyond K are zero.  Profile class "dense".
 *   label map    the K planes c[.][k] resampled from gh x gw to out_h x out_w as F.interpolate(mode="bilinear", align_corners=False) does (mmseg's
 *     resize), then the arg-max over k < K.  Per axis (g source cells, out target cells, o the target index), all f32:
 *       scale = (float)g / (float)out (IEEE division);  s = ((float)o + 0.5f) * scale - 0.5f (one multiply, one subtract), clamped below at 0;
 *       i0 = (int)s;  i1 = i0 + (i0 < g - 1);  l = s - (float)i0;  h = 1.0f - l.
 *     Value, with a, b the taps (y0, x0), (y0, x1) and c, d the taps (y1, x0), (y1, x1):  top = hx a + lx b;  bot = hx c + lx d;  v = hy top + ly bot;
 *     every product and every sum rounded on its own, no FMA contraction (so 0 * inf is a NaN, as written).  The winner is the first entry of
 *     vitx_topk's total order: value descending, then class index ascending; +0 and -0 tie; a NaN ranks last (a pixel of NaNs only gets class 0).
 *     label[y][x] u8 = the winner;  VITX_DENSE_SCORE: score[y][x] f32 = the winner's v bit for bit (a NaN as the quiet NaN 0x7fc00000: the payload of
 *     a computed NaN is the processor's choice);  VITX_DENSE_LOGITS: the patch logits [Np][K] f32 are kept for vitx_dense_read.
 *     The weights and the value are ONE definition (csrc/dense_resample.h) for the device kernel and for vitx_dense_labels_host: the same bits on any data.
 * Determinism: an image's outputs are the same bits at any batch size, position in the batch, sub-batch cut and stream count; the forward's
 *   probabilities and logits are the bits of the same context with last_layer_all_rows = 1 and no head (of the same context, when the last layer is
 *   not selected); a bank, a gallery and a dense head may all be set, none changes another.
 * vitx_dense_set: W host [K][Dc] f32, bias [K] or NULL (zeros); uploads W rounded (RNE) to the operand type and padded, allocates per sub-batch slice
 *   the operand rows and the logit scratch (vitx_dense_scratch_bytes) and the output buffers for the images one pass takes; synchronises the device.
 *   Setting again replaces the head; W NULL and K 0 turn the output off and free everything.  out_h = out_w = 0: the context's own img_h x img_w.
 *   VITX_ERR_ARG: NULL W with K > 0; K < 1; Dc != popcount(mask) D; mask bits at or beyond L, or more than 4 of them; a W or bias entry that is not
 *     finite; unknown flags; a negative output side, or one side 0.  VITX_ERR_UNSUPPORTED: K > 256; a ViTSTR context; out_h < gh, out_w < gw or either
 *     above 8192 (upsampling only); a pass whose operand rows capacity Np Dc 2 or logit rows capacity Np K_pad 4 leave the GEMMs' 32-bit byte window
 *     (0xf0000000), or of more than 65535 images.  VITX_ERR_NOMEM: an allocation fails (the head is then off).  All but the last are raised before any
 *     device call.
 * While a head is set, a forward of more than one pass is VITX_ERR_ARG and forwards do not use the hipGraph cache; profiling reports the m operand
 *   launches, the GEMM and the label kernel of a sub-batch as class "dense".  vitx_group_* has no dense head.
 * vitx_dense_read: synchronises and copies the last such forward's labels [n][out_h][out_w] and, unless NULL, score (VITX_DENSE_SCORE) and logits
 *   [n][Np][K] (VITX_DENSE_LOGITS); VITX_ERR_ARG before any such forward or for an output the flags did not ask for.  vitx_dense_device: the labels
 *   on the device, [capacity][out_h][out_w] u8, NULL while off.
 * The kernel on its own (device pointers; only enqueues; every check before any device call):
 *   vitx_op_dense_labels: d_logits [n gh gw][ld] f32 (image, then patch in raster order; columns K .. ld are never compared: they may hold anything)
 *     -> d_labels [n][out_h][out_w] u8 and, unless NULL, d_score [n][..][..] f32.  VITX_ERR_ARG: NULL d_logits or d_labels, n, gh, gw, K < 1, d_logits
 *     off a 16-byte or d_score off a 4-byte boundary, ld below K rounded up to 4 or no multiple of 4; VITX_ERR_UNSUPPORTED: K > 256, an output smaller
 *     than the grid or above 8192, n > 65535.
 *   vitx_dense_labels_host: the same arguments on host pointers, the same bits; makes no device call (any alignment).
 *   vitx_op_dense: the forward's launches on a given operand: d_a [M_pad][Dc] in `dtype` with the n gh gw operand rows (M_pad = that rounded up to 256;
 *     the call zeroes the rows beyond them), d_w [K_pad][Dc] `dtype` (zero rows beyond K), d_bias [K_pad] f32 -> d_logits [M_pad][K_pad] f32 (scratch and
 *     output: the patch logits in its first K columns), then the labels as above.  VITX_ERR_ARG also for a dtype other than VITX_F16 / VITX_BF16 and any
 *     pointer off a 16-byte boundary; VITX_ERR_UNSUPPORTED also for Dc not a multiple of 64 and rows beyond the GEMM's byte window. */
enum vitx_dense_flags { VITX_DENSE_SCORE = 1, VITX_DENSE_LOGITS = 2 };
int vitx_dense_set(vitx_ctx *c, const float *W /* host [K][Dc] */, const float *bias /* [K] or NULL */, int K, int Dc, uint64_t layer_mask,
                   int out_h, int out_w, int flags);  /* W NULL && K == 0: off, frees */
int vitx_dense_classes(const vitx_ctx *c);            /* K; 0 while off */
int vitx_dense_shape(const vitx_ctx *c, int *out_h, int *out_w);   /* 0 x 0 while off */
int vitx_dense_images(const vitx_ctx *c);
int vitx_dense_read(vitx_ctx *c, uint8_t *labels /* [n][out_h][out_w] */, float *score /* or NULL */, float *logits /* [n][Np][K] or NULL */);
const void *vitx_dense_device(const vitx_ctx *c);     /* [capacity][out_h][out_w] u8; NULL while off */
size_t vitx_dense_scratch_bytes(const vitx_ctx *c);   /* device bytes of operand rows + logit scratch over all slices; 0 while off */
int vitx_op_dense_labels(const void *d_logits /* [n gh gw][ld] f32 */, long ld, int n, int gh, int gw, int K, int out_h, int out_w, void *d_labels, void *d_score, void *stream);
int vitx_dense_labels_host(const float *logits, long ld, int n, int gh, int gw, int K, int out_h, int out_w, uint8_t *labels, float *score);
int vitx_op_dense(int dtype, void *d_a /* [M_pad][Dc] */, const void *d_w /* [K_pad][Dc] */, const void *d_bias /* [K_pad] f32 */, void *d_logits /* [M_pad][K_pad] f32 */,
                  int n, int gh, int gw, int K, int Dc, int out_h, int out_w, void *d_labels, void *d_score, void *stream);

/* ---- depth estimation: a binned linear head over patch and class tokens, depth maps on the device --------- */
/* An opt-in output of the forward beside the dense head, for the other family of linear heads DINOv2 is published with (mmseg's BNHead-style depth
 * head with classify = True, norm_strategy = "linear": a 1 x 1 convolution to K depth BINS over concat(patch token, class token) of one or four
 * layers, the tokens upsampled x 4 first).  Every forward then also writes, per image, an [out_h][out_w] f32 depth map.  Nothing else the forward
 * writes changes; with no head nothing is launched or allocated.  For one image with grid gh x gw, Np = gh gw patches, first patch row T, and the
 * selected layers l_1 < ... < l_m (1 <= m <= 4; mask 0 = the last layer):
 *   operand rows  A[t] = RNE_dtype(G_{l_1}[T + t]) ‖ ... ‖ RNE_dtype(G_{l_m}[T + t]), width Dc = m D, compact rows [n Np][Dc] of the sub-batch; with a
 *     class half Wc also a_cls = RNE(G_{l_1}[0]) ‖ ... ‖ RNE(G_{l_m}[0]), one row per image.  G_l = X_l, the raw f32 residual stream after layer l (what
 *     vitx_trace_read returns as stage l + 1), written by a streaming conversion kernel; under VITX_DEPTH_NORM G_l = F_l, the features section's
 *     final-norm value bit for bit, written by the stand-alone LayerNorm as the dense head's rows are.  dtype = the context's operand type; a
 *     VITX_MXFP8 context uses bf16.  A selected last layer makes the context evaluate EVERY row of the last layer while the head is set (the rule of
 *     VITX_FEAT_TOKENS, with its consequence: probabilities and logits are those of a last_layer_all_rows = 1 context, bit for bit).
 *   patch logits  c[t][k] = sum_i A[t][i] RNE_dtype(Wp[k][i]), f32 accumulation on the MFMA, through the head's GEMM dispatcher into [M_pad][K_pad] f32
 *     with a bias of zeros; K <= 256, K_pad = K rounded up to 128, weight rows beyond K are zero.
 *   offsets       o[img][k] = bias_k + sum_i a_cls[i] RNE_dtype(Wc[k][i]): one GEMM of the n class rows through the same dispatcher.  Without Wc
 *     o[img] = bias for every image and no GEMM is launched.
 *   fine plane    fh = u gh, fw = u gw, u = `upsample` in {1, 2, 4}.  For the fine cell (y, x): the axes and the value v_k of the dense-prediction
 *     section (scale = g / (u g)), its four taps being c[cell][k] + o[img][k] (one rounded add per tap); then for k ascending from 0, S = Tm = 0
 *     before the first, all f32, every operation rounded on its own:
 *       r = v_k < 0 ? 0 : v_k (a NaN stays a NaN);  p = r + 0.1f;  S = S + p;  q = p * bins[k];  Tm = Tm + q;      fine[y][x] = Tm / S (IEEE division).
 *     This is relu, + 0.1, the division by the sum and the expectation over the bin centres, with the division moved behind the sums and the
 *     upsampling moved behind the convolution (both linear, the weights sum to 1: equal in real arithmetic).
 *   depth map     d = the value of `fine` resampled from fh x fw to out_h x out_w with the same axis arithmetic, then
 *     d < min_depth ? min_depth : (d > max_depth ? max_depth : d).  A NaN -- in the fine plane and in the depth map -- is written as the quiet NaN
 *     0x7fc00000.  Output [n][out_h][out_w] f32.  The step, the quotient and the clamp are ONE definition (csrc/depth_bins.h) for the device kernels
 *     and for vitx_depth_host: the same bits on any data.
 * Determinism: an image's outputs are the same bits at any batch size, position in the batch, sub-batch cut and stream count; the forward's
 *   probabilities and logits are the bits of the same context with last_layer_all_rows = 1 and no head (of the same context, when the last layer is
 *   not selected); a bank, a gallery, a dense head and a depth head may all be set, none changes another.
 * vitx_depth_set: Wp host [K][Dc] f32, Wc [K][Dc] or NULL (no class half), bias [K] or NULL (zeros), bins [K] the bin centres; uploads the matrices
 *   rounded (RNE) to the operand type and padded, allocates per sub-batch slice the operand rows and the logit scratch (vitx_depth_scratch_bytes) and
 *   the output buffers for the images one pass takes; synchronises the device.  Setting again replaces the head; Wp NULL and K 0 turn the output off
 *   and free everything.  out_h = out_w = 0: the context's own img_h x img_w.  flags: VITX_DEPTH_NORM (above); VITX_DEPTH_LOGITS: the patch logits
 *   [Np][K] and the offsets [K] of every image are kept for vitx_depth_read; VITX_DEPTH_FINE: vitx_depth_read may return the fine plane.
 *   VITX_ERR_ARG: NULL Wp with K > 0, NULL bins; K < 1; Dc != popcount(mask) D; mask bits at or beyond L, or more than 4 of them; a Wp, Wc, bias or
 *     bins entry that is not finite; a bin <= 0; min_depth > max_depth or either not finite; unknown flags; a negative output side, or one side 0.
 *   VITX_ERR_UNSUPPORTED: K > 256; upsample not 1, 2 or 4; out_h < fh, out_w < fw or either above 8192; Wc on a context without a class token
 *     (VITX_POOL_MAP); a ViTSTR context; a pass whose operand rows or logit rows leave the GEMMs' 32-bit byte window (0xf0000000), or of more than
 *     65535 images.  VITX_ERR_NOMEM: an allocation fails (the head is then off).  All but the last are raised before any device call.
 * While a head is set, a forward of more than one pass is VITX_ERR_ARG and forwards do not use the hipGraph cache; profiling reports every launch
 *   of the feature as class "depth".  vitx_group_* has no depth head.
 * vitx_depth_read: synchronises and copies the last such forward's depth [n][out_h][out_w] and, unless NULL, fine [n][fh][fw] (VITX_DEPTH_FINE),
 *   logits [n][Np][K] and offsets [n][K] (VITX_DEPTH_LOGITS); VITX_ERR_ARG before any such forward or for an output the flags did not ask for.
 *   vitx_depth_device: the depth maps on the device, [capacity][out_h][out_w] f32, NULL while off.
 * The kernels on their own (device pointers; only enqueue; every check before any device call):
 *   vitx_op_depth_fine: d_logits [n gh gw][ld] f32 (image, then patch in raster order; columns K .. ld never reach a sum: they may hold anything),
 *     d_offsets [n][ld] f32 or NULL (nothing is added), d_bins [K] -> d_fine [n][u gh][u gw] f32.  VITX_ERR_ARG: a NULL pointer but d_offsets, n, gh, gw,
 *     K < 1, d_logits or d_offsets off a 16-byte boundary, ld below K rounded up to 4 or no multiple of 4; VITX_ERR_UNSUPPORTED: K > 256, u not in
 *     {1, 2, 4}, n > 65535, a fine side above 8192.
 *   vitx_op_depth_resize: d_fine [n][fh][fw] -> d_out [n][out_h][out_w] f32 (any 4-byte alignment), clamped.  VITX_ERR_ARG: a NULL pointer, a side
 *     < 1, a range that is not finite or not ordered; VITX_ERR_UNSUPPORTED: an output smaller than the plane or above 8192, n > 65535.
 *   vitx_depth_host: the two on host pointers (offsets [n][ld] or NULL), the same bits; fine unless NULL; makes no device call (any alignment).
 *   vitx_op_depth: the forward's launches on given operands: d_a [M_pad][Dc] in `dtype` with the n gh gw patch rows (M_pad = that rounded up to 256;
 *     the call zeroes the rows beyond them), d_wp [K_pad][Dc] (zero rows beyond K); d_acls [n_pad][Dc] (n_pad = n rounded up to 256) and d_wc
 *     [K_pad][Dc], both or neither; d_bias [K_pad] f32, d_bins [K] -> d_logits [M_pad + 1][K_pad] f32 (scratch and output: the patch logits in its first
 *     K columns; the last row is the zero bias the call writes), d_offsets [n_pad][K_pad] f32 (class half only), d_fine, d_depth.  VITX_ERR_ARG also for a
 *     dtype other than VITX_F16 / VITX_BF16 and a pointer off a 16-byte boundary (d_depth: 4); VITX_ERR_UNSUPPORTED also for Dc not a multiple of 64 and
 *     rows beyond the GEMM's byte window.
 *   vitx_op_depth_rows: the raw operand rows: d_y[row][0 .. D) in `dtype` (row stride ldy elements) = RNE(d_x[row][0 .. D)) (f32, row stride ldx). */
enum vitx_depth_flags { VITX_DEPTH_NORM = 1, VITX_DEPTH_LOGITS = 2, VITX_DEPTH_FINE = 4 };
int vitx_depth_set(vitx_ctx *c, const float *Wp /* host [K][Dc] */, const float *Wc /* host [K][Dc] or NULL */, const float *bias /* [K] or NULL */,
                   const float *bins /* [K] */, int K, int Dc, uint64_t layer_mask, int upsample, float min_depth, float max_depth,
                   int out_h, int out_w, int flags);  /* Wp NULL && K == 0: off, frees */
int vitx_depth_bins(const vitx_ctx *c);               /* K; 0 while off */
int vitx_depth_shape(const vitx_ctx *c, int *out_h, int *out_w, int *fine_h, int *fine_w);   /* 0 while off */
int vitx_depth_images(const vitx_ctx *c);
int vitx_depth_read(vitx_ctx *c, float *depth /* [n][out_h][out_w] */, float *fine /* [n][fh][fw] or NULL */, float *logits /* [n][Np][K] or NULL */,
                    float *offsets /* [n][K] or NULL */);
const void *vitx_depth_device(const vitx_ctx *c);     /* [capacity][out_h][out_w] f32; NULL while off */
size_t vitx_depth_scratch_bytes(const vitx_ctx *c);   /* device bytes of operand rows + logit scratch over all slices; 0 while off */
int vitx_op_depth_fine(const void *d_logits /* [n gh gw][ld] f32 */, long ld, const void *d_offsets /* [n][ld] or NULL */, const void *d_bins /* [K] */,
                       int n, int gh, int gw, int K, int upsample, void *d_fine, void *stream);
int vitx_op_depth_resize(const void *d_fine, int n, int fh, int fw, int out_h, int out_w, float min_depth, float max_depth, void *d_out, void *stream);
int vitx_depth_host(const float *logits, long ld, const float *offsets, const float *bins, int n, int gh, int gw, int K, int upsample, int out_h, int out_w,
                    float min_depth, float max_depth, float *depth, float *fine /* or NULL */);
int vitx_op_depth(int dtype, void *d_a /* [M_pad][Dc] */, const void *d_wp /* [K_pad][Dc] */, void *d_acls /* [n_pad][Dc] or NULL */, const void *d_wc /* or NULL */,
                  const void *d_bias /* [K_pad] f32 */, const void *d_bins /* [K] */, void *d_logits /* [M_pad + 1][K_pad] f32 */, void *d_offsets /* [n_pad][K_pad] */,
                  int n, int gh, int gw, int K, int Dc, int upsample, int out_h, int out_w, float min_depth, float max_depth, void *d_fine, void *d_depth, void *stream);
int vitx_op_depth_rows(int dtype, const void *d_x, long ldx, void *d_y, long ldy, int rows, int D, void *stream);

/* ---- the text tower (CLIP, SigLIP): token ids in, text embeddings out ---------------
 * The text half of a contrastive checkpoint is a second model file in the same container.  Header: hidden_size D, num_hidden_layers L,
 * num_attention_heads H, num_classes = E (the width of the projected embedding), patch_size = 0 (THE mark of a text file: no image file
 * has it), img_size = T (context length = rows of the position table).  Tensors: token_embed.weight [V][D] (f16 for ftype >= 1, f32 for
 * ftype 0; never block-quantised), pos_embed [T][D] f32, blocks.{i}.* exactly as in an image file, norm.weight / norm.bias (the tower's
 * final LayerNorm), head.weight [E][D] + head.bias [E] (CLIP: text_projection with a zero bias; SigLIP: head), and -- always present in
 * a text file --
 *     arch f32 [4] = {activation, eps, causal, eos + 1}
 * causal: 1 = row t attends keys 0 .. t (CLIP), 0 = no mask (SigLIP).  Slot 3: 0 = pool the last position (SigLIP); otherwise the
 * EOS token id plus one: pool the FIRST position whose id is EOS (CLIP).  Optional zs f32 [4] = {kind, scale, bias, 0}: the
 * checkpoint's enum vitx_zs_kind, exp(logit_scale) and logit_bias, so that a bank made from this file carries its scoring constants.
 * Loader errors (VITX_ERR_FORMAT): a wrong shape, a missing tensor, eos >= V, causal or kind outside its enum.
 *
 * There is no tokenizer and no attention mask in the engine: ids in, embeddings out.  Under CLIP's causal mask nothing behind the pooled
 * (EOS) row reaches it, so the pad ids after EOS do not matter; SigLIP is trained and served without a mask on padded rows.
 *
 * A text model takes no image context, group or resize (VITX_ERR_ARG before any device call), an image model no text context.
 *
 * vitx_text_create: dtype VITX_F16 or VITX_BF16 (VITX_MXFP8: VITX_ERR_UNSUPPORTED).  VITX_F16 here is PLAIN fp16 operands with the
 * ordinary attention: the hi / lo parity planes of an image context exist to match ggml's f32 q, k, v, and ggml has no text tower to
 * match.  T > 128, a head dim that is not a multiple of 8 up to 128, or a D outside the LayerNorm widths: VITX_ERR_UNSUPPORTED at
 * creation.  Weights upload once per (model, device, dtype) and are shared by the text contexts of a model; block-quantised matrices
 * are expanded once at upload.  One stream, no sub-batches, no graph cache, no LayerNorm fusion.
 *
 * vitx_text_embed: ids host int32 [n][T]; out host f32 [n][E]; flags 0 or VITX_TEXT_L2 (e / sqrt(sum e^2), f32).  VITX_ERR_ARG, checked
 * on the host before any device call: an id < 0 or >= V, a row without the EOS id (files with eos), n outside 1 .. max_prompts.
 * vitx_text_embed_device: the same with d_out on the device; ids stay a HOST pointer (they are checked, and the pooled positions are
 * computed, on the host, then copied: the caller's array is free when the call returns); only enqueues on `stream`, after waiting for the
 * previous call's upload of ids -- not for its forward -- to leave the context's staging buffer.
 * Forward: X = f32(tok[id]) + pos; per layer LayerNorm, qkv, attention (attention_text.hip), proj + residual, LayerNorm, fc1 with the
 * file's activation, fc2 + residual; the pooled row through the final LayerNorm; the head GEMM in f32.
 * Determinism: a prompt's embedding is a function of its own ids only -- the same bits at any n and any position in the batch.  The
 * GEMM dispatcher picks a kernel family by row count, so a text context PINS the family of each of its GEMMs at creation, from
 * max_prompts * T rows, to one of the two ring tilings (128 x 256, or 64 x 128 for few rows); the wide persistent kernels are not
 * used.  This is the "one kernel per token count" rule of the attention dispatcher.  The guarantee holds within a context: contexts
 * created with different max_prompts may pin different tilings. */
#define VITX_KIND_IMAGE 0
#define VITX_KIND_TEXT 1
#define VITX_TEXT_L2 1
#define VITX_TEXT_MAX_TOKENS 128
typedef struct vitx_text vitx_text;
int vitx_model_kind(const vitx_model *m);            /* VITX_KIND_IMAGE / VITX_KIND_TEXT (0 for NULL) */
/* V, T, causal (0 / 1), eos (the token id, or -1: pool the last position); any out pointer may be NULL.  VITX_ERR_ARG for an image model. */
int vitx_model_text_info(const vitx_model *m, int *V, int *T, int *causal, int *eos);
/* kind, scale, bias of the file's `zs` tensor; returns 1 when the file has one, 0 (outputs untouched) otherwise */
int vitx_model_text_zs(const vitx_model *m, int *kind, float *scale, float *bias);
int vitx_text_create(const vitx_model *m, int device, int max_prompts, int dtype, vitx_text **out);
void vitx_text_free(vitx_text *t);
int vitx_text_embed(vitx_text *t, const int32_t *ids /* host [n][T] */, int n, int flags /* 0 | VITX_TEXT_L2 */, float *out /* host [n][E] */);
int vitx_text_embed_device(vitx_text *t, const int32_t *ids /* host [n][T] */, int n, int flags, void *d_out /* [n][E] f32 */, void *stream);
/* Host only, no device call: the id checks of vitx_text_embed on ids [n][T] of text model m (VITX_ERR_ARG: an id < 0 or >= V, a row without the
 * EOS id in a file with eos) and, pooled != NULL, the position each prompt is pooled at. */
int vitx_text_check_ids(const vitx_model *m, const int32_t *ids, int n, int32_t *pooled /* [n] or NULL */);
int vitx_text_shares_weights(const vitx_text *t);    /* 1 when this context found its model's weights already on the device */
/* The three text kernels on the caller's device buffers (only enqueue).  text_embed: d_tok [V][D] f16 (table_f16 != 0) or f32, d_pos [T][D] f32,
 * d_ids int32 [n][T] (NOT checked: the caller guarantees 0 <= id < V), d_x f32 [n * T][D]; D a multiple of 8.  text_pool: d_z [n][D] (dtype) =
 * the rounded LayerNorm of row i * T + d_pooled[i] of d_x -- vitx_op_layernorm's bits for that row.  attention_text: d_qkv [n * T][3 D] ->
 * d_out [n * T][D]; 1 <= T <= 128, head dim a multiple of 8 up to 128 (else VITX_ERR_UNSUPPORTED); causal != 0: row t is attention over keys 0 .. t. */
int vitx_op_text_embed(int table_f16, const void *d_tok, const void *d_pos, const void *d_ids, void *d_x, int n, int T, int D, void *stream);
int vitx_op_text_pool(int dtype, const void *d_x, const void *d_pooled, const void *d_w, const void *d_b, void *d_z, int n, int T, int D, float eps, void *stream);
int vitx_op_attention_text(int dtype, const void *d_qkv, void *d_out, int n, int T, int D, int H, int causal, void *stream);
/* attention_generic.hip at any head dim it takes, 64 included (vitx_op_attention prefers the tuned families there): the yardstick of tools/text_cost.py */
int vitx_op_attention_generic(int dtype, const void *d_qkv, void *d_out, int n_img, int N, int D, int H, void *stream);

/* ---- packed batches: images of different shapes in one forward ---------------------
 * A rectangular context runs one shape.  A PACKED context takes n images, each with its own h_i x w_i (positive multiples of the patch
 * size), lays their tokens end to end in one [sum N_i][D] residual stream (N_i = T + (h_i / P)(w_i / P), T = 1 + the register tokens;
 * image i = rows row0[i] .. row0[i + 1] - 1) and runs ONE forward: a caller whose images have their own aspect ratios needs neither a
 * context per shape nor buckets.  GEMMs, LayerNorm, activation, gate and pre-norm work on rows and do not care where an image ends; the
 * patch embedding (the rectangular context's kernel, one launch per run of consecutive images of one shape, so a caller who sorts by shape
 * pays one launch per distinct shape), the rotary embeddings, the attention and the class-row gather go by the segment table.
 *
 * vitx_pack_create: scratch for max_tokens token rows and max_images images; dtype VITX_F16 or VITX_BF16.  VITX_F16 here is PLAIN fp16
 * operands with the ordinary attention (the text tower's rule: no hi / lo parity planes).  One stream, no sub-batches, no graph cache, no
 * LayerNorm fusion, no class-token tail; block-quantised matrices are expanded once at upload; the GEMMs go through the dispatcher with the
 * device's own tuning (every GEMM family gives the same bits).  options (NULL = all zero): pos_interp as in vitx_ctx_options; max_grids = the
 * grids whose tables the context caches (0 = 32).  VITX_ERR_UNSUPPORTED at creation, before any device call: a ViTSTR file, a
 * VITX_POOL_CLS_MEAN or VITX_POOL_MAP head, VITX_MXFP8, a head dim that is no multiple of 8 up to 128, a D outside the LayerNorm widths, a
 * max_tokens beyond the kernels' 32-bit buffer window.  VITX_ERR_ARG: a text model.
 *
 * Tables: the position table of a grid (the file's at the file's grid, else resampled on the device, pos_interp) and, for a file with
 * `rope`, its rotary table (vitx_model_rope_table, uploaded) are built the first time a call names the grid -- that call allocates -- and
 * cached; beyond max_grids the least recently used grid the current call does not name is dropped.  A table is freed or overwritten only
 * after the context's previous forward has finished (an event the call waits for on the host: such a call does not merely enqueue).
 * That wait is the only one: the call that builds a table allocates it (or takes over a dropped one), resamples on `stream` and uploads the
 * rotary table with an asynchronous copy from pinned memory on `stream`; the call that drops a table does not free it -- freeing device
 * memory waits for everything enqueued on the device, the caller's own stream included -- but keeps it for the next grid it can hold (up to
 * 2 max_grids such tables, the oldest is freed beyond that; vitx_pack_scratch_bytes counts the tables of cached grids only).  With the
 * caller's stream stalled in front of it, each kind of call returns while the stall runs (tests/test_gpu_stream_order.py).
 *
 * vitx_pack_forward: imgs = the images' f32 HWC pixels end to end (image i: h_i * w_i * 3 floats), shapes host int32 [n][2] = h, w; probs and
 * logits host [n][C].  vitx_pack_forward_device: the same on device pointers; shapes stay a HOST pointer, free when the call returns; only
 * enqueues on `stream` (0 = the context's own), after waiting for the previous call's upload of the segment tables -- not for its forward.
 * Forwards of one context share its scratch: the caller orders them, as with any context.  VITX_ERR_ARG, checked on the host before the first
 * device call (vitx_pack_check is that text): a shape that is not a positive multiple of the patch size, n outside 1 .. max_images, more than
 * max_tokens tokens, more distinct grids in one call than max_grids (vitx_pack_distinct_grids counts them).
 *
 * Features of the last layer (vitx_pack_feat_enable, flags VITX_FEAT_CLS | VITX_FEAT_TOKENS, 0 = off; with nothing enabled nothing is launched
 * or allocated): the f32 final norm of every row of the pack (vitx_op_layernorm_f32's bits), gathered by vitx_pack_feat_read: cls [n][D] = the
 * class rows, tokens [sum gh_i gw_i][D] = the patch rows, images end to end.
 *
 * Determinism: within a context an image's logits, probabilities and features are a function of its own pixels and shape -- the same bits
 * alone, at any position in a pack and beside any neighbours (NaN pixels included).  A pack of one shape gives the bits of a rectangular
 * context of that shape created with last_layer_all_rows = 1 wherever both run the same attention arithmetic (any head dim but 64, where an
 * image context prefers its tuned kernels and, in VITX_F16, the parity planes).
 *
 * The kernels on the caller's device buffers (only enqueue, but see below):
 *   vitx_op_attention_packed   d_qkv [rows][3 D] -> d_out [rows][D], d_row0 int32 [n + 1]; any N_i >= 1, head dim a multiple of 8 up to 128.  Image
 *                              i's rows have exactly the bits vitx_op_attention_generic(dtype, qkv + row0[i] * 3 D, .., 1, N_i, D, H) writes; nothing
 *                              outside rows row0[0] .. row0[n] - 1 is written.  A work item is (image, head, 64 queries): H * sum ceil(N_i / 64)
 *                              workgroups, found by a binary search of the workgroup index in the running count of query blocks.  TEST entry
 *                              point: it reads d_row0 back to build that count (synchronises); a packed context uploads both with one copy.
 *   vitx_op_rope_packed        vitx_op_rope on a pack: token t >= prefix of image i rotates by row t - prefix of the table that starts
 *                              d_table_off[i] floats into d_cos and d_sin; one launch for the pack; reads both tables back to check them (synchronises).
 *
 * The dense head on a pack (vitx_pack_dense_set): "dense prediction" above, word for word and per image -- the operand is RNE of the final-norm
 * patch tokens of the selected layers, the logits come from the dispatcher GEMM with f32 accumulation, labels and scores from
 * csrc/dense_resample.h -- with one label map per image AT ITS OWN SIZE, the maps end to end.  vitx_pack_dense_set has vitx_dense_set's
 * meaning and checks (K <= 256, one to four layers, Dc = popcount(layer_mask) D, 0 = the last layer, finite W and bias, flags
 * VITX_DENSE_SCORE | VITX_DENSE_LOGITS; W == NULL && K == 0: off, everything freed); max_pixels sizes the label and score buffers.
 * VITX_ERR_UNSUPPORTED before any device call when the operand or logit rows of max_tokens rows leave the GEMMs' 32-bit byte window.  A
 * refused set leaves the head that was set in place.  With no head set nothing is allocated or launched and the forward is unchanged.
 * Per forward: as each selected layer finishes, ONE stand-alone LayerNorm over all rows of the pack writes that layer's column slot of the
 * operand (the prefix rows are normalised too and never used); after the forward one GEMM over the pack's rows and ONE label launch
 * (vitx_op_dense_labels_packed's kernel): m + 2 kernel launches more, counted by vitx_pack_launches.  The tables of the label launch ride in
 * the call's one table upload.  By default image i's maps are h_i x w_i; vitx_pack_dense_out gives the NEXT forward call other shapes
 * [n][2] = (out_h, out_w), e.g. the sizes of the originals before an aspect-preserving resize (NULL / n = 0 withdraws them); that call
 * consumes them whether it runs or is refused.  VITX_ERR_ARG before the call's first device call, nothing launched or written, the context
 * usable: an n that differs from the call's, a side below the image's grid or above 8192 (upsampling only), more than max_pixels output
 * pixels in the call.  vitx_pack_dense_check is that text, host only; it returns pix0 [n + 1] (image i's maps are elements pix0[i] ..
 * pix0[i + 1] - 1) and tile0 [n + 1] (the running count of the label launch's 64 x 16 tiles); either may be NULL.
 * vitx_pack_dense_read (waits for the forward): labels [sum oh_i ow_i] u8 and score f32 the images end to end, logits [sum gh_i gw_i][K]
 * the kept patch logits (VITX_DENSE_LOGITS).  vitx_pack_dense_device: the device label buffer (NULL while off).  vitx_pack_dense_scratch_bytes:
 * the head's operand and logit scratch; all of the head's buffers count in vitx_pack_scratch_bytes.  An image's logits, labels and scores
 * are a function of its own pixels, shape and output shape: the same bits alone, at any position and beside any neighbours; a pack of one
 * shape gives the labels and kept logits of a rectangular context with the same head.
 *   vitx_op_dense_labels_packed   the label kernel on a pack: d_logits [rows][ld], HOST grids [n][2] = (gh, gw), outs [n][2] = (oh, ow) and
 *                              lrow [n] = image i's first logit row (its gh gw rows follow; rows between images are never read) -> d_labels u8
 *                              and (or NULL) d_score f32, image i's maps with the bits of vitx_op_dense_labels on that image alone, the maps end
 *                              to end; nothing else is written.  A work item is (image, 64 x 16 output tile), found by a binary search of the
 *                              workgroup index in the running tile count.  vitx_op_dense_labels's checks per image.  TEST entry point: it builds
 *                              and uploads the tables and frees them after the launch (synchronises).
 *
 * The depth head on a pack (vitx_pack_depth_set): "depth estimation" above, word for word and per image -- the operand is RNE of the raw or
 * (VITX_DEPTH_NORM) final-norm tokens of the selected layers, the patch logits and the class half's offsets come from the dispatcher GEMM with
 * f32 accumulation, the fine plane and the map from csrc/dense_resample.h and csrc/depth_bins.h -- with one fine plane (u gh_i x u gw_i) and one
 * depth map per image AT ITS OWN SIZE, planes and maps end to end.  vitx_pack_depth_set has vitx_depth_set's meaning, flags (VITX_DEPTH_NORM |
 * VITX_DEPTH_LOGITS | VITX_DEPTH_FINE) and value checks (K <= 256 finite positive bins, upsample 1, 2 or 4, one to four layers, Dc =
 * popcount(layer_mask) D, 0 = the last layer, finite halves and bias, a finite ordered depth range; Wp == NULL && K == 0: off, everything freed);
 * max_pixels sizes the depth buffer, the fine buffer holds upsample^2 max_tokens floats.  VITX_ERR_UNSUPPORTED before any device call when the
 * operand or logit rows of max_tokens rows leave the GEMMs' 32-bit byte window.  A refused set leaves the head that was set in place.  With no
 * depth head set nothing is allocated or launched for it.  Per forward: as each selected layer finishes, ONE launch over all rows of the pack
 * -- the stand-alone LayerNorm, or raw the streaming conversion -- writes that layer's column slot of the operand (prefix rows included);
 * after the forward the patch GEMM over the pack's rows (image i's first logit row is row0[i] + T), with a class half (Wc) one gather of the n
 * class rows row0[i] of that operand into compact rows and the short offsets GEMM (without Wc the bias is every image's offsets row and neither
 * is launched), then ONE fine launch and ONE resize launch (vitx_op_depth_fine_packed's and vitx_op_depth_resize_packed's kernels): m + 3
 * kernel launches more, m + 5 with a class half, counted by vitx_pack_launches.  The tables of both launches ride in the call's one table
 * upload.  By default image i's map is h_i x w_i; vitx_pack_depth_out gives the NEXT forward call other shapes, with vitx_pack_dense_out's
 * meaning: that call consumes them whether it runs or is refused.  Refused before the call's first device call, nothing launched or written,
 * the context usable: VITX_ERR_ARG for an n that differs from the call's, an output side below the image's fine plane or above 8192
 * (upsampling only), more than max_pixels output pixels in the call; VITX_ERR_UNSUPPORTED for a fine side above 8192.  vitx_pack_depth_check
 * is that text, host only; it returns pix0 and fine0 [n + 1] (image i's map is floats pix0[i] .. pix0[i + 1] - 1, its fine plane fine0[i] ..)
 * and ftile0 / otile0 [n + 1] (the running counts of the fine launch's 16 x 16 and the resize launch's 64 x 16 tiles); any may be NULL.
 * vitx_pack_depth_read (waits for the forward): depth [sum oh_i ow_i] and fine [sum u^2 gh_i gw_i] (VITX_DEPTH_FINE) f32 the images end to
 * end, logits [sum gh_i gw_i][K] the kept patch logits and offsets [n][K] (VITX_DEPTH_LOGITS; without a class half the bias n times).
 * vitx_pack_depth_device: the device depth buffer (NULL while off).  vitx_pack_depth_scratch_bytes: the head's operand, logit, class-row and
 * offset scratch; all of the head's buffers count in vitx_pack_scratch_bytes.  An image's logits, offsets, fine plane and map are a function
 * of its own pixels, shape and output shape: the same bits alone, at any position and beside any neighbours (the LDS of the fine launch and
 * its bin chunk come from the call's widest window; a lane carries its two sums across chunks in bin order, so no bit depends on them); a
 * pack of one shape gives the maps and kept logits of a rectangular context with the same head.  A dense head and a depth head may both be
 * set; neither changes the other's bits.
 *   vitx_op_depth_fine_packed  the fine kernel on a pack: d_logits [rows][ld], d_offsets [.][ld] or NULL, d_bins [K], HOST grids [n][2] = (gh, gw),
 *                              lrow [n] = image i's first logit row (its gh gw rows follow; rows between images are never read) and orow [n] = its
 *                              row of d_offsets -> d_fine f32, image i's plane with the bits of vitx_op_depth_fine on that image alone, the planes
 *                              end to end; nothing else is written.  A work item is (image, 16 x 16 fine tile), found by a binary search of the
 *                              workgroup index in the running tile count: a 1-D grid, so no bound on n.  vitx_op_depth_fine's checks per image.
 *   vitx_op_depth_resize_packed  the resize kernel on a pack: d_fine = the fine planes end to end, HOST fines [n][2] = (fh, fw) and outs [n][2] =
 *                              (oh, ow) -> d_out f32, image i's map with the bits of vitx_op_depth_resize on that image alone, the maps end to
 *                              end.  A work item is (image, 64 x 16 output tile).  vitx_op_depth_resize's checks per image.
 *                              Both are TEST entry points: they build and upload the tables and free them after the launch (synchronise).
 *
 * u8 sources (vitx_pack_u8_set): a pack fed from decoded u8 originals, each of its own size, instead of f32 pixels already resized.  ONE launch per
 * pack (vitx_op_preprocess_pack's kernel) stretches source i, u8 HWC [ny_i][nx_i][3], to image i's own h_i x w_i with Pillow's arithmetic and the
 * description's mean / std -- vitx_preprocess_rect's meaning, no crop, the aspect is the caller's (vitx_pack_fit_shapes: vitx_rect_shape per
 * image) -- into the context's pixel buffer, which the unchanged forward then reads: one kernel launch more, counted by vitx_pack_launches.  Image
 * i's pixels are the bits of vitx_preprocess_rect (and of vitx_preprocess_rect_device) on it alone, at any position and beside any neighbours:
 * a workgroup lays out its LDS by its image's own tiling, and no bit depends on the launch's LDS size (the largest tiling of the call).
 * vitx_pack_u8_set: pp (NULL: the file's, vitx_model_preproc) must pass the description's rules (VITX_ERR_ARG) and name a PIL filter
 * (VITX_ERR_UNSUPPORTED, vitx_preprocess_rect's rule), before any device call; it allocates the device staging of the host entry point
 * (max_src_bytes rounded up to 4) and the f32 pixel buffer (max_tokens P^2 3 floats, which vitx_pack_forward otherwise allocates at its first
 * call); both and the tables count in vitx_pack_scratch_bytes.  A refused set leaves what was set.  max_src_bytes = 0: off, everything the set
 * allocated is freed and vitx_pack_scratch_bytes returns to its value before.  While off nothing is allocated or launched and the forward is
 * unchanged.  vitx_pack_u8_sources declares, as vitx_pack_dense_out does for output shapes, that the NEXT forward call's d_imgs holds the u8
 * sources strictly end to end, no padding, with sizes src_shapes [n][2] = (ny, nx); `shapes` of that call stays the images' (output) shapes.
 * That call consumes the declaration whether it runs or is refused; the call after it takes f32 pixels again (NULL / n = 0 withdraws it;
 * VITX_ERR_ARG while u8 is off).  Alignment: sources start at every byte alignment; d_imgs itself must be 4-byte aligned and readable up to
 * its byte count rounded up to 4 (the kernel stages source rows by aligned dword loads; of a dword that straddles two sources, or the end, only the
 * row's own bytes are used).  vitx_pack_forward_device in that mode uploads the launch's tables in the call's one table upload and still only
 * enqueues.  Refused before the call's first device call, nothing launched or written, the context usable: VITX_ERR_ARG for a declaration whose
 * n differs from the call's, a d_imgs that is not 4-byte aligned, a source side outside 1 .. 2^20, more than max_src_bytes source bytes, more than
 * 2^31 - 1 tiles (32 x 8 output pixels each); VITX_ERR_UNSUPPORTED for an image whose down-scale needs more than 64 KiB of LDS per tile
 * (vitx_preprocess_rect_device_supports; the text names the image -- feed that pack through vitx_preprocess_rect).  vitx_pack_u8_check is that text,
 * host only (pp NULL: the file's; max_src_bytes 0: no bound); it returns src0 [n + 1] (source i is bytes src0[i] .. src0[i + 1] - 1), tile0 [n + 1]
 * (the running tile count) and *lds (the launch's dynamic LDS); any may be NULL.  vitx_pack_forward_u8 is the host entry point, vitx_pack_forward's
 * shape on u8: it declares the sources, uploads them (3 bytes per SOURCE pixel, where vitx_pack_forward uploads 12 per output pixel) on the context's
 * stream, runs the forward and copies the results back.  vitx_pack_forward refuses a call for which sources are declared (VITX_ERR_ARG).
 *   vitx_op_preprocess_pack    the kernel alone on the caller's device buffers: d_srcs as above, HOST src_shapes [n][2] = (ny, nx) and out_shapes
 *                              [n][2] = (h, w) -> d_out f32 HWC, the images end to end; nothing else is written.  A work item is (image, 32 x 8
 *                              output tile), found by a binary search of the workgroup index in the running tile count: a 1-D grid.  The
 *                              refusals above.  TEST entry point: it runs on the null stream, builds and uploads the tables and frees them after
 *                              the launch (synchronises).
 *
 * Attention maps on a pack (vitx_pack_attn_enable): "attention maps and attention rollout" above, word for word and per image.  Image i has N_i = T +
 * gh_i gw_i tokens; its class-token map of a selected layer is [H][N_i], its rollout row [N_i]; index 0 is the class token, then the registers, then
 * the patches in raster order of ITS OWN grid.  q and k are what the pack's QKV buffer holds after the layer's qkv GEMM (and, for a file with `rope`,
 * after the rotary launch): the point where an image context reads them.  A packed context has no parity planes.  vitx_pack_attn_enable(p,
 * layer_mask, flags, max_sq_tokens): vitx_attn_enable's mask and flags; mask 0 with flags 0 = off, the buffers are freed and vitx_pack_scratch_bytes
 * returns to its value before.  VITX_ATTN_ROLLOUT keeps two matrix arenas of max_sq_tokens floats each -- a call's matrices, N_i x N_i per image, lie
 * end to end in them -- and needs 1 <= max_sq_tokens <= 2^31 - 1.  VITX_ERR_ARG, before any device call: mask bits at or beyond L, unknown flags, a
 * bad max_sq_tokens.  Buffers: the maps, max_tokens * vitx_pack_attn_floats f32; with rollout the two arenas and, when the last layer is not
 * selected, max_tokens * H f32 for its class maps; all count in vitx_pack_scratch_bytes.  A refused or failed enable leaves the maps that were on.
 * Waits for the context's last forward.  vitx_pack_attn_floats: floats per TOKEN = popcount(mask) * H + (rollout ? 1 : 0).  Per forward, in front of
 * each layer's attention launch, the image forward's sequence on the packed kernels below: the class maps of a selected layer (1 launch); with
 * rollout the factor into arena l & 1 (L - 1 launches), the in-place step for 0 < l < L - 1 (max(L - 2, 0)), and on the last layer its class maps
 * (one launch more when it is not selected) and the row (1): all counted by vitx_pack_launches; the two tables of the rollout launches ride in the
 * call's one table upload.  With maps off nothing is launched or allocated.  Probabilities, logits, features and both heads keep their bits with
 * maps on: the kernels only read QKV.  Refused before the call's first device call with rollout on, nothing launched or written, the last forward's
 * maps still readable: VITX_ERR_UNSUPPORTED for an image above 1024 tokens (the text names the image), VITX_ERR_ARG when the call's sum of N_i^2
 * exceeds max_sq_tokens.  vitx_pack_attn_check is that text and the enable's argument checks, host only; it returns rblk0 [n + 1] (the running
 * count of ceil(N_i / 16), the work items of the factor and the step) and sq0 [n + 1] (the running sum of N_i^2: image i's matrix starts at float
 * sq0[i] of an arena); either may be NULL.  vitx_pack_attn_read (waits for the forward): the last forward's images end to end, image i at float
 * row0[i] * vitx_pack_attn_floats: the selected layers in ascending order, each [H][N_i], then the rollout row [N_i]; VITX_ERR_ARG before any
 * forward with maps on or when n_floats is below row0[n] * vitx_pack_attn_floats.  vitx_pack_attn_device: the device buffer in that layout (NULL
 * while off).  An image's maps and rollout row are a function of its own pixels and shape: the same bits alone, at any position and beside any
 * neighbours (the launches' register tiles and LDS pitch come from the call's widest image; key tiles beyond N_i are skipped or masked and add exact
 * zeros, the step's k loop ends at N_i, so no bit depends on them); a pack of one shape gives the maps of a rectangular context of that shape
 * wherever both hold the same q and k (any head dim but 64, see above).
 *   The kernels on a pack, TEST entry points: row0 [n + 1] is a HOST table (ascending, N_i >= 1); each call builds and uploads its
 *   tables, launches on the NULL STREAM and returns after synchronising -- they take no stream.  Image i has the bits of the fixed-shape entry point
 *   on that image alone.  A null pointer, n <= 0 or a table that does not ascend: VITX_ERR_ARG; an image above 1024 tokens where a matrix is involved:
 *   VITX_ERR_UNSUPPORTED.
 *   vitx_op_attention_map_packed  d_qkv [rows][3 D] -> d_cls (or NULL), image i's [H][N_i] class maps at float row0[i] * H, and d_mean (or NULL), its
 *                              [N_i][N_i] mean_h A_h at float sq0[i] = sum_(j < i) N_j^2; half_identity != 0: the rollout factor instead
 *                              (vitx_op_rollout_factor's entry).  Nothing else is written.
 *   vitx_op_rollout_step_packed   d_a <- d_a . d_r per image, both with image i's matrix at float sq0[i]; ranges that overlap: VITX_ERR_ARG.
 *   vitx_op_rollout_row_packed    d_cls as above, d_r (or NULL) as above -> d_out, image i's row [N_i] at float row0[i].
 * Not offered on packed contexts (each a later step): the other opt-in heads (zero-shot bank, gallery), the pooled
 * and attention-pooling heads, the F16 parity planes, LayerNorm fusion and sub-batch streams, a packed patch-embedding kernel, vitx_group_*;
 * of the dense and the depth head: downsampling, and a vit.h wrapper; of the u8 sources: crops and shortest-edge geometry (a source is stretched
 * to the given shape), the REF filters, JPEG decode on the device, and a vit.h wrapper; of the attention maps: full N x N maps as an output, rollout
 * above 1024 tokens per image, and a vit.h wrapper. */
typedef struct vitx_pack vitx_pack;
typedef struct { int pos_interp, max_grids, reserved[6]; } vitx_pack_options;
int vitx_pack_create(const vitx_model *m, int device, int max_tokens, int max_images, int dtype, const vitx_pack_options *opt, vitx_pack **out);
void vitx_pack_free(vitx_pack *p);
int vitx_pack_shares_weights(const vitx_pack *p);
/* host only: every refusal of a forward call but the grid count, and row0 [n + 1] (may be NULL) */
int vitx_pack_check(const vitx_model *m, const int32_t *shapes /* [n][2] = h, w */, int n, int max_tokens, int max_images, int32_t *row0);
/* host only: the distinct grids among shapes [n][2] -- what a forward call compares with max_grids (0 for NULL arguments) */
int vitx_pack_distinct_grids(const vitx_model *m, const int32_t *shapes, int n);
int vitx_pack_forward(vitx_pack *p, const float *imgs, const int32_t *shapes, int n, float *probs, float *logits /* or NULL */);
int vitx_pack_forward_device(vitx_pack *p, const void *d_imgs, const int32_t *shapes /* host */, int n, void *d_probs, void *d_logits, void *stream);
int vitx_pack_feat_enable(vitx_pack *p, int flags /* VITX_FEAT_CLS | VITX_FEAT_TOKENS, 0 = off */);
int vitx_pack_feat_read(vitx_pack *p, float *cls /* [n][D] or NULL */, float *tokens /* [sum gh_i gw_i][D], images end to end, or NULL */);
size_t vitx_pack_scratch_bytes(const vitx_pack *p);        /* device bytes of activation scratch and cached tables held now (weights not counted) */
int vitx_pack_launches(const vitx_pack *p, int *patch_embed);      /* kernel launches of the last forward call; *patch_embed: the patch embeddings among them */
int vitx_op_attention_packed(int dtype, const void *d_qkv, void *d_out, const void *d_row0 /* int32 [n + 1] */, int n, int D, int H, void *stream);
/* the same launch on tables the caller built and vouches for: d_qb0 int32 [n + 1] = the running count of ceil(N_i / 64), qblocks = d_qb0[n]; only enqueues */
int vitx_op_attention_packed_tables(int dtype, const void *d_qkv, void *d_out, const void *d_row0, const void *d_qb0, int n, long qblocks, int D, int H, void *stream);
int vitx_op_rope_packed(int dtype, void *d_qkv, long lo_off /* must be 0 */, const void *d_cos, const void *d_sin, const void *d_row0 /* int32 [n + 1] */,
                        const void *d_table_off /* int32 [n] */, int n, int prefix, int D, int H, void *stream);
int vitx_pack_dense_set(vitx_pack *p, const float *W /* [K][Dc] */, const float *bias /* [K] or NULL */, int K, int Dc, uint64_t layer_mask, long max_pixels, int flags);
int vitx_pack_dense_out(vitx_pack *p, const int32_t *out_shapes /* [n][2] = out_h, out_w; NULL: the images' own */, int n);
/* host only: every refusal a forward call adds while a dense head of K classes and max_pixels is set */
int vitx_pack_dense_check(const vitx_model *m, const int32_t *shapes, const int32_t *out_shapes /* or NULL */, int n, int K, long max_pixels,
                          int64_t *pix0 /* [n + 1] or NULL */, int32_t *tile0 /* [n + 1] or NULL */);
int vitx_pack_dense_read(vitx_pack *p, uint8_t *labels, float *score /* or NULL */, float *logits /* or NULL */);
const void *vitx_pack_dense_device(const vitx_pack *p);
size_t vitx_pack_dense_scratch_bytes(const vitx_pack *p);
int vitx_op_dense_labels_packed(const void *d_logits, long ld, const int32_t *grids /* host [n][2] */, const int32_t *outs /* host [n][2] */,
                                const int32_t *lrow /* host [n] */, int n, int K, void *d_labels, void *d_score /* or NULL */, void *stream);
/* the same in two steps, for callers that keep the tables: host only, tab int32 [n + 1 + 10 n] (the running tile count, then a row per image), its
 * tile count and widest window; then the launch on a table the caller uploaded and vouches for (only enqueues) */
int vitx_dense_pack_tables(const int32_t *grids, const int32_t *outs, const int32_t *lrow, int n, int32_t *tab, int *tiles, int *cells);
int vitx_op_dense_labels_packed_tables(const void *d_logits, long ld, const void *d_tab, int n, int tiles, int cells, int K, void *d_labels, void *d_score, void *stream);
int vitx_pack_depth_set(vitx_pack *p, const float *Wp /* [K][Dc] */, const float *Wc /* [K][Dc] or NULL */, const float *bias /* [K] or NULL */, const float *bins /* [K] */,
                        int K, int Dc, uint64_t layer_mask, int upsample, float min_depth, float max_depth, long max_pixels, int flags);
int vitx_pack_depth_out(vitx_pack *p, const int32_t *out_shapes /* [n][2] = out_h, out_w; NULL: the images' own */, int n);
/* host only: every refusal a forward call adds while a depth head of K bins, upsample and max_pixels is set */
int vitx_pack_depth_check(const vitx_model *m, const int32_t *shapes, const int32_t *out_shapes /* or NULL */, int n, int K, int upsample, long max_pixels,
                          int64_t *pix0 /* [n + 1] or NULL */, int64_t *fine0 /* [n + 1] or NULL */, int32_t *ftile0 /* [n + 1] or NULL */, int32_t *otile0 /* [n + 1] or NULL */);
int vitx_pack_depth_read(vitx_pack *p, float *depth, float *fine /* or NULL */, float *logits /* or NULL */, float *offsets /* or NULL */);
const void *vitx_pack_depth_device(const vitx_pack *p);
size_t vitx_pack_depth_scratch_bytes(const vitx_pack *p);
int vitx_op_depth_fine_packed(const void *d_logits, long ld, const void *d_offsets /* or NULL */, const void *d_bins, const int32_t *grids /* host [n][2] */,
                              const int32_t *lrow /* host [n] */, const int32_t *orow /* host [n]; NULL without d_offsets */, int n, int K, int upsample, void *d_fine, void *stream);
int vitx_op_depth_resize_packed(const void *d_fine, const int32_t *fines /* host [n][2] */, const int32_t *outs /* host [n][2] */, int n, float min_depth, float max_depth,
                                void *d_out, void *stream);
/* the same in two steps, for callers that keep the tables: host only, tab int32 [2 (n + 1) + 16 n] (the running fine and output tile counts, then a row per
 * image), its tile counts and widest window; then the launches on a table the caller uploaded and vouches for (only enqueue); ldo = 0: one offsets row for all */
int vitx_depth_pack_tables(const int32_t *grids, const int32_t *outs, const int32_t *lrow, const int32_t *orow, int n, int upsample, int32_t *tab, int *ftiles, int *otiles, int *cells);
int vitx_op_depth_fine_packed_tables(const void *d_logits, long ld, const void *d_offsets, long ldo, const void *d_bins, const void *d_tab, int n, int tiles, int cells, int K,
                                     void *d_fine, void *stream);
int vitx_op_depth_resize_packed_tables(const void *d_fine, const void *d_tab, int n, int tiles, float min_depth, float max_depth, void *d_out, void *stream);
/* u8 sources */
int vitx_pack_u8_set(vitx_pack *p, const vitx_preproc *pp /* NULL: the file's, vitx_model_preproc */, size_t max_src_bytes /* 0 = off */);
int vitx_pack_u8_sources(vitx_pack *p, const int32_t *src_shapes /* [n][2] = ny, nx; NULL: none */, int n);
int vitx_pack_forward_u8(vitx_pack *p, const uint8_t *srcs, const int32_t *src_shapes, const int32_t *shapes, int n, float *probs, float *logits /* or NULL */);
/* host only: every refusal a forward call adds while u8 sources are declared for it */
int vitx_pack_u8_check(const vitx_model *m, const vitx_preproc *pp, const int32_t *src_shapes, const int32_t *shapes, int n, size_t max_src_bytes,
                       int64_t *src0 /* [n + 1] or NULL */, int32_t *tile0 /* [n + 1] or NULL */, int *lds /* or NULL */);
/* host only: vitx_rect_shape per image, shapes [n][2] = h, w */
int vitx_pack_fit_shapes(const vitx_model *m, const int32_t *src_shapes, int n, int short_side, int max_long, int32_t *shapes);
int vitx_op_preprocess_pack(const vitx_preproc *pp, const void *d_srcs, const int32_t *src_shapes /* host [n][2] */, const int32_t *out_shapes /* host [n][2] */,
                            int n, void *d_out);
/* attention maps */
int vitx_pack_attn_enable(vitx_pack *p, uint64_t layer_mask, int flags /* VITX_ATTN_ROLLOUT */, long max_sq_tokens /* rollout: the call's sum of N_i^2 at most */);
int vitx_pack_attn_floats(const vitx_pack *p);             /* floats per token */
int vitx_pack_attn_read(vitx_pack *p, float *out, size_t n_floats);
const void *vitx_pack_attn_device(const vitx_pack *p);
/* host only: the enable's argument checks and every refusal a forward call adds while maps are on */
int vitx_pack_attn_check(const vitx_model *m, const int32_t *shapes, int n, uint64_t layer_mask, int flags, long max_sq_tokens,
                         int32_t *rblk0 /* [n + 1] or NULL */, int32_t *sq0 /* [n + 1] or NULL */);
int vitx_op_attention_map_packed(int dtype, const void *d_qkv, void *d_cls /* or NULL */, void *d_mean /* or NULL */, const int32_t *row0 /* host [n + 1] */, int n,
                                 int D, int H, int half_identity);
int vitx_op_rollout_step_packed(void *d_a, const void *d_r, const int32_t *row0 /* host [n + 1] */, int n);
int vitx_op_rollout_row_packed(const void *d_cls, const void *d_r /* or NULL */, void *d_out, const int32_t *row0 /* host [n + 1] */, int n, int H);

/* ---- MXFP8 operands (VITX_MXFP8, encoding above) ------------------------------- */
/* Host encoder: x f32 [rows][K] -> q [rows][k_pad] e4m3 bytes + scales [rows][k_pad / 32] (k_pad >= K, a multiple of 32; columns
 * K .. k_pad are zero elements, whole padding blocks get scale 127).  VITX_ERR_ARG on NULL or a bad size. */
int vitx_mxfp8_quantize(const float *x, int rows, int K, int k_pad, uint8_t *q, uint8_t *scales);
/* The device encoder on its own (device pointers, same arguments and bits as vitx_mxfp8_quantize; only enqueues). */
int vitx_op_quantize_mxfp8(const void *d_x, int rows, int K, int k_pad, void *d_q, void *d_scales, void *stream);
/* LayerNorm -> MX: d_x f32 [M][D] -> d_q [M][K_pad(D)] + d_scales [M][K_pad(D) / 32] of the f32 value vitx_op_layernorm rounds. */
int vitx_op_layernorm_mxfp8(const void *d_x, const void *d_w, const void *d_b, void *d_q, void *d_scales, int M, int D, float eps, void *stream);
/* C = A . W^T on MX operands (v_mfma_scale_f32_16x16x128_f8f6f4): d_a [M][K_pad] + d_a_scales [M][K_pad / 32]; d_w and d_w_scales hold
 * N rounded up to 128 rows (zero blocks beyond N); d_bias N f32.  K_pad = K rounded up to 128.  Any M.
 *   epi 0: out bf16 [M][N] = acc + bias                                            (qkv)
 *   epi 1: out MX [M][K_pad(N)] + d_out_scales [M][K_pad(N) / 32] of gelu_tanh(acc + bias), columns N .. K_pad(N) zero   (fc1)
 *   epi 2: out f32 [M][N] = (acc + bias) + out in place                            (fc2)
 * VITX_ERR_ARG on NULL pointers (d_out_scales only for epi 1) or another epi. */
int vitx_op_gemm_mxfp8(int epi, const void *d_a, const void *d_a_scales, const void *d_w, const void *d_w_scales, const void *d_bias, void *d_out,
                       void *d_out_scales, int M, int N, int K, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VITX_H */
