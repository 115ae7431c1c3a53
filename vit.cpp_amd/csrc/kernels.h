// kernels.h -- launchers of the hand-written CDNA4 (gfx950) kernels of the ViT forward path, one translation unit per kernel family
// (gemm*.hip, layernorm.hip, attention*.hip, patch_embed.hip, softmax_topk.hip, image_preprocess.hip, features.hip, quant.hip, ...): each
// declaration below names its file.
// Written for MI355X only: 64-lane wavefronts, v_mfma_f32_16x16x32_{f16,bf16} (GEMMs) / v_mfma_f32_32x32x16 (attention),
// global_load_lds (LDS-DMA) staging with a source-side XOR swizzle, 160 KiB LDS.
// The math each kernel implements is the ggml op sequence vit_encode_image emits
// (/root/reference/vit.cpp:718-941); per-kernel citations at the kernels.
// All pointers are device pointers; every launcher only enqueues on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/vitx.h"

namespace vitx {

enum { DT_F16 = 0, DT_BF16 = 1 };

// GEMM epilogues (C = A[M][K] . W[N][K]^T, f32 accumulate)
enum {
    EPI_BIAS = 0,        // out(dtype)[m][n] = acc + bias[n]                       qkv      (vit.cpp:820-821)
    EPI_BIAS_GELU = 1,   // out(dtype)[m][n] = gelu_tanh(round(acc + bias[n]))     fc1      (vit.cpp:889-893)
    EPI_BIAS_RESID = 2,  // out(f32)[m][n]   = (acc + bias[n]) + out[m][n]         proj/fc2 (vit.cpp:868-873, 896-900)
    EPI_BIAS_F32 = 3,    // out(f32)[m][n]   = acc + bias[n]                       head     (vit.cpp:927-928)
    EPI_PATCH = 4,       // out(f32)[m + (m/tpi + 1) * prefix][n] = (acc + bias[n]) + pos[(m%tpi + 1)][n]   (vit.cpp:772-797; prefix = 1 there)
    EPI_BIAS_HILO = 5,   // qkv of the F16 parity mode: v = acc + bias[n] kept to f32 grade as TWO 16-bit planes, out[m][n] = hi = round(v) and
                         // out[hilo_off + ..] = lo = round((v - hi) * 2048): the reference's q, k, v stay f32 into the attention products
                         // (vit.cpp:826-858: ggml_mul_mat of f32 views), and hi + lo / 2048 reproduces v to 2^-22
    EPI_BIAS_GELU_ERF = 6,  // fc1 of a VITX_ACT_GELU_ERF model:   EPI_BIAS_GELU with x Phi(x) (gelu_erf2) in place of gelu_tanh, same rounding points
    EPI_BIAS_QGELU = 7      // fc1 of a VITX_ACT_QUICK_GELU model: ... with x sigmoid(1.702 x) (quick_gelu2)
};
constexpr int EPI_COUNT = 8;
// the three fc1 epilogues: out(dtype) = act(acc + bias), and the activation each evaluates (enum vitx_activation, act2 of device_common.h)
constexpr __host__ __device__ bool epi_is_act(int epi) { return epi == EPI_BIAS_GELU || epi == EPI_BIAS_GELU_ERF || epi == EPI_BIAS_QGELU; }
constexpr __host__ __device__ int epi_act(int epi) { return epi == EPI_BIAS_GELU_ERF ? 1 : epi == EPI_BIAS_QGELU ? 2 : 0; }
constexpr int act_epi(int activation) { return activation == 1 ? EPI_BIAS_GELU_ERF : activation == 2 ? EPI_BIAS_QGELU : EPI_BIAS_GELU; }
constexpr float kHiLoScale = 2048.0f, kHiLoInv = 1.0f / 2048.0f;
// bytes of one output element: the operand type (qkv, fc1) or f32 (residual, head, patch embedding)
constexpr __host__ __device__ int epi_out_bytes(int epi) { return (epi == EPI_BIAS || epi_is_act(epi) || epi == EPI_BIAS_HILO) ? 2 : 4; }

struct GemmArgs {
    const void *A; const void *W; const float *bias; void *out; const float *pos;
    int M;        // rows computed (multiple of the M tile; buffers are padded to it)
    int M_real;   // rows stored
    int N;        // columns stored (real)
    int N_pad;    // columns of W available (multiple of the N tile; zero rows beyond N)
    int K;        // multiple of 64
    int lda, ldw, ldo;
    int tpi;      // EPI_PATCH: patch tokens per image (g*g)
    int prefix = 1;  // EPI_PATCH: tokens of an image in front of its patches: the class token + R register tokens (an image has tpi + prefix rows); 0: none, and pos has no class row
    long hilo_off;  // EPI_BIAS_HILO: ELEMENT offset of the lo plane behind `out` (a whole number of rows; the byte offset must fit 32 bits)
    int dbg;      // ablation bits of the ring kernel's laboratory build (VITX_LAB only; 0 in the product)
    // q4_0 weights kept in block form (launch_gemm_q4 only): W = nibble plane [N_pad][K/2] bytes (16 per block), Wscale = f16 block
    // scales [N_pad][K/32]; both planes are the file's block_q4_0 fields re-laid out, 4.5 bits per weight
    const uint16_t *Wscale;
    int group_m;  // ping-pong kernel: m-tiles per raster group (0 = the default, 8)
    // LayerNorm of the output rows fused into an EPI_BIAS_RESID GEMM on the ping-pong kernel (gemm_ln_fusable()): `ln` != nullptr.
    const struct GemmLn *ln;
    // A GEMM whose A operand is the output of a LayerNorm-fusing GEMM: `fix` = that launch's GemmLn (+ x = its X).  Before it loads anything,
    // every workgroup normalises the row blocks IT is going to read that were left behind (todo[rb] == epoch) -- no extra launch, no
    // dependency between workgroups (several may redo the same block: identical bits).  gemm_fix_capable() says whether the kernel the
    // shape selects does this; otherwise the caller launches launch_layernorm_fixup.
    const struct GemmLn *fix;
};
// The dense row-major case: A [M][K], W [N_pad][K], out [M][ldo] (ldo = N unless given); every other field zero
inline GemmArgs dense_gemm(const void *A, const void *W, const float *bias, void *out, int M, int M_real, int N, int N_pad, int K, int ldo = 0) {
    GemmArgs g{};
    g.A = A; g.W = W; g.bias = bias; g.out = out;
    g.M = M; g.M_real = M_real; g.N = N; g.N_pad = N_pad; g.K = K; g.lda = K; g.ldw = K; g.ldo = ldo ? ldo : N;
    return g;
}

// The LayerNorm that follows a residual GEMM (vit.cpp:881-885 after proj, :808-812 of the next layer after fc2), computed by the
// GEMM's own epilogue: every workgroup reduces its 256-column tile's per-row statistics from the accumulators, publishes them as
// data-tagged 8-byte granules, reads the statistics of the row block's other column tiles from its raster-adjacent peers (same
// round, same XCD), and normalises ITS OWN tile from registers into `out`: X is not re-read, no extra launch, no single-CU tail.
// All M (padded) rows are computed and stored: the buffers are padded to the row tile, pad rows stay finite and are never read
// for real rows.  A peer that does not answer within `timeout` (two such GEMMs on two streams can each hold CUs the other's
// workgroups wait for) makes the workgroup skip its tile and set todo[row block] = epoch; launch_layernorm_fixup() then
// normalises exactly those row blocks from X with the stand-alone arithmetic -- the same bits (ln_row.h "LayerNorm statistics").
struct GemmLn {
    const float *w, *b;           // [N]
    const float *x;               // consumer-side fix only (GemmArgs::fix): the f32 rows [M][N] the statistics are recomputed from
    void *out;                    // [M][N] operand type
    float eps;
    unsigned long long *sync;     // [M / 256][N / 256][256][2] granules {value bits, tag = epoch}, zeroed once
    unsigned *todo;               // [M / 256], zeroed once
    unsigned *fallbacks;          // [1] diagnostic counter: tiles that took the fix-up path
    unsigned epoch;               // unique per launch within the process, never 0 (frozen under graph replay: callers do not fuse while capturing)
    unsigned timeout;             // ticks of the 100 MHz wall clock
    int test;                     // parity tests only: 1 = every 5th tile pretends a time-out, 3 = and does not publish (its peers really time out)
};

// ---- block-quantised weights resident in HBM (quant.hip) -------------------------------------------
// ggml block types of the reference's quantised files (vit.cpp:384-414 picks the type, quantize.cpp:271-303 writes it)
enum { QT_Q4_0 = 2, QT_Q4_1 = 3, QT_Q5_0 = 6, QT_Q5_1 = 7, QT_Q8_0 = 8 };
// One matrix to expand: `src` holds N rows of nbk blocks in the file's layout (q4_0: the two planes described at GemmArgs::Wscale,
// scales at `scales`), dst is [n_pad][nbk * 32] in the operand type; rows N..n_pad are written as zeros.
struct DequantJob { const void *src; const void *scales; void *dst; int N, n_pad, nbk; };
// Expands up to 4 matrices of one block type in ONE launch: value = exactly what HostTensor::decode_f32 computes, rounded once (RNE) to
// the operand type -- bit-identical to the host-side expansion at upload.
hipError_t launch_dequant(int dtype, int qtype, const DequantJob *jobs, int njobs, hipStream_t stream);
// C = A . dequant(W)^T with the q4_0 blocks expanded inside the GEMM's LDS-fill path (gemm.hip; 128x128x64 tiles; any epilogue)
hipError_t launch_gemm_q4(int dtype, int epi, const GemmArgs &a, hipStream_t stream);
bool gemm_q4_supports(const GemmArgs &a);

// Per-device launch parameters: one immutable copy per device, built by tuning_for_device() under a lock, so contexts on several GPUs
// (or host threads) of one process never share launch state.  The product library reads NO environment variable here: the family
// overrides below are explicit parameters of vitx_op_gemm_ex / vitx_op_attention_ex (parity tests); only the laboratory build
// (-DVITX_LAB, tools/) maps VITX_* variables onto them.
enum { ATTN_AUTO = 0, ATTN_SINGLE = 1, ATTN_FLOW = 3, ATTN_PERSIST = 4, ATTN_STREAM = 5 };
struct Tuning {
    int device = 0;
    int n_cu = 256;          // compute units of THIS device
    int n_xcd = 8;           // XCDs (hipDeviceAttributeNumberOfXccs): the LayerNorm-fusing GEMM's peer mapping is built for exactly 8
    int gemm_cfg = -1;       // -1 automatic, 1 = the ping-pong kernel forced, else a ring configuration (445, 945, 245, 122)
    int skinny_tiles = 128;  // 64x128 tiles (cfg 122) when fewer than this many 128x256 tiles exist (r02f: 64 -> 128, batches of 4-16 images)
    int gemm_split = 0;      // 1: tail rows of a partial round re-tiled 128x256 in a second launch
    int gemm_balance = 1;    // 0: one workgroup per CU even when the last round of tiles is partial
    int group_m = 0;         // raster group height of the ping-pong kernel (0 = its default)
    int pp_flags = 0;        // ablation build of the ping-pong kernel (exists under VITX_LAB only)
    int gemm_dbg = 0;        // ablation bits of the ring kernel (honoured under VITX_LAB only)
    int attn_kernel = ATTN_AUTO;
    int attn_flags = 0;      // ablation build of the pipelined attention kernel (exists under VITX_LAB only)
    int attn_grid = 0;       // persistent attention: workgroups (0 = one per CU)
};
// Looks the device up (hipGetDevice when device < 0) and on first use of a device
// sets the dynamic-LDS attribute of every kernel instantiation on it (tuning.cpp).  Thread-safe.  Returns nullptr if HIP fails.
const Tuning *tuning_for_device(int device);

// The GEMM dispatcher (gemm.hip): picks the kernel family for the shape
hipError_t launch_gemm(const Tuning &t, int dtype, int epi, const GemmArgs &a, hipStream_t stream);
// true when launch_gemm runs this EPI_BIAS_RESID GEMM on the ping-pong kernel in one launch with whole rows (N == N_pad == ldo,
// N / 256 <= 4 column tiles), so that GemmArgs::ln may be set; the caller then launches launch_layernorm_fixup instead of launch_layernorm
bool gemm_ln_fusable(const Tuning &t, const GemmArgs &a);
// true when launch_gemm runs this GEMM on the ping-pong kernel, which honours GemmArgs::fix (K = the LayerNorm's row length, 256 .. 1024)
bool gemm_fix_capable(const Tuning &t, const GemmArgs &a);
// persistent grid of that GEMM (for the sub-batch cost model): workgroups per XCD are a multiple of the column tiles
int gemm_ln_grid(int n_cu, int M, int N);
// normalises the row blocks a fused GEMM left behind (todo[rb] == epoch) from x (layernorm.hip); a few microseconds when there are none
hipError_t launch_layernorm_fixup(int dtype, const float *x, const float *w, const float *b, void *y, int M, int D, float eps, const unsigned *todo, unsigned epoch, hipStream_t stream);
int gemm_ring_cfg(const Tuning &t, const GemmArgs &a);   // the ring configuration (245 or 122; 0: none) launch_gemm gives a shape that is not wide
int gemm_tile_m();   // M granularity the GEMM needs (buffer row padding)
int gemm_tile_n();

// Patch embedding in one launch (patch_embed.hip; vit.cpp:747-797): with T = 1 + n_reg prefix tokens and N = T + patches rows per image,
// X[b * N + T + t][:] = W . patch(b, t) + bias + pos[1 + t], X[b * N][:] = cls + pos[0], X[b * N + 1 + r][:] = reg[r] (no position term).
// img: f32 HWC [n_img][img_h][img_w][Cin], both sides multiples of P, patches in raster order with img_w / P per row (Cin = 3: RGB classifier input; 1: the grey ViTSTR input, extensions/vitstr.cpp/vitstr.cpp:713-731);
// w_perm: the [n_pad][k_pad] operand-type kernel with its K axis permuted by patch_embed_permute_k (host side, at upload); pos [1 + patches][D],
// cls [D], reg [n_reg][D] (nullptr when n_reg == 0).  cls == nullptr (n_reg == 0): no prefix token at all -- N = patches, X[b * N + t][:] = W . patch(b, t) + bias + pos[t],
// pos [patches][D] (a VITX_POOL_MAP model).
hipError_t launch_patch_embed(int dtype, const float *img, const void *w_perm, const float *bias, const float *pos, const float *cls, const float *reg, int n_reg,
                              float *X, int n_img, int img_h, int img_w, int P, int Cin, int D, int n_pad, int k_pad, hipStream_t stream);
void patch_embed_permute_k(const uint16_t *w, uint16_t *w_perm, int N, int Cin, int P, int k_pad);
// y[r][:] (dtype) = LN(x[r*ldx ...]) * w + b   (layernorm.hip; vit.cpp:808-812)
// group > 1: input row r = x + (r / group) * gstride + (r % group) * ldx (the first `group` tokens of every image: ViTSTR head)
hipError_t launch_layernorm(int dtype, const float *x, long ldx, const float *w, const float *b, void *y, long ldy, int M, int D, float eps, hipStream_t stream, int group = 1, long gstride = 0);
// y[r][:] (f32, NOT rounded) = LN(x[r][:]) * w + b, rows of D floats: the value launch_layernorm rounds -- same statistics, same operation order, every
// width of VITX_LN_WIDTHS.  y == x is allowed (a wave owns whole rows).  The pre-norm of a file with pre_norm.* (CLIP's pre_layrnorm), in place on X.
hipError_t launch_layernorm_f32(const float *x, const float *w, const float *b, float *y, int M, int D, float eps, hipStream_t stream);
// fused per-(image,head) attention  (vit.cpp:826-866): the dispatcher over the attention families (attention.hip)
hipError_t launch_attention(const Tuning &t, int dtype, const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream);
// Streaming two-pass kernel (attention_stream.hip), head dim 64, any token count.  precise = false: the long-sequence kernel of both
// operand types; precise = true (f16 only): the F16 parity mode's f32-grade products -- qkv is then the HI plane of the QKV GEMM's
// EPI_BIAS_HILO output and the LO plane lies lo_off elements behind it.
hipError_t launch_attention_stream(int dtype, bool precise, const void *qkv, void *out, int n_img, int N, int D, int H, long lo_off, hipStream_t stream);
bool attention_stream_supports(int n_img, int N, int D, int H);
// x[n] f32 -> hi[n] = round(x), lo[n] = round((x - hi) * 2048) in the operand type (what EPI_BIAS_HILO emits; parity-test entry point)
hipError_t launch_split_hilo(int dtype, const float *x, void *hi, void *lo, size_t n, hipStream_t stream);
// Attention of token 0 only (attention_cls.hip; the last layer of a classifier needs nothing else, vit.cpp:910-911): out[b][D] (dtype) from qkv[n_img * N][3 D]
// (lo_off != 0: the parity mode's lo plane, F16 only); xc != nullptr: also xc[b][D] = x[b * N][D] (the class rows of the f32 residual stream)
hipError_t launch_attention_cls(int dtype, const void *qkv, long lo_off, void *out, const float *x, float *xc, int n_img, int N, int D, int H, hipStream_t stream);
bool attention_cls_supports(int N, int D, int H);  // head_dim 8, 16, 32, 64 or 128
// Attention maps (attention_map.hip; vitx_attn_enable): f32 softmaxes of the operands in qkv (lo_off != 0: the parity mode's two planes, F16 only).
//   cls_map:   out[b * img_stride + h * N + j] = A_h[0][j] of image b (class-token row of every head)
//   head_mean: out[b][i][j] = mean_h A_h[i][j], or 0.5 mean_h A_h[i][j] + 0.5 [i == j] (half_identity: the rollout factor);  N <= kAttnMeanMaxTokens
//   rollout_step: a[b] <- a[b] . r[b] in place ([N][N] f32, exact f32 products);  rollout_row: out[b][k] = sum_j w_j r[b][j][k], w = row 0 of the
//   last layer's rollout factor from its class-token maps cls[b * cls_stride + h * N + j] (r == nullptr: out = w)
constexpr int kAttnMeanMaxTokens = 1024;
bool attention_map_supports(int N, int D, int H);      // head_dim a multiple of 8 up to 128, any token count
bool attention_mean_supports(int N, int D, int H);     // the same, at most kAttnMeanMaxTokens tokens
hipError_t launch_attention_cls_map(int dtype, const void *qkv, long lo_off, float *out, long img_stride, int n_img, int N, int D, int H, hipStream_t stream);
hipError_t launch_attention_head_mean(int dtype, const void *qkv, long lo_off, float *out, int n_img, int N, int D, int H, bool half_identity, hipStream_t stream);
hipError_t launch_rollout_step(float *a, const float *r, int n_img, int N, hipStream_t stream);
hipError_t launch_rollout_row(const float *cls, long cls_stride, const float *r, float *out, long out_stride, int n_img, int N, int H, hipStream_t stream);
// The same on a pack (vitx_pack_attn_enable): image i = rows row0[i] .. row0[i + 1] - 1 of qkv, N_i tokens, the fixed-shape launch's bits on that image
// alone (one body, attention_map_tile.h; no parity planes).  attn_pack_tables (host): rblk0 [n + 1] = the running count of ceil(N_i / 16), the
// work items of the head mean and the step; sq0 [n + 1] = the running sum of N_i^2, where image i's N_i x N_i matrix starts in out / a / r; *n_max =
// the widest image (the launches' NT); false when a count leaves 31 bits.  blocks = rblk0[n].  Device tables: row0, rblk0, sq0.
//   cls_map:  image i's [H][N_i] maps at float row0[i] * fpt + slot * H * N_i of out (fpt floats per token);
//   row:      its class maps at float row0[i] * cfpt + cslot * H * N_i of cls, its row [N_i] at float row0[i] * ofpt + ooff * N_i of out.
bool attn_pack_tables(const int32_t *row0, int n, int32_t *rblk0, int32_t *sq0, int *n_max);
hipError_t launch_attention_cls_map_packed(int dtype, const void *qkv, float *out, long fpt, int slot, const int *row0, int n, int D, int H, hipStream_t stream);
hipError_t launch_attention_head_mean_packed(int dtype, const void *qkv, float *out, const int *row0, const int *rblk0, const int *sq0, int n, int blocks, int n_max,
                                             int D, int H, bool half_identity, hipStream_t stream);
hipError_t launch_rollout_step_packed(float *a, const float *r, const int *row0, const int *rblk0, const int *sq0, int n, int blocks, int n_max, hipStream_t stream);
hipError_t launch_rollout_row_packed(const float *cls, long cfpt, int cslot, const float *r, float *out, long ofpt, long ooff, const int *row0, const int *sq0, int n,
                                     int n_max, int H, hipStream_t stream);
// Image embeddings and token features (features.hip; vitx_feat_enable): F = the f32 LayerNorm of launch_layernorm before its rounding.  Row t of
// image i is read at x + i * img_stride + t * row_stride; T = `first` is the first patch row (1 + the register tokens): cls[i * out_img_stride ..] =
// F[0], mean[..] = mean of F[T .. N-1], tokens[..] = F[T .. N-1] ([N-T][D]); any output may be nullptr (row 0 is read only for cls / z, rows T ..
// only for mean / tokens / z, rows 1 .. T-1 never); l2: cls and mean divided by their norm.
// z != nullptr: the pooled head's operand (VITX_POOL_CLS_MEAN), z[i][0 .. D) = RNE(F[0]), z[i][D .. 2 D) = RNE(mean) in the operand type `dtype`,
// rows of 2 D elements, rounded BEFORE any l2 -- the same launch that serves the features.
// Every width of VITX_LN_WIDTHS; pointers 16-byte aligned, strides multiples of 4 floats.
hipError_t launch_features(const float *x, long row_stride, long img_stride, const float *w, const float *b, float *cls, float *mean, float *tokens,
                           long out_img_stride, int n_img, int N, int D, float eps, bool l2, hipStream_t stream, int first = 1, void *z = nullptr, int dtype = DT_F16);
// The pooling kernel of the attention-pooling head (attention_pool.hip; include/vitx.h "no class token and the attention-pooling head"): with F[t] the
// f32 final-norm row of token t (launch_features' F, same statistics and operation order), s_{h,t} = u_h . F[t], p_h = softmax_t(s_h),
// M_h = sum_t p_{h,t} F[t], all f32.  Row t of image i is read at x + i * img_stride + t * row_stride; u [H][D] f32.  Outputs, each may be nullptr:
// M [n_img][H][D] f32; m16 [n_img][H][D] = RNE(M) in the operand type `dtype` (the value projection's A operand); p [n_img][H][N] f32.
// Every width of VITX_LN_WIDTHS, 1 <= H <= kPoolMaxHeads, any N >= 1; one workgroup per image and group of heads, no atomics.  hipErrorInvalidValue otherwise.
constexpr int kPoolMaxHeads = 32;
hipError_t launch_attention_pool(const float *x, long row_stride, long img_stride, const float *w, const float *b, float eps, const float *u, float *M, void *m16, int dtype,
                                 float *p, int n_img, int N, int D, int H, hipStream_t stream);
// The end of the pooled tail: e [n_img][D] f32 -> z [n_img][D] = RNE(e) in `dtype` (the head GEMM's operand) and, cls != nullptr, the feature
// cls[i * out_img_stride ..] = e[i] (l2: divided by its norm, VITX_FEAT_L2's arithmetic).  One wave per image.
hipError_t launch_pool_embed(const float *e, void *z, int dtype, float *cls, long out_img_stride, bool l2, int n_img, int D, hipStream_t stream);
// Zero-shot classification (zeroshot.hip; include/vitx.h "zero-shot classification"): the two kernels around the bank GEMM.
//   zs_embed: row i of z (f32, at z + i * z_stride floats) -> a[i][0 .. E) = RNE(z / sqrt(sum z^2)) in `dtype`, an all-zero row stays zero; rows
//             n .. m_pad of a are written as zeros.  E a multiple of 64; z rows 16-byte aligned (z_stride a multiple of 4).
//   zs_score: acc [n][ld] f32 -> logits[i * out_img_stride + k] = acc[i][k] * scale + bias and probs[..] = softmax over k < K (VITX_ZS_SOFTMAX) or
//             the sigmoid (VITX_ZS_SIGMOID); columns K .. ld are never read.  One workgroup per image.
// hipErrorInvalidValue for a shape outside that.
hipError_t launch_zs_embed(int dtype, const float *z, long z_stride, void *a, int n, int m_pad, int E, hipStream_t stream);
// zs_embed with an f32 result, unrounded (VITX_TEXT_L2): a[i][0 .. E) = z / sqrt(sum z^2), dense rows of E floats, a != z; the same kernel text, one more instantiation
hipError_t launch_zs_embed_f32(const float *z, long z_stride, float *a, int n, int E, hipStream_t stream);
hipError_t launch_zs_score(const float *acc, int ld, float *probs, float *logits, long out_img_stride, int n, int K, int kind, float scale, float bias, hipStream_t stream);
// zs_embed on rows that are already in the operand type (the head GEMM's operand Z; z_stride in elements, a multiple of 4): every element widened to
// f32 first, then the same kernel text -- one more instantiation, not a second rule
hipError_t launch_zs_embed_operand(int dtype, const void *z, long z_stride, void *a, int n, int m_pad, int E, hipStream_t stream);
// Nearest neighbours in a gallery (nn_select.hip; include/vitx.h "nearest neighbours in a gallery"): the streaming selection around the chunk GEMMs.
//   nn_select: scores [n][ld] f32, columns 0 .. cols of one chunk (columns cols .. ld never read), column j = gallery row base_index + j (below 2^31)
//              -> merged into state [n][kNnSegs][k] 64-bit keys (nn_state_bytes); first: the state is initialised by this launch, not read.
//   nn_finish: state -> pairs [n][k] {f32 score, i32 index} best first (launch_topk's layout); labels != nullptr ([every index in the state] i32 in
//              [0, n_labels)): also vote [n][n_labels] f32 with temperature T > 0.
// 1 <= k <= kNnMaxK.  hipErrorInvalidValue for a shape outside that.
constexpr int kNnSegs = 8, kNnMaxK = 64;
size_t nn_state_bytes(int n, int k);
hipError_t launch_nn_select(const float *scores, long ld, int n, int cols, long base_index, void *state, int k, bool first, hipStream_t stream);
hipError_t launch_nn_finish(const void *state, int n, int k, const int *labels, int n_labels, float temperature, void *pairs, float *vote, hipStream_t stream);
// The label map of the dense head (dense_label.hip; include/vitx.h "dense prediction"): logits [n * gh * gw][ld] f32 (ld a multiple of 4, at least K rounded
// up to 4; columns K .. ld never compared; 16-byte aligned) -> labels [n][out_h][out_w] u8 and, score != nullptr, score [n][out_h][out_w] f32: the K
// planes resampled bilinearly (dense_resample.h) and arg-maxed in vitx_topk's order.  1 <= K <= kDenseMaxK, gh <= out_h <= kDenseMaxOut (and w),
// n <= 65535.  hipErrorInvalidValue for a shape outside that (dense_labels_supports).
constexpr int kDenseMaxK = 256, kDenseMaxOut = 8192;
bool dense_labels_supports(long ld, int n, int gh, int gw, int K, int out_h, int out_w);
hipError_t launch_dense_labels(const float *logits, long ld, int n, int gh, int gw, int K, int out_h, int out_w, uint8_t *labels, float *score, hipStream_t stream);
// The same on a PACK (include/vitx.h "packed batches", the dense head): image i has its own first logit row lrow[i], grid grids[i] = (gh, gw) and output
// outs[i] = (oh, ow); its maps start pix0[i] elements into labels and score (the maps end to end), bit for bit what launch_dense_labels writes for it alone.
//   dense_pack_tables   host only, the one place the tables are built (the launch, vitx_pack_dense_check and a later head on packs): pix0 [n + 1] = the
//                       running pixel count, tile0 [n + 1] = the running count of kDenseTileW x kDenseTileH tiles, *cells = the widest tile window of any
//                       image (it sizes the LDS and the class chunk of the launch); any of the three may be NULL.  false: a grid below 1, an output
//                       outside grid .. kDenseMaxOut, or more than 2^31 - 1 tiles.
//   dense_pack_seg      the device table's rows seg [n][kDenseSegInts]: lrow, gh, gw, oh, ow, pix0 (low, high word), the bits of dense_scale for y and x, 0
//   launch_dense_labels_packed   tile0 and seg on the device; tiles = tile0[n] and cells from dense_pack_tables: the caller built the tables
constexpr int kDenseSegInts = 10;
bool dense_pack_tables(const int32_t *grids, const int32_t *outs, int n, int64_t *pix0, int32_t *tile0, int *cells);
void dense_pack_seg(const int32_t *grids, const int32_t *outs, const int32_t *lrow, const int64_t *pix0, int n, int32_t *seg);
hipError_t launch_dense_labels_packed(const float *logits, long ld, const int *tile0, const int *seg, int n, int tiles, int cells, int K, uint8_t *labels, float *score,
                                      hipStream_t stream);
// The tail of the depth head (depth_map.hip; include/vitx.h "depth estimation"; the arithmetic: dense_resample.h + depth_bins.h).
//   depth_fine:   logits [n * gh * gw][ld] f32 (ld a multiple of 4, at least K rounded up to 4; columns K .. ld never summed; 16-byte aligned) + offsets
//                 (row img * ldo, ldo floats apart -- ldo == 0: one row for every image; nullptr: nothing is added), bins [K] -> fine [n][u gh][u gw] f32
//   depth_resize: fine [n][fh][fw] -> out [n][out_h][out_w] f32 (any 4-byte alignment), clamped to lo .. hi; fh <= out_h <= kDepthMaxOut (and w)
//   depth_rows:   y[row][0 .. D) (dtype, row stride ldy elements) = RNE(x row), row = g * group + r read at x + g * gstride + r * ldx; D % 8 == 0
// 1 <= K <= kDepthMaxK, u in {1, 2, 4}, n <= 65535.  hipErrorInvalidValue for a shape outside that (depth_*_supports).
bool depth_fine_supports(long ld, long ldo, int n, int gh, int gw, int K, int u);
bool depth_resize_supports(int n, int fh, int fw, int out_h, int out_w);
hipError_t launch_depth_fine(const float *logits, long ld, const float *offsets, long ldo, const float *bins, int n, int gh, int gw, int K, int u, float *fine, hipStream_t stream);
hipError_t launch_depth_resize(const float *fine, int n, int fh, int fw, int out_h, int out_w, float lo, float hi, float *out, hipStream_t stream);
hipError_t launch_depth_rows(int dtype, const float *x, long ldx, void *y, long ldy, long rows, int D, hipStream_t stream, int group = 1, long gstride = 0);
// The same tail on a PACK (include/vitx.h "packed batches", the depth head): image i has its own first logit row lrow[i], offsets row orow[i] (row
// orow[i] * ldo of `offsets`), grid grids[i] = (gh, gw), fine plane (u gh, u gw) and output outs[i] = (oh, ow); its fine plane starts fine0[i] floats
// into `fine`, its map pix0[i] floats into `out` (planes and maps end to end), bit for bit what launch_depth_fine / launch_depth_resize write for it alone.
//   depth_pack_tables   host only, the one place the tables are built: pix0 / fine0 [n + 1] = the running pixel counts of the maps and the fine planes,
//                       ftile0 / otile0 [n + 1] = the running counts of kDepthTile x kDepthTile fine tiles and kDepthOutW x kDepthOutH output tiles, *cells =
//                       the widest fine-tile window of any image (it sizes the LDS and the bin chunk of the launch); any of the five may be NULL.  false:
//                       u not 1, 2 or 4, a grid below 1, a fine side above kDepthMaxOut, an output outside fine .. kDepthMaxOut, or more than 2^31 - 1 tiles.
//   depth_pack_seg      the device table's rows seg [n][kDepthSegInts]: lrow, orow, gh, gw, u gh, u gw, oh, ow, fine0 (low, high word), pix0 (low, high
//                       word), the bits of dense_scale for the fine plane's y and x and for the map's y and x
//   launch_depth_*_packed   ftile0 / otile0 and seg on the device; tiles = ftile0[n] / otile0[n] and cells from depth_pack_tables: the caller built the tables
//   depth_gather        dst[i][0 .. Dc) = src[rows[i]][0 .. Dc), operand-type rows of Dc elements (Dc % 8 == 0), rows [n] on the device
constexpr int kDepthSegInts = 16;
bool depth_pack_tables(const int32_t *grids, const int32_t *outs, int n, int u, int64_t *pix0, int64_t *fine0, int32_t *ftile0, int32_t *otile0, int *cells);
void depth_pack_seg(const int32_t *grids, const int32_t *outs, const int32_t *lrow, const int32_t *orow, const int64_t *fine0, const int64_t *pix0, int n, int u, int32_t *seg);
hipError_t launch_depth_fine_packed(const float *logits, long ld, const float *offsets, long ldo, const float *bins, const int *ftile0, const int *seg, int n, int tiles,
                                    int cells, int K, float *fine, hipStream_t stream);
hipError_t launch_depth_resize_packed(const float *fine, const int *otile0, const int *seg, int n, int tiles, float lo, float hi, float *out, hipStream_t stream);
hipError_t launch_depth_gather(const void *src, int Dc, const int *rows, void *dst, int n, hipStream_t stream);
// The text tower (include/vitx.h "the text tower"; text_embed.hip, attention_text.hip).
//   text_embed: X[i][t][:] (f32) = f32(tok[ids[i * T + t]][:]) + pos[t][:]; tok [V][D] f16 (table_f16) or f32, ids checked by the caller; D % 8 == 0
//   text_pool:  z[i][:] (dtype) = RNE(final LayerNorm of X row i * T + pooled[i]), LnRow's bits; rows n .. m_pad zeros; every width of VITX_LN_WIDTHS
//   attention_text: qkv [n * T][3 D] -> out [n * T][D] (dtype), 1 <= T <= 128, head dim a multiple of 8 up to 128; causal != 0: row t attends keys 0 .. t
hipError_t launch_text_embed(bool table_f16, const void *tok, const float *pos, const int *ids, float *X, int n, int T, int D, hipStream_t stream);
hipError_t launch_text_pool(int dtype, const float *X, const int *pooled, const float *w, const float *b, void *z, int n, int m_pad, int T, int D, float eps, hipStream_t stream);
hipError_t launch_attention_text(int dtype, const void *qkv, void *out, int n, int T, int D, int H, int causal, hipStream_t stream);
bool attention_text_supports(int T, int D, int H);
// Rotary position embeddings (rope.hip; include/vitx.h "rotary position embeddings"), in place on qkv [n_img * N][3 D] (lo_off != 0: the parity mode's
// lo plane, F16 only): q and k of every token t >= prefix rotated by cos / sin [N - prefix][hd / 2] f32, half-split pairs (j, j + hd / 2) of each head;
// v columns, prefix rows and everything behind row n_img * N untouched.  Any even head dim; 16-byte accesses where hd / 2 is a multiple of 8.
hipError_t launch_rope(int dtype, void *qkv, long lo_off, const float *cos, const float *sin, int n_img, int N, int prefix, int D, int H, hipStream_t stream);
bool rope_supports(int D, int H);
// Packed batches (include/vitx.h "packed batches"): images of different token counts end to end, image i = rows row0[i] .. row0[i + 1] - 1 (device
// int32 [n + 1]); the three kernels that must know where an image begins.
//   attention_packed: qkv [rows][3 D] -> out [rows][D], image i's rows with the bits of launch_attention_generic on that image alone (attention_packed.hip);
//                     qb0 [n + 1] device: the running count of 64-query blocks, qblocks = qb0[n] on the host
//   rope_packed:      launch_rope's kernel text; image i's table ([N_i - prefix][hd / 2]) starts toff[i] floats into cos and sin; patch_rows = all patch
//                     rows of the pack, toff_aligned = every toff[i] is a multiple of 4 (the 16-byte form needs it)
//   pool_rows:        launch_text_pool's kernel text on absolute rows: z[i][:] = RNE(final LayerNorm of X row rows[i]); rows n .. m_pad zeros
hipError_t launch_attention_packed(int dtype, const void *qkv, void *out, const int *row0, const int *qb0, int n, long qblocks, int D, int H, hipStream_t stream);
bool attention_packed_supports(int D, int H);      // attention_generic_supports
hipError_t launch_rope_packed(int dtype, void *qkv, const float *cos, const float *sin, const int *row0, const int *toff, int n, long patch_rows, bool toff_aligned, int prefix, int D,
                              int H, hipStream_t stream);
hipError_t launch_pool_rows(int dtype, const float *X, const int *rows, const float *w, const float *b, void *z, int n, int m_pad, int D, float eps, hipStream_t stream);
// The gate of a gated MLP (swiglu.hip; include/vitx.h "gated MLP"): in [rows][ld_in] of `dtype`, gate in columns 0 .. F-1, up in F .. 2F-1 ->
// out[r][j] = RNE(silu(f32 gate) * f32 up), j < F, rows of ld_out elements; nothing else of `out` is touched.  hipErrorInvalidValue, before any
// launch, for F % 8 != 0, a pointer off a 16-byte boundary, a leading dimension that is no multiple of 8, ld_in < 2 F or ld_out < F.
hipError_t launch_swiglu(int dtype, const void *in, long ld_in, void *out, long ld_out, long rows, int F, hipStream_t stream);
// pos [1 + gy_in * gx_in][D] f32 -> out [1 + gy_out * gx_out][D] f32 (pos_resample.hip; the arithmetic: pos_resample.h); only enqueues
hipError_t launch_pos_resample(const float *pos, int gy_in, int gx_in, int D, int gy_out, int gx_out, int interp, float *out, hipStream_t stream);
bool attention_supports(int N, int D, int H);     // any token count; head_dim 64 (tuned kernels) or any other multiple of 8 up to 128 (generic kernel)
bool attention_single_pass_supports(int N);       // instantiation table of the register-resident kernel
bool layernorm_supports(int D);
// The LayerNorm instantiation table (hidden size D, columns per lane VEC, pieces NV; D = 64 VEC NV: LnRow<VEC, NV> of ln_row.h), ONE list for every
// kernel that normalises a row: widths of the timm ViTs (SO400M 1152, ViT-g 1408, ViT-G 1664, ...) and of small test models
#define VITX_LN_WIDTHS(X)                                                                                                  \
    X(64, 1, 1) X(128, 2, 1) X(192, 1, 3) X(256, 4, 1) X(384, 2, 3) X(512, 4, 2) X(768, 4, 3) X(1024, 4, 4) X(1280, 4, 5) X(1536, 4, 6) \
    X(320, 1, 5) X(448, 1, 7) X(576, 1, 9) X(640, 2, 5) X(896, 2, 7) X(1152, 2, 9) X(1408, 2, 11) X(1664, 2, 13) X(2048, 4, 8)
// The table's one dispatcher: f(integral_constant<int, VEC>, integral_constant<int, NV>) for D's row; false, and f not called, if D has none
template <typename F> bool ln_for_width(int D, F &&f) {
    switch (D) {
#define VITX_LN_CASE(DD, VEC, NV) case DD: f(std::integral_constant<int, VEC>{}, std::integral_constant<int, NV>{}); return true;
        VITX_LN_WIDTHS(VITX_LN_CASE)
#undef VITX_LN_CASE
    default: return false;
    }
}
// class softmax with the reference's fp16 (or bf16) exp rounding (softmax_topk.hip; vit.cpp:931)
hipError_t launch_softmax(int dtype, const float *logits, float *probs, int rows, int cols, int ld, hipStream_t stream);
// u8 HWC [n][ny][nx][3] -> f32 HWC [n][S][S][3], resized and normalised (image_preprocess.hip; bit for bit the host version in preprocess.cpp)
hipError_t launch_preprocess(const void *u8, float *out, int n, int nx, int ny, int S, int bicubic, hipStream_t stream);
// the same by a description (include/vitx.h vitx_preproc): the reference's resize with its mean / std, or Pillow's resize + centre crop, one launch.
// hipErrorInvalidValue for an invalid description or source, or a down-scale whose tile does not fit the LDS (preprocess_ex_supports)
hipError_t launch_preprocess_ex(const vitx_preproc &p, const void *u8, float *out, int n, int nx, int ny, hipStream_t stream);
bool preprocess_ex_supports(const vitx_preproc &p, int nx, int ny);
// the PIL kernel with a rectangular output window: the whole source stretched to out_w x out_h with the description's filter and mean / std
// (vitx_preprocess_rect_device); hipErrorInvalidValue also for a REF filter
hipError_t launch_preprocess_rect(const vitx_preproc &p, const void *u8, float *out, int n, int nx, int ny, int out_w, int out_h, hipStream_t stream);
bool preprocess_rect_supports(const vitx_preproc &p, int nx, int ny, int out_w, int out_h);
// The PIL kernel on a PACK (pp_pil_packed_kernel): source i u8 HWC [ny_i][nx_i][3], the sources strictly end to end, stretched to its own oh_i x ow_i, the
// f32 HWC outputs end to end; image i's floats are the bits of launch_preprocess_rect on it alone.  A work item is (image, 32 x 8 output tile).
//   pp_pack_tables   host only, the one place the tables are built and the one text of every refusal (the context's forward, vitx_pack_u8_check, the
//                    op): src_shapes [n][2] = (ny, nx), out_shapes [n][2] = (oh, ow) -> src0 [n + 1] bytes, dst0 [n + 1] floats, tile0 [n + 1] the
//                    running tile count, seg [n][kPpSegInts] the device table's rows -- source byte offset and destination float offset (low, high
//                    word each), nx, ny, ow, oh, tiles_x, then the image's own kx, ky, rows, span, stage of pp_tiling -- and *lds, the largest
//                    pp_tiling().lds of the call; any output may be NULL.  VITX_OK, or the refusal's code with "<api>: ..." as the error text:
//                    VITX_ERR_ARG for an invalid description or a side out of range, VITX_ERR_UNSUPPORTED for a REF filter and for an image whose
//                    tiling is above PP_LDS_LIMIT (the text names the image), VITX_ERR_ARG for more than 2^31 - 1 tiles.
//   launch_preprocess_pack   tile0 and seg on the device; tiles = tile0[n] and lds from pp_pack_tables: the caller built the tables.  u8 is 4-byte
//                    aligned and readable up to its byte count rounded up to 4 (the staged dword loads).
constexpr int kPpSegInts = 14;
int pp_pack_tables(const char *api, const vitx_preproc &p, const int32_t *src_shapes, const int32_t *out_shapes, int n, int64_t *src0, int64_t *dst0, int32_t *tile0,
                   int32_t *seg, int *lds);
hipError_t launch_preprocess_pack(const vitx_preproc &p, const void *u8, float *out, const int *tile0, const int *seg, int n, int tiles, int lds, hipStream_t stream);
// out[row][k] = {f32 probability, i32 class} of the k largest entries of probs[row][0..cols), descending, ties by the lower class index
// (softmax_topk.hip; the sort of vit_predict, vit.cpp:1043-1057, on the device: the multi-GPU gather then moves 8 k bytes per row instead of 4 cols)
hipError_t launch_topk(const float *probs, int rows, int cols, int k, void *out_pairs, hipStream_t stream);
// one workgroup that does nothing for `microseconds` of the 100 MHz wall clock (probe.hip; stream-concurrency probe of the execution context)
hipError_t launch_spin(int microseconds, hipStream_t stream);
// the same, writing its first and last wall-clock reading (100 MHz ticks) to stamps[0..1] (device memory)
hipError_t launch_spin_stamp(int microseconds, long long *stamps, hipStream_t stream);


// ---- MXFP8 operands (gemm_mx8.hip; include/vitx.h VITX_MXFP8, the encoding: mxfp8.h) ---------------------------------
// C = A . W^T on v_mfma_scale_f32_16x16x128_f8f6f4.  a.A = elements [M_real][K], a.W = [N_pad][K] (K = K_pad, a multiple of 128;
// N_pad a multiple of 128), scales [rows][K / 32] beside them.  EPI_BIAS -> bf16 [M][ldo]; EPI_BIAS_RESID -> f32 [M][ldo] += ;
// EPI_BIAS_GELU -> MX elements a.out [M][ldo] (ldo = the next GEMM's K_pad) + out_scales [M][ldo / 32] of gelu_tanh(acc + bias).
hipError_t launch_gemm_mx8(int epi, const GemmArgs &a, const uint8_t *a_scales, const uint8_t *w_scales, uint8_t *out_scales, hipStream_t stream);
bool gemm_mx8_supports(const GemmArgs &a);
// LayerNorm -> MX: the f32 value launch_layernorm rounds, encoded; rows [M][k_pad] + [M][k_pad / 32], columns D .. k_pad zero (scale 127)
hipError_t launch_layernorm_mx8(const float *x, long ldx, const float *w, const float *b, uint8_t *q, uint8_t *s, int k_pad, int M, int D, float eps, hipStream_t stream);
// x f32 [rows][K] -> MX [rows][k_pad] (test entry point of the device encoder)
hipError_t launch_quantize_mx8(const float *x, int rows, int K, int k_pad, uint8_t *q, uint8_t *s, hipStream_t stream);
// host encoder (mxfp8.cpp): the same rule, bit for bit
void mxfp8_encode_rows(const float *x, int rows, int K, int k_pad, uint8_t *q, uint8_t *scales);

// internal: kernel families.  `prepare` = only set the dynamic-LDS attribute of the instantiation (device bring-up).
hipError_t launch_gemm_ring(const Tuning &t, int dtype, int epi, const GemmArgs &a, int cfg, hipStream_t stream, bool prepare = false);
bool gemm_ring_supports(const GemmArgs &a, int cfg);
hipError_t launch_gemm_pp(int dtype, int epi, const GemmArgs &a, int n_cu, hipStream_t stream, int flags = 0, bool prepare = false);
bool gemm_pp_supports(const GemmArgs &a);
// free-running wide kernels (gemm_w4.hip; LABORATORY BUILD ONLY: tools/Makefile), waves = 8: two waves per SIMD, 128 x 64 of C per wave; 4: one
// per SIMD, 128 x 128 per wave.  EPI_BIAS, EPI_BIAS_GELU (tanh only: hipErrorInvalidValue for the other activations); same bits as the other families
hipError_t launch_gemm_w4(int dtype, int epi, const GemmArgs &a, int n_cu, hipStream_t stream, int flags = 0, bool prepare = false, int waves = 8);
bool gemm_w4_supports(const GemmArgs &a);
bool attention_persist_supports(int n_img, int N, int D);      // attention_persist.hip: 193..224 tokens, the whole QKV tensor below 0xf0000000 bytes
bool attention_generic_supports(int D, int H);                 // attention_generic.hip: head_dim any multiple of 8 up to 128

// FN<_Float16>(args) for DT_F16, FN<__bf16>(args) for any other dtype: how a launcher that takes `int dtype` enters its per-type template.
// VITX_BY_DTYPE2: FN has one more template argument X after the type.
#define VITX_BY_DTYPE(dtype, FN, ...) ((dtype) == DT_F16 ? FN<_Float16>(__VA_ARGS__) : FN<__bf16>(__VA_ARGS__))
#define VITX_BY_DTYPE2(dtype, FN, X, ...) ((dtype) == DT_F16 ? FN<_Float16, X>(__VA_ARGS__) : FN<__bf16, X>(__VA_ARGS__))

// The rest is reached from inside the library only (launch_attention, tuning_for_device) and stays out of its dynamic symbol table.
#pragma GCC visibility push(hidden)
// The attention families launch_attention chooses among, head dim 64 unless said otherwise; each checks nothing launch_attention has checked.
hipError_t launch_attention_single(int dtype, const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream);      // attention_single.hip: N per attention_single_pass_supports
hipError_t launch_attention_flow(int dtype, const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream, int flags = 0);      // attention_flow.hip: any N
hipError_t launch_attention_persist(int dtype, const void *qkv, void *out, int n_img, int N, int D, int H, int n_cu, hipStream_t stream, int flags = 0);      // attention_persist.hip
hipError_t launch_attention_generic(int dtype, const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream);      // attention_generic.hip
// Device bring-up: every kernel instantiation that needs more than 64 KiB of LDS gets its dynamic-LDS attribute on the current device, by the
// file that holds the instantiation table.  tuning_for_device runs these once per device.
hipError_t prepare_gemm(const Tuning &t);              // gemm.hip: ring, ping-pong and q4_0 GEMMs (laboratory build: gemm_w4 too)
hipError_t prepare_patch_embed();                      // patch_embed.hip
hipError_t prepare_attention();                        // attention.hip: the four below, each in its family's file
hipError_t prepare_attention_single();
hipError_t prepare_attention_flow();
hipError_t prepare_attention_persist();
hipError_t prepare_attention_stream();
hipError_t prepare_attention_text();                   // attention_text.hip
hipError_t prepare_dense();                            // dense_label.hip
hipError_t prepare_depth();                            // depth_map.hip
#pragma GCC visibility pop

}  // namespace vitx
