// attention_map.hip -- attention maps and attention rollout (vitx_attn_enable, vitx_op_attention_map).
//
// Opt-in outputs of the forward: what the model looked at.  The kernels only READ the QKV scratch a layer's qkv projection wrote
// ([n_img * N][3 D] in the operand type; q of head h at column h * hd, k at D + h * hd) and write buffers of their own, so the
// forward's own results do not change.  Semantics (include/vitx.h): the maps are f32 softmaxes of the context's own q, k --
// s = (q . k) / sqrt(hd) in f32, A = expf(s - max) / sum -- not the rounded numerators the attention kernels multiply v with.
//   attn_cls_map_kernel    class-token row A_h[0][0..N) of every head: one query row against N keys, bound by reading K: VALU f32 FMAs on
//                          16-byte loads, one workgroup per (image, head), the raw scores parked in the output row itself;
//   attn_head_mean_kernel  mean_h A_h (or 0.5 mean_h A_h + 0.5 I, the rollout factor) for a block of 16 query rows: S = Q K^T on
//                          v_mfma_f32_16x16x32 (parity mode: hi.hi + (hi.lo + lo.hi) / 2048), every score and the head mean in registers;
//   attn_rollout_step_kernel  R_l = A^_l R_(l-1) on v_mfma_f32_16x16x4_f32 (exact f32), in place over A^_l: a workgroup owns a block of
//                          16 rows of A^_l and reads all of them into LDS before it writes any of them;
//   attn_rollout_row_kernel   the last factor: row 0 of A^_(L-1) R_(L-2) from the last layer's class-token maps (a GEMV).
// The bodies live in attention_map_tile.h.  Each kernel has a *_packed_kernel twin over the same body for a packed context (vitx_pack_attn_enable),
// where image i has its own N_i = row0[i + 1] - row0[i]: the class map's and the row's work items are (image, head) and (image); the head mean's
// and the step's are (image, 16-row block), found by a scalar binary search of the workgroup index in rblk0 [n + 1], the running count of
// ceil(N_i / 16), and image i's N_i x N_i matrix starts at float sq0[i], the running sum of N_j^2.  1-D grids, no atomics, one writer per element.
#include <hip/hip_runtime.h>
#include <math.h>

#include "attention_map_tile.h"
#include "kernels.h"

namespace vitx {
namespace {

template <typename T, int NPP, bool PLANES>
__global__ __launch_bounds__(256) void attn_cls_map_kernel(const T *__restrict__ qkv, long lo_off, float *__restrict__ out, long img_stride,
                                                          int N, int D, int H, int NP, float scale) {
    const int item = blockIdx.x, b = item / H, h = item - b * H;      // out row of head h of image b: out + b * img_stride + h * N
    map_cls_item<T, NPP, PLANES>(qkv + (size_t)b * N * ((size_t)3 * D), lo_off, out + (size_t)b * img_stride + (size_t)h * N, N, D, h, D / H, NP, scale);
}
// a pack: image b = rows row0[b] .. of qkv; its [H][N_b] maps start at float row0[b] * fpt + slot * H * N_b of out (fpt floats per token)
template <typename T, int NPP>
__global__ __launch_bounds__(256) void attn_cls_map_packed_kernel(const T *__restrict__ qkv, float *__restrict__ out, long fpt, int slot, const int *__restrict__ row0,
                                                                 int D, int H, int NP, float scale) {
    const int item = blockIdx.x, b = item / H, h = item - b * H;
    const int r0 = row0[b], N = row0[b + 1] - r0;
    map_cls_item<T, NPP, false>(qkv + (size_t)r0 * ((size_t)3 * D), 0, out + (size_t)r0 * fpt + ((size_t)slot * H + h) * N, N, D, h, D / H, NP, scale);
}

template <typename T, int NT, bool PLANES>
__global__ __launch_bounds__(256) void attn_head_mean_kernel(const T *__restrict__ qkv, long lo_off, float *__restrict__ out, int N, int D, int H,
                                                            float scale, int half_identity) {
    const int qblocks = (N + 15) / 16;
    const int b = blockIdx.x / qblocks, q0 = (blockIdx.x - b * qblocks) * 16;
    map_head_mean_block<T, NT, PLANES>(qkv + (size_t)b * N * ((size_t)3 * D), lo_off, out + (size_t)b * N * N, N, D, H, q0, scale, half_identity);
}
template <typename T, int NT>
__global__ __launch_bounds__(256) void attn_head_mean_packed_kernel(const T *__restrict__ qkv, float *__restrict__ out, const int *__restrict__ row0,
                                                                   const int *__restrict__ rblk0, const int *__restrict__ sq0, int n, int D, int H, float scale,
                                                                   int half_identity) {
    const int b = map_find_image(rblk0, n, blockIdx.x);
    const int r0 = row0[b], N = row0[b + 1] - r0, q0 = (blockIdx.x - rblk0[b]) * 16;
    map_head_mean_block<T, NT, false>(qkv + (size_t)r0 * ((size_t)3 * D), 0, out + (size_t)sq0[b], N, D, H, q0, scale, half_identity);
}

template <int NT>
__global__ __launch_bounds__(256) void attn_rollout_step_kernel(float *__restrict__ a, const float *__restrict__ r, int N) {
    const int rblocks = (N + 15) / 16;
    const int b = blockIdx.x / rblocks, i0 = (blockIdx.x - b * rblocks) * 16;
    rollout_step_block<NT>(a + (size_t)b * N * N, r + (size_t)b * N * N, N, i0);
}
template <int NT>
__global__ __launch_bounds__(256) void attn_rollout_step_packed_kernel(float *__restrict__ a, const float *__restrict__ r, const int *__restrict__ row0,
                                                                      const int *__restrict__ rblk0, const int *__restrict__ sq0, int n) {
    const int b = map_find_image(rblk0, n, blockIdx.x);
    const int N = row0[b + 1] - row0[b], i0 = (blockIdx.x - rblk0[b]) * 16;
    rollout_step_block<NT>(a + (size_t)sq0[b], r + (size_t)sq0[b], N, i0);
}

__global__ __launch_bounds__(256) void attn_rollout_row_kernel(const float *__restrict__ cls, long cls_stride, const float *__restrict__ r,
                                                              float *__restrict__ out, long out_stride, int N, int H) {
    const int b = blockIdx.x;
    rollout_row_image(cls + (size_t)b * cls_stride, r ? r + (size_t)b * N * N : nullptr, out + (size_t)b * out_stride, N, H);
}
// a pack: image b's class maps [H][N_b] start at float row0[b] * cfpt + cslot * H * N_b of cls, its row at float row0[b] * ofpt + ooff * N_b of out
__global__ __launch_bounds__(256) void attn_rollout_row_packed_kernel(const float *__restrict__ cls, long cfpt, int cslot, const float *__restrict__ r,
                                                                     float *__restrict__ out, long ofpt, long ooff, const int *__restrict__ row0,
                                                                     const int *__restrict__ sq0, int H) {
    const int b = blockIdx.x;
    const int r0 = row0[b], N = row0[b + 1] - r0;
    rollout_row_image(cls + (size_t)r0 * cfpt + (size_t)cslot * H * N, r ? r + (size_t)sq0[b] : nullptr, out + (size_t)r0 * ofpt + (size_t)ooff * N, N, H);
}

template <typename T, bool PLANES>
hipError_t launch_cls_map_t(const void *qkv, long lo_off, float *out, long img_stride, int n_img, int N, int D, int H, hipStream_t st) {
    const int np = D / H / 8;
    const float scale = 1.0f / sqrtf((float)(D / H));
    const dim3 grid((unsigned)((size_t)n_img * H)), blk(256);
#define VITX_MAPC(NPP) hipLaunchKernelGGL((attn_cls_map_kernel<T, NPP, PLANES>), grid, blk, 0, st, (const T *)qkv, lo_off, out, img_stride, N, D, H, np, scale)
    if (np <= 1) VITX_MAPC(1);
    else if (np <= 2) VITX_MAPC(2);
    else if (np <= 4) VITX_MAPC(4);
    else if (np <= 8) VITX_MAPC(8);
    else VITX_MAPC(16);
#undef VITX_MAPC
    return hipGetLastError();
}

template <typename T, bool PLANES>
hipError_t launch_head_mean_t(const void *qkv, long lo_off, float *out, int n_img, int N, int D, int H, bool half_identity, hipStream_t st) {
    const float scale = 1.0f / sqrtf((float)(D / H));
    const dim3 grid((unsigned)((size_t)n_img * ((N + 15) / 16))), blk(256);
    const int nt = (N + 63) / 64;
#define VITX_MAPM(NT) hipLaunchKernelGGL((attn_head_mean_kernel<T, NT, PLANES>), grid, blk, 0, st, (const T *)qkv, lo_off, out, N, D, H, scale, half_identity ? 1 : 0)
    if (nt <= 1) VITX_MAPM(1);
    else if (nt <= 2) VITX_MAPM(2);
    else if (nt <= 4) VITX_MAPM(4);
    else if (nt <= 8) VITX_MAPM(8);
    else VITX_MAPM(16);
#undef VITX_MAPM
    return hipGetLastError();
}

template <typename T>
hipError_t launch_cls_map_packed_t(const void *qkv, float *out, long fpt, int slot, const int *row0, int n, int D, int H, hipStream_t st) {
    const int np = D / H / 8;
    const float scale = 1.0f / sqrtf((float)(D / H));
    const dim3 grid((unsigned)((size_t)n * H)), blk(256);
#define VITX_MAPC(NPP) hipLaunchKernelGGL((attn_cls_map_packed_kernel<T, NPP>), grid, blk, 0, st, (const T *)qkv, out, fpt, slot, row0, D, H, np, scale)
    if (np <= 1) VITX_MAPC(1);
    else if (np <= 2) VITX_MAPC(2);
    else if (np <= 4) VITX_MAPC(4);
    else if (np <= 8) VITX_MAPC(8);
    else VITX_MAPC(16);
#undef VITX_MAPC
    return hipGetLastError();
}

template <typename T>
hipError_t launch_head_mean_packed_t(const void *qkv, float *out, const int *row0, const int *rblk0, const int *sq0, int n, int blocks, int n_max, int D, int H,
                                     bool half_identity, hipStream_t st) {
    const float scale = 1.0f / sqrtf((float)(D / H));
    const dim3 grid((unsigned)blocks), blk(256);
    const int nt = (n_max + 63) / 64;
#define VITX_MAPM(NT) hipLaunchKernelGGL((attn_head_mean_packed_kernel<T, NT>), grid, blk, 0, st, (const T *)qkv, out, row0, rblk0, sq0, n, D, H, scale, half_identity ? 1 : 0)
    if (nt <= 1) VITX_MAPM(1);
    else if (nt <= 2) VITX_MAPM(2);
    else if (nt <= 4) VITX_MAPM(4);
    else if (nt <= 8) VITX_MAPM(8);
    else VITX_MAPM(16);
#undef VITX_MAPM
    return hipGetLastError();
}

}  // namespace

bool attention_map_supports(int N, int D, int H) { return H > 0 && D % H == 0 && (D / H) % 8 == 0 && D / H <= 128 && N > 0; }
bool attention_mean_supports(int N, int D, int H) { return attention_map_supports(N, D, H) && N <= kAttnMeanMaxTokens; }

hipError_t launch_attention_cls_map(int dtype, const void *qkv, long lo_off, float *out, long img_stride, int n_img, int N, int D, int H, hipStream_t st) {
    if (!attention_map_supports(N, D, H) || n_img <= 0 || (lo_off && dtype != DT_F16)) return hipErrorInvalidValue;
    if (dtype == DT_F16) return lo_off ? launch_cls_map_t<_Float16, true>(qkv, lo_off, out, img_stride, n_img, N, D, H, st)
                                       : launch_cls_map_t<_Float16, false>(qkv, 0, out, img_stride, n_img, N, D, H, st);
    return launch_cls_map_t<__bf16, false>(qkv, 0, out, img_stride, n_img, N, D, H, st);
}

hipError_t launch_attention_head_mean(int dtype, const void *qkv, long lo_off, float *out, int n_img, int N, int D, int H, bool half_identity, hipStream_t st) {
    if (!attention_mean_supports(N, D, H) || n_img <= 0 || (lo_off && dtype != DT_F16)) return hipErrorInvalidValue;
    if (dtype == DT_F16) return lo_off ? launch_head_mean_t<_Float16, true>(qkv, lo_off, out, n_img, N, D, H, half_identity, st)
                                       : launch_head_mean_t<_Float16, false>(qkv, 0, out, n_img, N, D, H, half_identity, st);
    return launch_head_mean_t<__bf16, false>(qkv, 0, out, n_img, N, D, H, half_identity, st);
}

hipError_t launch_rollout_step(float *a, const float *r, int n_img, int N, hipStream_t st) {
    if (n_img <= 0 || N <= 0 || N > kAttnMeanMaxTokens) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((size_t)n_img * ((N + 15) / 16))), blk(256);
    const int nt = (N + 63) / 64;
    if (nt <= 1) hipLaunchKernelGGL((attn_rollout_step_kernel<1>), grid, blk, 0, st, a, r, N);
    else if (nt <= 2) hipLaunchKernelGGL((attn_rollout_step_kernel<2>), grid, blk, 0, st, a, r, N);
    else if (nt <= 4) hipLaunchKernelGGL((attn_rollout_step_kernel<4>), grid, blk, 0, st, a, r, N);
    else if (nt <= 8) hipLaunchKernelGGL((attn_rollout_step_kernel<8>), grid, blk, 0, st, a, r, N);
    else hipLaunchKernelGGL((attn_rollout_step_kernel<16>), grid, blk, 0, st, a, r, N);
    return hipGetLastError();
}

hipError_t launch_rollout_row(const float *cls, long cls_stride, const float *r, float *out, long out_stride, int n_img, int N, int H, hipStream_t st) {
    if (n_img <= 0 || N <= 0 || N > kAttnMeanMaxTokens || H <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attn_rollout_row_kernel, dim3((unsigned)n_img), dim3(256), 0, st, cls, cls_stride, r, out, out_stride, N, H);
    return hipGetLastError();
}

// ---- a pack (kernels.h): the tables, then the four launches ----
bool attn_pack_tables(const int32_t *row0, int n, int32_t *rblk0, int32_t *sq0, int *n_max) {
    int64_t blk = 0, sq = 0;
    int widest = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t N = row0[i + 1] - row0[i];
        rblk0[i] = (int32_t)blk; sq0[i] = (int32_t)sq;
        blk += (N + 15) / 16; sq += N * N;
        if (N > widest) widest = (int)N;
        if (sq > 0x7fffffffLL || blk > 0x7fffffffLL) return false;
    }
    rblk0[n] = (int32_t)blk; sq0[n] = (int32_t)sq;
    if (n_max) *n_max = widest;
    return true;
}

hipError_t launch_attention_cls_map_packed(int dtype, const void *qkv, float *out, long fpt, int slot, const int *row0, int n, int D, int H, hipStream_t st) {
    if (!attention_map_supports(1, D, H) || n <= 0 || fpt < H || slot < 0 || (dtype != DT_F16 && dtype != DT_BF16)) return hipErrorInvalidValue;
    if (dtype == DT_F16) return launch_cls_map_packed_t<_Float16>(qkv, out, fpt, slot, row0, n, D, H, st);
    return launch_cls_map_packed_t<__bf16>(qkv, out, fpt, slot, row0, n, D, H, st);
}

hipError_t launch_attention_head_mean_packed(int dtype, const void *qkv, float *out, const int *row0, const int *rblk0, const int *sq0, int n, int blocks, int n_max,
                                             int D, int H, bool half_identity, hipStream_t st) {
    if (!attention_mean_supports(n_max, D, H) || n <= 0 || blocks < n || (dtype != DT_F16 && dtype != DT_BF16)) return hipErrorInvalidValue;
    if (dtype == DT_F16) return launch_head_mean_packed_t<_Float16>(qkv, out, row0, rblk0, sq0, n, blocks, n_max, D, H, half_identity, st);
    return launch_head_mean_packed_t<__bf16>(qkv, out, row0, rblk0, sq0, n, blocks, n_max, D, H, half_identity, st);
}

hipError_t launch_rollout_step_packed(float *a, const float *r, const int *row0, const int *rblk0, const int *sq0, int n, int blocks, int n_max, hipStream_t st) {
    if (n <= 0 || blocks < n || n_max <= 0 || n_max > kAttnMeanMaxTokens) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), blk(256);
    const int nt = (n_max + 63) / 64;
    if (nt <= 1) hipLaunchKernelGGL((attn_rollout_step_packed_kernel<1>), grid, blk, 0, st, a, r, row0, rblk0, sq0, n);
    else if (nt <= 2) hipLaunchKernelGGL((attn_rollout_step_packed_kernel<2>), grid, blk, 0, st, a, r, row0, rblk0, sq0, n);
    else if (nt <= 4) hipLaunchKernelGGL((attn_rollout_step_packed_kernel<4>), grid, blk, 0, st, a, r, row0, rblk0, sq0, n);
    else if (nt <= 8) hipLaunchKernelGGL((attn_rollout_step_packed_kernel<8>), grid, blk, 0, st, a, r, row0, rblk0, sq0, n);
    else hipLaunchKernelGGL((attn_rollout_step_packed_kernel<16>), grid, blk, 0, st, a, r, row0, rblk0, sq0, n);
    return hipGetLastError();
}

hipError_t launch_rollout_row_packed(const float *cls, long cfpt, int cslot, const float *r, float *out, long ofpt, long ooff, const int *row0, const int *sq0, int n,
                                     int n_max, int H, hipStream_t st) {
    if (n <= 0 || n_max <= 0 || n_max > kAttnMeanMaxTokens || H <= 0 || cfpt < H || cslot < 0 || ofpt < 1 || ooff < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attn_rollout_row_packed_kernel, dim3((unsigned)n), dim3(256), 0, st, cls, cfpt, cslot, r, out, ofpt, ooff, row0, sq0, H);
    return hipGetLastError();
}

}  // namespace vitx
