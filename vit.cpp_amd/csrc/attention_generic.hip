// attention_generic.hip -- attention for head dims other than 64 (any multiple of 8 up to 128), any token count.
#include "attention_rows.h"

namespace vitx {

// ------------------------------------------------------------------------------------------------
// Attention for head dimensions other than 64 (vit.cpp:826-866 is generic in n_enc_head_dim; timm's ViT-H/14 has 80, 8-head variants
// 96 / 128, small models 32): any multiple of 8 up to 128.  Not a tuned kernel -- every model the benchmarks name has head_dim 64 -- but
// the same arithmetic as the other three: S^T = K . Q^T by v_mfma_f32_16x16x32 over the head dim zero-padded to a multiple of 32, two
// passes over the keys (row maximum; then exp per AttnExpRt<T>, row sum of the rounded numerators, O^T = V^T . P^T), scores in the
// four lanes (lane & 15, lane >> 4) of a query.  One wave per 16-query tile, four tiles per workgroup, no workgroup barrier.  The
// arithmetic itself is attention_rows16 (attention_rows.h), shared with the packed kernel of attention_packed.hip.
// ------------------------------------------------------------------------------------------------
template <typename T, int NK2>
__global__ __launch_bounds__(256) void attention_generic_kernel(const T *__restrict__ qkv, T *__restrict__ out, int N, int D, int H, int DH, float scale, int qblocks) {
    constexpr int ROWB = NK2 * 32 * 2;                // LDS row bytes of the padded head dim
    __shared__ __attribute__((aligned(16))) char smem[4 * 32 * ROWB];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blockIdx.x / qblocks, qb = blockIdx.x - item * qblocks;
    const int b = item / H, h = item - b * H;
    const int q0 = (qb * 4 + wave) * 16;
    if (q0 >= N) return;                              // no barrier in this kernel: a wave without queries simply leaves
    // q of the image's token 0 (k at + D, v at + 2 D); the image's output row 0
    attention_rows16<T, NK2>(qkv + (size_t)b * N * 3 * D + (size_t)h * DH, out + (size_t)b * N * D + (size_t)h * DH, N, D, DH, scale, q0, smem + wave * (32 * ROWB));
}
bool attention_generic_supports(int D, int H) { return H > 0 && D % H == 0 && (D / H) % 8 == 0 && D / H >= 8 && D / H <= 128; }
template <typename T>
static hipError_t launch_attention_generic_t(const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream) {
    const int DH = D / H, nk2 = (DH + 31) / 32, qblocks = (N + 63) / 64;
    const float scale = 1.0f / sqrtf((float)DH);
    const dim3 grid((unsigned)((size_t)n_img * H * qblocks)), blk(256);
    switch (nk2) {
    case 1: hipLaunchKernelGGL((attention_generic_kernel<T, 1>), grid, blk, 0, stream, (const T *)qkv, (T *)out, N, D, H, DH, scale, qblocks); break;
    case 2: hipLaunchKernelGGL((attention_generic_kernel<T, 2>), grid, blk, 0, stream, (const T *)qkv, (T *)out, N, D, H, DH, scale, qblocks); break;
    case 3: hipLaunchKernelGGL((attention_generic_kernel<T, 3>), grid, blk, 0, stream, (const T *)qkv, (T *)out, N, D, H, DH, scale, qblocks); break;
    case 4: hipLaunchKernelGGL((attention_generic_kernel<T, 4>), grid, blk, 0, stream, (const T *)qkv, (T *)out, N, D, H, DH, scale, qblocks); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
hipError_t launch_attention_generic(int dtype, const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream) {
    return VITX_BY_DTYPE(dtype, launch_attention_generic_t, qkv, out, n_img, N, D, H, stream);
}

}  // namespace vitx
