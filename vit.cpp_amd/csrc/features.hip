// features.hip -- image embeddings and token features (vitx_feat_enable, vitx_op_features; the contract: include/vitx.h).
//
// F = ((X - mean) * rstd) * norm.weight + norm.bias of the f32 residual stream X, per row, in f32: LnRow::norm (ln_row.h), the row
// layernorm_kernel (layernorm.hip) rounds to the operand type, WITHOUT that rounding -- so F rounded to nearest even IS what that kernel
// stores (-ffp-contract=off, as for every kernel of the library).
//
// One workgroup per image, W waves (feat_waves; one wave when only the class row is asked for), one pass over the image's rows, every row read once:
//   * wave W - 1 takes the class row (row 0) first, when the class embedding is asked for;
//   * wave w takes the patch rows T + w, T + w + W, ... in ascending order (T = `first`: 1 + the register tokens, which are never read):
//     stores F (TOKENS) and adds it to per-lane column accumulators (MEAN).  Rows go two at a time at the widths up to 1024 (both rows'
//     loads are issued before either is used);
//   * the W partial sums are added into one LDS row in wave order, ((p_0 + p_1) + p_2) + ..., then divided by N - T.
// The pooled head (VITX_POOL_CLS_MEAN) takes its operand from the same pass: z[i] = RNE(F[0]) ‖ RNE(mean) in the operand type, rounded from
// the very registers the f32 features are stored from (before VITX_FEAT_L2), so RNE(feature) == the head operand by construction.
// No atomics, nothing depends on the batch: an image's bits are a function of its own rows, N and D only.
// Column ownership follows the statistics helpers: lane l holds columns c * 256 + 4 l .. + 3 of tile c (tiled widths: 16-byte loads and
// stores, 1 KiB contiguous per wave instruction) or (i * 64 + l) * VEC .. of piece i (flat widths, VEC of the instantiation table).
#include "device_common.h"
#include "ln_row.h"
#include "kernels.h"

namespace vitx {

namespace {

// waves per workgroup: 16 (4 per SIMD, 128 VGPRs each) up to 768 columns; 8 above, where a row, the accumulators and the second row or the
// weights of a piece need more than 128 registers per lane (checked with -save-temps: no instantiation spills)
constexpr int feat_waves(int D) { return D <= 768 ? 16 : 8; }

template <int VEC, int NV>
__global__ __launch_bounds__(feat_waves(64 * VEC * NV) * 64) void features_kernel(const float *__restrict__ x, long row_stride, long img_stride, const float *__restrict__ w,
                                                                   const float *__restrict__ b, float *__restrict__ cls, float *__restrict__ mean, float *__restrict__ tokens,
                                                                   long out_img_stride, int N, float eps, int l2, int first, void *__restrict__ z, int z_bf16) {
    typedef LnRow<VEC, NV> R;
    constexpr int D = 64 * VEC * NV;
    constexpr int U = D <= 1024 ? 2 : 1;          // patch rows per step of a wave
    __shared__ float pool[D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const float *xi = x + (size_t)blockIdx.x * img_stride;
    const size_t out_off = (size_t)blockIdx.x * out_img_stride;
    float f[U][NV][VEC];
    if ((cls || z) && wave == W - 1) {
        R::norm(xi, w, b, eps, lane, f[0]);
        if (z) {
            if (z_bf16) R::store_rne((__bf16 *)z + (size_t)blockIdx.x * 2 * D, lane, f[0]);
            else R::store_rne((_Float16 *)z + (size_t)blockIdx.x * 2 * D, lane, f[0]);
        }
        if (cls) {
            if (l2) R::l2(f[0]);
            R::store(cls + out_off, lane, f[0]);
        }
    }
    if (!mean && !tokens && !z) return;
    float acc[NV][VEC];
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[i][j] = 0.0f;
    float *tok = tokens ? tokens + out_off : nullptr;
    for (int t = first + wave; t < N; t += U * W) {
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (t + u * W < N) R::norm(xi + (size_t)(t + u * W) * row_stride, w, b, eps, lane, f[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t + u * W >= N) break;
            if (tok) R::store(tok + (size_t)(t + u * W - first) * D, lane, f[u]);
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[i][j] += f[u][i][j];
        }
    }
    if (!mean && !z) return;
    // the waves' partial sums, added in wave order into one row of LDS (a wave without rows adds its zeros)
    for (int k = 0; k < W; ++k) {
        if (wave == k) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int j = 0; j < VEC; ++j) { float *p = pool + R::col(i, lane) + j; *p = k == 0 ? acc[i][j] : *p + acc[i][j]; }
        }
        __syncthreads();
    }
    if (wave != 0) return;
    const float cnt = (float)(N - first);
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < VEC; ++j) f[0][i][j] = pool[R::col(i, lane) + j] / cnt;
    if (z) {
        if (z_bf16) R::store_rne((__bf16 *)z + (size_t)blockIdx.x * 2 * D + D, lane, f[0]);
        else R::store_rne((_Float16 *)z + (size_t)blockIdx.x * 2 * D + D, lane, f[0]);
    }
    if (!mean) return;
    if (l2) R::l2(f[0]);
    R::store(mean + out_off, lane, f[0]);
}

}  // namespace

// F of n_img images of N rows (row t of image i at x + i * img_stride + t * row_stride), T = first: cls[i * out_img_stride ..] = F[0] [D],
// mean[i * out_img_stride ..] = mean of F[T .. N-1] [D], tokens[i * out_img_stride ..] = F[T .. N-1] [N - T][D]; any output may be nullptr.
// z: the pooled head's operand rows [n_img][2 D] in `dtype` (kernels.h).  Row 0 is read only for cls / z, rows T .. only for mean / tokens / z.
// hipErrorInvalidValue: no instantiation for D (layernorm_supports), first outside 0 .. N, or first = 0 with cls / z.
hipError_t launch_features(const float *x, long row_stride, long img_stride, const float *w, const float *b, float *cls, float *mean, float *tokens,
                           long out_img_stride, int n_img, int N, int D, float eps, bool l2, hipStream_t stream, int first, void *z, int dtype) {
    if (first < 0 || first > N || (first == 0 && (cls || z))) return hipErrorInvalidValue;     // first = 0: a model without prefix tokens has no class row
    const bool rows = mean || tokens || z;
    const dim3 grid(n_img), blk(64 * (rows ? feat_waves(D) : 1));
    const bool ok = ln_for_width(D, [&](auto vec, auto nv) {
        hipLaunchKernelGGL((features_kernel<vec(), nv()>), grid, blk, 0, stream, x, row_stride, img_stride, w, b, cls, mean, tokens, out_img_stride, N, eps, l2 ? 1 : 0, first, z, dtype == DT_BF16 ? 1 : 0);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace vitx
