// layernorm.hip -- the stand-alone LayerNorm and the fix-up pass behind the LayerNorm-fusing GEMMs.
#include "kernels.h"
#include "epilogue16.h"
#include "device_common.h"

namespace vitx {

// ------------------------------------------------------------------------------------------------
// LayerNorm (ggml_norm + ggml_mul + ggml_add_inplace, vit.cpp:808-812, 881-885, 915-919):
// mean, then biased variance of (x-mean), y = ((x-mean) * 1/sqrt(var+eps)) * w + b, rounded to the
// operand type of the GEMM that consumes it.  One wave per row, row kept in registers.
// Hidden sizes that are 1..4 tiles of 256 columns (256, 512, 768, 1024: every model the wide GEMMs run) take the TILED statistics
// of device_common.h, the definition the LayerNorm fused into the residual GEMMs (gemm_pp.hip) follows too: a row gets the same
// bits whichever of the two produced it.  Lane l of the wave holds piece l of each tile (w = l >> 4, j = (l >> 3) & 1, k = l & 7):
// one fully coalesced 1 KiB load per tile.
// ------------------------------------------------------------------------------------------------
template <typename T, int VEC, int NV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float *__restrict__ x, long ldx, const float *__restrict__ w, const float *__restrict__ b,
                                                        T *__restrict__ y, long ldy, int M, float eps, int group, long gstride) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    // input row: group == 1 -> row * ldx; otherwise rows come in groups (row / group) * gstride + (row % group) * ldx
    // (the first `group` tokens of every image: the ViTSTR head, vitstr.cpp:864-883)
    const float *xr = group == 1 ? x + (size_t)row * ldx : x + (size_t)(row / group) * gstride + (size_t)(row % group) * ldx;
    T *yr = y + (size_t)row * ldy;
    if constexpr (VEC == 4 && NV <= LN_MAX_TILES) { ln_row_tiled<T, NV>(xr, w, b, yr, eps, lane); return; }
    float v[NV][VEC];
    float scale;
    ln_flat_stats<VEC, NV>(xr, eps, lane, v, scale);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = (i * 64 + lane) * VEC;
        T o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) { float t = v[i][j] * scale; t = t * w[idx + j]; o[j] = (T)(t + b[idx + j]); }
        if constexpr (VEC == 4) *(typename Elem<T>::v4 *)(yr + idx) = typename Elem<T>::v4{o[0], o[1], o[2], o[3]};
        else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) yr[idx + j] = o[j];
        }
    }
}

// The same LayerNorm with the f32 result stored as it is (launch_layernorm_f32: the pre-norm of a file with pre_norm.*, in place on the residual
// stream): the statistics and the operation order of ln_row_tiled / the flat path above, so that RNE(y) is layernorm_kernel's output bit for bit.
// One wave per row; the whole row is in registers before the first store, so y == x is allowed.
template <int VEC, int NV>
__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float *x, const float *__restrict__ w, const float *__restrict__ b, float *y, int M, float eps) {
    constexpr int D = 64 * VEC * NV;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float *xr = x + (size_t)row * D;
    float *yr = y + (size_t)row * D;
    if constexpr (VEC == 4 && NV <= LN_MAX_TILES) {
        f32x4 v[NV];
        float mean, rstd;
        ln_tiled_stats<NV>(xr, eps, lane, v, mean, rstd);
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const int idx = c * 256 + lane * 4;
            const f32x4 ww = *(const f32x4 *)(w + idx), bb = *(const f32x4 *)(b + idx);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) { float t = (v[c][e] - mean) * rstd; t = t * ww[e]; o[e] = t + bb[e]; }
            *(f32x4 *)(yr + idx) = o;
        }
    } else {
        float v[NV][VEC];
        float scale;
        ln_flat_stats<VEC, NV>(xr, eps, lane, v, scale);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = (i * 64 + lane) * VEC;
            float o[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) { float t = v[i][j] * scale; t = t * w[idx + j]; o[j] = t + b[idx + j]; }
            if constexpr (VEC == 4) *(f32x4 *)(yr + idx) = f32x4{o[0], o[1], o[2], o[3]};
            else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) yr[idx + j] = o[j];
            }
        }
    }
}
hipError_t launch_layernorm_f32(const float *x, const float *w, const float *b, float *y, int M, int D, float eps, hipStream_t stream) {
    const dim3 grid((M + 3) / 4), blk(256);
#define VITX_LN_CASE(DD, VEC, NV) \
    case DD: hipLaunchKernelGGL((layernorm_f32_kernel<VEC, NV>), grid, blk, 0, stream, x, w, b, y, M, eps); break;
    switch (D) {
        VITX_LN_WIDTHS(VITX_LN_CASE)
    default: return hipErrorInvalidValue;
    }
#undef VITX_LN_CASE
    return hipGetLastError();
}

// Row blocks a LayerNorm-fusing GEMM left behind (GemmLn: todo[rb] == epoch): 64 workgroups, every wave takes one row of each such
// block -- no single-CU tail.  With nothing to do (the normal case) a workgroup reads the flags and exits.
template <typename T, int NT>
__global__ __launch_bounds__(256) void layernorm_fixup_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ b, T *__restrict__ y,
                                                              int n_blocks, float eps, const unsigned *__restrict__ todo, unsigned epoch) {
    const int lane = threadIdx.x & 63, wv = blockIdx.x * 4 + (threadIdx.x >> 6), nwv = gridDim.x * 4;
    // 64 flags per pass, one per lane (r03a: a serial scan of the ~200 flags made this launch 16 us with nothing to do, 0.5 ms per forward)
    for (int base = 0; base < n_blocks; base += 64) {
        const int rb_l = base + lane;
        const bool hit = rb_l < n_blocks && __builtin_nontemporal_load(todo + rb_l) == epoch;
        unsigned long long mask = __ballot(hit);
        while (mask) {
            const int rb = base + __builtin_ctzll(mask);
            mask &= mask - 1;
            for (int r = wv; r < 256; r += nwv) {
                const size_t row = (size_t)rb * 256 + r;
                ln_row_tiled<T, NT>(x + row * (NT * 256), w, b, y + row * (NT * 256), eps, lane);
            }
        }
    }
}
hipError_t launch_layernorm_fixup(int dtype, const float *x, const float *w, const float *b, void *y, int M, int D, float eps, const unsigned *todo, unsigned epoch, hipStream_t stream) {
    if (M % 256 || D % 256 || D / 256 < 1 || D / 256 > LN_MAX_TILES) return hipErrorInvalidValue;
    const dim3 grid(64), blk(256);
    const int nb = M / 256;
#define VITX_FIX_CASE(NT)                                                                                   \
    case NT:                                                                                                \
        if (dtype == DT_F16) hipLaunchKernelGGL((layernorm_fixup_kernel<_Float16, NT>), grid, blk, 0, stream, x, w, b, (_Float16 *)y, nb, eps, todo, epoch); \
        else hipLaunchKernelGGL((layernorm_fixup_kernel<__bf16, NT>), grid, blk, 0, stream, x, w, b, (__bf16 *)y, nb, eps, todo, epoch);                    \
        break;
    switch (D / 256) { VITX_FIX_CASE(1) VITX_FIX_CASE(2) VITX_FIX_CASE(3) VITX_FIX_CASE(4) default: return hipErrorInvalidValue; }
#undef VITX_FIX_CASE
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_layernorm_t(const float *x, long ldx, const float *w, const float *b, void *y, long ldy, int M, int D, float eps, hipStream_t stream, int group, long gstride) {
    const dim3 grid((M + 3) / 4), blk(256);
#define VITX_LN_CASE(DD, VEC, NV) \
    case DD: hipLaunchKernelGGL((layernorm_kernel<T, VEC, NV>), grid, blk, 0, stream, x, ldx, w, b, (T *)y, ldy, M, eps, group, gstride); break;
    switch (D) {
        VITX_LN_WIDTHS(VITX_LN_CASE)
    default: return hipErrorInvalidValue;
    }
#undef VITX_LN_CASE
    return hipGetLastError();
}
bool layernorm_supports(int D) {
#define VITX_LN_SUPPORTED(DD, VEC, NV) case DD:
    switch (D) { VITX_LN_WIDTHS(VITX_LN_SUPPORTED) return true; default: return false; }
#undef VITX_LN_SUPPORTED
}
hipError_t launch_layernorm(int dtype, const float *x, long ldx, const float *w, const float *b, void *y, long ldy, int M, int D, float eps, hipStream_t stream, int group, long gstride) {
    if (group < 1) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_layernorm_t, x, ldx, w, b, y, ldy, M, D, eps, stream, group, gstride);
}

}  // namespace vitx
