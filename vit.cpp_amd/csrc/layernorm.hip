// layernorm.hip -- the stand-alone LayerNorm and the fix-up pass behind the LayerNorm-fusing GEMMs.
#include "kernels.h"
#include "epilogue16.h"
#include "device_common.h"
#include "ln_row.h"

namespace vitx {

// ------------------------------------------------------------------------------------------------
// LayerNorm (ggml_norm + ggml_mul + ggml_add_inplace, vit.cpp:808-812, 881-885, 915-919):
// mean, then biased variance of (x-mean), y = ((x-mean) * 1/sqrt(var+eps)) * w + b, rounded to the
// operand type of the GEMM that consumes it.  One wave per row, row kept in registers: the row is LnRow's (ln_row.h), so it gets
// the same bits whichever normalising kernel produced it.  Hidden sizes that are 1..4 tiles of 256 columns (256, 512, 768, 1024: every
// model the wide GEMMs run) take its TILED statistics, the definition the LayerNorm fused into the residual GEMMs (gemm_pp.hip) follows too.
// ------------------------------------------------------------------------------------------------
template <typename T, int VEC, int NV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float *__restrict__ x, long ldx, const float *__restrict__ w, const float *__restrict__ b,
                                                        T *__restrict__ y, long ldy, int M, float eps, int group, long gstride) {
    typedef LnRow<VEC, NV> R;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    // input row: group == 1 -> row * ldx; otherwise rows come in groups (row / group) * gstride + (row % group) * ldx
    // (the first `group` tokens of every image: the ViTSTR head, vitstr.cpp:864-883)
    const float *xr = group == 1 ? x + (size_t)row * ldx : x + (size_t)(row / group) * gstride + (size_t)(row % group) * ldx;
    T *yr = y + (size_t)row * ldy;
    R::each(xr, w, b, eps, lane, [&](int, int idx, const float (&o)[VEC]) { R::put_rne(yr + idx, o); });
}

// The same LayerNorm with the f32 result stored as it is (launch_layernorm_f32: the pre-norm of a file with pre_norm.*, in place on the residual
// stream): RNE(y) is layernorm_kernel's output bit for bit.  One wave per row; each() has read the whole row before the first store, so
// y == x is allowed.
template <int VEC, int NV>
__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float *x, const float *__restrict__ w, const float *__restrict__ b, float *y, int M, float eps) {
    typedef LnRow<VEC, NV> R;
    constexpr int D = 64 * VEC * NV;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float *yr = y + (size_t)row * D;
    R::each(x + (size_t)row * D, w, b, eps, lane, [&](int, int idx, const float (&o)[VEC]) { R::put(yr + idx, o); });
}
hipError_t launch_layernorm_f32(const float *x, const float *w, const float *b, float *y, int M, int D, float eps, hipStream_t stream) {
    const dim3 grid((M + 3) / 4), blk(256);
    const bool ok = ln_for_width(D, [&](auto vec, auto nv) { hipLaunchKernelGGL((layernorm_f32_kernel<vec(), nv()>), grid, blk, 0, stream, x, w, b, y, M, eps); });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
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
template <typename T, int NT>
static hipError_t launch_layernorm_fixup_t(const float *x, const float *w, const float *b, void *y, int nb, float eps, const unsigned *todo, unsigned epoch, hipStream_t stream) {
    hipLaunchKernelGGL((layernorm_fixup_kernel<T, NT>), dim3(64), dim3(256), 0, stream, x, w, b, (T *)y, nb, eps, todo, epoch);
    return hipGetLastError();
}
hipError_t launch_layernorm_fixup(int dtype, const float *x, const float *w, const float *b, void *y, int M, int D, float eps, const unsigned *todo, unsigned epoch, hipStream_t stream) {
    if (M % 256 || D % 256) return hipErrorInvalidValue;
    const int nb = M / 256;
    switch (D / 256) {
    case 1: return VITX_BY_DTYPE2(dtype, launch_layernorm_fixup_t, 1, x, w, b, y, nb, eps, todo, epoch, stream);
    case 2: return VITX_BY_DTYPE2(dtype, launch_layernorm_fixup_t, 2, x, w, b, y, nb, eps, todo, epoch, stream);
    case 3: return VITX_BY_DTYPE2(dtype, launch_layernorm_fixup_t, 3, x, w, b, y, nb, eps, todo, epoch, stream);
    case 4: return VITX_BY_DTYPE2(dtype, launch_layernorm_fixup_t, 4, x, w, b, y, nb, eps, todo, epoch, stream);
    default: return hipErrorInvalidValue;
    }
}

template <typename T>
static hipError_t launch_layernorm_t(const float *x, long ldx, const float *w, const float *b, void *y, long ldy, int M, int D, float eps, hipStream_t stream, int group, long gstride) {
    const dim3 grid((M + 3) / 4), blk(256);
    const bool ok = ln_for_width(D, [&](auto vec, auto nv) {
        hipLaunchKernelGGL((layernorm_kernel<T, vec(), nv()>), grid, blk, 0, stream, x, ldx, w, b, (T *)y, ldy, M, eps, group, gstride);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}
bool layernorm_supports(int D) { return ln_for_width(D, [](auto, auto) {}); }
hipError_t launch_layernorm(int dtype, const float *x, long ldx, const float *w, const float *b, void *y, long ldy, int M, int D, float eps, hipStream_t stream, int group, long gstride) {
    if (group < 1) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_layernorm_t, x, ldx, w, b, y, ldy, M, D, eps, stream, group, gstride);
}

}  // namespace vitx
