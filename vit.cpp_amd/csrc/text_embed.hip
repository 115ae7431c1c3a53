// text_embed.hip -- the two ends of a text tower around its blocks (text_forward.cpp; include/vitx.h "the text tower"):
//   text_embed_kernel   X[i][t][:] = f32(tok[ids[i][t]][:]) + pos[t][:]: one f32 add per element, the table held as filed (f16 or f32);
//   text_pool_kernel    the pooled row of every prompt through the final LayerNorm (LnRow: the project's one row definition), rounded to the
//                       operand type: the head GEMM's A rows; rows n .. m_pad are written as zeros (the GEMM multiplies whole row tiles);
//                       launch_pool_rows is the same kernel on absolute row indices (the class rows of a packed context);
// (VITX_TEXT_L2 is zs_embed_kernel's f32 instantiation, zeroshot.hip.)
// No atomics; a prompt's bits depend on its own ids only.
#include "device_common.h"
#include "kernels.h"
#include "ln_row.h"

namespace vitx {

namespace {

// One thread per 16-byte piece of a table row (8 f16 or 4 f32 columns); rows = n * T token rows, ids checked on the host (0 <= id < V).
template <typename TT>
__global__ __launch_bounds__(256) void text_embed_kernel(const TT *__restrict__ tok, const float *__restrict__ pos, const int *__restrict__ ids, float *__restrict__ X, long rows, int T, int D) {
    constexpr int PC = 16 / (int)sizeof(TT);            // columns per piece
    const int ppr = D / PC;
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= rows * ppr) return;
    const long row = gi / ppr;
    const int c0 = (int)(gi - row * ppr) * PC, t = (int)(row % T);
    const TT *src = tok + (size_t)ids[row] * D + c0;
    const float *pr = pos + (size_t)t * D + c0;
    float *xr = X + (size_t)row * D + c0;
    if constexpr (sizeof(TT) == 2) {
        const half8 e = *(const half8 *)src;
        const f32x4 p0 = *(const f32x4 *)pr, p1 = *(const f32x4 *)(pr + 4);
        *(f32x4 *)xr = f32x4{(float)e[0] + p0[0], (float)e[1] + p0[1], (float)e[2] + p0[2], (float)e[3] + p0[3]};
        *(f32x4 *)(xr + 4) = f32x4{(float)e[4] + p1[0], (float)e[5] + p1[1], (float)e[6] + p1[2], (float)e[7] + p1[3]};
    } else {
        const f32x4 e = *(const f32x4 *)src, p0 = *(const f32x4 *)pr;
        *(f32x4 *)xr = f32x4{e[0] + p0[0], e[1] + p0[1], e[2] + p0[2], e[3] + p0[3]};
    }
}

// One wave per prompt, four per workgroup: row i * T + pooled[i] of X -> z[i][:]
template <typename T16, int VEC, int NV>
__global__ __launch_bounds__(256) void text_pool_kernel(const float *__restrict__ X, const int *__restrict__ pooled, const float *__restrict__ w, const float *__restrict__ b,
                                                        T16 *__restrict__ z, int n, int m_pad, int T, float eps) {
    typedef LnRow<VEC, NV> R;
    constexpr int D = 64 * VEC * NV;
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m_pad) return;
    T16 *zr = z + (size_t)i * D;
    if (i >= n) {
        const float zero[VEC] = {};
#pragma unroll
        for (int p = 0; p < NV; ++p) R::put_rne(zr + R::col(p, lane), zero);
        return;
    }
    const float *xr = X + ((size_t)i * T + pooled[i]) * D;
    R::each(xr, w, b, eps, lane, [&](int, int idx, const float (&o)[VEC]) { R::put_rne(zr + idx, o); });
}

}  // namespace

hipError_t launch_text_embed(bool table_f16, const void *tok, const float *pos, const int *ids, float *X, int n, int T, int D, hipStream_t stream) {
    if (n <= 0 || T <= 0 || D <= 0 || D % 8) return hipErrorInvalidValue;
    const long rows = (long)n * T, pieces = rows * (D / (table_f16 ? 8 : 4));
    if (pieces > 0x7fffffffL * 256) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((pieces + 255) / 256)), blk(256);
    if (table_f16) hipLaunchKernelGGL(text_embed_kernel<_Float16>, grid, blk, 0, stream, (const _Float16 *)tok, pos, ids, X, rows, T, D);
    else hipLaunchKernelGGL(text_embed_kernel<float>, grid, blk, 0, stream, (const float *)tok, pos, ids, X, rows, T, D);
    return hipGetLastError();
}

template <typename T16>
static hipError_t launch_text_pool_t(const float *X, const int *pooled, const float *w, const float *b, void *z, int n, int m_pad, int T, int D, float eps, hipStream_t stream) {
    const dim3 grid((m_pad + 3) / 4), blk(256);
    const bool ok = ln_for_width(D, [&](auto vec, auto nv) {
        hipLaunchKernelGGL((text_pool_kernel<T16, vec(), nv()>), grid, blk, 0, stream, X, pooled, w, b, (T16 *)z, n, m_pad, T, eps);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}
hipError_t launch_text_pool(int dtype, const float *X, const int *pooled, const float *w, const float *b, void *z, int n, int m_pad, int T, int D, float eps, hipStream_t stream) {
    if (n <= 0 || m_pad < n || T <= 0) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_text_pool_t, X, pooled, w, b, z, n, m_pad, T, D, eps, stream);
}
// the same kernel with absolute row indices (T = 0: row i * 0 + rows[i]): the class rows of a packed context
hipError_t launch_pool_rows(int dtype, const float *X, const int *rows, const float *w, const float *b, void *z, int n, int m_pad, int D, float eps, hipStream_t stream) {
    if (n <= 0 || m_pad < n) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_text_pool_t, X, rows, w, b, z, n, m_pad, 0, D, eps, stream);
}

}  // namespace vitx
