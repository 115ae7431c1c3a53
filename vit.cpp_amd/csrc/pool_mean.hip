// pool_mean.hip -- the raw-mean head (VITX_POOL_MEAN_NORM; the contract: include/vitx.h "the mean-pool head"): m = the mean of an image's raw
// patch rows X[T .. N-1] of the f32 residual stream, e = LnRow::norm(m) with norm.* and the file's eps, z = RNE(e) in the operand type.
// Two launches, no atomics:
//   * pool_mean_part_kernel, one workgroup per (image, chunk of kPoolMeanChunkRows patch rows, counted from the image's own first patch row).  There are
//     no per-row statistics, so a row does not belong to a wave: thread (g, l) owns the 16-byte column group g of the rows r0 + l, r0 + l + RL, ... of
//     its chunk (RL row-lanes, pm_row_lanes(D)).  It issues the non-temporal loads of up to four of its rows before the first add, then adds them in
//     ascending row order; the RL row-lanes of a column group meet in LDS, ((a_0 + a_1) + a_2) + ..., and row-lane 0 writes the chunk's sums to
//     part [image][chunk][D].
//   * pool_mean_combine_kernel, one wave per image: the chunk sums in ascending order, one division by N - T -> m; LnRow::norm_loaded(m) -> e; m and e in
//     f32 (either may be left out; e optionally divided by its norm for the VITX_FEAT_CLS feature), z = RNE(e), and the zero pad rows n .. m_pad - 1 of z.
// The chunk length is a constant, never a function of the batch: an image's m, e, z are a function of its own rows, N, T and D only (NaN included).
// The compiler's figures for gfx950 (-Rpass-analysis=kernel-resource-usage), part kernel: 29 - 30 VGPRs and 0 bytes of scratch at every width, LDS =
// (RL - 1) D 4 bytes; combine kernel (one wave; the _Float16 instantiations): no LDS, 0 bytes of scratch.  No instantiation spills.
//   D        64   128   192   256   320   384   448   512   576   640   768   896  1024  1152  1280  1408  1536  1664  2048
//   threads 256   512   768  1024   640   768   896  1024   576   640   768   896  1024   576   640   704   768   832  1024
//   LDS    3840  7680 11520 15360  8960 10752 12544 14336  6912  7680  9216 10752 12288  4608  5120  5632  6144  6656  8192
//   combine  18    21    24    24    29    33    35    41    41    44    48    56    60    64    60    66    68    66    70   VGPRs
#include "device_common.h"
#include "ln_row.h"
#include "kernels.h"

namespace vitx {

namespace {

// row-lanes per column group: as many as 1024 threads hold, a power of two, 16 at the most (a chunk has 64 rows: four per lane, one round of loads)
constexpr int pm_row_lanes(int D) {
    const int fit = 1024 / (D / 4);
    int r = 1;
    while (2 * r <= fit && 2 * r <= 16) r *= 2;
    return r;
}
constexpr int kPmInFlight = 4;         // rows a lane has in flight

template <int D>
__global__ __launch_bounds__((D / 4) * pm_row_lanes(D)) void pool_mean_part_kernel(const float *__restrict__ x, long row_stride, long img_stride, int first, int N,
                                                                                   int chunks, float *__restrict__ part) {
    constexpr int G = D / 4, RL = pm_row_lanes(D);
    __shared__ f32x4 join[RL > 1 ? RL - 1 : 1][G];
    const int g = threadIdx.x % G, l = threadIdx.x / G;
    const int img = blockIdx.x / chunks, chunk = blockIdx.x - img * chunks;
    const int r0 = first + chunk * kPoolMeanChunkRows, r1 = min(r0 + kPoolMeanChunkRows, N);
    const float *xc = x + (size_t)img * img_stride + 4 * g;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int r = r0 + l; r < r1; r += kPmInFlight * RL) {
        f32x4 v[kPmInFlight];
#pragma unroll
        for (int u = 0; u < kPmInFlight; ++u)
            if (r + u * RL < r1) v[u] = __builtin_nontemporal_load((const f32x4 *)(xc + (size_t)(r + u * RL) * row_stride));
#pragma unroll
        for (int u = 0; u < kPmInFlight; ++u)
            if (r + u * RL < r1) acc = acc + v[u];
    }
    if (RL > 1) {
        if (l > 0) join[l - 1][g] = acc;
        __syncthreads();
    }
    if (l > 0) return;
#pragma unroll
    for (int k = 1; k < RL; ++k) acc = acc + join[k - 1][g];       // a row-lane without rows adds its zeros
    *(f32x4 *)(part + (size_t)blockIdx.x * D + 4 * g) = acc;
}

template <typename T16, int VEC, int NV>
__global__ __launch_bounds__(64) void pool_mean_combine_kernel(const float *__restrict__ part, int chunks, int n, float cnt, const float *__restrict__ w, const float *__restrict__ b, float eps,
                                                               float *__restrict__ m_out, float *__restrict__ e_out, long e_stride, int l2, T16 *__restrict__ z) {
    typedef LnRow<VEC, NV> R;
    constexpr int D = 64 * VEC * NV;
    const int i = blockIdx.x, lane = threadIdx.x;
    float f[NV][VEC];
    if (i >= n) {                      // a pad row of the head operand
#pragma unroll
        for (int q = 0; q < NV; ++q)
#pragma unroll
            for (int j = 0; j < VEC; ++j) f[q][j] = 0.0f;
        R::store_rne(z + (size_t)i * D, lane, f);
        return;
    }
    const float *p0 = part + (size_t)i * chunks * D;
    typename R::Raw m;
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int col = R::col(q, lane) + j;
            float s = p0[col];
            for (int k = 1; k < chunks; ++k) s = s + p0[(size_t)k * D + col];
            m[q][j] = f[q][j] = s / cnt;
        }
    if (m_out) R::store(m_out + (size_t)i * D, lane, f);
    R::norm_loaded(m, w, b, eps, lane, f);
    R::store_rne(z + (size_t)i * D, lane, f);
    if (!e_out) return;
    if (l2) R::l2(f);
    R::store(e_out + (size_t)i * e_stride, lane, f);
}

template <typename T16>
hipError_t launch_pool_mean_t(const float *x, long row_stride, long img_stride, int n, int N, int first, int D, const float *w, const float *b, float eps, float *part,
                              float *m_out, float *e_out, long e_stride, bool l2, void *z, int m_pad, hipStream_t stream) {
    const int chunks = pool_mean_chunks(N - first);
    const bool ok = ln_for_width(D, [&](auto vec, auto nv) {
        constexpr int DD = 64 * vec() * nv();
        hipLaunchKernelGGL((pool_mean_part_kernel<DD>), dim3(n * chunks), dim3((DD / 4) * pm_row_lanes(DD)), 0, stream, x, row_stride, img_stride, first, N, chunks, part);
        hipLaunchKernelGGL((pool_mean_combine_kernel<T16, vec(), nv()>), dim3(m_pad), dim3(64), 0, stream, part, chunks, n, (float)(N - first), w, b, eps, m_out, e_out, e_stride,
                           l2 ? 1 : 0, (T16 *)z);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_pool_mean(const float *x, long row_stride, long img_stride, int n_img, int N, int first, int D, const float *w, const float *b, float eps, float *part,
                            float *m, float *e, long e_stride, bool l2, void *z, int dtype, int m_pad, hipStream_t stream) {
    if (!x || !w || !b || !part || !z || n_img <= 0 || first < 0 || first >= N || m_pad < n_img || (long)n_img * pool_mean_chunks(N - first) > 0x7fffffffl || row_stride % 4 || img_stride % 4 || e_stride % 4) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_pool_mean_t, x, row_stride, img_stride, n_img, N, first, D, w, b, eps, part, m, e, e_stride, l2, z, m_pad, stream);
}

}  // namespace vitx
