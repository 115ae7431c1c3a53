// features_packed.hip -- the class row and the mean patch embedding of every image of a PACK (include/vitx.h "packed batches": pool_head =
// VITX_PACK_POOL_CLS_MEAN and VITX_FEAT_MEAN): images of different row counts end to end, image i = rows row0[i] .. row0[i + 1] - 1 of the f32 residual
// stream, its first T rows the class and register rows.  F is features.hip's F: LnRow::norm of a row, f32, unrounded.  Two launches, no atomics.
//
// feat_pool_part_kernel: a work item is (image, chunk of kFeatPoolChunkRows = 128 consecutive PATCH rows of it), cut from the image's own first patch
// row; a 1-D grid of sum_i ceil((N_i - T) / 128) workgroups, each finding its image by the family's scalar binary search of the workgroup index in the
// running chunk count pc0 [n + 1] (feat_pool_chunks).  A workgroup has W = feat_pool_waves(D) waves, fixed per width (16 up to 768 columns, 8 above: the
// register budget of features.hip), never a function of the pack:
//   * wave w takes rows w, w + W, w + 2 W, .. of the chunk in ascending order, two rows per step: the loads of BOTH rows (LnRow::load, 16-byte loads at
//     the tiled widths) are issued before the first row's statistics, so two rows are in flight per wave (read in the assembly: at D 768 six
//     global_load_dwordx4, then s_waitcnt vmcnt(5)).  Three things make it so: the loads stand apart from the arithmetic (LnRow::load / norm_loaded),
//     no branch stands between them (a second row past the chunk's end is read as the chunk's last row, normalised and dropped by a select), and a
//     scheduling barrier behind the loads keeps the scheduler from moving them down.  One row per step above 1024 columns (two rows and the
//     accumulators do not fit the registers there).  F is added into per-lane f32 column accumulators -- LnRow's column ownership;
//   * each wave parks its partial row in LDS [W][D]; behind ONE barrier thread t adds column t, t + 64 W, .. over the waves in wave order,
//     ((p_0 + p_1) + p_2) + .. (a wave without rows adds its zeros), and stores the chunk's column sums to part[chunk][D];
//   * in an image's chunk 0 the last wave first normalises the class row row0[i]: z[i][0 .. D) = RNE(F[0]) in the operand type and cls[i] = F[0] (f32,
//     with l2 divided by its norm) from the same registers -- launch_pool_rows' row, bit for bit.
// feat_pool_combine_kernel: one workgroup of 256 threads per row of z.  Row i < n: thread t owns columns t, t + 256, ..; it adds the image's chunk rows
// in ascending chunk order and divides ONCE by N_i - T: z[i][D .. 2 D) = RNE(mean), then mean[i] = the f32 mean (with l2 divided by its norm: per-thread
// sums of squares in column order, a butterfly per wave, the four waves in order).  Rows n .. m_pad - 1 of z are written as zeros (the head GEMM
// multiplies whole row tiles).
// An image's cls, mean and z are a function of its own rows, N_i, T and D: the same bits alone, at any position in a pack, beside any neighbours; rows
// behind an image are never read.  The mean's order is the pack's own -- not the image context's (features.hip sums an image in one workgroup).
// As hipcc reports (-save-temps, gfx950), VGPRs / scratch bytes / LDS bytes per instantiation of the part kernel -- none spills:
//   D 64: 30/0/4096   128: 34/0/8192   192: 41/0/12288   256: 48/0/16384   320: 51/0/20480   384: 74/0/24576   448: 61/0/28672   512: 69/0/32768
//   576: 72/0/36864   640: 126/0/40960   768: 94/0/49152   896: 154/0/28672   1024: 114/0/32768   1152: 94/0/36864   1280: 112/0/40960
//   1408: 122/0/45056   1536: 126/0/49152   1664: 126/0/53248   2048: 160/0/65536;   the combine kernel (both operand types): 22/0/16.
// (16 waves per workgroup leave 128 VGPRs per lane, 8 waves 256: every instantiation fits its launch bound.)
// Cost: profiles/pack_mean_cost.txt (tools/pack_mean_cost.py); include/vitx.h has the figures and what is unmeasured.
#include "device_common.h"
#include "ln_row.h"
#include "kernels.h"

namespace vitx {

namespace {

// the image of workgroup wg: pc0[lo] <= wg < pc0[lo + 1], uniform addresses (scalar loads)
__device__ __forceinline__ int fp_find_image(const int *__restrict__ pc0, int n, int wg) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pc0[mid] <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

template <int VEC, int NV>
__global__ __launch_bounds__(feat_pool_waves(64 * VEC * NV) * 64) void feat_pool_part_kernel(const float *__restrict__ x, const int *__restrict__ row0, const int *__restrict__ pc0, int n,
                                                                                         int T, const float *__restrict__ w, const float *__restrict__ b, float eps,
                                                                                         float *__restrict__ part, float *__restrict__ cls, void *__restrict__ z, int z_bf16, int l2) {
    typedef LnRow<VEC, NV> R;
    constexpr int D = 64 * VEC * NV, W = feat_pool_waves(D);
    constexpr int U = D <= 1024 ? 2 : 1;          // patch rows per step of a wave
    __shared__ __attribute__((aligned(16))) float pool[W][D];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wg = blockIdx.x, img = fp_find_image(pc0, n, wg), c = wg - pc0[img];
    const int r_img = row0[img], Np = row0[img + 1] - r_img - T;      // >= 1: the host cut the chunks
    const int left = Np - c * kFeatPoolChunkRows, nrows = left < kFeatPoolChunkRows ? left : kFeatPoolChunkRows;
    const float *xc = x + ((size_t)r_img + T + (size_t)c * kFeatPoolChunkRows) * D;
    float f[NV][VEC];
    if (c == 0 && wave == W - 1 && (cls || z)) {
        R::norm(x + (size_t)r_img * D, w, b, eps, lane, f);
        if (z) {
            if (z_bf16) R::store_rne((__bf16 *)z + (size_t)img * 2 * D, lane, f);
            else R::store_rne((_Float16 *)z + (size_t)img * 2 * D, lane, f);
        }
        if (cls) {
            if (l2) R::l2(f);
            R::store(cls + (size_t)img * D, lane, f);
        }
    }
    if (!part) return;
    float acc[NV][VEC];
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[i][j] = 0.0f;
    for (int t = wave; t < nrows; t += U * W) {
        // Every row's loads are issued here, before the first row's statistics wait for anything.  A row past the chunk's end is read as the chunk's
        // last row (inside the image), normalised like any other and dropped by a select: with a branch around it the compiler sinks that row's loads
        // behind the first row's arithmetic (read in the assembly), and then only one row is ever in flight
        typename R::Raw raw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = t + u * W < nrows ? t + u * W : nrows - 1;
            R::load(xc + (size_t)r * D, lane, raw[u]);
        }
        __builtin_amdgcn_sched_barrier(0);        // the scheduler would move the later pieces' loads down into the first row's statistics
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ok = t + u * W < nrows;
            R::norm_loaded(raw[u], w, b, eps, lane, f);
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[i][j] = ok ? acc[i][j] + f[i][j] : acc[i][j];
        }
    }
    R::store(pool[wave], lane, acc);
    __syncthreads();
    float *pr = part + (size_t)wg * D;
    for (int col = threadIdx.x; col < D; col += W * 64) {
        float s = pool[0][col];
#pragma unroll
        for (int k = 1; k < W; ++k) s = s + pool[k][col];
        pr[col] = s;
    }
}

template <typename T16>
__global__ __launch_bounds__(256) void feat_pool_combine_kernel(const float *__restrict__ part, const int *__restrict__ row0, const int *__restrict__ pc0, int n, int T, int D,
                                                                float *__restrict__ mean, T16 *__restrict__ z, int l2) {
    __shared__ float ssq[4];
    const int i = blockIdx.x;
    if (i >= n) {        // a pad row of z (the grid has such rows only with z)
        for (int col = threadIdx.x; col < 2 * D; col += 256) z[(size_t)i * 2 * D + col] = (T16)0.0f;
        return;
    }
    const int c0 = pc0[i], nc = pc0[i + 1] - c0;
    const float cnt = (float)(row0[i + 1] - row0[i] - T);
    const float *p0 = part + (size_t)c0 * D;
    float m[kFeatPoolMaxD / 256], ss = 0.0f;      // columns threadIdx.x + 256 q: the operand and the feature are rounded and stored from these registers
#pragma unroll
    for (int q = 0; q < kFeatPoolMaxD / 256; ++q) {
        const int col = threadIdx.x + 256 * q;
        m[q] = 0.0f;
        if (col < D) {
            float s = p0[col];
            for (int k = 1; k < nc; ++k) s = s + p0[(size_t)k * D + col];
            m[q] = s / cnt;
            if (z) z[(size_t)i * 2 * D + D + col] = (T16)m[q];
        }
        ss += m[q] * m[q];
    }
    if (!mean) return;
    float nrm = 0.0f;
    if (l2) {            // uniform: every thread reaches the barrier
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
        if ((threadIdx.x & 63) == 0) ssq[threadIdx.x >> 6] = ss;
        __syncthreads();
        nrm = sqrtf(((ssq[0] + ssq[1]) + ssq[2]) + ssq[3]);
    }
#pragma unroll
    for (int q = 0; q < kFeatPoolMaxD / 256; ++q) {
        const int col = threadIdx.x + 256 * q;
        if (col < D) mean[(size_t)i * D + col] = nrm > 0.0f ? m[q] / nrm : m[q];     // an all-zero vector stays zero
    }
}

template <typename T16>
hipError_t launch_feat_pool_t(const float *x, const int *row0, const int *pc0, int n, int chunks, int T, const float *w, const float *b, float eps, float *part, float *cls,
                              float *mean, void *z, int m_pad, int D, bool l2, hipStream_t stream) {
    const bool ok = ln_for_width(D, [&](auto vec, auto nv) {
        static_assert(64 * vec() * nv() <= kFeatPoolMaxD, "the combine kernel holds kFeatPoolMaxD / 256 columns per thread");
        hipLaunchKernelGGL((feat_pool_part_kernel<vec(), nv()>), dim3(chunks), dim3(feat_pool_waves(D) * 64), 0, stream, x, row0, pc0, n, T, w, b, eps, part, cls, z,
                           std::is_same<T16, __bf16>::value ? 1 : 0, l2 ? 1 : 0);
    });
    if (!ok) return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !part) return e;
    hipLaunchKernelGGL((feat_pool_combine_kernel<T16>), dim3(z ? m_pad : n), dim3(256), 0, stream, part, row0, pc0, n, T, D, mean, (T16 *)z, l2 ? 1 : 0);
    return hipGetLastError();
}

}  // namespace

bool feat_pool_chunks(const int32_t *row0, int n, int T, int32_t *pc0) {
    if (!row0 || n <= 0 || T < 0) return false;
    int64_t c = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t np = (int64_t)row0[i + 1] - row0[i] - T;
        if (np < 1) return false;
        if (pc0) pc0[i] = (int32_t)c;
        c += (np + kFeatPoolChunkRows - 1) / kFeatPoolChunkRows;
        if (c > 0x7fffffffLL) return false;
    }
    if (pc0) pc0[n] = (int32_t)c;
    return true;
}

hipError_t launch_feat_pool_packed(const float *x, const int *row0, const int *pc0, int n, int chunks, int T, const float *w, const float *b, float eps, float *part, float *cls,
                                   float *mean, void *z, int dtype, int m_pad, int D, bool l2, hipStream_t stream) {
    if (n <= 0 || chunks < n || T < 0 || (!cls && !mean && !z) || ((mean || z) && !part) || (z && (T < 1 || m_pad < n)) || (cls && T < 1)) return hipErrorInvalidValue;
    if (!mean && !z) part = nullptr;     // the class rows alone: no patch row is read, no second launch
    return VITX_BY_DTYPE(dtype, launch_feat_pool_t, x, row0, pc0, n, chunks, T, w, b, eps, part, cls, mean, z, m_pad, D, l2, stream);
}

}  // namespace vitx
