// depth_map.hip -- the tail of the depth head (vitx_depth_set, vitx_op_depth_fine, vitx_op_depth_resize; the contract: include/vitx.h "depth
// estimation"): K bin logits per grid cell -> one depth per fine cell -> the depth map.
//   depth_fine:   logits [n * gh * gw][ld] f32 (row = image, then patch in raster order; columns K .. ld never reach a sum), offsets [n][..] f32 added
//                 to every cell of an image -> fine [n][u gh][u gw] f32: the K planes resampled bilinearly x u (dense_resample.h), then the bins reduced
//                 in ascending order (depth_bins.h: relu, + 0.1, the two running sums, one division).
//   depth_resize: fine [n][fh][fw] -> depth [n][out_h][out_w] f32, the same resampling on one plane, then the clamp.
//   depth_rows:   the raw operand rows: f32 rows with a row and a group stride -> rows of the operand type (RNE) with a stride and a column offset.
// depth_fine: a workgroup of 256 lanes owns a kDepthTile x kDepthTile tile of one image's fine cells, one cell per lane.  The grid cells the tile
// touches form a window of ncx x ncy cells (at u = 4 about 5 x 5, at u = 1 at most 17 x 17); the window's logits go to LDS as [cell][KCp] rows --
// every logit loaded ONCE per workgroup, 16 bytes per lane, non-temporal (the GEMM wrote them one launch ago and nothing reads them again), the
// image's offset added on the way in -- in chunks of KC bins when window x K does not fit the LDS budget; a lane keeps its two sums across chunks.
// A lane reads the four taps of 4 bins per ds_read_b128 and resamples them as one vector; KCp / 4 is odd, so the rows of neighbouring cells start in
// different 16-byte slots of the bank row.  bins[k] is indexed by the loop counter alone: wave-uniform, a scalar load.  No atomics; one writer per
// element; an image's plane depends on its own logits and offsets only.
// depth_resize: a workgroup owns kDepthOutW x kDepthOutH output pixels, 4 of a row per lane; the taps come straight from the fine plane (16 Np floats
// per image: it stays in L2).  A lane's 4 pixels leave as one 16-byte store where the row allows it (a row whose start is off the 16-byte boundary,
// and the last columns of a width that is no multiple of 4, go element by element -- dense_label's rule for its score).
#include "device_common.h"
#include "kernels.h"
#include "dense_resample.h"
#include "depth_bins.h"

namespace vitx {

namespace {

constexpr int kDepthLds = 64 * 1024;           // dynamic LDS of one workgroup at most: two and more workgroups per CU inside gfx950's 160 KiB
constexpr int kDepthPack = 4;                  // output pixels per lane of depth_resize: one row, consecutive x
static_assert(kDepthTile * kDepthTile == 256 && kDepthOutW == 16 * kDepthPack && kDepthOutH == 16, "256 lanes per workgroup");

__global__ __launch_bounds__(256) void depth_fine_kernel(const float *__restrict__ logits, long ld, const float *__restrict__ offsets, long ldo,
                                                         const float *__restrict__ bins, int gh, int gw, int K, int fh, int fw, float sy, float sx,
                                                         float *__restrict__ fine, int KC, int KCp, int cells_max) {
    extern __shared__ f32x4 depth_lds[];       // [cell][KCp / 4] groups of 4 bins
    const int KCq = KCp >> 2;
    const int tid = threadIdx.x, tx = tid & (kDepthTile - 1), ty = tid / kDepthTile;
    const int img = blockIdx.z, X0 = blockIdx.x * kDepthTile, Y0 = blockIdx.y * kDepthTile;
    const int X1 = min(X0 + kDepthTile - 1, fw - 1), Y1 = min(Y0 + kDepthTile - 1, fh - 1);
    // the window of grid cells: the source index grows with the target index, so the first cell's i0 and the last cell's i1 bound it
    const int cx0 = dense_axis(gw, sx, X0).i0, cy0 = dense_axis(gh, sy, Y0).i0;
    const int ncx = dense_axis(gw, sx, X1).i1 - cx0 + 1, ncy = dense_axis(gh, sy, Y1).i1 - cy0 + 1;
    if (ncx * ncy > cells_max) return;         // workgroup-uniform; the launcher's bound on the window says never -- and nothing is written past the LDS if it were wrong
    const int y = min(Y0 + ty, fh - 1), x = min(X0 + tx, fw - 1);      // lanes past the edge compute a cell of the edge and store nothing
    const DenseAxis ay = dense_axis(gh, sy, y), ax = dense_axis(gw, sx, x);
    const int r0 = (ay.i0 - cy0) * ncx - cx0, r1 = (ay.i1 - cy0) * ncx - cx0;
    const int o_a = (r0 + ax.i0) * KCq, o_b = (r0 + ax.i1) * KCq, o_c = (r1 + ax.i0) * KCq, o_d = (r1 + ax.i1) * KCq;
    const float *lg = logits + (size_t)img * gh * gw * ld;
    const float *off = offsets ? offsets + (size_t)img * ldo : nullptr;
    const int K4 = (K + 3) & ~3, cells = ncx * ncy;
    DepthAcc acc = depth_acc_init();
    for (int k0 = 0; k0 < K4; k0 += KC) {
        const int q4 = min(KC, K4 - k0) >> 2, total = cells * q4;
        if (k0) __syncthreads();               // every lane has read the previous chunk
        for (int idx = tid; idx < total; idx += 256) {
            const int cell = idx / q4, q = idx - cell * q4, cy = cell / ncx, cx = cell - cy * ncx;
            f32x4 v = __builtin_nontemporal_load((const f32x4 *)(lg + ((size_t)(cy0 + cy) * gw + (cx0 + cx)) * ld + k0 + 4 * q));
            if (off) v = v + *(const f32x4 *)(off + k0 + 4 * q);       // one rounded add per tap, made once per workgroup
            depth_lds[cell * KCq + q] = v;
        }
        __syncthreads();
        for (int q = 0; q < q4; ++q) {
            const f32x4 v = dense_value(ax.h, ax.l, ay.h, ay.l, depth_lds[o_a + q], depth_lds[o_b + q], depth_lds[o_c + q], depth_lds[o_d + q]);
            const int k = k0 + 4 * q;          // wave-uniform: the bins and the bound on K are scalar
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k + e < K) depth_step(acc, v[e], bins[k + e]);     // a pad column never reaches the sums
        }
    }
    if (Y0 + ty < fh && X0 + tx < fw) fine[((size_t)img * fh + y) * fw + x] = depth_quotient(acc);
}

__global__ __launch_bounds__(256) void depth_resize_kernel(const float *__restrict__ fine, int fh, int fw, int out_h, int out_w, float sy, float sx,
                                                           float lo, float hi, float *__restrict__ out) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int img = blockIdx.z, yy = blockIdx.y * kDepthOutH + ty, x0 = blockIdx.x * kDepthOutW + tx * kDepthPack;
    if (yy >= out_h || x0 >= out_w) return;
    const DenseAxis ay = dense_axis(fh, sy, yy);
    const float *p0 = fine + ((size_t)img * fh + ay.i0) * fw, *p1 = fine + ((size_t)img * fh + ay.i1) * fw;
    float d[kDepthPack];
#pragma unroll
    for (int p = 0; p < kDepthPack; ++p) {
        const DenseAxis ax = dense_axis(fw, sx, min(x0 + p, out_w - 1));
        d[p] = depth_clamp(dense_value(ax.h, ax.l, ay.h, ay.l, p0[ax.i0], p0[ax.i1], p1[ax.i0], p1[ax.i1]), lo, hi);
    }
    const size_t pix = ((size_t)img * out_h + yy) * out_w + x0;
    if (x0 + kDepthPack <= out_w && ((uintptr_t)(out + pix) & 15) == 0) {
        *(f32x4 *)(out + pix) = f32x4{d[0], d[1], d[2], d[3]};
    } else {
#pragma unroll
        for (int p = 0; p < kDepthPack; ++p) if (x0 + p < out_w) out[pix + p] = d[p];
    }
}

// 8 elements per lane: two 16-byte loads, one 16-byte packed store
template <typename T> __global__ __launch_bounds__(256) void depth_rows_kernel(const float *__restrict__ x, long ldx, long gstride, int group, void *__restrict__ y,
                                                                                long ldy, size_t total, int D8) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t row = idx / D8;
    const int ch = (int)(idx - row * D8);
    const size_t g = row / group, r = row - g * group;
    const float *src = x + g * gstride + r * ldx + ch * 8;
    const f32x4 a = *(const f32x4 *)src, b = *(const f32x4 *)(src + 4);
    typedef float f32x8 __attribute__((ext_vector_type(8)));
    const f32x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    *(typename Elem<T>::v8 *)((T *)y + row * ldy + ch * 8) = __builtin_convertvector(v, typename Elem<T>::v8);
}

template <typename T> hipError_t depth_rows_launch(const float *x, long ldx, long gstride, int group, void *y, long ldy, size_t rows, int D, hipStream_t stream) {
    const size_t total = rows * (D / 8);
    hipLaunchKernelGGL(depth_rows_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, ldx, gstride, group, y, ldy, total, D / 8);
    return hipGetLastError();
}

}  // namespace

hipError_t prepare_depth() { return hipFuncSetAttribute((const void *)depth_fine_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDepthLds); }

bool depth_fine_supports(long ld, long ldo, int n, int gh, int gw, int K, int u) {
    return n >= 1 && n <= 65535 && gh >= 1 && gw >= 1 && K >= 1 && K <= kDepthMaxK && (u == 1 || u == 2 || u == 4) && ld >= ((K + 3) & ~3) && ld % 4 == 0 &&
           (ldo == 0 || (ldo >= ((K + 3) & ~3) && ldo % 4 == 0)) && (size_t)n * gh * gw <= 0x7fffffffu && (size_t)u * gh <= kDepthMaxOut && (size_t)u * gw <= kDepthMaxOut;
}

hipError_t launch_depth_fine(const float *logits, long ld, const float *offsets, long ldo, const float *bins, int n, int gh, int gw, int K, int u, float *fine,
                             hipStream_t stream) {
    if (!depth_fine_supports(ld, ldo, n, gh, gw, K, u) || ((uintptr_t)logits & 15) || ((uintptr_t)offsets & 15)) return hipErrorInvalidValue;
    const int fh = u * gh, fw = u * gw;
    const float sy = dense_scale(gh, fh), sx = dense_scale(gw, fw);
    // the window of a tile: the source positions of its first and last cell lie (T - 1) * scale apart, so their cells at most floor of that + 1,
    // the second tap one more; one cell of margin for the rounding of the float positions.  The kernel checks its own window against the product.
    const int wx = std::min(gw, (int)((kDepthTile - 1) * sx) + 4), wy = std::min(gh, (int)((kDepthTile - 1) * sy) + 4), cells = wx * wy;
    const int K4 = (K + 3) & ~3;
    int KC = K4, KCp = 0;
    for (; KC >= 4; KC -= 4) {
        KCp = KC + (((KC >> 2) & 1) ? 0 : 4);          // row stride of the LDS image: an odd number of 16-byte slots
        if ((size_t)cells * KCp * 4 <= (size_t)kDepthLds) break;
    }
    if (KC < 4) return hipErrorInvalidValue;           // 19 x 19 cells x 12 floats fit: not reached
    const dim3 grid((fw + kDepthTile - 1) / kDepthTile, (fh + kDepthTile - 1) / kDepthTile, n);
    hipLaunchKernelGGL(depth_fine_kernel, grid, dim3(256), (size_t)cells * KCp * 4, stream, logits, ld, offsets, ldo, bins, gh, gw, K, fh, fw, sy, sx, fine, KC, KCp, cells);
    return hipGetLastError();
}

bool depth_resize_supports(int n, int fh, int fw, int out_h, int out_w) {
    return n >= 1 && n <= 65535 && fh >= 1 && fw >= 1 && out_h >= fh && out_w >= fw && out_h <= kDepthMaxOut && out_w <= kDepthMaxOut;
}

hipError_t launch_depth_resize(const float *fine, int n, int fh, int fw, int out_h, int out_w, float lo, float hi, float *out, hipStream_t stream) {
    if (!depth_resize_supports(n, fh, fw, out_h, out_w)) return hipErrorInvalidValue;
    const dim3 grid((out_w + kDepthOutW - 1) / kDepthOutW, (out_h + kDepthOutH - 1) / kDepthOutH, n);
    hipLaunchKernelGGL(depth_resize_kernel, grid, dim3(256), 0, stream, fine, fh, fw, out_h, out_w, dense_scale(fh, out_h), dense_scale(fw, out_w), lo, hi, out);
    return hipGetLastError();
}

hipError_t launch_depth_rows(int dtype, const float *x, long ldx, void *y, long ldy, long rows, int D, hipStream_t stream, int group, long gstride) {
    if (rows < 1 || D < 8 || D % 8 || ldx % 4 || ldy % 8 || group < 1 || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) || gstride % 4 ||
        (size_t)rows * (D / 8) > 0x7fffffffull * 256) return hipErrorInvalidValue;
    if (group == 1 || gstride == 0) { group = 1; gstride = ldx; }
    return VITX_BY_DTYPE(dtype, depth_rows_launch, x, ldx, gstride, group, y, ldy, (size_t)rows, D, stream);
}

}  // namespace vitx
