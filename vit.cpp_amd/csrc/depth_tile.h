// depth_tile.h -- what one workgroup of the depth head's tail computes on its tile: the ONE body each that the fixed-shape kernels (depth_fine_kernel,
// depth_resize_kernel: a launch of images of one shape) and the packed kernels (depth_fine_packed_kernel, depth_resize_packed_kernel: a pack of
// images, each with its own grid, fine plane and output) run, in the manner of dense_tile.h: the kernels differ in how a workgroup finds its image
// and its tile, never in what it computes there.  The arithmetic is dense_resample.h's and depth_bins.h's.
//   depth_fine_tile:   lg [gh * gw][ld] f32, the image's own logit rows (columns K .. ld never reach a sum), off [K rounded up to 4] f32 the image's
//                      offsets (nullptr: nothing is added) -> fine [fh][fw] f32, the image's own plane; the tile is the kDepthTile x kDepthTile cells
//                      from (X0, Y0), one cell per lane.  The grid cells the tile touches form a window of ncx x ncy cells (at u = 4 about 5 x 5, at
//                      u = 1 at most 17 x 17); the window's logits go to LDS as [cell][KCp] rows -- every logit loaded ONCE per workgroup, 16 bytes
//                      per lane, non-temporal (the GEMM wrote them one launch ago and nothing reads them again), the image's offset added on the way
//                      in -- in chunks of KC bins when window x K does not fit the LDS of the launch; a lane keeps its two sums across chunks, the
//                      bins in ascending order, so a cell's bits do not depend on KC, KCp or cells_max (a pack takes them from its largest window).
//                      A lane reads the four taps of 4 bins per ds_read_b128 and resamples them as one vector; KCp / 4 is odd, so the rows of
//                      neighbouring cells start in different 16-byte slots of the bank row.  bins[k] is indexed by the loop counter alone:
//                      wave-uniform, a scalar load.
//   depth_resize_tile: fine [fh][fw] -> out [out_h][out_w] f32, the image's own planes; the tile is the kDepthOutW x kDepthOutH pixels from (X0, Y0),
//                      4 of a row per lane; the taps come straight from the fine plane (it stays in L2), then the clamp.  A lane's 4 pixels leave as
//                      one 16-byte store where the row allows it (a row whose start is off the 16-byte boundary, and the last columns of a width that
//                      is no multiple of 4, go element by element -- dense_tile's rule for its score).
// No atomics; one writer per element; nothing outside the image's own fh x fw and out_h x out_w elements is written.
#pragma once
#include "device_common.h"
#include "dense_resample.h"
#include "depth_bins.h"

namespace vitx {

constexpr int kDepthPack = 4;                  // output pixels per lane of depth_resize_tile: one row, consecutive x
static_assert(kDepthTile * kDepthTile == 256 && kDepthOutW == 16 * kDepthPack && kDepthOutH == 16, "256 lanes per workgroup");

extern __shared__ f32x4 depth_lds[];           // [cell][KCp / 4] groups of 4 bins: the dynamic LDS of both fine kernels

// Called by all 256 lanes of the workgroup with workgroup-uniform arguments (it holds barriers)
__device__ __forceinline__ void depth_fine_tile(const float *__restrict__ lg, long ld, const float *__restrict__ off, const float *__restrict__ bins, int gh, int gw,
                                                int K, int fh, int fw, float sy, float sx, float *__restrict__ fine, int X0, int Y0, int KC, int KCp, int cells_max) {
    const int KCq = KCp >> 2;
    const int tid = threadIdx.x, tx = tid & (kDepthTile - 1), ty = tid / kDepthTile;
    const int X1 = min(X0 + kDepthTile - 1, fw - 1), Y1 = min(Y0 + kDepthTile - 1, fh - 1);
    // the window of grid cells: the source index grows with the target index, so the first cell's i0 and the last cell's i1 bound it
    const int cx0 = dense_axis(gw, sx, X0).i0, cy0 = dense_axis(gh, sy, Y0).i0;
    const int ncx = dense_axis(gw, sx, X1).i1 - cx0 + 1, ncy = dense_axis(gh, sy, Y1).i1 - cy0 + 1;
    if (ncx * ncy > cells_max) return;         // workgroup-uniform; the launcher's bound on the window says never -- and nothing is written past the LDS if it were wrong
    const int y = min(Y0 + ty, fh - 1), x = min(X0 + tx, fw - 1);      // lanes past the edge compute a cell of the edge and store nothing
    const DenseAxis ay = dense_axis(gh, sy, y), ax = dense_axis(gw, sx, x);
    const int r0 = (ay.i0 - cy0) * ncx - cx0, r1 = (ay.i1 - cy0) * ncx - cx0;
    const int o_a = (r0 + ax.i0) * KCq, o_b = (r0 + ax.i1) * KCq, o_c = (r1 + ax.i0) * KCq, o_d = (r1 + ax.i1) * KCq;
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
    if (Y0 + ty < fh && X0 + tx < fw) fine[(size_t)y * fw + x] = depth_quotient(acc);
}

__device__ __forceinline__ void depth_resize_tile(const float *__restrict__ fine, int fh, int fw, int out_h, int out_w, float sy, float sx, float lo, float hi,
                                                  float *__restrict__ out, int X0, int Y0) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int yy = Y0 + ty, x0 = X0 + tx * kDepthPack;
    if (yy >= out_h || x0 >= out_w) return;
    const DenseAxis ay = dense_axis(fh, sy, yy);
    const float *p0 = fine + (size_t)ay.i0 * fw, *p1 = fine + (size_t)ay.i1 * fw;
    float d[kDepthPack];
#pragma unroll
    for (int p = 0; p < kDepthPack; ++p) {
        const DenseAxis ax = dense_axis(fw, sx, min(x0 + p, out_w - 1));
        d[p] = depth_clamp(dense_value(ax.h, ax.l, ay.h, ay.l, p0[ax.i0], p0[ax.i1], p1[ax.i0], p1[ax.i1]), lo, hi);
    }
    const size_t pix = (size_t)yy * out_w + x0;
    if (x0 + kDepthPack <= out_w && ((uintptr_t)(out + pix) & 15) == 0) {
        *(f32x4 *)(out + pix) = f32x4{d[0], d[1], d[2], d[3]};
    } else {
#pragma unroll
        for (int p = 0; p < kDepthPack; ++p) if (x0 + p < out_w) out[pix + p] = d[p];
    }
}

}  // namespace vitx
