// dense_tile.h -- one output tile of the dense head's label map: the ONE body dense_label_kernel (a launch of images of one shape) and
// dense_label_packed_kernel (a pack of images, each with its own grid and output) run, in the manner of attention_rows.h: the kernels differ in
// how a workgroup finds its image and its tile, never in what it computes there.  The arithmetic is dense_resample.h's.
//   lg [gh * gw][ld] f32: the image's own logit rows (columns K .. ld are never compared) -> labels [out_h][out_w] u8 and, score != nullptr,
//   score [out_h][out_w] f32, the image's own maps; the tile is the kDenseTileW x kDenseTileH pixels from (X0, Y0).
// The grid cells the tile's pixels touch form a window of ncx x ncy cells (upsampling only: at most one cell more than the tile's pixels per axis; at
// the usual scale 16 a 64 x 16 tile touches about 6 x 3); the window's logits go to LDS as [cell][KCp] rows -- every logit loaded ONCE per workgroup,
// 16 bytes per lane, non-temporal (the GEMM wrote them one launch ago and nothing reads them again) -- in chunks of KC classes when window x K does
// not fit the LDS of the launch; a lane keeps the running winner of its 4 pixels (class, value) across chunks, the classes in ascending order, so
// a pixel's bits do not depend on KC, KCp or cells_max (a pack takes them from its largest window).  A lane reads the taps of 4 classes per
// ds_read_b128 and computes them as one vector (packed f32 multiplies and adds); KCp / 4 is odd, so the rows of neighbouring cells start in
// different 16-byte slots of the bank row.  Where the 4 pixels of every lane of a wave share their two source columns -- always at the usual
// scales, 4 | 16 -- the four taps are read once for the 4 pixels.  Labels leave as one 4-byte store per lane, scores as one 16-byte store, where
// the row allows it (compact rows of out_w: a row whose start is off the pack's boundary, and the last columns of a width that is no multiple of 4,
// go element by element).  No atomics; one writer per element; nothing outside the image's own out_h x out_w elements is written.
#pragma once
#include "device_common.h"
#include "dense_resample.h"

namespace vitx {

constexpr int kDensePack = 4;                  // pixels per lane: one row, consecutive x
static_assert(kDenseTileW == 16 * kDensePack && kDenseTileH == 16, "256 lanes: 16 x 16, each with kDensePack pixels of a row");

extern __shared__ f32x4 dense_lds[];           // [cell][KCp / 4] groups of 4 classes: the dynamic LDS of both kernels

// Called by all 256 lanes of the workgroup with workgroup-uniform arguments (it holds barriers)
__device__ __forceinline__ void dense_tile(const float *__restrict__ lg, long ld, int gh, int gw, int K, int out_h, int out_w, float sy, float sx,
                                           uint8_t *__restrict__ labels, float *__restrict__ score, int X0, int Y0, int KC, int KCp, int cells_max) {
    const int KCq = KCp >> 2;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int X1 = min(X0 + kDenseTileW - 1, out_w - 1), Y1 = min(Y0 + kDenseTileH - 1, out_h - 1);
    // the window of grid cells: the source index grows with the target index, so the first pixel's i0 and the last pixel's i1 bound it
    const int cx0 = dense_axis(gw, sx, X0).i0, cy0 = dense_axis(gh, sy, Y0).i0;
    const int ncx = dense_axis(gw, sx, X1).i1 - cx0 + 1, ncy = dense_axis(gh, sy, Y1).i1 - cy0 + 1;
    if (ncx * ncy > cells_max) return;         // workgroup-uniform; the launcher's bound on the window says never -- and nothing is written past the LDS if it were wrong
    const int y = min(Y0 + ty, out_h - 1);     // lanes past the edge compute a pixel of the edge and store nothing
    const DenseAxis ay = dense_axis(gh, sy, y);
    const int r0 = (ay.i0 - cy0) * ncx - cx0, r1 = (ay.i1 - cy0) * ncx - cx0;
    int o_a[kDensePack], o_b[kDensePack], o_c[kDensePack], o_d[kDensePack];        // the four taps' rows in the LDS image (in groups of 4 floats)
    float hx[kDensePack], lx[kDensePack];
    DenseBest best[kDensePack];
#pragma unroll
    for (int p = 0; p < kDensePack; ++p) {
        const DenseAxis ax = dense_axis(gw, sx, min(X0 + tx * kDensePack + p, out_w - 1));
        o_a[p] = (r0 + ax.i0) * KCq; o_b[p] = (r0 + ax.i1) * KCq; o_c[p] = (r1 + ax.i0) * KCq; o_d[p] = (r1 + ax.i1) * KCq;
        hx[p] = ax.h; lx[p] = ax.l;
        best[p] = dense_best_init();
    }
    // wave-uniform: the 4 pixels of every lane share the cell pair of pixel 0 (the taps are then read once per lane, not once per pixel)
    const bool shared = __all(o_a[1] == o_a[0] && o_b[1] == o_b[0] && o_a[2] == o_a[0] && o_b[2] == o_b[0] && o_a[3] == o_a[0] && o_b[3] == o_b[0]);
    const int K4 = (K + 3) & ~3, cells = ncx * ncy;
    for (int k0 = 0; k0 < K4; k0 += KC) {
        const int q4 = min(KC, K4 - k0) >> 2, total = cells * q4;
        if (k0) __syncthreads();               // every lane has read the previous chunk
        for (int idx = tid; idx < total; idx += 256) {
            const int cell = idx / q4, q = idx - cell * q4, cy = cell / ncx, cx = cell - cy * ncx;
            const f32x4 v = __builtin_nontemporal_load((const f32x4 *)(lg + ((size_t)(cy0 + cy) * gw + (cx0 + cx)) * ld + k0 + 4 * q));
            dense_lds[cell * KCq + q] = v;
        }
        __syncthreads();
        // 4 classes of one pixel: the value as a vector, then the classes in ascending order; a pad column never reaches the comparison
        auto offer4 = [&](int p, int q, f32x4 a, f32x4 b, f32x4 c, f32x4 d) {
            const f32x4 v = dense_value(hx[p], lx[p], ay.h, ay.l, a, b, c, d);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = k0 + 4 * q + e;
                if (k < K) dense_offer(best[p], v[e], k);
            }
        };
        if (shared) {
            for (int q = 0; q < q4; ++q) {
                const f32x4 a = dense_lds[o_a[0] + q], b = dense_lds[o_b[0] + q], c = dense_lds[o_c[0] + q], d = dense_lds[o_d[0] + q];
#pragma unroll
                for (int p = 0; p < kDensePack; ++p) offer4(p, q, a, b, c, d);
            }
        } else {
            for (int q = 0; q < q4; ++q) {
#pragma unroll
                for (int p = 0; p < kDensePack; ++p)
                    offer4(p, q, dense_lds[o_a[p] + q], dense_lds[o_b[p] + q], dense_lds[o_c[p] + q], dense_lds[o_d[p] + q]);
            }
        }
    }
    const int yy = Y0 + ty, x0 = X0 + tx * kDensePack;
    if (yy >= out_h || x0 >= out_w) return;
    const size_t pix = (size_t)yy * out_w + x0;
    const bool whole = x0 + kDensePack <= out_w;
    if (whole && ((uintptr_t)(labels + pix) & 3) == 0) {
        *(uint32_t *)(labels + pix) = (uint32_t)best[0].cls | ((uint32_t)best[1].cls << 8) | ((uint32_t)best[2].cls << 16) | ((uint32_t)best[3].cls << 24);
    } else {
#pragma unroll
        for (int p = 0; p < kDensePack; ++p) if (x0 + p < out_w) labels[pix + p] = (uint8_t)best[p].cls;
    }
    if (!score) return;
    if (whole && ((uintptr_t)(score + pix) & 15) == 0) {
        *(f32x4 *)(score + pix) = f32x4{dense_score(best[0]), dense_score(best[1]), dense_score(best[2]), dense_score(best[3])};
    } else {
#pragma unroll
        for (int p = 0; p < kDensePack; ++p) if (x0 + p < out_w) score[pix + p] = dense_score(best[p]);
    }
}

}  // namespace vitx
