// depth_map.hip -- the tail of the depth head (vitx_depth_set, vitx_op_depth_fine, vitx_op_depth_resize; the contract: include/vitx.h "depth
// estimation"): K bin logits per grid cell -> one depth per fine cell -> the depth map.
//   depth_fine:   logits [n * gh * gw][ld] f32 (row = image, then patch in raster order; columns K .. ld never reach a sum), offsets [n][..] f32 added
//                 to every cell of an image -> fine [n][u gh][u gw] f32: the K planes resampled bilinearly x u (dense_resample.h), then the bins reduced
//                 in ascending order (depth_bins.h: relu, + 0.1, the two running sums, one division).
//   depth_resize: fine [n][fh][fw] -> depth [n][out_h][out_w] f32, the same resampling on one plane, then the clamp.
//   depth_rows:   the raw operand rows: f32 rows with a row and a group stride -> rows of the operand type (RNE) with a stride and a column offset.
// What a workgroup computes on its tile is depth_tile.h's depth_fine_tile and depth_resize_tile, one text for the fixed-shape and the packed kernels:
//   depth_fine_kernel / depth_resize_kernel   images of ONE shape; the grid is tiles x tiles x images.
//   depth_fine_packed_kernel / depth_resize_packed_kernel   a PACK (vitx_pack_depth_set, vitx_op_depth_fine_packed, vitx_op_depth_resize_packed): image i
//                 has its own first logit row, offsets row, grid (gh_i, gw_i), fine plane (u gh_i, u gw_i) starting fine0_i floats into `fine`, and output
//                 (oh_i, ow_i) starting pix0_i floats into `out` (planes and maps end to end).  A work item is (image, 16 x 16 fine tile) or (image, 64 x 16
//                 output tile) and the grid is 1-D, sum_i tiles_i workgroups -- nothing uses blockIdx.z, so no n <= 65535.  A workgroup finds its image by a
//                 wave-uniform binary search of blockIdx.x in the running tile count (ftile0 / otile0 [n + 1]), as dense_label_packed_kernel does: every
//                 load of the search and of the image's table row has a uniform address.  The LDS of the fine launch and the bin chunk come from the
//                 widest window of any image of the call; an image's bits do not depend on them (depth_tile.h).
//   depth_gather:  the class rows of a pack: dst[i][:] = src[rows[i]][:], rows of Dc operand elements, 16 bytes per lane.
#include "kernels.h"
#include "depth_tile.h"

namespace vitx {

namespace {

constexpr int kDepthLds = 64 * 1024;           // dynamic LDS of one workgroup at most: two and more workgroups per CU inside gfx950's 160 KiB

__global__ __launch_bounds__(256) void depth_fine_kernel(const float *__restrict__ logits, long ld, const float *__restrict__ offsets, long ldo,
                                                         const float *__restrict__ bins, int gh, int gw, int K, int fh, int fw, float sy, float sx,
                                                         float *__restrict__ fine, int KC, int KCp, int cells_max) {
    const size_t img = blockIdx.z;
    depth_fine_tile(logits + img * gh * gw * ld, ld, offsets ? offsets + img * ldo : nullptr, bins, gh, gw, K, fh, fw, sy, sx, fine + img * fh * fw,
                    blockIdx.x * kDepthTile, blockIdx.y * kDepthTile, KC, KCp, cells_max);
}

__global__ __launch_bounds__(256) void depth_resize_kernel(const float *__restrict__ fine, int fh, int fw, int out_h, int out_w, float sy, float sx,
                                                           float lo, float hi, float *__restrict__ out) {
    const size_t img = blockIdx.z;
    depth_resize_tile(fine + img * fh * fw, fh, fw, out_h, out_w, sy, sx, lo, hi, out + img * out_h * out_w, blockIdx.x * kDepthOutW, blockIdx.y * kDepthOutH);
}

// the image of workgroup wg: tile0[lo] <= wg < tile0[lo + 1].  A binary search on uniform addresses (scalar loads).  A 64-ary search by the wave (64
// probes per load, a ballot, two dependent loads for n <= 4096) was measured in its place and was no faster: x1.20 against x1.17 on the resize launch
// of profiles/pack_depth_cost.txt -- what the packed resize pays is the prologue as a whole in front of a microsecond of work, not the search's depth.
__device__ __forceinline__ int depth_pack_image(const int *__restrict__ tile0, int n, int wg) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile0[mid] <= wg) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ size_t depth_seg_off(const int *s) { return (size_t)(uint32_t)s[0] | ((size_t)(uint32_t)s[1] << 32); }

// seg [n][kDepthSegInts]: depth_pack_seg's rows.  The scales are the host's dense_scale values, carried as bits.
__global__ __launch_bounds__(256) void depth_fine_packed_kernel(const float *__restrict__ logits, long ld, const float *__restrict__ offsets, long ldo,
                                                                const float *__restrict__ bins, const int *__restrict__ ftile0, const int *__restrict__ seg, int n,
                                                                int K, float *__restrict__ fine, int KC, int KCp, int cells_max) {
    const int wg = blockIdx.x, img = depth_pack_image(ftile0, n, wg);
    const int *s = seg + (size_t)img * kDepthSegInts;
    const int lrow = s[0], orow = s[1], gh = s[2], gw = s[3], fh = s[4], fw = s[5];
    const int item = wg - ftile0[img], tw = (fw + kDepthTile - 1) / kDepthTile, tyi = item / tw, txi = item - tyi * tw;
    depth_fine_tile(logits + (size_t)lrow * ld, ld, offsets ? offsets + (size_t)orow * ldo : nullptr, bins, gh, gw, K, fh, fw, __int_as_float(s[12]), __int_as_float(s[13]),
                    fine + depth_seg_off(s + 8), txi * kDepthTile, tyi * kDepthTile, KC, KCp, cells_max);
}

__global__ __launch_bounds__(256) void depth_resize_packed_kernel(const float *__restrict__ fine, const int *__restrict__ otile0, const int *__restrict__ seg, int n,
                                                                  float lo, float hi, float *__restrict__ out) {
    const int wg = blockIdx.x, img = depth_pack_image(otile0, n, wg);
    const int *s = seg + (size_t)img * kDepthSegInts;
    const int fh = s[4], fw = s[5], out_h = s[6], out_w = s[7];
    const int item = wg - otile0[img], tw = (out_w + kDepthOutW - 1) / kDepthOutW, tyi = item / tw, txi = item - tyi * tw;
    depth_resize_tile(fine + depth_seg_off(s + 8), fh, fw, out_h, out_w, __int_as_float(s[14]), __int_as_float(s[15]), lo, hi, out + depth_seg_off(s + 10),
                      txi * kDepthOutW, tyi * kDepthOutH);
}

// q = 16-byte pieces per row; one piece per lane
__global__ __launch_bounds__(256) void depth_gather_kernel(const uint4 *__restrict__ src, const int *__restrict__ rows, uint4 *__restrict__ dst, int n, int q) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * q) return;
    const size_t i = idx / q, c = idx - i * q;
    dst[i * q + c] = src[(size_t)rows[i] * q + c];
}

// the window of a fine tile: the source positions of its first and last cell lie (T - 1) * scale apart, so their cells at most floor of that + 1,
// the second tap one more; one cell of margin for the rounding of the float positions.  The kernel checks its own window against the product.
int depth_window(int gh, int gw, int u) {
    const float sy = dense_scale(gh, u * gh), sx = dense_scale(gw, u * gw);
    return std::min(gw, (int)((kDepthTile - 1) * sx) + 4) * std::min(gh, (int)((kDepthTile - 1) * sy) + 4);
}

// the bin chunk KC and the row stride KCp of the LDS image (an odd number of 16-byte slots) for a window of `cells`; false: nothing fits
bool depth_chunk(int cells, int K, int *KC_out, int *KCp_out) {
    int KC = (K + 3) & ~3, KCp = 0;
    for (; KC >= 4; KC -= 4) {
        KCp = KC + (((KC >> 2) & 1) ? 0 : 4);
        if ((size_t)cells * KCp * 4 <= (size_t)kDepthLds) break;
    }
    *KC_out = KC; *KCp_out = KCp;
    return KC >= 4;                            // 19 x 19 cells x 12 floats fit: always
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

hipError_t prepare_depth() {
    const hipError_t e = hipFuncSetAttribute((const void *)depth_fine_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDepthLds);
    return e != hipSuccess ? e : hipFuncSetAttribute((const void *)depth_fine_packed_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDepthLds);
}

bool depth_fine_supports(long ld, long ldo, int n, int gh, int gw, int K, int u) {
    return n >= 1 && n <= 65535 && gh >= 1 && gw >= 1 && K >= 1 && K <= kDepthMaxK && (u == 1 || u == 2 || u == 4) && ld >= ((K + 3) & ~3) && ld % 4 == 0 &&
           (ldo == 0 || (ldo >= ((K + 3) & ~3) && ldo % 4 == 0)) && (size_t)n * gh * gw <= 0x7fffffffu && (size_t)u * gh <= kDepthMaxOut && (size_t)u * gw <= kDepthMaxOut;
}

hipError_t launch_depth_fine(const float *logits, long ld, const float *offsets, long ldo, const float *bins, int n, int gh, int gw, int K, int u, float *fine,
                             hipStream_t stream) {
    if (!depth_fine_supports(ld, ldo, n, gh, gw, K, u) || ((uintptr_t)logits & 15) || ((uintptr_t)offsets & 15)) return hipErrorInvalidValue;
    const int fh = u * gh, fw = u * gw;
    const float sy = dense_scale(gh, fh), sx = dense_scale(gw, fw);
    const int cells = depth_window(gh, gw, u);
    int KC, KCp;
    if (!depth_chunk(cells, K, &KC, &KCp)) return hipErrorInvalidValue;
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

bool depth_pack_tables(const int32_t *grids, const int32_t *outs, int n, int u, int64_t *pix0, int64_t *fine0, int32_t *ftile0, int32_t *otile0, int *cells) {
    if (u != 1 && u != 2 && u != 4) return false;
    int64_t px = 0, fpx = 0, ft = 0, ot = 0;
    int widest = 0;
    for (int i = 0; i < n; ++i) {
        const int gh = grids[2 * i], gw = grids[2 * i + 1], oh = outs[2 * i], ow = outs[2 * i + 1];
        if (gh < 1 || gw < 1 || (int64_t)u * gh > kDepthMaxOut || (int64_t)u * gw > kDepthMaxOut) return false;
        const int fh = u * gh, fw = u * gw;
        if (oh < fh || ow < fw || oh > kDepthMaxOut || ow > kDepthMaxOut) return false;
        if (pix0) pix0[i] = px;
        if (fine0) fine0[i] = fpx;
        if (ftile0) ftile0[i] = (int32_t)ft;
        if (otile0) otile0[i] = (int32_t)ot;
        px += (int64_t)oh * ow; fpx += (int64_t)fh * fw;
        ft += (int64_t)((fw + kDepthTile - 1) / kDepthTile) * ((fh + kDepthTile - 1) / kDepthTile);
        ot += (int64_t)((ow + kDepthOutW - 1) / kDepthOutW) * ((oh + kDepthOutH - 1) / kDepthOutH);
        if (ft > 0x7fffffff || ot > 0x7fffffff) return false;
        widest = std::max(widest, depth_window(gh, gw, u));
    }
    if (pix0) pix0[n] = px;
    if (fine0) fine0[n] = fpx;
    if (ftile0) ftile0[n] = (int32_t)ft;
    if (otile0) otile0[n] = (int32_t)ot;
    if (cells) *cells = widest;
    return true;
}

void depth_pack_seg(const int32_t *grids, const int32_t *outs, const int32_t *lrow, const int32_t *orow, const int64_t *fine0, const int64_t *pix0, int n, int u, int32_t *seg) {
    auto put64 = [](int32_t *s, int64_t v) { s[0] = (int32_t)(uint32_t)((uint64_t)v & 0xffffffffu); s[1] = (int32_t)(uint32_t)((uint64_t)v >> 32); };
    for (int i = 0; i < n; ++i) {
        int32_t *s = seg + (size_t)i * kDepthSegInts;
        s[0] = lrow[i]; s[1] = orow[i]; s[2] = grids[2 * i]; s[3] = grids[2 * i + 1]; s[4] = u * s[2]; s[5] = u * s[3]; s[6] = outs[2 * i]; s[7] = outs[2 * i + 1];
        put64(s + 8, fine0[i]); put64(s + 10, pix0[i]);
        s[12] = __builtin_bit_cast(int32_t, dense_scale(s[2], s[4])); s[13] = __builtin_bit_cast(int32_t, dense_scale(s[3], s[5]));
        s[14] = __builtin_bit_cast(int32_t, dense_scale(s[4], s[6])); s[15] = __builtin_bit_cast(int32_t, dense_scale(s[5], s[7]));
    }
}

hipError_t launch_depth_fine_packed(const float *logits, long ld, const float *offsets, long ldo, const float *bins, const int *ftile0, const int *seg, int n, int tiles,
                                    int cells, int K, float *fine, hipStream_t stream) {
    if (n < 1 || tiles < n || cells < 1 || K < 1 || K > kDepthMaxK || ld < ((K + 3) & ~3) || ld % 4 || (ldo != 0 && (ldo < ((K + 3) & ~3) || ldo % 4)) ||
        ((uintptr_t)logits & 15) || ((uintptr_t)offsets & 15) || !logits || !bins || !ftile0 || !seg || !fine) return hipErrorInvalidValue;
    int KC, KCp;
    if (!depth_chunk(cells, K, &KC, &KCp)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(depth_fine_packed_kernel, dim3((unsigned)tiles), dim3(256), (size_t)cells * KCp * 4, stream, logits, ld, offsets, ldo, bins, ftile0, seg, n, K, fine,
                       KC, KCp, cells);
    return hipGetLastError();
}

hipError_t launch_depth_resize_packed(const float *fine, const int *otile0, const int *seg, int n, int tiles, float lo, float hi, float *out, hipStream_t stream) {
    if (n < 1 || tiles < n || !fine || !otile0 || !seg || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(depth_resize_packed_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, fine, otile0, seg, n, lo, hi, out);
    return hipGetLastError();
}

hipError_t launch_depth_gather(const void *src, int Dc, const int *rows, void *dst, int n, hipStream_t stream) {
    if (n < 1 || Dc < 8 || Dc % 8 || !src || !rows || !dst || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return hipErrorInvalidValue;
    const size_t total = (size_t)n * (Dc / 8);
    hipLaunchKernelGGL(depth_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const uint4 *)src, rows, (uint4 *)dst, n, Dc / 8);
    return hipGetLastError();
}

hipError_t launch_depth_rows(int dtype, const float *x, long ldx, void *y, long ldy, long rows, int D, hipStream_t stream, int group, long gstride) {
    if (rows < 1 || D < 8 || D % 8 || ldx % 4 || ldy % 8 || group < 1 || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) || gstride % 4 ||
        (size_t)rows * (D / 8) > 0x7fffffffull * 256) return hipErrorInvalidValue;
    if (group == 1 || gstride == 0) { group = 1; gstride = ldx; }
    return VITX_BY_DTYPE(dtype, depth_rows_launch, x, ldx, gstride, group, y, ldy, (size_t)rows, D, stream);
}

}  // namespace vitx
