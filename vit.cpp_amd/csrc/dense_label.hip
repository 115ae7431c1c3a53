// dense_label.hip -- the label map of the dense head (vitx_dense_set, vitx_op_dense_labels, vitx_pack_dense_set, vitx_op_dense_labels_packed; the
// contract: include/vitx.h "dense prediction"): the K logit planes of an image's gh x gw patch grid resampled bilinearly to out_h x out_w
// (dense_resample.h: ONE definition of the weights and of the value, shared with the host function) and arg-maxed over k < K in vitx_topk's order.
// A workgroup owns a kDenseTileW x kDenseTileH tile of one image's output; what it does there is dense_tile (dense_tile.h), one text for both kernels:
//   dense_label_kernel          images of ONE shape: logits [n * gh * gw][ld] f32 (row = image, then patch in raster order) -> labels [n][out_h][out_w]
//                               u8 and, score != nullptr, score [n][out_h][out_w] f32 = the winner's value.  The grid is tiles x tiles x images.
//   dense_label_packed_kernel   a PACK: image i has its own first logit row lrow_i, grid (gh_i, gw_i), output (oh_i, ow_i) and first output element
//                               pix0_i (the maps end to end).  A work item is (image, tile) and the grid is sum_i tiles_i workgroups, so one 4096 x 4096
//                               output beside two hundred 224 x 224 ones balances itself.  A workgroup finds its image by a wave-uniform binary search
//                               of blockIdx.x in tile0 [n + 1], the running tile count, as attention_packed_kernel does with qb0: every load of the
//                               search and of the image's table row has a uniform address.  The LDS of the launch and the class chunk come from the
//                               largest window of any image of the call; an image's bits do not depend on them (dense_tile.h).  Only the rows
//                               lrow_i .. lrow_i + gh_i gw_i - 1 are read, columns below K rounded up to 4; nothing outside elements pix0_0 .. pix0_n - 1
//                               is written.
#include "kernels.h"
#include "dense_tile.h"

namespace vitx {

namespace {

constexpr int kDenseLds = 64 * 1024;           // dynamic LDS of one workgroup at most: two and more workgroups per CU inside gfx950's 160 KiB

__global__ __launch_bounds__(256) void dense_label_kernel(const float *__restrict__ logits, long ld, int gh, int gw, int K, int out_h, int out_w,
                                                          float sy, float sx, uint8_t *__restrict__ labels, float *__restrict__ score,
                                                          int KC, int KCp, int cells_max) {
    const size_t img = blockIdx.z, px = (size_t)out_h * out_w;
    dense_tile(logits + img * gh * gw * ld, ld, gh, gw, K, out_h, out_w, sy, sx, labels + img * px, score ? score + img * px : nullptr,
               blockIdx.x * kDenseTileW, blockIdx.y * kDenseTileH, KC, KCp, cells_max);
}

// seg [n][kDenseSegInts]: dense_pack_seg's rows.  The scales are the host's dense_scale values, carried as bits.
__global__ __launch_bounds__(256) void dense_label_packed_kernel(const float *__restrict__ logits, long ld, const int *__restrict__ tile0, const int *__restrict__ seg,
                                                                 int n, int K, uint8_t *__restrict__ labels, float *__restrict__ score, int KC, int KCp, int cells_max) {
    const int wg = blockIdx.x;
    int lo = 0, hi = n;                        // the image: tile0[lo] <= wg < tile0[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile0[mid] <= wg) lo = mid; else hi = mid;
    }
    const int *s = seg + (size_t)lo * kDenseSegInts;
    const int lrow = s[0], gh = s[1], gw = s[2], out_h = s[3], out_w = s[4];
    const size_t pix0 = (size_t)(uint32_t)s[5] | ((size_t)(uint32_t)s[6] << 32);
    const float sy = __int_as_float(s[7]), sx = __int_as_float(s[8]);
    const int item = wg - tile0[lo], tw = (out_w + kDenseTileW - 1) / kDenseTileW, tyi = item / tw, txi = item - tyi * tw;
    dense_tile(logits + (size_t)lrow * ld, ld, gh, gw, K, out_h, out_w, sy, sx, labels + pix0, score ? score + pix0 : nullptr,
               txi * kDenseTileW, tyi * kDenseTileH, KC, KCp, cells_max);
}

// the window of a tile: the source positions of its first and last pixel lie (T - 1) * scale apart, so their cells at most floor of that + 1,
// the second tap one more; one cell of margin for the rounding of the float positions.  The kernel checks its own window against the product.
int dense_window(int gh, int gw, int out_h, int out_w) {
    const float sy = dense_scale(gh, out_h), sx = dense_scale(gw, out_w);
    return std::min(gw, (int)((kDenseTileW - 1) * sx) + 4) * std::min(gh, (int)((kDenseTileH - 1) * sy) + 4);
}

// the class chunk KC and the row stride KCp of the LDS image (an odd number of 16-byte slots) for a window of `cells`; false: nothing fits
bool dense_chunk(int cells, int K, int *KC_out, int *KCp_out) {
    int KC = (K + 3) & ~3, KCp = 0;
    for (; KC >= 4; KC -= 4) {
        KCp = KC + (((KC >> 2) & 1) ? 0 : 4);
        if ((size_t)cells * KCp * 4 <= (size_t)kDenseLds) break;
    }
    *KC_out = KC; *KCp_out = KCp;
    return KC >= 4;                            // 67 x 19 cells x 12 floats fit: always
}

}  // namespace

hipError_t prepare_dense() {
    const hipError_t e = hipFuncSetAttribute((const void *)dense_label_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDenseLds);
    return e != hipSuccess ? e : hipFuncSetAttribute((const void *)dense_label_packed_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDenseLds);
}

bool dense_labels_supports(long ld, int n, int gh, int gw, int K, int out_h, int out_w) {
    return n >= 1 && n <= 65535 && gh >= 1 && gw >= 1 && K >= 1 && K <= kDenseMaxK && out_h >= gh && out_w >= gw && out_h <= kDenseMaxOut && out_w <= kDenseMaxOut &&
           ld >= ((K + 3) & ~3) && ld % 4 == 0 && (size_t)n * gh * gw <= 0x7fffffffu;
}

hipError_t launch_dense_labels(const float *logits, long ld, int n, int gh, int gw, int K, int out_h, int out_w, uint8_t *labels, float *score, hipStream_t stream) {
    if (!dense_labels_supports(ld, n, gh, gw, K, out_h, out_w) || ((uintptr_t)logits & 15)) return hipErrorInvalidValue;
    const float sy = dense_scale(gh, out_h), sx = dense_scale(gw, out_w);
    const int cells = dense_window(gh, gw, out_h, out_w);
    int KC, KCp;
    if (!dense_chunk(cells, K, &KC, &KCp)) return hipErrorInvalidValue;
    const dim3 grid((out_w + kDenseTileW - 1) / kDenseTileW, (out_h + kDenseTileH - 1) / kDenseTileH, n);
    hipLaunchKernelGGL(dense_label_kernel, grid, dim3(256), (size_t)cells * KCp * 4, stream, logits, ld, gh, gw, K, out_h, out_w, sy, sx, labels, score, KC, KCp, cells);
    return hipGetLastError();
}

bool dense_pack_tables(const int32_t *grids, const int32_t *outs, int n, int64_t *pix0, int32_t *tile0, int *cells) {
    int64_t px = 0, tiles = 0;
    int widest = 0;
    for (int i = 0; i < n; ++i) {
        const int gh = grids[2 * i], gw = grids[2 * i + 1], oh = outs[2 * i], ow = outs[2 * i + 1];
        if (gh < 1 || gw < 1 || oh < gh || ow < gw || oh > kDenseMaxOut || ow > kDenseMaxOut) return false;
        if (pix0) pix0[i] = px;
        if (tile0) tile0[i] = (int32_t)tiles;
        px += (int64_t)oh * ow;
        tiles += (int64_t)((ow + kDenseTileW - 1) / kDenseTileW) * ((oh + kDenseTileH - 1) / kDenseTileH);
        if (tiles > 0x7fffffff) return false;
        widest = std::max(widest, dense_window(gh, gw, oh, ow));
    }
    if (pix0) pix0[n] = px;
    if (tile0) tile0[n] = (int32_t)tiles;
    if (cells) *cells = widest;
    return true;
}

void dense_pack_seg(const int32_t *grids, const int32_t *outs, const int32_t *lrow, const int64_t *pix0, int n, int32_t *seg) {
    for (int i = 0; i < n; ++i) {
        int32_t *s = seg + (size_t)i * kDenseSegInts;
        s[0] = lrow[i]; s[1] = grids[2 * i]; s[2] = grids[2 * i + 1]; s[3] = outs[2 * i]; s[4] = outs[2 * i + 1];
        s[5] = (int32_t)(uint32_t)((uint64_t)pix0[i] & 0xffffffffu); s[6] = (int32_t)(uint32_t)((uint64_t)pix0[i] >> 32);
        s[7] = __builtin_bit_cast(int32_t, dense_scale(s[1], s[3])); s[8] = __builtin_bit_cast(int32_t, dense_scale(s[2], s[4]));
        s[9] = 0;
    }
}

hipError_t launch_dense_labels_packed(const float *logits, long ld, const int *tile0, const int *seg, int n, int tiles, int cells, int K, uint8_t *labels, float *score,
                                      hipStream_t stream) {
    if (n < 1 || tiles < n || cells < 1 || K < 1 || K > kDenseMaxK || ld < ((K + 3) & ~3) || ld % 4 || ((uintptr_t)logits & 15) || !tile0 || !seg || !labels) return hipErrorInvalidValue;
    int KC, KCp;
    if (!dense_chunk(cells, K, &KC, &KCp)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dense_label_packed_kernel, dim3((unsigned)tiles), dim3(256), (size_t)cells * KCp * 4, stream, logits, ld, tile0, seg, n, K, labels, score, KC, KCp, cells);
    return hipGetLastError();
}

}  // namespace vitx
