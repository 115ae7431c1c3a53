// image_preprocess.hip -- device-side image resize + normalisation (the host version: preprocess.cpp).
#include <algorithm>

#include "kernels.h"
#include "epilogue16.h"
#include "device_common.h"
#include "model_file.h"
#include "preproc_resample.h"
#include "preproc_tile.h"

namespace vitx {

// ------------------------------------------------------------------------------------------------
// Device-side vit_image_preprocess (vit.cpp:289-305; bicubic 204-287, bilinear 130-196): u8 HWC
// [n][ny][nx][3] -> f32 HWC [n][S][S][3], one thread per output pixel.  Operation for operation the
// host version in preprocess.cpp (double cubic coefficients narrowed to float, float polynomial,
// roundf / clamp / narrow to u8, (q - mean) / std with IEEE division; the library is built with
// -ffp-contract=off), so the two agree bit for bit.
// ------------------------------------------------------------------------------------------------
// mean / std of channel k: the ImageNet literals of vit_image_preprocess, or a description's own (vitx_preproc::mean255 / std255)
struct PpImageNet {
    __device__ __forceinline__ float mean(int k) const { return k == 0 ? 123.675f : (k == 1 ? 116.280f : 103.530f); }
    __device__ __forceinline__ float sd(int k) const { return k == 0 ? 58.395f : (k == 1 ? 57.120f : 57.375f); }
};
template <class NORM> __device__ __forceinline__ float pp_norm(float v, int k, const NORM &nm) {
    const unsigned char q = (unsigned char)fminf(fmaxf(roundf(v), 0.0f), 255.0f);
    return ((float)q - nm.mean(k)) / nm.sd(k);
}
__device__ __forceinline__ float pp_cubic(float p0, float p1, float p2, float p3, float t) {
    const float d0 = p0 - p1, d2 = p2 - p1, d3 = p3 - p1;
    const float a1 = (float)(-1.0 / 3 * d0 + d2 - 1.0 / 6 * d3);
    const float a2 = (float)(1.0 / 2 * d0 + 1.0 / 2 * d2);
    const float a3 = (float)(-1.0 / 6 * d0 - 1.0 / 2 * d2 + 1.0 / 6 * d3);
    return p1 + a1 * t + a2 * t * t + a3 * t * t * t;
}
__device__ __forceinline__ int pp_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool BICUBIC, class NORM>
__device__ __forceinline__ void preprocess_body(const unsigned char *__restrict__ src, float *__restrict__ dst, int n, int nx, int ny, int S, const NORM &nm) {
    const long total = (long)n * S * S;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
        const int b = (int)(id / ((long)S * S)), rem = (int)(id - (long)b * S * S), i = rem / S, j = rem - i * S;
        const unsigned char *im = src + (size_t)b * nx * ny * 3;
        float *o = dst + (size_t)id * 3;
        if (BICUBIC) {
            const float tx = (float)nx / (float)S, ty = (float)ny / (float)S;
            const int y = (int)(ty * i), x = (int)(tx * j);
            const float dy = ty * i - y, dx = tx * j - x;
            const int x0 = pp_clamp(x - 1, 0, nx - 1), x1 = pp_clamp(x, 0, nx - 1), x2 = pp_clamp(x + 1, 0, nx - 1), x3 = pp_clamp(x + 2, 0, nx - 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float C[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const unsigned char *r = im + (size_t)pp_clamp(y - 1 + jj, 0, ny - 1) * nx * 3 + k;
                    C[jj] = pp_cubic(r[x0 * 3], r[x1 * 3], r[x2 * 3], r[x3 * 3], dx);
                }
                o[k] = pp_norm(pp_cubic(C[0], C[1], C[2], C[3], dy), k, nm);
            }
        } else {
            const float xs = nx / (float)S, ys = ny / (float)S;
            const float sy = (i + 0.5f) * ys - 0.5f, sx = (j + 0.5f) * xs - 0.5f;
            const int y0 = sy < 0.0f ? 0 : (int)floorf(sy), y1 = y0 + 1 < ny - 1 ? y0 + 1 : ny - 1;
            const int x0 = sx < 0.0f ? 0 : (int)floorf(sx), x1 = x0 + 1 < nx - 1 ? x0 + 1 : nx - 1;
            const float dy = sy - y0, dx = sx - x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v00 = im[3 * ((size_t)y0 * nx + x0) + c], v01 = im[3 * ((size_t)y0 * nx + x1) + c];
                const float v10 = im[3 * ((size_t)y1 * nx + x0) + c], v11 = im[3 * ((size_t)y1 * nx + x1) + c];
                const float v0 = v00 * (1.0f - dx) + v01 * dx, v1 = v10 * (1.0f - dx) + v11 * dx;
                o[c] = pp_norm(v0 * (1.0f - dy) + v1 * dy, c, nm);
            }
        }
    }
}
template <bool BICUBIC>
__global__ __launch_bounds__(256) void preprocess_kernel(const unsigned char *__restrict__ src, float *__restrict__ dst, int n, int nx, int ny, int S) {
    preprocess_body<BICUBIC>(src, dst, n, nx, ny, S, PpImageNet());
}
// the same resize with a description's own mean / std (vitx_preprocess_ex_device with a REF filter)
template <bool BICUBIC>
__global__ __launch_bounds__(256) void preprocess_ms_kernel(const unsigned char *__restrict__ src, float *__restrict__ dst, int n, int nx, int ny, int S, PpMeanStd nm) {
    preprocess_body<BICUBIC>(src, dst, n, nx, ny, S, nm);
}
hipError_t launch_preprocess(const void *u8, float *out, int n, int nx, int ny, int S, int bicubic, hipStream_t stream) {
    const long total = (long)n * S * S;
    const int blocks = (int)std::min<long>((total + 255) / 256, 256L * 64);
    if (bicubic) hipLaunchKernelGGL(preprocess_kernel<true>, dim3(blocks), dim3(256), 0, stream, (const unsigned char *)u8, out, n, nx, ny, S);
    else hipLaunchKernelGGL(preprocess_kernel<false>, dim3(blocks), dim3(256), 0, stream, (const unsigned char *)u8, out, n, nx, ny, S);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Pillow's Image.resize on u8 + centre crop + mean / std (include/vitx.h "each model's own preprocessing"; the arithmetic: preproc_resample.h,
// shared with the host loop in preprocess.cpp, so both give Pillow's bits).  A workgroup of 4 waves owns a PP_TW x PP_TH (32 x 8) tile of one
// image's output window; what it does there is pp_pil_tile (preproc_tile.h), one text for both kernels:
//   pp_pil_kernel          sources of ONE size: u8 HWC [n][ny][nx][3] -> f32 HWC [n][SH][SW][3] in one launch (the window is SW x SH: square for a
//                          description, any pair for vitx_preprocess_rect_device).  The grid is tiles x images.
//   pp_pil_packed_kernel   a PACK: source i is u8 HWC [ny_i][nx_i][3], the sources strictly end to end (so they start at every alignment mod 4),
//                          stretched to its own h_i x w_i, the f32 outputs end to end, in one launch.  A work item is (image, tile) and the grid is
//                          sum_i tiles_i workgroups, 1-D; a workgroup finds its image by a wave-uniform binary search of blockIdx.x in tile0 [n + 1],
//                          the running tile count, as dense_label_packed_kernel does.  The image's table row (pp_pack_tables) gives its offsets, sizes
//                          and its OWN tiling; the two PilAxis are rebuilt by pil_axis, the VITX_HD function the host sized the tiling with.  The
//                          launch's LDS is the largest tiling of the call; an image's bits depend neither on it nor on its neighbours.
// Every LDS size comes from pp_tiling() on the host, computed with the same pil_bounds; the body clamps its own spans to them.
// ------------------------------------------------------------------------------------------------
struct PpPilArgs {
    const unsigned char *src; float *dst;
    int tiles_x;
    PpTileGeom g;
    PpMeanStd nm;
};

__global__ __launch_bounds__(256) void pp_pil_kernel(const PpPilArgs a) {
    const int bx = blockIdx.x % a.tiles_x, by = blockIdx.x / a.tiles_x, b = blockIdx.y;
    pp_pil_tile(a.src + (size_t)b * a.g.nx * a.g.ny * 3, a.dst + (size_t)b * a.g.SH * a.g.SW * 3, a.g, a.nm, bx * PP_TW, by * PP_TH);
}

// seg [n][kPpSegInts]: pp_pack_tables's rows
__global__ __launch_bounds__(256) void pp_pil_packed_kernel(const unsigned char *__restrict__ srcs, float *__restrict__ dst, const int *__restrict__ tile0,
                                                            const int *__restrict__ seg, int n, int bicubic, const PpMeanStd nm) {
    const int wg = blockIdx.x;
    int lo = 0, hi = n;                        // the image: tile0[lo] <= wg < tile0[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile0[mid] <= wg) lo = mid; else hi = mid;
    }
    const int *s = seg + (size_t)lo * kPpSegInts;
    const size_t src0 = (size_t)(uint32_t)s[0] | ((size_t)(uint32_t)s[1] << 32), dst0 = (size_t)(uint32_t)s[2] | ((size_t)(uint32_t)s[3] << 32);
    PpTileGeom g;
    g.nx = s[4]; g.ny = s[5]; g.SW = s[6]; g.SH = s[7]; g.left = 0; g.top = 0;
    const int tiles_x = s[8];
    g.kx = s[9]; g.ky = s[10]; g.rows = s[11]; g.span = s[12]; g.stage = s[13];
    g.ax = pil_axis(bicubic, g.nx, g.SW); g.ay = pil_axis(bicubic, g.ny, g.SH);
    const int item = wg - tile0[lo], by = item / tiles_x, bx = item - by * tiles_x;
    pp_pil_tile(srcs + src0, dst + dst0, g, nm, bx * PP_TW, by * PP_TH);
}

static hipError_t launch_pp_pil(const vitx_preproc &p, const PpGeom &g, const PpMeanStd &nm, const void *u8, float *out, int n, int nx, int ny, hipStream_t stream);

bool preprocess_ex_supports(const vitx_preproc &p, int nx, int ny) {
    PpGeom g;
    if (pp_check(p) || pp_geometry(p, nx, ny, g)) return false;
    if (!pp_filter_is_pil(p.filter)) return true;
    const int bicubic = p.filter == VITX_PP_PIL_BICUBIC;
    return pp_tiling(g, pil_axis(bicubic, nx, g.W), pil_axis(bicubic, ny, g.H)).lds <= (size_t)PP_LDS_LIMIT;
}

hipError_t launch_preprocess_ex(const vitx_preproc &p, const void *u8, float *out, int n, int nx, int ny, hipStream_t stream) {
    PpGeom g;
    if (n <= 0 || pp_check(p) || pp_geometry(p, nx, ny, g)) return hipErrorInvalidValue;
    const PpMeanStd nm = {p.mean255[0], p.mean255[1], p.mean255[2], p.std255[0], p.std255[1], p.std255[2]};
    if (!pp_filter_is_pil(p.filter)) {
        const vitx_preproc d = pp_default(g.SW);
        bool imagenet = true;
        for (int c = 0; c < 3; ++c) imagenet = imagenet && p.mean255[c] == d.mean255[c] && p.std255[c] == d.std255[c];
        const int bicubic = p.filter == VITX_PP_REF_BICUBIC;
        if (imagenet) return launch_preprocess(u8, out, n, nx, ny, g.SW, bicubic, stream);
        const long total = (long)n * g.SW * g.SW;
        const int blocks = (int)std::min<long>((total + 255) / 256, 256L * 64);
        if (bicubic) hipLaunchKernelGGL(preprocess_ms_kernel<true>, dim3(blocks), dim3(256), 0, stream, (const unsigned char *)u8, out, n, nx, ny, g.SW, nm);
        else hipLaunchKernelGGL(preprocess_ms_kernel<false>, dim3(blocks), dim3(256), 0, stream, (const unsigned char *)u8, out, n, nx, ny, g.SW, nm);
        return hipGetLastError();
    }
    return launch_pp_pil(p, g, nm, u8, out, n, nx, ny, stream);
}

// pp_pil_kernel on the window of g: the one launch of both the description's geometry and vitx_preprocess_rect_device's
static hipError_t launch_pp_pil(const vitx_preproc &p, const PpGeom &g, const PpMeanStd &nm, const void *u8, float *out, int n, int nx, int ny, hipStream_t stream) {
    PpPilArgs a;
    const int bicubic = p.filter == VITX_PP_PIL_BICUBIC;
    a.g.ax = pil_axis(bicubic, nx, g.W); a.g.ay = pil_axis(bicubic, ny, g.H);
    const PpTiling t = pp_tiling(g, a.g.ax, a.g.ay);
    if (t.lds > (size_t)PP_LDS_LIMIT) return hipErrorInvalidValue;
    a.g.nx = nx; a.g.ny = ny; a.g.SW = g.SW; a.g.SH = g.SH; a.g.left = g.left; a.g.top = g.top;
    a.tiles_x = (g.SW + PP_TW - 1) / PP_TW;
    a.g.kx = t.kx; a.g.ky = t.ky; a.g.rows = t.rows; a.g.span = t.span; a.g.stage = t.stage; a.nm = nm;
    const int tiles = a.tiles_x * ((g.SH + PP_TH - 1) / PP_TH);
    for (int i0 = 0; i0 < n; i0 += 65535) {                   // gridDim.y: images
        const int ni = std::min(n - i0, 65535);
        a.src = (const unsigned char *)u8 + (size_t)i0 * nx * ny * 3;
        a.dst = out + (size_t)i0 * g.SH * g.SW * 3;
        hipLaunchKernelGGL(pp_pil_kernel, dim3(tiles, ni), dim3(256), t.lds, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

bool preprocess_rect_supports(const vitx_preproc &p, int nx, int ny, int out_w, int out_h) {
    PpGeom g;
    if (pp_check(p) || !pp_filter_is_pil(p.filter) || pp_geometry_rect(nx, ny, out_w, out_h, g)) return false;
    const int bicubic = p.filter == VITX_PP_PIL_BICUBIC;
    return pp_tiling(g, pil_axis(bicubic, nx, g.W), pil_axis(bicubic, ny, g.H)).lds <= (size_t)PP_LDS_LIMIT;
}

hipError_t launch_preprocess_rect(const vitx_preproc &p, const void *u8, float *out, int n, int nx, int ny, int out_w, int out_h, hipStream_t stream) {
    PpGeom g;
    if (n <= 0 || pp_check(p) || !pp_filter_is_pil(p.filter) || pp_geometry_rect(nx, ny, out_w, out_h, g)) return hipErrorInvalidValue;
    const PpMeanStd nm = {p.mean255[0], p.mean255[1], p.mean255[2], p.std255[0], p.std255[1], p.std255[2]};
    return launch_pp_pil(p, g, nm, u8, out, n, nx, ny, stream);
}

// ---- a pack of sources (include/vitx.h "packed batches", u8 sources) -------------------------------------------------------------------
int pp_pack_tables(const char *api, const vitx_preproc &p, const int32_t *src_shapes, const int32_t *out_shapes, int n, int64_t *src0, int64_t *dst0, int32_t *tile0,
                   int32_t *seg, int *lds) {
    if (!src_shapes || !out_shapes || n < 1) { set_error("%s: invalid argument", api); return VITX_ERR_ARG; }
    if (const char *bad = pp_check(p)) { set_error("%s: %s", api, bad); return VITX_ERR_ARG; }
    if (!pp_filter_is_pil(p.filter)) { set_error("%s: the reference's filters resize to squares only (use a PIL filter)", api); return VITX_ERR_UNSUPPORTED; }
    const int bicubic = p.filter == VITX_PP_PIL_BICUBIC;
    int64_t sb = 0, df = 0, tiles = 0;
    size_t most = 0;
    PpTiling t{};
    for (int i = 0; i < n; ++i) {
        const int ny = src_shapes[2 * i], nx = src_shapes[2 * i + 1], oh = out_shapes[2 * i], ow = out_shapes[2 * i + 1];
        PpGeom g;
        if (const char *bad = pp_geometry_rect(nx, ny, ow, oh, g)) { set_error("%s: image %d: %s", api, i, bad); return VITX_ERR_ARG; }
        // a run of images of one source and output size shares one tiling
        const bool same = i > 0 && src_shapes[2 * i - 2] == ny && src_shapes[2 * i - 1] == nx && out_shapes[2 * i - 2] == oh && out_shapes[2 * i - 1] == ow;
        if (!same) t = pp_tiling(g, pil_axis(bicubic, nx, ow), pil_axis(bicubic, ny, oh));
        if (t.lds > (size_t)PP_LDS_LIMIT) {
            set_error("%s: image %d: a %d x %d source resized to %d x %d needs more than 64 KiB of LDS per tile (use vitx_preprocess_rect)", api, i, nx, ny, ow, oh);
            return VITX_ERR_UNSUPPORTED;
        }
        const int tiles_x = (ow + PP_TW - 1) / PP_TW;
        if (src0) src0[i] = sb;
        if (dst0) dst0[i] = df;
        if (tile0) tile0[i] = (int32_t)tiles;
        if (seg) {
            int32_t *s = seg + (size_t)i * kPpSegInts;
            s[0] = (int32_t)(uint32_t)((uint64_t)sb & 0xffffffffu); s[1] = (int32_t)(uint32_t)((uint64_t)sb >> 32);
            s[2] = (int32_t)(uint32_t)((uint64_t)df & 0xffffffffu); s[3] = (int32_t)(uint32_t)((uint64_t)df >> 32);
            s[4] = nx; s[5] = ny; s[6] = ow; s[7] = oh; s[8] = tiles_x;
            s[9] = t.kx; s[10] = t.ky; s[11] = t.rows; s[12] = t.span; s[13] = t.stage;
        }
        sb += (int64_t)nx * ny * 3;
        df += (int64_t)ow * oh * 3;
        tiles += (int64_t)tiles_x * ((oh + PP_TH - 1) / PP_TH);
        if (tiles > 0x7fffffff) { set_error("%s: the call's outputs hold more than 2^31 - 1 tiles", api); return VITX_ERR_ARG; }
        most = std::max(most, t.lds);
    }
    if (src0) src0[n] = sb;
    if (dst0) dst0[n] = df;
    if (tile0) tile0[n] = (int32_t)tiles;
    if (lds) *lds = (int)most;
    return VITX_OK;
}

hipError_t launch_preprocess_pack(const vitx_preproc &p, const void *u8, float *out, const int *tile0, const int *seg, int n, int tiles, int lds, hipStream_t stream) {
    if (n < 1 || tiles < n || lds < 1 || lds > PP_LDS_LIMIT || pp_check(p) || !pp_filter_is_pil(p.filter) || !u8 || !out || !tile0 || !seg || ((uintptr_t)u8 & 3)) return hipErrorInvalidValue;
    const PpMeanStd nm = {p.mean255[0], p.mean255[1], p.mean255[2], p.std255[0], p.std255[1], p.std255[2]};
    hipLaunchKernelGGL(pp_pil_packed_kernel, dim3((unsigned)tiles), dim3(256), (size_t)lds, stream, (const unsigned char *)u8, out, tile0, seg, n,
                       (int)(p.filter == VITX_PP_PIL_BICUBIC), nm);
    return hipGetLastError();
}

}  // namespace vitx
