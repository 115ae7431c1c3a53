// image_preprocess.hip -- device-side image resize + normalisation (the host version: preprocess.cpp).
#include <algorithm>

#include "kernels.h"
#include "epilogue16.h"
#include "device_common.h"
#include "model_file.h"
#include "preproc_resample.h"

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
struct PpMeanStd {
    float m0, m1, m2, s0, s1, s2;
    __device__ __forceinline__ float mean(int k) const { return k == 0 ? m0 : (k == 1 ? m1 : m2); }
    __device__ __forceinline__ float sd(int k) const { return k == 0 ? s0 : (k == 1 ? s1 : s2); }
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
// shared with the host loop in preprocess.cpp, so both give Pillow's bits).  u8 HWC [n][ny][nx][3] -> f32 HWC [n][SH][SW][3] in ONE launch (the window is SW x SH: square for a description,
// any pair for vitx_preprocess_rect_device).
// A workgroup of 4 waves owns a PP_TW x PP_TH (32 x 8) tile of one image's output window:
//   A  lanes 0 .. 39 (32 columns, then 8 rows; indices past the window's edge repeat its last one) find first / n of their target index and
//      the weight total ww, in double;
//   B  every lane fills the fixed-point coefficient rows k[32][kx], k[8][ky] (one IEEE divide per tap);
//   C  horizontal pass: wave w takes source rows y0 + w, y0 + w + 4, ... of the rows [y0, y0 + R) the tile's vertical taps span.  The row's
//      bytes [3 x0, 3 (x0 + span)) are staged in LDS by aligned dword loads (consecutive lanes, consecutive dwords: the first and the last
//      dword may reach up to 3 bytes outside the span but never leave a dword that holds a byte of it), then 96 (column, channel) sums per row
//      read the taps as LDS bytes -- the three channels of a pixel and neighbouring taps share dwords -- and write u8 to h[R][96];
//   D  vertical pass over h, clamp, normalise, f32 stores: 96 consecutive floats per tile row.
// Every LDS size comes from pp_tiling() on the host, computed with the same pil_bounds; the kernel clamps its own spans to them, so an index
// cannot leave the allocation whatever the arithmetic gives.
// ------------------------------------------------------------------------------------------------
struct PpPilArgs {
    const unsigned char *src; float *dst;
    int nx, ny, SW, SH, left, top, tiles_x;
    PilAxis ax, ay;
    int kx, ky, rows, span, stage;
    PpMeanStd nm;
};

__global__ __launch_bounds__(256) void pp_pil_kernel(const PpPilArgs a) {
    constexpr int NP = PP_TW + PP_TH, LINE = PP_TW * 3;
    extern __shared__ __attribute__((aligned(16))) unsigned char pp_lds[];
    double *s_ww = (double *)pp_lds;                          // [NP]
    int *s_first = (int *)(s_ww + NP), *s_n = s_first + NP;   // [NP] each
    int32_t *s_kx = (int32_t *)(s_n + NP);                    // [PP_TW][kx]
    int32_t *s_ky = s_kx + PP_TW * a.kx;                      // [PP_TH][ky]
    unsigned char *s_h = (unsigned char *)(s_ky + PP_TH * a.ky);      // [rows][LINE]
    unsigned char *s_stage = s_h + (size_t)a.rows * LINE;     // [PP_WAVES][stage], dword aligned: LINE is a multiple of 4

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int bx = blockIdx.x % a.tiles_x, by = blockIdx.x / a.tiles_x, b = blockIdx.y;
    const int ox0 = bx * PP_TW, oy0 = by * PP_TH;
    auto target = [&](int p) {                                // the resized image's index of table row p
        if (p < PP_TW) { const int o = ox0 + p; return a.left + (o < a.SW ? o : a.SW - 1); }
        const int o = oy0 + p - PP_TW; return a.top + (o < a.SH ? o : a.SH - 1);
    };
    if (tid < NP) {
        const PilAxis &ax = tid < PP_TW ? a.ax : a.ay;
        int first, n;
        pil_bounds(ax, target(tid), first, n);
        s_first[tid] = first; s_n[tid] = n;
        s_ww[tid] = pil_total(ax, target(tid), first, n);
    }
    __syncthreads();
    for (int idx = tid; idx < PP_TW * a.kx + PP_TH * a.ky; idx += 256) {
        const bool isx = idx < PP_TW * a.kx;
        const int rel = isx ? idx : idx - PP_TW * a.kx, ks = isx ? a.kx : a.ky;
        const int p = rel / ks + (isx ? 0 : PP_TW), j = rel - (rel / ks) * ks;
        (isx ? s_kx : s_ky)[rel] = j < s_n[p] ? pil_coeff(isx ? a.ax : a.ay, target(p), s_first[p], j, s_ww[p]) : 0;
    }
    // the source window of this tile, clamped to what the host sized the LDS for
    const int x0 = s_first[0], y0 = s_first[PP_TW];
    int span = 0, R = 0;
    for (int c = 0; c < PP_TW; ++c) span = max(span, s_first[c] + s_n[c] - x0);
    for (int r = 0; r < PP_TH; ++r) R = max(R, s_first[PP_TW + r] + s_n[PP_TW + r] - y0);
    span = min(span, a.span); R = min(R, a.rows);
    __syncthreads();

    const unsigned char *img = a.src + (size_t)b * a.nx * a.ny * 3;
    unsigned char *stage = s_stage + (size_t)wave * a.stage;
    for (int r0 = 0; r0 < R; r0 += PP_WAVES) {                // uniform trip count: the barriers are reached by all four waves
        const int r = r0 + wave;
        int shift = 0;
        if (r < R) {
            const unsigned char *rowp = img + ((size_t)(y0 + r) * a.nx + x0) * 3;
            shift = (int)((uintptr_t)rowp & 3);
            const uint32_t *al = (const uint32_t *)(rowp - shift);
            const int ndw = (shift + 3 * span + 3) >> 2;      // <= stage / 4: stage = 3 * span rounded up to a dword, plus one dword
            for (int d = lane; d < ndw; d += 64) ((uint32_t *)stage)[d] = al[d];
        }
        __syncthreads();
        if (r < R) {
            for (int e = lane; e < LINE; e += 64) {
                const int c = e / 3, ch = e - c * 3;
                const int rel = min(s_first[c] - x0, span), nt = min(s_n[c], span - rel);
                const unsigned char *px = stage + shift + rel * 3 + ch;
                const int32_t *k = s_kx + c * a.kx;
                int32_t acc = 1 << (PIL_PRECISION_BITS - 1);
                for (int j = 0; j < nt; ++j) acc += (int32_t)px[j * 3] * k[j];
                s_h[r * LINE + e] = (unsigned char)pil_clip8(acc);
            }
        }
        __syncthreads();
    }

    float *out = a.dst + (size_t)b * a.SH * a.SW * 3;
    for (int item = tid; item < PP_TH * LINE; item += 256) {
        const int ty = item / LINE, e = item - ty * LINE, tx = e / 3, ch = e - tx * 3;
        const int oy = oy0 + ty, ox = ox0 + tx;
        if (oy >= a.SH || ox >= a.SW) continue;
        const int rel = min(s_first[PP_TW + ty] - y0, R), nt = min(s_n[PP_TW + ty], R - rel);
        const unsigned char *m = s_h + rel * LINE + e;
        const int32_t *k = s_ky + ty * a.ky;
        int32_t acc = 1 << (PIL_PRECISION_BITS - 1);
        for (int i = 0; i < nt; ++i) acc += (int32_t)m[i * LINE] * k[i];
        out[((size_t)oy * a.SW + ox) * 3 + ch] = ((float)pil_clip8(acc) - a.nm.mean(ch)) / a.nm.sd(ch);
    }
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
    a.ax = pil_axis(bicubic, nx, g.W); a.ay = pil_axis(bicubic, ny, g.H);
    const PpTiling t = pp_tiling(g, a.ax, a.ay);
    if (t.lds > (size_t)PP_LDS_LIMIT) return hipErrorInvalidValue;
    a.nx = nx; a.ny = ny; a.SW = g.SW; a.SH = g.SH; a.left = g.left; a.top = g.top;
    a.tiles_x = (g.SW + PP_TW - 1) / PP_TW;
    a.kx = t.kx; a.ky = t.ky; a.rows = t.rows; a.span = t.span; a.stage = t.stage; a.nm = nm;
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

}  // namespace vitx
