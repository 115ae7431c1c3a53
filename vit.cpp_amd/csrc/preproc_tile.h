// preproc_tile.h -- one output tile of Pillow's Image.resize on u8 with mean / std: the ONE body pp_pil_kernel (n sources of one size, one output
// window) and pp_pil_packed_kernel (a pack of sources, each with its own size and its own output) run, in the manner of dense_tile.h and
// depth_tile.h: the kernels differ in how a workgroup finds its image and its tile, never in what it computes there.  The arithmetic is
// preproc_resample.h's, shared with the host loop in preprocess.cpp.
//   img u8 HWC [ny][nx][3]: the image's own source -> out f32 HWC [SH][SW][3], the image's own output window (its corner at (left, top) of the
//   resized image ax.out x ay.out); the tile is the PP_TW x PP_TH (32 x 8) output pixels from (ox0, oy0).
// A workgroup of 4 waves:
//   A  lanes 0 .. 39 (32 columns, then 8 rows; indices past the window's edge repeat its last one) find first / n of their target index and
//      the weight total ww, in double;
//   B  every lane fills the fixed-point coefficient rows k[32][kx], k[8][ky] (one IEEE divide per tap);
//   C  horizontal pass: wave w takes source rows y0 + w, y0 + w + 4, ... of the rows [y0, y0 + R) the tile's vertical taps span.  The row's
//      bytes [3 x0, 3 (x0 + span)) are staged in LDS by aligned dword loads (consecutive lanes, consecutive dwords: the first and the last
//      dword may reach up to 3 bytes outside the span but never leave a dword that holds a byte of it -- so a source may start at any byte of a
//      buffer that is 4-byte aligned and readable up to its byte count rounded up to 4; what a straddling dword holds of a neighbour is never
//      used), then 96 (column, channel) sums per row read the taps as LDS bytes -- the three channels of a pixel and neighbouring taps share
//      dwords -- and write u8 to h[R][96];
//   D  vertical pass over h, clamp, normalise, f32 stores: 96 consecutive floats per tile row.
// The LDS is laid out by the image's OWN kx, ky, rows, span, stage (pp_tiling() on the host, computed with the same pil_bounds) from the start of
// the launch's dynamic LDS, which holds at least the image's own pp_tiling().lds; the body clamps its spans to them, so an index cannot leave
// the allocation whatever the arithmetic gives, and no bit depends on how much LDS the launch has beyond that.  No atomics; one writer per
// element; nothing outside the image's own SH x SW x 3 floats is written.
#pragma once
#include "preproc_resample.h"

namespace vitx {

// mean / std of channel k of a description (vitx_preproc::mean255 / std255)
struct PpMeanStd {
    float m0, m1, m2, s0, s1, s2;
    __device__ __forceinline__ float mean(int k) const { return k == 0 ? m0 : (k == 1 ? m1 : m2); }
    __device__ __forceinline__ float sd(int k) const { return k == 0 ? s0 : (k == 1 ? s1 : s2); }
};

// one image's geometry and tiling, workgroup-uniform
struct PpTileGeom {
    int nx, ny, SW, SH, left, top;
    PilAxis ax, ay;
    int kx, ky, rows, span, stage;
};

extern __shared__ __attribute__((aligned(16))) unsigned char pp_lds[];      // the dynamic LDS of both kernels

// Called by all 256 lanes of the workgroup with workgroup-uniform arguments (it holds barriers)
__device__ __forceinline__ void pp_pil_tile(const unsigned char *__restrict__ img, float *__restrict__ out, const PpTileGeom &a, const PpMeanStd &nm, int ox0, int oy0) {
    constexpr int NP = PP_TW + PP_TH, LINE = PP_TW * 3;
    double *s_ww = (double *)pp_lds;                          // [NP]
    int *s_first = (int *)(s_ww + NP), *s_n = s_first + NP;   // [NP] each
    int32_t *s_kx = (int32_t *)(s_n + NP);                    // [PP_TW][kx]
    int32_t *s_ky = s_kx + PP_TW * a.kx;                      // [PP_TH][ky]
    unsigned char *s_h = (unsigned char *)(s_ky + PP_TH * a.ky);      // [rows][LINE]
    unsigned char *s_stage = s_h + (size_t)a.rows * LINE;     // [PP_WAVES][stage], dword aligned: LINE is a multiple of 4

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
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
    // the source window of this tile, clamped to what the host sized the image's LDS for
    const int x0 = s_first[0], y0 = s_first[PP_TW];
    int span = 0, R = 0;
    for (int c = 0; c < PP_TW; ++c) span = max(span, s_first[c] + s_n[c] - x0);
    for (int r = 0; r < PP_TH; ++r) R = max(R, s_first[PP_TW + r] + s_n[PP_TW + r] - y0);
    span = min(span, a.span); R = min(R, a.rows);
    __syncthreads();

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

    for (int item = tid; item < PP_TH * LINE; item += 256) {
        const int ty = item / LINE, e = item - ty * LINE, tx = e / 3, ch = e - tx * 3;
        const int oy = oy0 + ty, ox = ox0 + tx;
        if (oy >= a.SH || ox >= a.SW) continue;
        const int rel = min(s_first[PP_TW + ty] - y0, R), nt = min(s_n[PP_TW + ty], R - rel);
        const unsigned char *m = s_h + rel * LINE + e;
        const int32_t *k = s_ky + ty * a.ky;
        int32_t acc = 1 << (PIL_PRECISION_BITS - 1);
        for (int i = 0; i < nt; ++i) acc += (int32_t)m[i * LINE] * k[i];
        out[((size_t)oy * a.SW + ox) * 3 + ch] = ((float)pil_clip8(acc) - nm.mean(ch)) / nm.sd(ch);
    }
}

}  // namespace vitx
