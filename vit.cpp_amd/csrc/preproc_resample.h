// preproc_resample.h -- Pillow's Image.resize on u8 (bilinear, bicubic), ONE definition of the arithmetic for the host loop (preprocess.cpp) and
// the device kernel (image_preprocess.hip), and the geometry both derive from a vitx_preproc (include/vitx.h "each model's own preprocessing").
// Both are compiled with -ffp-contract=off; the coefficients use only double add, subtract, multiply, IEEE divide, compares and truncating
// casts, the pixels int32 multiply-adds and an arithmetic shift, so host and device produce the same bits -- Pillow's.
//
// Per axis (in = source length, out = resized length, o = target index), everything in double:
//   scale = (double)in / out;  fs = max(scale, 1.0);  support = S0 * fs  (S0: bilinear 1.0, bicubic 2.0);  ss = 1.0 / fs
//   center = (o + 0.5) * scale;  first = max((int)(center - support + 0.5), 0);  n = min((int)(center + support + 0.5), in) - first
//   w_j = f((j + first - center + 0.5) * ss);  ww = ((w_0 + w_1) + w_2) + ...;  ww != 0: w_j = w_j / ww
//   k_j = w_j < 0 ? (int)(-0.5 + w_j * 4194304.0) : (int)(0.5 + w_j * 4194304.0)
// n never exceeds ksize = (int)ceil(support) * 2 + 1 (Pillow sizes its coefficient rows by it); pil_bounds clamps to it all the same.
// An axis with in == out is the identity: one tap, k = 2^22.
// Per pixel and channel: acc = 2^21 + sum_j px_j * k_j;  q = clamp(acc >> 22, 0, 255).  sum |k_j| * 255 stays below 2^31.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vitx.h"

#ifndef VITX_HD
#define VITX_HD __host__ __device__ inline
#endif

namespace vitx {

enum { PIL_PRECISION_BITS = 22 };

struct PilAxis {
    int in, out, bicubic, ksize;      // ksize: the most taps a target index can have
    double scale, support, ss;
};

VITX_HD PilAxis pil_axis(int bicubic, int in, int out) {
    PilAxis a;
    a.in = in; a.out = out; a.bicubic = bicubic;
    a.scale = (double)in / out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = (bicubic ? 2.0 : 1.0) * fs;
    a.ss = 1.0 / fs;
    a.ksize = in == out ? 1 : (int)ceil(a.support) * 2 + 1;
    return a;
}

VITX_HD double pil_filter(int bicubic, double x) {
    if (x < 0.0) x = -x;
    if (!bicubic) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// first source index and tap count of target index o: 0 <= first, first + n <= in, 0 <= n <= ksize
VITX_HD void pil_bounds(const PilAxis &a, int o, int &first, int &n) {
    if (a.in == a.out) { first = o; n = 1; return; }
    const double center = (o + 0.5) * a.scale;
    int lo = (int)(center - a.support + 0.5), hi = (int)(center + a.support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > a.in) hi = a.in;
    if (lo > a.in) lo = a.in;
    first = lo;
    n = hi - lo;
    if (n < 0) n = 0;
    if (n > a.ksize) n = a.ksize;
}

VITX_HD double pil_raw(const PilAxis &a, int o, int first, int j) {
    const double center = (o + 0.5) * a.scale;
    return pil_filter(a.bicubic, (j + first - center + 0.5) * a.ss);
}

VITX_HD double pil_total(const PilAxis &a, int o, int first, int n) {
    double ww = 0.0;
    for (int j = 0; j < n; ++j) ww += pil_raw(a, o, first, j);
    return ww;
}

VITX_HD int32_t pil_coeff(const PilAxis &a, int o, int first, int j, double ww) {
    if (a.in == a.out) return 1 << PIL_PRECISION_BITS;
    double w = pil_raw(a, o, first, j);
    if (ww != 0.0) w = w / ww;
    return w < 0.0 ? (int32_t)(-0.5 + w * 4194304.0) : (int32_t)(0.5 + w * 4194304.0);
}

VITX_HD int pil_clip8(int32_t acc) {
    const int32_t q = acc >> PIL_PRECISION_BITS;
    return q < 0 ? 0 : (q > 255 ? 255 : q);
}

// ---- geometry of one (description, source size) pair ----------------------------------------------------------------------
struct PpGeom {
    int W, H;          // the resized image
    int left, top;     // the crop window's corner in it
    int SW, SH;        // the output window's width and height (equal for a description: pp_check; any pair for vitx_preprocess_rect)
};

enum { PP_MAX_SIDE = 16384, PP_MAX_SRC = 1 << 20 };

inline bool pp_filter_is_pil(int f) { return f == VITX_PP_PIL_BILINEAR || f == VITX_PP_PIL_BICUBIC; }

// The source-independent rules; nullptr = fine, else what is wrong
inline const char *pp_check(const vitx_preproc &p) {
    if (p.resize_mode != VITX_PP_STRETCH && p.resize_mode != VITX_PP_SHORTEST_EDGE) return "unknown resize_mode";
    if (p.filter < VITX_PP_REF_BICUBIC || p.filter > VITX_PP_PIL_BICUBIC) return "unknown filter";
    if (p.crop_round != 0 && p.crop_round != 1) return "unknown crop_round";
    if (p.resize_a <= 0 || p.resize_a > PP_MAX_SIDE) return "resize_a must be in 1 .. 16384";
    if (p.resize_mode == VITX_PP_STRETCH && (p.resize_b <= 0 || p.resize_b > PP_MAX_SIDE)) return "resize_b must be in 1 .. 16384 (STRETCH)";
    if (p.resize_mode == VITX_PP_SHORTEST_EDGE && p.resize_b != 0) return "resize_b must be 0 (SHORTEST_EDGE)";
    if (p.crop < 0 || p.crop > PP_MAX_SIDE) return "crop must be in 0 .. 16384";
    if (!pp_filter_is_pil(p.filter) && (p.resize_mode != VITX_PP_STRETCH || p.crop != 0)) return "the reference's filters stretch and do not crop";
    if (p.crop > p.resize_a || (p.resize_mode == VITX_PP_STRETCH && p.crop > p.resize_b)) return "the crop is larger than the resized image (padding is not offered)";
    if (p.crop == 0 && (p.resize_mode != VITX_PP_STRETCH || p.resize_a != p.resize_b)) return "the output must be square (a crop, or a stretch to equal sides)";
    for (int c = 0; c < 3; ++c) {
        if (!(p.mean255[c] >= -3.402823466e38f && p.mean255[c] <= 3.402823466e38f)) return "mean255 must be finite";
        if (!(p.std255[c] > 0.0f && p.std255[c] <= 3.402823466e38f)) return "std255 must be finite and positive";
    }
    return nullptr;
}

inline int pp_crop_offset(int d, int crop_round) {
    if (d % 2 == 0 || !crop_round) return d / 2;
    const int k = d / 2;               // d / 2.0 = k + 0.5: half to even
    return k % 2 == 0 ? k : k + 1;
}

// nullptr = fine and g filled, else what is wrong.  pp_check(p) has passed.
inline const char *pp_geometry(const vitx_preproc &p, int nx, int ny, PpGeom &g) {
    if (nx <= 0 || ny <= 0 || nx > PP_MAX_SRC || ny > PP_MAX_SRC) return "the source sides must be in 1 .. 2^20";
    if (p.resize_mode == VITX_PP_STRETCH) { g.W = p.resize_a; g.H = p.resize_b; }
    else {
        const int s = nx <= ny ? nx : ny, l = nx <= ny ? ny : nx;
        const double lv = (double)((int64_t)p.resize_a * l) / (double)s;
        if (!(lv <= (double)PP_MAX_SRC)) return "the resized long side exceeds 2^20";
        const int le = (int)lv;
        if (nx <= ny) { g.W = p.resize_a; g.H = le; } else { g.W = le; g.H = p.resize_a; }
    }
    g.SW = g.SH = p.crop ? p.crop : p.resize_a;
    if (p.crop > g.W || p.crop > g.H) return "the crop is larger than the resized image (padding is not offered)";
    g.left = p.crop ? pp_crop_offset(g.W - p.crop, p.crop_round) : 0;
    g.top = p.crop ? pp_crop_offset(g.H - p.crop, p.crop_round) : 0;
    return nullptr;
}

// vitx_preprocess_rect (include/vitx.h "rectangular contexts"): the whole source stretched to out_w x out_h, no crop; the description gives the
// filter and mean / std only.  nullptr = fine and g filled, else what is wrong.  pp_check(p) has passed.
inline const char *pp_geometry_rect(int nx, int ny, int out_w, int out_h, PpGeom &g) {
    if (nx <= 0 || ny <= 0 || nx > PP_MAX_SRC || ny > PP_MAX_SRC) return "the source sides must be in 1 .. 2^20";
    if (out_w <= 0 || out_h <= 0 || out_w > PP_MAX_SIDE || out_h > PP_MAX_SIDE) return "the output sides must be in 1 .. 16384";
    g.W = g.SW = out_w; g.H = g.SH = out_h; g.left = g.top = 0;
    return nullptr;
}

// The aspect-preserving shape of vitx_rect_shape, in integers only; nullptr = fine, else what is wrong
inline const char *pp_rect_shape(int nx, int ny, int patch, int short_side, int max_long, int &out_w, int &out_h) {
    if (nx <= 0 || ny <= 0 || nx > PP_MAX_SRC || ny > PP_MAX_SRC) return "the source sides must be in 1 .. 2^20";
    if (patch <= 0 || short_side <= 0 || short_side % patch || short_side > PP_MAX_SIDE) return "short_side must be a positive multiple of patch, at most 16384";
    if (max_long != 0 && (max_long < short_side || max_long % patch || max_long > PP_MAX_SIDE)) return "max_long must be 0 or a multiple of patch in short_side .. 16384";
    const int s = nx <= ny ? nx : ny, l = nx <= ny ? ny : nx;
    int64_t lg = (int64_t)short_side * l / s / patch * patch;          // >= short_side: l >= s and short_side is a multiple of patch
    if (max_long != 0 && lg > max_long) lg = max_long;
    if (lg > PP_MAX_SIDE) return "the long side exceeds 16384 (set max_long)";
    if (nx <= ny) { out_w = short_side; out_h = (int)lg; } else { out_w = (int)lg; out_h = short_side; }
    return nullptr;
}

// ---- the device kernel's tiling: what one workgroup keeps in LDS (image_preprocess.hip) -----------------------------------------
enum { PP_TW = 32, PP_TH = 8, PP_WAVES = 4, PP_LDS_LIMIT = 64 * 1024 };

struct PpTiling {
    int kx, ky;        // coefficient row lengths (PilAxis::ksize of either axis)
    int rows;          // most source rows the vertical taps of one tile span
    int span;          // most source pixels the horizontal taps of one tile span
    int stage;         // bytes of one wave's staged source row: 3 * span rounded up to a dword, plus one dword for the alignment of its start
    size_t lds;        // bytes of dynamic LDS
};

inline PpTiling pp_tiling(const PpGeom &g, const PilAxis &ax, const PilAxis &ay) {
    PpTiling t;
    t.kx = ax.ksize; t.ky = ay.ksize; t.rows = 1; t.span = 1;
    for (int o0 = 0; o0 < g.SW; o0 += PP_TW) {                // each axis is walked to its own length
        const int o1 = (o0 + PP_TW < g.SW ? o0 + PP_TW : g.SW) - 1;
        int f0, n0, f1, n1;
        pil_bounds(ax, g.left + o0, f0, n0); pil_bounds(ax, g.left + o1, f1, n1);
        // first and first + n never decrease with o, so the tile's span runs from its first column's first tap to its last column's last
        const int s = (f1 + n1 > f0 + n0 ? f1 + n1 : f0 + n0) - f0;
        if (s > t.span) t.span = s;
    }
    for (int o0 = 0; o0 < g.SH; o0 += PP_TH) {
        const int o1 = (o0 + PP_TH < g.SH ? o0 + PP_TH : g.SH) - 1;
        int f0, n0, f1, n1;
        pil_bounds(ay, g.top + o0, f0, n0); pil_bounds(ay, g.top + o1, f1, n1);
        const int s = (f1 + n1 > f0 + n0 ? f1 + n1 : f0 + n0) - f0;
        if (s > t.rows) t.rows = s;
    }
    t.stage = (3 * t.span + 3) / 4 * 4 + 4;
    // doubles first (16-byte aligned base), then the int32 tables, then the byte tiles: see pp_pil_kernel
    t.lds = (size_t)(PP_TW + PP_TH) * (8 + 4 + 4) + 4 * ((size_t)PP_TW * t.kx + (size_t)PP_TH * t.ky) + (size_t)t.rows * (PP_TW * 3) + (size_t)PP_WAVES * t.stage;
    return t;
}

}  // namespace vitx
