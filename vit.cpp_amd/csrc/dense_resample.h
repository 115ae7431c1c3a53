// dense_resample.h -- the bilinear resampling of the dense head's logit planes (include/vitx.h "dense prediction"), ONE definition of the arithmetic
// for the host function (vitx_dense_labels_host, dense_host.cpp) and the device kernel (dense_label.hip).  Both are compiled with
// -ffp-contract=off and use only f32 add, subtract, multiply, IEEE divide and int <-> float conversions, so they produce the same bits.
//
// F.interpolate(mode="bilinear", align_corners=False), per axis (g = source cells, out = target cells, o = target index):
//   scale = (float)g / (float)out;  s = ((float)o + 0.5f) * scale - 0.5f, clamped below at 0;  i0 = (int)s;  i1 = i0 + (i0 < g - 1);
//   l = s - (float)i0;  h = 1.0f - l
// Value of a pixel from its four taps a = v(y0, x0), b = v(y0, x1), c = v(y1, x0), d = v(y1, x1):
//   top = hx a + lx b;  bot = hx c + lx d;  v = hy top + ly bot          (every product and every sum rounded on its own)
// The winner among the classes is the first entry of vitx_topk's total order (topk_rank.h: value descending, then index ascending, +0 and -0 tie,
// NaN last): walking the classes upwards from class 0, a class takes the pixel only when it comes strictly earlier in that order than the best so
// far -- it is a number and the best so far is smaller or a NaN.  Ties stay with the lower index, a NaN never takes it, a pixel of NaNs keeps class 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef VITX_HD
#define VITX_HD __host__ __device__ inline
#endif

namespace vitx {

struct DenseAxis {
    int i0, i1;            // the two source cells
    float l, h;            // their weights: h for i0, l for i1
};

VITX_HD float dense_scale(int g, int out) { return (float)g / (float)out; }

VITX_HD DenseAxis dense_axis(int g, float scale, int o) {
    DenseAxis ax;
    float s = ((float)o + 0.5f) * scale - 0.5f;
    if (s < 0.0f) s = 0.0f;
    ax.i0 = (int)s;
    if (ax.i0 > g - 1) ax.i0 = g - 1;          // never taken for out >= g (s < g - 1/2): keeps every index inside the grid whatever the caller passes
    ax.i1 = ax.i0 + (ax.i0 < g - 1 ? 1 : 0);
    ax.l = s - (float)ax.i0;
    ax.h = 1.0f - ax.l;
    return ax;
}

// T = float, or a vector of floats (the kernel computes 4 classes of a pixel at a time): the same operations element by element
template <typename T> VITX_HD T dense_value(float hx, float lx, float hy, float ly, T a, T b, T c, T d) {
    const T top = hx * a + lx * b, bot = hx * c + lx * d;
    return hy * top + ly * bot;
}

// The running winner of one pixel over the classes met in ascending order
struct DenseBest {
    int cls;
    float v;               // the winner's value: a NaN only while every class so far was one (then cls == 0)
};
VITX_HD DenseBest dense_best_init() { DenseBest b; b.cls = 0; b.v = __builtin_bit_cast(float, 0x7fc00000u); return b; }
// !(v <= b.v): v is above the best, or one of the two is a NaN; with v == v: v is a number that beats a number, or the first number after NaNs
VITX_HD void dense_offer(DenseBest &b, float v, int k) {
    if (!(v <= b.v) && v == v) { b.cls = k; b.v = v; }
}
// The score that is written: the winner's value bit for bit; a NaN (a pixel of NaNs only) as the quiet NaN 0x7fc00000, whose payload and sign
// would otherwise be the processor's choice
VITX_HD float dense_score(const DenseBest &b) { return b.v != b.v ? __builtin_bit_cast(float, 0x7fc00000u) : b.v; }

// The launch geometry of dense_label.hip: a workgroup owns kDenseTileW x kDenseTileH output pixels
constexpr int kDenseTileW = 64, kDenseTileH = 16;

}  // namespace vitx
