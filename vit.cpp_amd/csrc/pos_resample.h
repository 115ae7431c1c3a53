// pos_resample.h -- resampling of the position-embedding grid (include/vitx.h: vitx_pos_embed_resample), ONE definition of the arithmetic
// for the host loop (pos_resample_host.cpp) and the device kernel (pos_resample.hip).  Both are compiled with -ffp-contract=off and use only
// f32 add, subtract, multiply, IEEE divide, floorf, fabsf and int <-> float conversions, so they produce the same bits.
//
// Per axis (in = source cells, out = target cells, o = target index), scale = (float)in / (float)out (computed on the HOST in both paths):
//   VITX_POS_BICUBIC     x = scale * ((float)o + 0.5f) - 0.5f;  i0 = floorf(x);  t = x - i0;  A = -0.75f
//                        taps i0 - 1 .. i0 + 2, each index clamped to [0, in - 1];
//                        w0 = ((A (t+1) - 5A)(t+1) + 8A)(t+1) - 4A;  w1 = ((A+2) t - (A+3)) t t + 1;  w2 = the w1 form of 1 - t;  w3 = the w0 form of 2 - t
//   VITX_POS_BICUBIC_AA  support = scale >= 1 ? 2 scale : 2;  inv = scale >= 1 ? 1 / scale : 1;  center = scale * ((float)o + 0.5f);  a = -0.5f
//                        first = max((int)(center - support + 0.5f), 0);  n = min((int)(center + support + 0.5f), in) - first   (truncating casts)
//                        f_j = k(((float)(first + j) - center + 0.5f) * inv),  k(x): |x| < 1: ((a+2)|x| - (a+3))|x||x| + 1;  |x| < 2: (((|x|-5)|x| + 8)|x| - 4) a;  else 0
//                        total = ((f_0 + f_1) + f_2) + ...;  w_j = f_j / total   (taps outside the grid are never formed: the rest is normalised)
// Per output cell and channel, with v(iy, ix) the source value (horizontal first, then vertical, every sum left to right):
//   h_i = ((v(iy_i, ix_0) wx_0 + v(iy_i, ix_1) wx_1) + v(iy_i, ix_2) wx_2) + ...        out = ((h_0 wy_0 + h_1 wy_1) + h_2 wy_2) + ...
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#ifndef VITX_HD
#define VITX_HD __host__ __device__ inline
#endif

namespace vitx {

enum { POS_BICUBIC = 0, POS_BICUBIC_AA = 1 };

struct PosAxis {
    int first, n;          // first tap index (BICUBIC: before clamping, may be -1) and tap count
    float t;               // BICUBIC: the fraction
    float center, inv, total;   // BICUBIC_AA
};

VITX_HD float pos_scale(int in, int out) { return (float)in / (float)out; }

VITX_HD float pos_aa_filter(float x) {
    const float a = -0.5f;
    x = fabsf(x);
    if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
    if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * a;
    return 0.0f;
}
VITX_HD float pos_aa_raw(const PosAxis &ax, int j) { return pos_aa_filter(((float)(ax.first + j) - ax.center + 0.5f) * ax.inv); }

VITX_HD PosAxis pos_axis(int interp, int in, int out, float scale, int o) {
    PosAxis ax;
    ax.t = 0.0f; ax.center = 0.0f; ax.inv = 1.0f; ax.total = 1.0f;
    if (interp == POS_BICUBIC) {
        const float x = scale * ((float)o + 0.5f) - 0.5f, fl = floorf(x);
        ax.first = (int)fl - 1; ax.n = 4; ax.t = x - fl;
        return ax;
    }
    const float support = scale >= 1.0f ? 2.0f * scale : 2.0f;
    ax.inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
    ax.center = scale * ((float)o + 0.5f);
    int lo = (int)(ax.center - support + 0.5f), hi = (int)(ax.center + support + 0.5f);
    if (lo < 0) lo = 0;
    if (hi > in) hi = in;
    ax.first = lo; ax.n = hi - lo;
    float total = 0.0f;
    for (int j = 0; j < ax.n; ++j) { const float f = pos_aa_raw(ax, j); total = j == 0 ? f : total + f; }
    ax.total = total;
    return ax;
}

VITX_HD int pos_axis_index(const PosAxis &ax, int in, int j) {
    const int i = ax.first + j;
    return i < 0 ? 0 : (i > in - 1 ? in - 1 : i);
}

VITX_HD float pos_axis_weight(int interp, const PosAxis &ax, int j) {
    if (interp == POS_BICUBIC) {
        const float A = -0.75f;
        const float x = j == 0 ? ax.t + 1.0f : j == 1 ? ax.t : j == 2 ? 1.0f - ax.t : 2.0f - ax.t;
        if (j == 1 || j == 2) return ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
        return ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
    }
    const float f = pos_aa_raw(ax, j);
    return ax.total != 0.0f ? f / ax.total : f;
}

typedef float pos_f32x4 __attribute__((ext_vector_type(4)));

// V consecutive channels d .. d + V - 1 of one output cell; grid = the source grid [gy_in * gx_in][D] (the table without its class row).
// V == 4 reads 16-byte vectors: grid and D * 4 bytes must be 16-byte aligned.
template <int V> VITX_HD void pos_cell(const float *grid, int gy_in, int gx_in, int D, int interp, const PosAxis &ay, const PosAxis &ax, int d, float (&out)[V]) {
    float acc[V];
    for (int e = 0; e < V; ++e) acc[e] = 0.0f;
    for (int i = 0; i < ay.n; ++i) {
        const float wy = pos_axis_weight(interp, ay, i);
        const float *row = grid + (size_t)pos_axis_index(ay, gy_in, i) * gx_in * D + d;
        float h[V];
        for (int e = 0; e < V; ++e) h[e] = 0.0f;
        for (int j = 0; j < ax.n; ++j) {
            const float wx = pos_axis_weight(interp, ax, j);
            const float *p = row + (size_t)pos_axis_index(ax, gx_in, j) * D;
            float v[V];
            if constexpr (V == 4) { const pos_f32x4 q = *(const pos_f32x4 *)p; v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3]; }
            else { for (int e = 0; e < V; ++e) v[e] = p[e]; }
            for (int e = 0; e < V; ++e) { const float pr = v[e] * wx; h[e] = j == 0 ? pr : h[e] + pr; }
        }
        for (int e = 0; e < V; ++e) { const float pr = h[e] * wy; acc[e] = i == 0 ? pr : acc[e] + pr; }
    }
    for (int e = 0; e < V; ++e) out[e] = acc[e];
}

// argument rule shared by the host and the device entry points; 0 = fine
inline bool pos_resample_args_ok(const void *pos, int gy_in, int gx_in, int D, int gy_out, int gx_out, int interp, const void *out) {
    if (!pos || !out || gy_in <= 0 || gx_in <= 0 || D <= 0 || gy_out <= 0 || gx_out <= 0) return false;
    if (interp != POS_BICUBIC && interp != POS_BICUBIC_AA) return false;
    // element offsets stay below 2^31 (the kernel's thread index is 32-bit)
    const long long lim = 0x7fffffffLL;
    return (1LL + (long long)gy_in * gx_in) * D <= lim && (1LL + (long long)gy_out * gx_out) * D <= lim;
}

}  // namespace vitx
