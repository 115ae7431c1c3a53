// depth_bins.h -- the bins-to-depth arithmetic of the depth head (include/vitx.h "depth estimation"), ONE definition for the host function
// (vitx_depth_host, depth_host.cpp) and the device kernels (depth_map.hip).  Both are compiled with -ffp-contract=off and use only f32 add,
// multiply, compare and IEEE divide, so they produce the same bits.  The resampling around it is dense_resample.h's, unchanged.
//
// One fine cell, from the resampled logit v_k of every bin, k ascending from 0 (S = Tm = 0 before the first):
//   r = v_k < 0 ? 0 : v_k  (a NaN stays a NaN);  p = r + 0.1f;  S = S + p;  q = p * bins[k];  Tm = Tm + q
//   fine = Tm / S
// -- mmseg's norm_strategy = "linear" (relu, + 0.1, division by the sum, expectation over the bin centres) with the division moved behind the sums.
// One output pixel, from the resampled fine value d:  d < lo ? lo : (d > hi ? hi : d).
// A NaN is written as the quiet NaN 0x7fc00000, in the fine plane and in the depth map: the payload and sign of a computed NaN are the
// processor's choice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef VITX_HD
#define VITX_HD __host__ __device__ inline
#endif

namespace vitx {

struct DepthAcc {
    float S, Tm;           // the sum of the bins' masses so far, and of mass x centre
};
VITX_HD DepthAcc depth_acc_init() { DepthAcc a; a.S = 0.0f; a.Tm = 0.0f; return a; }
VITX_HD void depth_step(DepthAcc &a, float v, float bin) {
    const float r = v < 0.0f ? 0.0f : v;
    const float p = r + 0.1f;
    a.S = a.S + p;
    const float q = p * bin;
    a.Tm = a.Tm + q;
}
VITX_HD float depth_quiet(float d) { return d != d ? __builtin_bit_cast(float, 0x7fc00000u) : d; }
VITX_HD float depth_quotient(const DepthAcc &a) { return depth_quiet(a.Tm / a.S); }
VITX_HD float depth_clamp(float d, float lo, float hi) { return depth_quiet(d < lo ? lo : (d > hi ? hi : d)); }

// The launch geometry of depth_map.hip: a workgroup owns kDepthTile x kDepthTile fine cells (one per lane), or kDepthOutW x kDepthOutH output pixels
// (4 of a row per lane)
constexpr int kDepthTile = 16, kDepthOutW = 64, kDepthOutH = 16;
constexpr int kDepthMaxK = 256, kDepthMaxOut = 8192;

}  // namespace vitx
