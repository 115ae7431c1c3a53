// depth_host.cpp -- the depth head's tail on host pointers (vitx_depth_host; include/vitx.h "depth estimation"): dense_resample.h's and
// depth_bins.h's arithmetic in plain loops, the bins of a fine cell walked upwards.  The same bits as depth_map.hip on any data; no device call.
// depth_fine_args / depth_resize_args: the checks the device entry points (ops.cpp) and this function share -- none needs a device.
#include <cmath>
#include <vector>

#include "dense_resample.h"
#include "depth_bins.h"
#include "heads.h"

namespace vitx {

int depth_fine_args(const char *name, const void *logits, long ld, const void *bins, int n, int gh, int gw, int K, int u, const void *fine) {
    if (!logits || !bins || !fine || n < 1 || gh < 1 || gw < 1 || K < 1) { set_error("%s: invalid argument", name); return VITX_ERR_ARG; }
    if (ld < ((K + 3) & ~3) || ld % 4) { set_error("%s: ld = %ld must be a multiple of 4 and at least K = %d rounded up to 4", name, ld, K); return VITX_ERR_ARG; }
    if (K > kDepthMaxK) { set_error("%s: K = %d bins above %d", name, K, kDepthMaxK); return VITX_ERR_UNSUPPORTED; }
    if (u != 1 && u != 2 && u != 4) { set_error("%s: upsample = %d, not 1, 2 or 4", name, u); return VITX_ERR_UNSUPPORTED; }
    if (n > 65535 || (size_t)n * gh * gw > 0x7fffffffu || (size_t)u * gh > (size_t)kDepthMaxOut || (size_t)u * gw > (size_t)kDepthMaxOut) {
        set_error("%s: %d images of %d x %d patches x %d in one launch", name, n, gh, gw, u);
        return VITX_ERR_UNSUPPORTED;
    }
    return VITX_OK;
}

int depth_resize_args(const char *name, const void *fine, int n, int fh, int fw, int out_h, int out_w, float lo, float hi, const void *out) {
    if (!fine || !out || n < 1 || fh < 1 || fw < 1 || out_h < 1 || out_w < 1) { set_error("%s: invalid argument", name); return VITX_ERR_ARG; }
    if (!std::isfinite(lo) || !std::isfinite(hi) || lo > hi) { set_error("%s: the depth range %g .. %g must be finite and ordered", name, (double)lo, (double)hi); return VITX_ERR_ARG; }
    if (out_h < fh || out_w < fw || out_h > kDepthMaxOut || out_w > kDepthMaxOut) { set_error("%s: output %d x %d outside the fine plane %d x %d .. %d (upsampling only)", name, out_h, out_w, fh, fw, kDepthMaxOut); return VITX_ERR_UNSUPPORTED; }
    if (n > 65535) { set_error("%s: %d images in one launch", name, n); return VITX_ERR_UNSUPPORTED; }
    return VITX_OK;
}

}  // namespace vitx
using namespace vitx;

extern "C" int vitx_depth_host(const float *logits, long ld, const float *offsets, const float *bins, int n, int gh, int gw, int K, int upsample, int out_h, int out_w,
                               float min_depth, float max_depth, float *depth, float *fine_out) {
    if (const int rc = depth_fine_args("vitx_depth_host", logits, ld, bins, n, gh, gw, K, upsample, depth)) return rc;
    const int fh = upsample * gh, fw = upsample * gw;
    if (const int rc = depth_resize_args("vitx_depth_host", logits, n, fh, fw, out_h, out_w, min_depth, max_depth, depth)) return rc;
    std::vector<float> plane((size_t)fh * fw), cell((size_t)gh * gw * K);
    const float sy = dense_scale(gh, fh), sx = dense_scale(gw, fw), ty = dense_scale(fh, out_h), tx = dense_scale(fw, out_w);
    std::vector<DenseAxis> axs(fw), bxs(out_w);
    for (int x = 0; x < fw; ++x) axs[x] = dense_axis(gw, sx, x);
    for (int x = 0; x < out_w; ++x) bxs[x] = dense_axis(fw, tx, x);
    for (int i = 0; i < n; ++i) {
        // the taps: one rounded add per logit
        for (int t = 0; t < gh * gw; ++t)
            for (int k = 0; k < K; ++k) {
                const float c = logits[((size_t)i * gh * gw + t) * ld + k];
                cell[(size_t)t * K + k] = offsets ? c + offsets[(size_t)i * ld + k] : c;
            }
        for (int y = 0; y < fh; ++y) {
            const DenseAxis ay = dense_axis(gh, sy, y);
            for (int x = 0; x < fw; ++x) {
                const DenseAxis &ax = axs[x];
                const float *a = &cell[((size_t)ay.i0 * gw + ax.i0) * K], *b = &cell[((size_t)ay.i0 * gw + ax.i1) * K];
                const float *c = &cell[((size_t)ay.i1 * gw + ax.i0) * K], *d = &cell[((size_t)ay.i1 * gw + ax.i1) * K];
                DepthAcc acc = depth_acc_init();
                for (int k = 0; k < K; ++k) depth_step(acc, dense_value(ax.h, ax.l, ay.h, ay.l, a[k], b[k], c[k], d[k]), bins[k]);
                plane[(size_t)y * fw + x] = depth_quotient(acc);
            }
        }
        if (fine_out) std::copy(plane.begin(), plane.end(), fine_out + (size_t)i * fh * fw);
        for (int y = 0; y < out_h; ++y) {
            const DenseAxis ay = dense_axis(fh, ty, y);
            const float *p0 = &plane[(size_t)ay.i0 * fw], *p1 = &plane[(size_t)ay.i1 * fw];
            for (int x = 0; x < out_w; ++x) {
                const DenseAxis &ax = bxs[x];
                depth[((size_t)i * out_h + y) * out_w + x] = depth_clamp(dense_value(ax.h, ax.l, ay.h, ay.l, p0[ax.i0], p0[ax.i1], p1[ax.i0], p1[ax.i1]), min_depth, max_depth);
            }
        }
    }
    return VITX_OK;
}
