// heads.cpp -- the launch sequences of the zero-shot bank, the gallery, the dense head and the depth head (heads.h): what a forward runs after
// its classifier (SliceForward, forward.cpp) and what vitx_op_zeroshot / _nn / _dense / _depth run on the caller's buffers (ops.cpp) -- one text.
// Behind them the set path of the patch heads: the argument checks and the upload that an image context and a packed context share.
#include <cmath>

#include "context.h"
#include "depth_bins.h"

namespace vitx {

namespace {

constexpr double eb = 2.0;                               // operand bytes

// the first HIP error of a sequence ends it
#define HEAD_TRY(expr) do { const hipError_t e__ = (expr); if (e__ != hipSuccess) return e__; } while (0)

// One dispatcher GEMM with an f32 output (+ its profile record)
hipError_t gemm_f32(const HeadLaunch &l, int pc, const GemmArgs &a) {
    double flops, bytes;
    gemm_work(EPI_BIAS_F32, a.M_real, a.N, a.K, false, false, &flops, &bytes);
    ProfScope ps(l.prof, l.st, pc, flops, bytes);
    return launch_gemm(l.tune, l.dtype, EPI_BIAS_F32, a, l.st);
}

}  // namespace

hipError_t head_zeroshot(const HeadLaunch &l, const float *z, long ldz, void *a, const void *bank, const float *zero, float *acc, float *probs, float *logits,
                         long out_stride, int n, int K, int E, int kind, float scale, float bias) {
    const int Kpad = round_up(K, gemm_tile_n()), Mz = round_up(n, gemm_tile_m());
    {
        ProfScope ps(l.prof, l.st, PC_ZEROSHOT, 0, (double)n * E * 4 + (double)Mz * E * eb);
        HEAD_TRY(launch_zs_embed(l.dtype, z, ldz, a, n, Mz, E, l.st));
    }
    HEAD_TRY(gemm_f32(l, PC_ZEROSHOT, dense_gemm(a, bank, zero, acc, Mz, n, K, Kpad, E, Kpad)));
    ProfScope ps(l.prof, l.st, PC_ZEROSHOT, 0, (double)n * K * 4 * (kind == VITX_ZS_SOFTMAX ? 7 : 3));
    return launch_zs_score(acc, Kpad, probs, logits, out_stride, n, K, kind, scale, bias, l.st);
}

hipError_t head_nearest(const HeadLaunch &l, const void *z, long ldz, bool z_is_operand, void *a, const void *gallery, const float *zero, float *acc, void *state,
                        long G, int E, int k, int chunk, const int *labels, int nlabels, float T, void *pairs, float *vote, int n) {
    const int Mz = round_up(n, gemm_tile_m());
    {
        ProfScope ps(l.prof, l.st, PC_NN, 0, (double)n * E * (z_is_operand ? eb : 4) + (double)Mz * E * eb);
        if (z_is_operand) HEAD_TRY(launch_zs_embed_operand(l.dtype, z, ldz, a, n, Mz, E, l.st));
        else HEAD_TRY(launch_zs_embed(l.dtype, (const float *)z, ldz, a, n, Mz, E, l.st));
    }
    for (long g0 = 0; g0 < G; g0 += chunk) {
        const int cols = (int)std::min<long>(chunk, G - g0);
        HEAD_TRY(gemm_f32(l, PC_NN, dense_gemm(a, (const char *)gallery + (size_t)g0 * E * 2, zero, acc, Mz, n, cols, round_up(cols, gemm_tile_n()), E, chunk)));
        ProfScope ps(l.prof, l.st, PC_NN, 0, (double)n * cols * 4);
        HEAD_TRY(launch_nn_select(acc, chunk, n, cols, g0, state, k, g0 == 0, l.st));
    }
    ProfScope ps(l.prof, l.st, PC_NN, 0, (double)n * kNnSegs * k * 8 + (double)n * (k * 8 + nlabels * 4));
    return launch_nn_finish(state, n, k, labels, nlabels, T, pairs, vote, l.st);
}

hipError_t head_linear(const HeadLaunch &l, int pc, void *a, const void *W, const float *bias, float *acc, int rows, int K, int Dc, float *keep) {
    const int Kpad = round_up(K, gemm_tile_n()), Mr = round_up(rows, gemm_tile_m());
    if (Mr > rows) HEAD_TRY(hipMemsetAsync((char *)a + (size_t)rows * Dc * 2, 0, (size_t)(Mr - rows) * Dc * 2, l.st));
    HEAD_TRY(gemm_f32(l, pc, dense_gemm(a, W, bias, acc, Mr, rows, K, Kpad, Dc, Kpad)));
    if (keep) HEAD_TRY(hipMemcpy2DAsync(keep, (size_t)K * 4, acc, (size_t)Kpad * 4, (size_t)K * 4, rows, hipMemcpyDeviceToDevice, l.st));
    return hipSuccess;
}

hipError_t head_dense(const HeadLaunch &l, void *a, const void *W, const float *bias, float *acc, int n, int gh, int gw, int K, int Dc, int oh, int ow,
                      uint8_t *labels, float *score, float *keep) {
    const int rows = n * gh * gw, Kpad = round_up(K, gemm_tile_n());
    const size_t px = (size_t)oh * ow;
    HEAD_TRY(head_linear(l, PC_DENSE, a, W, bias, acc, rows, K, Dc, keep));
    ProfScope ps(l.prof, l.st, PC_DENSE, 9.0 * n * (double)px * K, (double)rows * Kpad * 4 + (double)n * px * (score ? 5 : 1));
    return launch_dense_labels(acc, Kpad, n, gh, gw, K, oh, ow, labels, score, l.st);
}

hipError_t head_dense_packed(const HeadLaunch &l, void *a, const void *W, const float *bias, float *acc, int rows, int K, int Dc, const int *tile0, const int *seg,
                             int n, int tiles, int cells, long pixels, uint8_t *labels, float *score, float *keep) {
    const int Kpad = round_up(K, gemm_tile_n());
    HEAD_TRY(head_linear(l, PC_DENSE, a, W, bias, acc, rows, K, Dc, keep));
    ProfScope ps(l.prof, l.st, PC_DENSE, 9.0 * (double)pixels * K, (double)rows * Kpad * 4 + (double)pixels * (score ? 5 : 1));
    return launch_dense_labels_packed(acc, Kpad, tile0, seg, n, tiles, cells, K, labels, score, l.st);
}

hipError_t head_depth(const HeadLaunch &l, void *a, const void *Wp, const float *zero, float *acc, void *ac, const void *Wc, const float *bias, float *o,
                      const float *bins, int n, int gh, int gw, int K, int Dc, int u, int oh, int ow, float lo, float hi, float *fine, float *depth,
                      float *keep, float *keep_off) {
    const int rows = n * gh * gw, Kpad = round_up(K, gemm_tile_n());
    const size_t px = (size_t)oh * ow, fpx = (size_t)u * gh * u * gw;
    HEAD_TRY(head_linear(l, PC_DEPTH, a, Wp, zero, acc, rows, K, Dc, keep));
    if (Wc) HEAD_TRY(head_linear(l, PC_DEPTH, ac, Wc, bias, o, n, K, Dc, keep_off));
    {
        ProfScope ps(l.prof, l.st, PC_DEPTH, 11.0 * n * (double)fpx * K, (double)rows * Kpad * 4 + (double)n * fpx * 4);
        HEAD_TRY(launch_depth_fine(acc, Kpad, Wc ? o : bias, Wc ? Kpad : 0, bins, n, gh, gw, K, u, fine, l.st));
    }
    ProfScope ps(l.prof, l.st, PC_DEPTH, 7.0 * n * (double)px, (double)n * (fpx + px) * 4);
    return launch_depth_resize(fine, n, u * gh, u * gw, oh, ow, lo, hi, depth, l.st);
}

hipError_t head_depth_packed(const HeadLaunch &l, void *a, const void *Wp, const float *zero, float *acc, void *ac, const void *Wc, const float *bias, float *o,
                             const float *bins, int rows, int K, int Dc, const int *row0, const int *ftile0, const int *otile0, const int *seg, int n, int ftiles,
                             int otiles, int cells, long fine_px, long pixels, float lo, float hi, float *fine, float *depth, float *keep, float *keep_off) {
    const int Kpad = round_up(K, gemm_tile_n());
    HEAD_TRY(head_linear(l, PC_DEPTH, a, Wp, zero, acc, rows, K, Dc, keep));
    if (Wc) {
        {
            ProfScope ps(l.prof, l.st, PC_DEPTH, 0, 2.0 * n * Dc * eb);
            HEAD_TRY(launch_depth_gather(a, Dc, row0, ac, n, l.st));
        }
        HEAD_TRY(head_linear(l, PC_DEPTH, ac, Wc, bias, o, n, K, Dc, keep_off));
    }
    {
        ProfScope ps(l.prof, l.st, PC_DEPTH, 11.0 * (double)fine_px * K, (double)rows * Kpad * 4 + (double)fine_px * 4);
        HEAD_TRY(launch_depth_fine_packed(acc, Kpad, Wc ? o : bias, Wc ? Kpad : 0, bins, ftile0, seg, n, ftiles, cells, K, fine, l.st));
    }
    ProfScope ps(l.prof, l.st, PC_DEPTH, 7.0 * (double)pixels, (double)(fine_px + pixels) * 4);
    return launch_depth_resize_packed(fine, otile0, seg, n, otiles, lo, hi, depth, l.st);
}

int patch_head_mask(const char *api, int L, int D, int Dc, uint64_t *mask) {
    if (*mask == 0) *mask = 1ull << (L - 1);
    if (L < 64 && (*mask >> L)) { set_error("%s: layer mask selects a layer at or beyond L = %d", api, L); return VITX_ERR_ARG; }
    const int m = __builtin_popcountll(*mask);
    if (m > 4) { set_error("%s: %d layers selected, at most 4", api, m); return VITX_ERR_ARG; }
    if (Dc != m * D) { set_error("%s: the head's width %d is not %d layers x D = %d", api, Dc, m, m * D); return VITX_ERR_ARG; }
    return VITX_OK;
}

int dense_head_args(const char *api, const float *W, int K, int Dc, int flags, int L, int D, uint64_t *mask) {
    if (!W) { set_error("%s: NULL weights with K = %d", api, K); return VITX_ERR_ARG; }
    if (K < 1) { set_error("%s: K = %d classes", api, K); return VITX_ERR_ARG; }
    if (flags & ~(VITX_DENSE_SCORE | VITX_DENSE_LOGITS)) { set_error("%s: unknown flags 0x%x", api, flags); return VITX_ERR_ARG; }
    return patch_head_mask(api, L, D, Dc, mask);
}

int dense_head_values(const char *api, const float *W, const float *bias, int K, int Dc) {
    for (size_t i = 0, nb = (size_t)K * Dc; i < nb; ++i)
        if (!std::isfinite(W[i])) { set_error("%s: weight [%zu][%zu] is not finite", api, i / Dc, i % Dc); return VITX_ERR_ARG; }
    if (bias) for (int k = 0; k < K; ++k)
        if (!std::isfinite(bias[k])) { set_error("%s: bias [%d] is not finite", api, k); return VITX_ERR_ARG; }
    if (K > kDenseMaxK) { set_error("%s: K = %d classes above %d (labels are bytes)", api, K, kDenseMaxK); return VITX_ERR_UNSUPPORTED; }
    return VITX_OK;
}

int depth_head_args(const char *api, const float *Wp, const float *bins, int K, int Dc, int flags, int L, int D, uint64_t *mask) {
    if (!Wp || !bins) { set_error("%s: NULL weights or bins with K = %d", api, K); return VITX_ERR_ARG; }
    if (K < 1) { set_error("%s: K = %d bins", api, K); return VITX_ERR_ARG; }
    if (flags & ~(VITX_DEPTH_NORM | VITX_DEPTH_LOGITS | VITX_DEPTH_FINE)) { set_error("%s: unknown flags 0x%x", api, flags); return VITX_ERR_ARG; }
    return patch_head_mask(api, L, D, Dc, mask);
}

int depth_head_values(const char *api, const float *Wp, const float *Wc, const float *bias, const float *bins, int K, int Dc, float min_depth, float max_depth, int upsample) {
    if (!std::isfinite(min_depth) || !std::isfinite(max_depth) || min_depth > max_depth) { set_error("%s: the depth range %g .. %g must be finite and ordered", api, (double)min_depth, (double)max_depth); return VITX_ERR_ARG; }
    for (const float *W : {Wp, Wc})
        if (W) for (size_t i = 0, nb = (size_t)K * Dc; i < nb; ++i)
            if (!std::isfinite(W[i])) { set_error("%s: %s weight [%zu][%zu] is not finite", api, W == Wp ? "patch" : "class", i / Dc, i % Dc); return VITX_ERR_ARG; }
    for (int k = 0; k < K; ++k) {
        if (bias && !std::isfinite(bias[k])) { set_error("%s: bias [%d] is not finite", api, k); return VITX_ERR_ARG; }
        if (!std::isfinite(bins[k]) || !(bins[k] > 0.0f)) { set_error("%s: bin [%d] = %g is not a finite positive depth", api, k, (double)bins[k]); return VITX_ERR_ARG; }
    }
    if (K > kDepthMaxK) { set_error("%s: K = %d bins above %d", api, K, kDepthMaxK); return VITX_ERR_UNSUPPORTED; }
    if (upsample != 1 && upsample != 2 && upsample != 4) { set_error("%s: upsample = %d, not 1, 2 or 4", api, upsample); return VITX_ERR_UNSUPPORTED; }
    return VITX_OK;
}

hipError_t upload_operand(int dtype, const DevMem &dst, const float *W, int K, int Kpad, int Dc) {
    const std::vector<uint16_t> hw = operand_matrix_host(dtype, W, nullptr, K, Dc, Kpad, Dc, 0, 0);
    return hipMemcpy(dst.p, hw.data(), hw.size() * 2, hipMemcpyHostToDevice);
}

hipError_t dense_head_upload(const DenseHead &dn, int dtype, const float *W, const float *bias) {
    HEAD_TRY(upload_operand(dtype, dn.W, W, dn.K, dn.Kpad, dn.Dc));
    HEAD_TRY(hipMemset(dn.bias.p, 0, (size_t)dn.Kpad * 4));
    if (bias) HEAD_TRY(hipMemcpy(dn.bias.p, bias, (size_t)dn.K * 4, hipMemcpyHostToDevice));
    return hipSuccess;
}

// the halves go up rounded (RNE) to the operand type; the zero rows beyond K come from operand_matrix_host, the zero biases from the memset
hipError_t depth_head_upload(const DepthHead &dp, int dtype, const float *Wp, const float *Wc, const float *bias, const float *bins) {
    HEAD_TRY(upload_operand(dtype, dp.Wp, Wp, dp.K, dp.Kpad, dp.Dc));
    if (Wc) HEAD_TRY(upload_operand(dtype, dp.Wc, Wc, dp.K, dp.Kpad, dp.Dc));
    for (const DevMem *m : {&dp.bias, &dp.zero, &dp.bins}) HEAD_TRY(hipMemset(m->p, 0, (size_t)dp.Kpad * 4));
    if (bias) HEAD_TRY(hipMemcpy(dp.bias.p, bias, (size_t)dp.K * 4, hipMemcpyHostToDevice));
    return hipMemcpy(dp.bins.p, bins, (size_t)dp.K * 4, hipMemcpyHostToDevice);
}

}  // namespace vitx
