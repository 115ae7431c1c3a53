// attention.hip -- which attention family runs a shape (launch_attention), and the device bring-up of all of them (prepare_attention).
#include <algorithm>

#include "kernels.h"

namespace vitx {

bool attention_supports(int N, int D, int H) { return N > 0 && (D == H * 64 || attention_generic_supports(D, H)); }      // any token count; head_dim 64 (tuned kernels) or any multiple of 8 up to 128
// Kernel choice (measured, 128 x 12 heads bf16: 197 tokens 52 vs 55 us, 257 tokens 77 vs 92 us single-pass vs pipelined;
// 64 x 16 heads x 577 tokens 282 vs 241 us -- profiles/r02_attention.txt):
//   193..224 tokens: the persistent single-pass kernel at EVERY batch size (its 16x16x32 products group the f32 sums differently from the
//   32x32x16 kernels: one kernel per token count keeps an image's result independent of the batch it arrives in); otherwise single-pass
//   (all scores in registers) up to 288 tokens where instantiated, the pipelined two-pass kernel for everything else.
// t.attn_kernel (vitx_op_attention_ex, tests): ATTN_SINGLE / ATTN_FLOW / ATTN_PERSIST force one family.
hipError_t launch_attention(const Tuning &t, int dtype, const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream) {
    if (!attention_supports(N, D, H) || n_img <= 0) return hipErrorInvalidValue;
    if (D != H * 64) return launch_attention_generic(dtype, qkv, out, n_img, N, D, H, stream);
    // 193..224 tokens: the persistent single-pass kernel (K/V of the next item by LDS-DMA under the current item's softmax)
    if ((t.attn_kernel == ATTN_PERSIST || t.attn_kernel == ATTN_AUTO) && N > 192 && N <= 224) {
        // 32-bit buffer offsets bound one launch (~4.4 k ViT-B images): a larger sub-batch is cut into several launches of the SAME kernel rather than
        // handed to another family (whose f32 sums are grouped differently: an image's result must not depend on the batch it arrives in -- r03 advisor)
        const size_t per_img = (size_t)N * 3 * D * 2;
        const int max_img = (int)std::min<size_t>((size_t)n_img, (0xf0000000u - 1) / per_img);
        if (max_img < 1) return hipErrorInvalidValue;
        for (int i0 = 0; i0 < n_img; i0 += max_img) {
            const int ni = std::min(max_img, n_img - i0);
            const char *q = (const char *)qkv + (size_t)i0 * per_img; char *o = (char *)out + (size_t)i0 * N * D * 2;
            const hipError_t e = launch_attention_persist(dtype, q, o, ni, N, D, H, t.attn_grid > 0 ? t.attn_grid : t.n_cu, stream, t.attn_flags);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    if (t.attn_kernel == ATTN_PERSIST) return hipErrorInvalidValue;
    if (t.attn_kernel == ATTN_STREAM) return launch_attention_stream(dtype, false, qkv, out, n_img, N, D, H, 0, stream);
    const bool single = attention_single_pass_supports(N) && (N <= 288 || t.attn_kernel == ATTN_SINGLE);
    if (t.attn_kernel == ATTN_FLOW || !single) return launch_attention_flow(dtype, qkv, out, n_img, N, D, H, stream, t.attn_flags);
    return launch_attention_single(dtype, qkv, out, n_img, N, D, H, stream);
}

// Device bring-up of the families whose kernels ask for more than 64 KiB of LDS (the generic and the class-token kernel do not)
hipError_t prepare_attention() {
    hipError_t e = prepare_attention_flow();
    if (e == hipSuccess) e = prepare_attention_stream();
    if (e == hipSuccess) e = prepare_attention_persist();
    if (e == hipSuccess) e = prepare_attention_single();
    return e;
}

}  // namespace vitx
