// mxfp8.cpp -- host encoder of the MXFP8 operand type (include/vitx.h, VITX_MXFP8).  The engine encodes the qkv, fc1 and fc2
// weights with it once at upload; the tests compare every device producer with it bit for bit.
#include <math.h>

#include "../../include/vitx.h"
#include "model_file.h"
#include "mxfp8.h"

namespace vitx {

void mxfp8_encode_rows(const float *x, int rows, int K, int k_pad, uint8_t *q, uint8_t *scales) {
    const int nb = k_pad / kMxBlock;
    for (int r = 0; r < rows; ++r) {
        const float *xr = x + (size_t)r * K;
        uint8_t *qr = q + (size_t)r * k_pad, *sr = scales + (size_t)r * nb;
        for (int b = 0; b < nb; ++b) {
            const int k0 = b * kMxBlock, k1 = k0 + kMxBlock < K ? k0 + kMxBlock : K;
            float amax = 0.0f;
            for (int k = k0; k < k1; ++k) amax = fmaxf(amax, fabsf(xr[k]));
            const int e = mx_block_exp(amax);
            sr[b] = (uint8_t)(e + 127);
            for (int k = k0; k < k0 + kMxBlock; ++k) qr[k] = k < k1 ? mx_e4m3_rne(mx_scale_down(xr[k], e)) : 0;
        }
    }
}

}  // namespace vitx

extern "C" int vitx_mxfp8_quantize(const float *x, int rows, int K, int k_pad, uint8_t *q, uint8_t *scales) {
    if (!x || !q || !scales || rows <= 0 || K <= 0 || k_pad < K || k_pad % vitx::kMxBlock) { vitx::set_error("vitx_mxfp8_quantize: invalid argument"); return VITX_ERR_ARG; }
    vitx::mxfp8_encode_rows(x, rows, K, k_pad, q, scales);
    return VITX_OK;
}
