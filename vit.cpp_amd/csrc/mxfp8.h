// mxfp8.h -- the MXFP8 block encoding of include/vitx.h (VITX_MXFP8), one definition for the host encoder (mxfp8.cpp) and
// every device producer (the LayerNorm -> MX kernel, the fc1 GELU -> MX epilogue and the test launch in gemm_mx8.hip).
//   block = 32 consecutive K elements of one row; elements OCP e4m3fn; one E8M0 scale byte s; value = q * 2^(s - 127)
//   a = max |x_i| = m * 2^E (m in [1, 2), exact from the bits, f32 subnormals included); e = E - 8 if m <= 1.75 else E - 7
//   (the smallest e with a * 2^-e <= 448, so nothing saturates); e >= -127; s = e + 127; q_i = RNE_e4m3(x_i * 2^-e); a == 0: s = 127, q = 0
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#define VITX_HD __host__ __device__ inline

namespace vitx {

constexpr int kMxBlock = 32;       // elements per scale
constexpr int kMxKStep = 128;      // K of one v_mfma_scale_f32_16x16x128_f8f6f4: rows are padded to a multiple of it
VITX_HD int mx_k_pad(int K) { return (K + kMxKStep - 1) / kMxKStep * kMxKStep; }

VITX_HD uint32_t mx_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
VITX_HD float mx_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// block exponent e of a block whose largest magnitude is `amax` (>= 0, finite); the scale byte is e + 127
VITX_HD int mx_block_exp(float amax) {
    const uint32_t u = mx_bits(amax) & 0x7fffffffu;
    if (u == 0) return 0;
    uint32_t ef = u >> 23, man = u & 0x7fffffu;
    int E;
    if (ef) E = (int)ef - 127;
    else {                          // subnormal: normalise the mantissa so that its leading one sits at bit 23
        int sh = 0;
        while (!(man & 0x800000u)) { man <<= 1; ++sh; }
        man &= 0x7fffffu;
        E = -126 - sh;
    }
    int e = man <= 0x600000u ? E - 8 : E - 7;       // m <= 1.75 <=> the 23-bit fraction <= 0.75 * 2^23
    return e < -127 ? -127 : e;
}

// e4m3fn code of y, round to nearest even; |y| <= 448 (what the block exponent guarantees)
VITX_HD uint8_t mx_e4m3_rne(float y) {
    const uint32_t u = mx_bits(y), sign = (u >> 24) & 0x80u, a = u & 0x7fffffffu;
    uint32_t code;
    if (a < 0x3c800000u) {          // below 2^-6, the smallest normal: multiples of 2^-9 (the product is exact, rintf rounds to even)
        code = (uint32_t)__builtin_rintf(mx_float(a) * 512.0f);        // 0 .. 8 (8 = the smallest normal, 0x08)
    } else {                        // keep 3 fraction bits, ties to even; a carry moves into the exponent by itself
        const uint32_t r = (a + 0x7ffffu + ((a >> 20) & 1u)) >> 20;
        code = r - (120u << 3);     // f32 exponent 127 + E  ->  e4m3 exponent 7 + E
    }
    return (uint8_t)(sign | code);
}

// x * 2^-e exactly (e in -127 .. 120: 2^-e is a normal f32)
VITX_HD float mx_scale_down(float x, int e) { return x * mx_float((uint32_t)(127 - e) << 23); }

}  // namespace vitx
