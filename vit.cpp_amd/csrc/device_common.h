// device_common.h -- types and helpers shared by the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace vitx {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define GPTR(p) ((const __attribute__((address_space(1))) void *)(p))
#define LPTR(p) ((__attribute__((address_space(3))) void *)(p))

template <typename T> struct Elem;
template <> struct Elem<_Float16> {
    typedef half8 v8; typedef half4 v4;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 mfma16(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    typedef short bits4 __attribute__((ext_vector_type(4)));      // half the k-slots of mfma16: lane group g holds k = 4 g .. 4 g + 3
    static __device__ __forceinline__ f32x4 mfma16k16(bits4 a, bits4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(v4, a), __builtin_bit_cast(v4, b), c, 0, 0, 0); }
};
template <> struct Elem<__bf16> {
    typedef bf16x8 v8; typedef bf16x4 v4;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 mfma16(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    typedef short bits4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ f32x4 mfma16k16(bits4 a, bits4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0); }
};
template <typename T> __device__ __forceinline__ float rnd(float x) { return (float)(T)x; }   // round-trip through the operand type

// Packed pair helpers for the softmax inner loop (gfx950: v_cvt_pk_{f16,bf16}_f32, v_fma_mix_f32, v_dot2c_f32_{f16,bf16}).
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <typename T> struct Pair;
template <> struct Pair<_Float16> {
    typedef _Float16 v2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ float sum2(v2 p, float acc) { return __builtin_amdgcn_fdot2(p, v2{(_Float16)1.0f, (_Float16)1.0f}, acc, false); }
};
template <> struct Pair<__bf16> {
    typedef __bf16 v2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ float sum2(v2 p, float acc) { return __builtin_amdgcn_fdot2_f32_bf16(p, v2{(__bf16)1.0f, (__bf16)1.0f}, acc, false); }
};
// (T)a, (T)b rounded to nearest even in one instruction
template <typename T> __device__ __forceinline__ typename Pair<T>::v2 round_pair(float a, float b) { return __builtin_convertvector((f32x2{a, b}), typename Pair<T>::v2); }

// tanh-GELU of the reference (ggml_gelu_f32): 0.5*x*(1+tanh(sqrt(2/pi)*x*(1+0.044715*x*x))),
// evaluated as x*sigmoid(2u) = x / (1 + exp(-2u)), algebraically identical and stable in both tails.
// With u = c*x*(1 + a*x^2): exp(-2u) = exp2(x * (B + A*x^2)), B = -2*c*log2(e), A = B*a -- 3 multiplies, 1 fma, 1 add,
// v_exp_f32 and v_rcp_f32 per element (the straightforward form needs 7 multiplies; the GELU epilogue is VALU-bound).
// Saturates correctly: x -> -inf gives exp2(+inf) = inf, rcp = 0, result -0; x -> +inf gives exp2(-inf) = 0, result x.
__device__ __forceinline__ float gelu_tanh(float x) {
    constexpr float B = -2.0f * 0.79788456080286535588f * 1.44269504088896340736f;
    constexpr float A = B * 0.044715f;
    const float p = __builtin_fmaf(x * x, A, B);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * p));
}

// two elements at a time: the multiplies / fma / add become v_pk_*_f32 (exp and rcp stay scalar, quarter rate)
__device__ __forceinline__ f32x2 gelu_tanh2(f32x2 x) {
    constexpr float B = -2.0f * 0.79788456080286535588f * 1.44269504088896340736f;
    constexpr float A = B * 0.044715f;
    const f32x2 p = __builtin_elementwise_fma(x * x, f32x2{A, A}, f32x2{B, B});
    const f32x2 t = x * p;
    const f32x2 d = f32x2{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])} + f32x2{1.0f, 1.0f};
    return x * f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
}

// QuickGELU (CLIP; ggml_gelu_quick): x * sigmoid(1.702 x) = x / (1 + exp2(-1.702 log2(e) x)) -- the shape of gelu_tanh2 without the cubic term:
// 2 packed multiplies, 1 packed add, v_exp_f32 and v_rcp_f32 per element.
__device__ __forceinline__ f32x2 quick_gelu2(f32x2 x) {
    constexpr float B = -1.702f * 1.44269504088896340736f;
    const f32x2 t = x * f32x2{B, B};
    const f32x2 d = f32x2{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])} + f32x2{1.0f, 1.0f};
    return x * f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
}

// erf-GELU (nn.GELU, HuggingFace "gelu"): x * Phi(x).  With z = |x| / sqrt(2) and q = erfc(z) / 2 in (0, 1/2]:
//   Phi(x) = q for x < 0, 1 - q for x >= 0   =>   x Phi(x) = max(x, 0) - |x| q
// so the negative tail is the product |x| q itself (full relative accuracy of q: nothing like 1 + erf cancels) and the positive side subtracts a
// term that is at most x / 2.  q = (poly(t) * t) * exp(-z^2), t = 1 / (1 + p z): Abramowitz & Stegun 7.1.26, |error of erfc| <= 1.5e-7, with
// the 1/2 folded into the coefficients and 1 / sqrt(2) into p and the exponent: exp(-z^2) = exp2(-log2(e) / 2 * x^2).
// Per element: one v_min (|x| as a source modifier, clamped at 16 where exp2 has long flushed to 0 -- keeps inf * 0 out), one v_max, v_rcp_f32,
// v_exp_f32; per pair: 6 v_pk_fma_f32 and 3 v_pk_mul_f32.  No branch, no range split (the device library's erff is a multi-range polynomial).
__device__ __forceinline__ f32x2 gelu_erf2(f32x2 x) {
    constexpr float P = 0.3275911f * 0.70710678118654752440f;
    constexpr float E = -0.5f * 1.44269504088896340736f;
    constexpr float A1 = 0.5f * 0.254829592f, A2 = 0.5f * -0.284496736f, A3 = 0.5f * 1.421413741f, A4 = 0.5f * -1.453152027f, A5 = 0.5f * 1.061405429f;
    const f32x2 ax = f32x2{__builtin_fminf(__builtin_fabsf(x[0]), 16.0f), __builtin_fminf(__builtin_fabsf(x[1]), 16.0f)};
    const f32x2 d = __builtin_elementwise_fma(ax, f32x2{P, P}, f32x2{1.0f, 1.0f});
    const f32x2 t = f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    const f32x2 s = (ax * ax) * f32x2{E, E};
    const f32x2 e = f32x2{__builtin_amdgcn_exp2f(s[0]), __builtin_amdgcn_exp2f(s[1])};
    f32x2 p = __builtin_elementwise_fma(t, f32x2{A5, A5}, f32x2{A4, A4});
    p = __builtin_elementwise_fma(p, t, f32x2{A3, A3});
    p = __builtin_elementwise_fma(p, t, f32x2{A2, A2});
    p = __builtin_elementwise_fma(p, t, f32x2{A1, A1});
    const f32x2 q = (p * t) * e;
    return __builtin_elementwise_fma(-ax, q, f32x2{__builtin_fmaxf(x[0], 0.0f), __builtin_fmaxf(x[1], 0.0f)});
}

// The MLP activation by its id (enum vitx_activation: 0 tanh-GELU, 1 erf-GELU, 2 QuickGELU), a compile-time choice: no run-time branch in an epilogue
template <int ACT> __device__ __forceinline__ f32x2 act2(f32x2 x) {
    static_assert(ACT >= 0 && ACT <= 2, "enum vitx_activation");
    if constexpr (ACT == 1) return gelu_erf2(x);
    else if constexpr (ACT == 2) return quick_gelu2(x);
    else return gelu_tanh2(x);
}

// fc1 epilogue activation of two adjacent outputs (ggml_gelu through the fp16 table, /root/reference/vit.cpp:893).
//   F16 (parity mode): the table's semantics -- argument rounded to fp16, result rounded to fp16 (ggml_gelu_quick goes through the same kind of table).
//   BF16 (the dtype BASELINE names): there is no bf16 rounding point in the reference to reproduce, so the argument stays f32 and only
//   the stored value is rounded (it is the next GEMM's operand): one convert and two unpacks per pair less, same tolerance band.
// ACT: the activation (act2); the rounding points are the same for all three.
template <typename T, int ACT = 0> struct GeluOut;
template <int ACT> struct GeluOut<_Float16, ACT> {
    static __device__ __forceinline__ Pair<_Float16>::v2 pair(float v0, float v1) {
        const Pair<_Float16>::v2 p = round_pair<_Float16>(v0, v1);
        const f32x2 y = act2<ACT>(f32x2{(float)p[0], (float)p[1]});
        return round_pair<_Float16>(y[0], y[1]);
    }
};
template <int ACT> struct GeluOut<__bf16, ACT> {
    static __device__ __forceinline__ Pair<__bf16>::v2 pair(float v0, float v1) {
        const f32x2 y = act2<ACT>(f32x2{v0, v1});
        return round_pair<__bf16>(y[0], y[1]);
    }
};
template <typename T, int ACT = 0> __device__ __forceinline__ typename Pair<T>::v2 gelu_out_pair(float v0, float v1) { return GeluOut<T, ACT>::pair(v0, v1); }

// Softmax numerators of the attention kernels for two adjacent keys (ggml_soft_max, /root/reference/vit.cpp:856).
//   F16 (parity mode): e = round(exp(round(s/8 - max/8))) -- the fp16 exp table's semantics; nmx = -max * kScale, kScale = 1/8 (exact).
//   BF16: e = round_bf16(exp2(s * log2(e)/8 - max * log2(e)/8)): one fma and one v_exp_f32 per key, no rounded exponent.
template <typename T> struct AttnExp;
template <> struct AttnExp<_Float16> {
    static constexpr float kScale = 0.125f;
    static __device__ __forceinline__ Pair<_Float16>::v2 pair(float s0, float s1, float nmx) {
        const f32x2 d = __builtin_elementwise_fma(f32x2{s0, s1}, f32x2{0.125f, 0.125f}, f32x2{nmx, nmx});       // one v_pk_fma_f32: same bits as two fmaf
        const Pair<_Float16>::v2 dh = round_pair<_Float16>(d[0], d[1]);
        const f32x2 t = f32x2{(float)dh[0], (float)dh[1]} * f32x2{1.44269504f, 1.44269504f};
        return round_pair<_Float16>(__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1]));
    }
};
template <> struct AttnExp<__bf16> {
    static constexpr float kScale = 0.125f * 1.44269504088896340736f;
    static __device__ __forceinline__ Pair<__bf16>::v2 pair(float s0, float s1, float nmx) {
        const f32x2 d = __builtin_elementwise_fma(f32x2{s0, s1}, f32x2{kScale, kScale}, f32x2{nmx, nmx});        // one v_pk_fma_f32: same bits as two fmaf
        return round_pair<__bf16>(__builtin_amdgcn_exp2f(d[0]), __builtin_amdgcn_exp2f(d[1]));
    }
};

// The same with a run-time score scale 1 / sqrt(head_dim) (attention_generic_kernel: head dims other than 64; ggml_scale_inplace,
// /root/reference/vit.cpp:853).  k(scale) is what multiplies the raw score AND the row maximum (nmx = -max * k).
template <typename T> struct AttnExpRt;
template <> struct AttnExpRt<_Float16> {
    static __device__ __forceinline__ float k(float scale) { return scale; }
    static __device__ __forceinline__ Pair<_Float16>::v2 pair(float s0, float s1, float nmx, float kk) {
        const f32x2 d = __builtin_elementwise_fma(f32x2{s0, s1}, f32x2{kk, kk}, f32x2{nmx, nmx});
        const Pair<_Float16>::v2 dh = round_pair<_Float16>(d[0], d[1]);
        const f32x2 t = f32x2{(float)dh[0], (float)dh[1]} * f32x2{1.44269504f, 1.44269504f};
        return round_pair<_Float16>(__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1]));
    }
};
template <> struct AttnExpRt<__bf16> {
    static __device__ __forceinline__ float k(float scale) { return scale * 1.44269504088896340736f; }
    static __device__ __forceinline__ Pair<__bf16>::v2 pair(float s0, float s1, float nmx, float kk) {
        const f32x2 d = __builtin_elementwise_fma(f32x2{s0, s1}, f32x2{kk, kk}, f32x2{nmx, nmx});
        return round_pair<__bf16>(__builtin_amdgcn_exp2f(d[0]), __builtin_amdgcn_exp2f(d[1]));
    }
};

// Reductions over the four 16-lane rows of a wave (lanes l, l ^ 16, l ^ 32, l ^ 48) without the LDS crossbar: v_permlane16_swap /
// v_permlane32_swap (gfx950) exchange rows in the VALU -- no ds_bpermute, no lgkmcnt wait in the middle of a dependent chain.
// swap16(x, x) leaves {row 0, row 0, row 2, row 2} and {row 1, row 1, row 3, row 3}; swap32 of the result {lower half, lower half} and
// {upper half, upper half}: after both steps every lane holds the combination of all four rows.
// (elements are copied out before the bit cast: __builtin_bit_cast applied to a[1] of the returned vector reads element 0 -- hipcc 7.2)
__device__ __forceinline__ void rows_swap16(float x, float &u, float &v) {
    const auto a = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, x), false, false);
    const unsigned a0 = a[0], a1 = a[1];
    u = __builtin_bit_cast(float, a0); v = __builtin_bit_cast(float, a1);
}
__device__ __forceinline__ void rows_swap32(float x, float &u, float &v) {
    const auto a = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, x), false, false);
    const unsigned a0 = a[0], a1 = a[1];
    u = __builtin_bit_cast(float, a0); v = __builtin_bit_cast(float, a1);
}
__device__ __forceinline__ float rows4_max(float x) {
    float u, v;
    rows_swap16(x, u, v); x = fmaxf(u, v);
    rows_swap32(x, u, v); return fmaxf(u, v);
}
__device__ __forceinline__ float rows4_sum(float x) {       // (row 0 + row 1) + (row 2 + row 3) in every lane: the same bits everywhere
    float u, v;
    rows_swap16(x, u, v); x = u + v;
    rows_swap32(x, u, v); return u + v;
}

// ------------------------------------------------------------------------------------------------
// LDS tile image shared by the GEMM and attention kernels: rows of 64 elements (128 B = 8 slots of
// 16 B).  Two rows form one 256-B bank line; the 16 slots of a line are XOR-ed with (line & 15) so a
// ds_read_b128 lane group (16 rows, same logical slot) touches 16 distinct slots: conflict-free.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int swz_byte(int row, int slot /*0..7*/) {
    const int line = row >> 1;
    const int s16 = ((row & 1) << 3) | slot;
    return line * 256 + ((s16 ^ (line & 15)) << 4);
}
// inverse: physical 16-B slot index p (within the tile) -> logical (row, slot)
__device__ __forceinline__ void swz_inv(int p, int &row, int &slot) {
    const int line = p >> 4;
    const int s16 = (p & 15) ^ (line & 15);
    row = line * 2 + (s16 >> 3);
    slot = s16 & 7;
}


}  // namespace vitx
