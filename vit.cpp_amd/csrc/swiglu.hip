// swiglu.hip -- the gate of a gated (SwiGLU) MLP (include/vitx.h "gated MLP"), between the two GEMMs of such an MLP: fc1 has written rows
// [rows][ld_in] of the operand type with the gate projection in columns 0 .. F-1 and the up projection in columns F .. 2F-1; this pass writes
//     out[r][j] = RNE( silu(g) * u ),   g = f32(in[r][j]), u = f32(in[r][F + j]),   silu(g) = g / (1 + exp(-g)),   j < F
// into rows [rows][ld_out], the A operand of fc2.  g and u are widened to f32, the sigmoid and both products are f32, and only the stored value is
// rounded -- in both operand types: the reference has no gated MLP, so the F16 parity mode has no fp16 table whose rounding points it would honour.
// silu is evaluated as g * rcp(1 + exp2(-log2(e) g)), the form of quick_gelu2 (device_common.h): g -> -inf gives exp2 = inf, rcp = 0, the result
// -0; g -> +inf gives exp2 = 0, the result g u.  Finite for every finite operand pair whose product g u is finite.
// A streaming pass in the manner of rope.hip: one thread owns 8 consecutive columns -- one 16-byte load of the gate piece, one of the up piece, one
// 16-byte store.  No LDS, no atomics; every element has exactly one writer, so a row's bits depend on nothing but that row.  Columns F .. ld_out of
// `out` and everything behind row `rows` are never touched.  Both tensors are written by one launch and read once by the next: loads and the
// store are non-temporal (gemm_pp.hip "Cache-policy bits": the MLP hidden tensor streams through the caches instead of evicting X and the weights).
#include "device_common.h"
#include "kernels.h"

namespace vitx {

namespace {

template <typename T>
__global__ __launch_bounds__(256) void swiglu_kernel(const T *__restrict__ in, long ld_in, T *__restrict__ out, long ld_out, long units, int F8) {
    typedef typename Elem<T>::v8 V;
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= units) return;
    long row; int c;                                                      // the row, the group of 8 columns within it
    if (units <= 0x7fffffffL) {                                           // (uniform) a 32-bit division wherever the launch allows it
        const unsigned g = (unsigned)gi, r = g / (unsigned)F8;
        row = r; c = (int)(g - r * (unsigned)F8);
    } else {
        row = gi / F8; c = (int)(gi - row * F8);
    }
    const T *pg = in + (size_t)row * ld_in + c * 8, *pu = pg + (size_t)F8 * 8;
    const V vg = __builtin_nontemporal_load((const V *)pg), vu = __builtin_nontemporal_load((const V *)pu);
    constexpr float B = -1.44269504088896340736f;
    V o;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const f32x2 g = f32x2{(float)vg[e], (float)vg[e + 1]}, u = f32x2{(float)vu[e], (float)vu[e + 1]};
        const f32x2 t = g * f32x2{B, B};
        const f32x2 d = f32x2{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])} + f32x2{1.0f, 1.0f};
        const f32x2 s = g * f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
        const typename Pair<T>::v2 p = round_pair<T>(s[0] * u[0], s[1] * u[1]);
        o[e] = p[0]; o[e + 1] = p[1];
    }
    __builtin_nontemporal_store(o, (V *)(out + (size_t)row * ld_out + c * 8));
}

template <typename T>
hipError_t launch_swiglu_t(const void *in, long ld_in, void *out, long ld_out, long units, int F8, hipStream_t stream) {
    hipLaunchKernelGGL((swiglu_kernel<T>), dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, (const T *)in, ld_in, (T *)out, ld_out, units, F8);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_swiglu(int dtype, const void *in, long ld_in, void *out, long ld_out, long rows, int F, hipStream_t stream) {
    if ((dtype != DT_F16 && dtype != DT_BF16) || !in || !out || rows <= 0 || F <= 0 || F % 8 || ld_in % 8 || ld_out % 8 || ld_in < 2L * F || ld_out < F ||
        (uintptr_t)in % 16 || (uintptr_t)out % 16) return hipErrorInvalidValue;
    const long units = rows * (F / 8);
    if (units > 0x7fffffffL * 256) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_swiglu_t, in, ld_in, out, ld_out, units, F / 8, stream);
}

}  // namespace vitx
