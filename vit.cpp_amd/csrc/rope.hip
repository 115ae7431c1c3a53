// rope.hip -- rotary position embeddings on q and k of the patch tokens (include/vitx.h "rotary position embeddings"), in place on the buffer the
// qkv GEMM has written: rows [n_img * N][3 D], columns q | k | v, the F16 parity mode's lo plane lo_off elements behind.
// For image i, token t >= prefix (patch p = t - prefix), s in {q, k}, head h, j < hd / 2, with a = element h hd + j, b = element h hd + hd / 2 + j,
// c = cos[p][j], sn = sin[p][j] (f32 tables [N - prefix][hd / 2], built on the host: vitx_model_rope_table):
//     a' = a c - b sn      b' = b c + a sn
// every product rounded to f32, then the sum (no fma: the library is built with -ffp-contract=off), the result rounded RNE to the operand type.
// Two planes: the operand is f32(hi) + f32(lo) / 2048 and the result is split again as EPI_BIAS_HILO splits (hi = RNE(v), lo = RNE((v - hi) 2048)).
// v columns, prefix rows and rows beyond n_img * N are never touched.
// A streaming pass: one thread owns VEC consecutive j of a head's first half and the matching VEC of its second half -- VEC = 8: 16-byte loads and
// stores of the operands, the table rows as f32x4 (the table is a few hundred KB at most and stays in cache); VEC = 1: head dims whose half is no
// multiple of 8.  No LDS, no atomics; every element has exactly one writer, so an image's bits depend on nothing but its own rows.
// PACKED (launch_rope_packed; include/vitx.h "packed batches"): the same kernel text on a pack of images of different grids laid end to end,
// image i = rows row0[i] .. row0[i + 1] - 1 with `prefix` rows in front of its patches; its table starts toff[i] floats into cs and sn (one arena
// each).  Patch row q of the pack belongs to the last image with row0[i] - row0[0] - i prefix <= q: a binary search per thread.
#include "device_common.h"
#include "kernels.h"

namespace vitx {

namespace {

template <typename T, int VEC> struct RopeVec { T e[VEC]; };

template <typename T, int VEC, bool PLANES, bool PACKED>
__global__ __launch_bounds__(256) void rope_kernel(T *__restrict__ qkv, long lo_off, const float *__restrict__ cs, const float *__restrict__ sn, long units, int N, int prefix,
                                                   int D, int hd, const int *__restrict__ row0, const int *__restrict__ toff, int n) {
    typedef RopeVec<T, VEC> __attribute__((aligned(VEC * 2))) V;
    const int half = hd >> 1, uph = half / VEC, ups = (D >> 1) / VEC;      // units per head half, per q (or k) of a row
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= units) return;
    const int P = N - prefix;
    long pr, img;                                                         // patch row over all images, its image
    int w, p;                                                             // unit within the row, patch within the image
    long row, tab = 0;                                                    // the token row in qkv; the image's table offset
    if constexpr (PACKED) {
        pr = gi / (2 * ups); w = (int)(gi - pr * (2 * ups));
        const long first = row0[0];                                       // patch rows in front of image i: row0[i] - first - i prefix
        int lo = 0, hi = n;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((long)row0[mid] - first - (long)mid * prefix <= pr) lo = mid; else hi = mid;
        }
        img = lo; p = (int)(pr - ((long)row0[lo] - first - (long)lo * prefix));
        row = (long)row0[lo] + prefix + p; tab = toff[lo];
    } else if (units <= 0x7fffffffL) {                                           // (uniform) 32-bit divisions wherever the launch allows them
        const unsigned g = (unsigned)gi, q = g / (unsigned)(2 * ups), i = q / (unsigned)P;
        pr = q; w = (int)(g - q * (unsigned)(2 * ups)); img = i; p = (int)(q - i * (unsigned)P);
    } else {
        pr = gi / (2 * ups); w = (int)(gi - pr * (2 * ups)); img = pr / P; p = (int)(pr - img * P);
    }
    if constexpr (!PACKED) row = img * N + prefix + p;
    const int s = w / ups, x = w - s * ups, h = x / uph, j0 = (x - h * uph) * VEC;
    T *pa = qkv + ((size_t)row * 3 + s) * D + h * hd + j0, *pb = pa + half;
    const float *pc = cs + tab + (size_t)p * half + j0, *ps = sn + tab + (size_t)p * half + j0;
    float a[VEC], b[VEC], c[VEC], t[VEC];
    {
        const V va = *(const V *)pa, vb = *(const V *)pb;
#pragma unroll
        for (int e = 0; e < VEC; ++e) { a[e] = (float)va.e[e]; b[e] = (float)vb.e[e]; }
        if constexpr (PLANES) {
            const V la = *(const V *)(pa + lo_off), lb = *(const V *)(pb + lo_off);
#pragma unroll
            for (int e = 0; e < VEC; ++e) { a[e] = a[e] + (float)la.e[e] * kHiLoInv; b[e] = b[e] + (float)lb.e[e] * kHiLoInv; }
        }
    }
    if constexpr (VEC % 4 == 0) {
#pragma unroll
        for (int e = 0; e < VEC; e += 4) {
            const f32x4 c4 = *(const f32x4 *)(pc + e), s4 = *(const f32x4 *)(ps + e);
#pragma unroll
            for (int k = 0; k < 4; ++k) { c[e + k] = c4[k]; t[e + k] = s4[k]; }
        }
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) { c[e] = pc[e]; t[e] = ps[e]; }
    }
    V oa, ob, la, lb;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const float ra = a[e] * c[e] - b[e] * t[e], rb = b[e] * c[e] + a[e] * t[e];
        oa.e[e] = (T)ra; ob.e[e] = (T)rb;
        if constexpr (PLANES) { la.e[e] = (T)((ra - (float)oa.e[e]) * kHiLoScale); lb.e[e] = (T)((rb - (float)ob.e[e]) * kHiLoScale); }
    }
    *(V *)pa = oa; *(V *)pb = ob;
    if constexpr (PLANES) { *(V *)(pa + lo_off) = la; *(V *)(pb + lo_off) = lb; }
}

template <typename T, int VEC>
hipError_t launch_rope_t(void *qkv, long lo_off, const float *cs, const float *sn, long units, int N, int prefix, int D, int hd, hipStream_t stream) {
    const dim3 grid((unsigned)((units + 255) / 256)), blk(256);
    if constexpr (std::is_same<T, _Float16>::value) {
        if (lo_off) { hipLaunchKernelGGL((rope_kernel<T, VEC, true, false>), grid, blk, 0, stream, (T *)qkv, lo_off, cs, sn, units, N, prefix, D, hd, nullptr, nullptr, 0); return hipGetLastError(); }
    }
    hipLaunchKernelGGL((rope_kernel<T, VEC, false, false>), grid, blk, 0, stream, (T *)qkv, 0L, cs, sn, units, N, prefix, D, hd, nullptr, nullptr, 0);
    return hipGetLastError();
}
// the packed form: one operand plane (a packed context has no parity planes)
template <typename T, int VEC>
hipError_t launch_rope_packed_t(void *qkv, const float *cs, const float *sn, long units, int prefix, int D, int hd, const int *row0, const int *toff, int n, hipStream_t stream) {
    const dim3 grid((unsigned)((units + 255) / 256)), blk(256);
    hipLaunchKernelGGL((rope_kernel<T, VEC, false, true>), grid, blk, 0, stream, (T *)qkv, 0L, cs, sn, units, 0, prefix, D, hd, row0, toff, n);
    return hipGetLastError();
}

}  // namespace

bool rope_supports(int D, int H) { return D > 0 && H > 0 && D % H == 0 && (D / H) % 2 == 0; }

hipError_t launch_rope(int dtype, void *qkv, long lo_off, const float *cs, const float *sn, int n_img, int N, int prefix, int D, int H, hipStream_t stream) {
    if (!rope_supports(D, H) || n_img <= 0 || prefix < 0 || prefix > N || lo_off < 0 || (lo_off && dtype != DT_F16)) return hipErrorInvalidValue;
    if (prefix == N) return hipSuccess;                                  // no patch row: nothing to rotate
    const int hd = D / H;
    // the wide form needs every piece on a 16-byte boundary: hd / 2 and the row length in whole groups of 8 elements, aligned bases, an aligned lo plane
    const bool wide = (hd / 2) % 8 == 0 && (uintptr_t)qkv % 16 == 0 && (uintptr_t)cs % 16 == 0 && (uintptr_t)sn % 16 == 0 && lo_off % 8 == 0;
    const long units = (long)n_img * (N - prefix) * (wide ? D / 8 : D);
    if (units > 0x7fffffffL * 256) return hipErrorInvalidValue;
    if (wide) return VITX_BY_DTYPE2(dtype, launch_rope_t, 8, qkv, lo_off, cs, sn, units, N, prefix, D, hd, stream);
    return VITX_BY_DTYPE2(dtype, launch_rope_t, 1, qkv, lo_off, cs, sn, units, N, prefix, D, hd, stream);
}

// patch_rows = row0[n] - row0[0] - n * prefix, toff_aligned = every toff[i] is a multiple of 4 floats: both known to the caller, who built the tables
hipError_t launch_rope_packed(int dtype, void *qkv, const float *cs, const float *sn, const int *row0, const int *toff, int n, long patch_rows, bool toff_aligned, int prefix, int D,
                              int H, hipStream_t stream) {
    if (!rope_supports(D, H) || n <= 0 || prefix < 0 || patch_rows < 0 || !row0 || !toff) return hipErrorInvalidValue;
    if (patch_rows == 0) return hipSuccess;
    const int hd = D / H;
    const bool wide = (hd / 2) % 8 == 0 && (uintptr_t)qkv % 16 == 0 && (uintptr_t)cs % 16 == 0 && (uintptr_t)sn % 16 == 0 && toff_aligned;
    const long units = patch_rows * (wide ? D / 8 : D);
    if (units > 0x7fffffffL * 256) return hipErrorInvalidValue;
    if (wide) return VITX_BY_DTYPE2(dtype, launch_rope_packed_t, 8, qkv, cs, sn, units, prefix, D, hd, row0, toff, n, stream);
    return VITX_BY_DTYPE2(dtype, launch_rope_packed_t, 1, qkv, cs, sn, units, prefix, D, hd, row0, toff, n, stream);
}

}  // namespace vitx
