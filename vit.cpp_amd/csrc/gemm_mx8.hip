// gemm_mx8.hip -- the MXFP8 operand mode (include/vitx.h, VITX_MXFP8): the block-scaled GEMM of qkv, fc1 and fc2 on
// v_mfma_scale_f32_16x16x128_f8f6f4, the LayerNorm that writes its A operand, and a test launch of the device encoder.
//
// Operands (mxfp8.h): elements [rows][K_pad] e4m3fn bytes, scales [rows][K_pad / 32] E8M0 bytes, K_pad a multiple of 128.
// One MFMA consumes one 128-deep K step.  Lane l (l15 = l & 15, g4 = l >> 4) feeds row l15 of each operand: bytes 0..15 of its
// 32 are k = 16 g4 .. 16 g4 + 15, bytes 16..31 are k = 64 + 16 g4 .. (measured with exact integer data, tests/test_gpu_mxfp8.py), and
// its scale register carries the scale of block g4 of row l15 in bits 0..7 (opsel 0) -- a block other lanes' bytes belong to.  The
// scale dword of a row holds the row's four blocks of the K step, so a lane shifts it right by 8 g4.
// As in every other family the products are SWAPPED, acc = mfma(W fragment, A fragment): lane (l15, g4) register e then holds
// C[row l15][column 4 g4 + e] and epilogue16.h stores EPI_BIAS (bf16) and EPI_BIAS_RESID (f32) unchanged.
//
// Structure: 128 x 128 tile, 4 waves (2 x 2, 64 x 64 each: 4 x 4 accumulators), one 128-byte K step per stage, two stages; every
// operand byte and every scale dword arrives by LDS-DMA (global_load_lds), the next stage is issued right after the one barrier
// per K step.  A rows beyond M_real are read from row M_real - 1 (never stored); W must hold N_pad = N rounded up to 128 rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vitx.h"
#include "device_common.h"
#include "epilogue16.h"
#include "kernels.h"
#include "ln_row.h"
#include "mxfp8.h"

namespace vitx {
namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int MX_BM = 128, MX_BN = 128, MX_BK = 128;
constexpr int MX_TILE = MX_BM * MX_BK;                   // bytes of one operand tile per stage
constexpr int MX_STAGE = 2 * MX_TILE + (MX_BM + MX_BN) * 4;       // A, W, then one scale dword per A row and per W row
constexpr int MX_LDS = 2 * MX_STAGE;

__device__ __forceinline__ f32x4 mx_mfma(i32x8 w, i32x8 a, f32x4 c, int sw, int sa) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, a, c, 0, 0, 0, sw, 0, sa);
}

// Four values of one block with block exponent e -> four e4m3 bytes (little-endian in a dword).  The producers take the block maximum
// over the lanes that hold the block first; max is exact and order-free, so every producer matches the host encoder bit for bit.
__device__ __forceinline__ uint32_t mx_pack4(const float (&v)[4], int e) {
    return (uint32_t)mx_e4m3_rne(mx_scale_down(v[0], e)) | ((uint32_t)mx_e4m3_rne(mx_scale_down(v[1], e)) << 8) |
           ((uint32_t)mx_e4m3_rne(mx_scale_down(v[2], e)) << 16) | ((uint32_t)mx_e4m3_rne(mx_scale_down(v[3], e)) << 24);
}

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_mx8_kernel(GemmArgs g, const uint8_t *__restrict__ a_s, const uint8_t *__restrict__ w_s, uint8_t *__restrict__ o_s) {
    __shared__ __attribute__((aligned(16))) char smem[MX_LDS];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
    const int n0 = blockIdx.x * MX_BN, m0 = blockIdx.y * MX_BM;
    const int ldk = g.K, lds = g.K / 32;
    const uint8_t *A = (const uint8_t *)g.A, *W = (const uint8_t *)g.W;

    // DMA sources: 16-B piece p = i * 256 + tid of a tile is (row, slot) = swz_inv(p) -- the swizzled image of device_common.h
    const uint8_t *asrc[4], *wsrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int row, slot; swz_inv(i * 256 + tid, row, slot);
        const int ar = min(m0 + row, g.M_real - 1);
        asrc[i] = A + (size_t)ar * ldk + slot * 16;
        wsrc[i] = W + (size_t)(n0 + row) * ldk + slot * 16;
    }
    // scale dwords: wave 0 / 1 -> A rows 0..63 / 64..127, wave 2 / 3 -> W rows 0..63 / 64..127
    const uint8_t *ssrc;
    {
        const int r = (wave & 1) * 64 + lane;
        ssrc = wave < 2 ? a_s + (size_t)min(m0 + r, g.M_real - 1) * lds : w_s + (size_t)(n0 + r) * lds;
    }
    auto issue = [&](int kt, int stage) {
        char *base = smem + stage * MX_STAGE + wave * 1024;
#pragma unroll
        for (int i = 0; i < 4; ++i) __builtin_amdgcn_global_load_lds(GPTR(asrc[i] + kt * MX_BK), LPTR(base + i * 4096), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) __builtin_amdgcn_global_load_lds(GPTR(wsrc[i] + kt * MX_BK), LPTR(base + MX_TILE + i * 4096), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(GPTR(ssrc + kt * 4), LPTR(smem + stage * MX_STAGE + 2 * MX_TILE + wave * 256), 4, 0, 0);
    };

    int a_rd[4], w_rd[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) a_rd[t] = swz_byte(wm * 64 + t * 16 + l15, g4);       // 16-B slots g4 and g4 + 4 (offset ^ 64)
#pragma unroll
    for (int u = 0; u < 4; ++u) w_rd[u] = MX_TILE + swz_byte(wn * 64 + u * 16 + l15, g4);
    const int sh = 8 * g4;

    f32x4 acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[t][u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int nk = g.K / MX_BK;
    issue(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nk) issue(kt + 1, (kt + 1) & 1);
        const char *st = smem + (kt & 1) * MX_STAGE;
        i32x8 af[4], wf[4];
        int as[4], ws[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const i32x4 lo = *(const i32x4 *)(st + a_rd[t]), hi = *(const i32x4 *)(st + (a_rd[t] ^ 64));
            af[t] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            as[t] = *(const int *)(st + 2 * MX_TILE + (wm * 64 + t * 16 + l15) * 4) >> sh;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const i32x4 lo = *(const i32x4 *)(st + w_rd[u]), hi = *(const i32x4 *)(st + (w_rd[u] ^ 64));
            wf[u] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            ws[u] = *(const int *)(st + 2 * MX_TILE + (MX_BM + wn * 64 + u * 16 + l15) * 4) >> sh;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[t][u] = mx_mfma(wf[u], af[t], acc[t][u], ws[u], as[t]);
    }

    const int row0 = m0 + wm * 64 + l15, col0 = n0 + wn * 64 + 4 * g4;
    if constexpr (EPI == EPI_BIAS_GELU) {
        // fc1 -> MX: column blocks of 32 = tiles u = 2 b, 2 b + 1; a row's 8 values of a block sit in the 4 lanes l15 + 16 g4.
        // out = elements [M][ldo] (ldo = the next GEMM's K_pad), o_s = scales [M][ldo / 32]; columns >= N are encoded as zeros.
#pragma unroll
        for (int bq = 0; bq < 2; ++bq) {
            float v[2][4];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = col0 + (2 * bq + h) * 16;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[h][e] = (c + e < g.N) ? g.bias[c + e] : 0.0f;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int row = row0 + t * 16;
                float y[2][4];
                float amax = 0.0f;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int c = col0 + (2 * bq + h) * 16;
                    const f32x4 s = acc[t][2 * bq + h] + f32x4{v[h][0], v[h][1], v[h][2], v[h][3]};
                    const f32x2 p0 = gelu_tanh2(f32x2{s[0], s[1]}), p1 = gelu_tanh2(f32x2{s[2], s[3]});
                    y[h][0] = p0[0]; y[h][1] = p0[1]; y[h][2] = p1[0]; y[h][3] = p1[1];
#pragma unroll
                    for (int e = 0; e < 4; ++e) { if (c + e >= g.N) y[h][e] = 0.0f; amax = fmaxf(amax, fabsf(y[h][e])); }
                }
                amax = fmaxf(amax, __shfl_xor(amax, 16));
                amax = fmaxf(amax, __shfl_xor(amax, 32));
                if (row >= g.M_real) continue;
                const int e = mx_block_exp(amax);
                uint8_t *o = (uint8_t *)g.out + (size_t)row * g.ldo;
#pragma unroll
                for (int h = 0; h < 2; ++h) *(uint32_t *)(o + col0 + (2 * bq + h) * 16) = mx_pack4(y[h], e);
                if (g4 == 0) o_s[(size_t)row * (g.ldo / 32) + (n0 + wn * 64 + bq * 32) / 32] = (uint8_t)(e + 127);
            }
        }
    } else {
        const bool full = m0 + MX_BM <= g.M_real && n0 + MX_BN <= g.N;
        if (full) epilogue16<__bf16, EPI, 4, 4, true>(g, acc, row0, col0);
        else epilogue16<__bf16, EPI, 4, 4, false>(g, acc, row0, col0);
    }
}

// One wave per row: the f32 row the bf16 LayerNorm rounds (LnRow, ln_row.h), encoded.
// A 32-column block is 32 / VEC consecutive lanes.  Columns D .. k_pad are written as zero elements with scale 127.
template <int VEC, int NV>
__global__ __launch_bounds__(256) void layernorm_mx8_kernel(const float *__restrict__ x, long ldx, const float *__restrict__ w, const float *__restrict__ b,
                                                            uint8_t *__restrict__ q, uint8_t *__restrict__ s, int k_pad, int M, float eps) {
    typedef LnRow<VEC, NV> R;
    constexpr int D = 64 * VEC * NV;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float *xr = x + (size_t)row * ldx;
    uint8_t *qr = q + (size_t)row * k_pad, *sr = s + (size_t)row * (k_pad / 32);
    auto store = [&](int idx, const float (&o)[VEC]) {
        float amax = 0.0f;
#pragma unroll
        for (int j = 0; j < VEC; ++j) amax = fmaxf(amax, fabsf(o[j]));
#pragma unroll
        for (int m = 1; m < 32 / VEC; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
        const int e = mx_block_exp(amax);
        if constexpr (VEC == 4) *(uint32_t *)(qr + idx) = mx_pack4(o, e);
        else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) qr[idx + j] = mx_e4m3_rne(mx_scale_down(o[j], e));
        }
        if ((idx & 31) == 0) sr[idx / 32] = (uint8_t)(e + 127);
    };
    R::each(xr, w, b, eps, lane, [&](int, int idx, const float (&o)[VEC]) { store(idx, o); });
    for (int k = D + lane * 4; k < k_pad; k += 256) *(uint32_t *)(qr + k) = 0u;
    for (int k = D / 32 + lane; k < k_pad / 32; k += 64) sr[k] = 127;
}

// Test launch of the device encoder: one thread per 32-element block of x [rows][K] f32 (elements beyond K are zeros)
__global__ void quantize_mx8_kernel(const float *__restrict__ x, int rows, int K, int k_pad, uint8_t *__restrict__ q, uint8_t *__restrict__ s) {
    const int nb = k_pad / 32;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)rows * nb) return;
    const int r = (int)(i / nb), bk = (int)(i % nb), k0 = bk * 32;
    const float *xr = x + (size_t)r * K;
    float amax = 0.0f;
    for (int k = k0; k < k0 + 32 && k < K; ++k) amax = fmaxf(amax, fabsf(xr[k]));
    const int e = mx_block_exp(amax);
    s[i] = (uint8_t)(e + 127);
    for (int k = k0; k < k0 + 32; ++k) q[(size_t)r * k_pad + k] = k < K ? mx_e4m3_rne(mx_scale_down(xr[k], e)) : 0;
}

}  // namespace

bool gemm_mx8_supports(const GemmArgs &a) {
    return a.M_real > 0 && a.N > 0 && a.K > 0 && a.K % MX_BK == 0 && a.N_pad % MX_BN == 0 && a.N_pad >= a.N && (a.N_pad / MX_BN) <= 65535 &&
           (a.M_real + MX_BM - 1) / MX_BM <= 65535;
}

hipError_t launch_gemm_mx8(int epi, const GemmArgs &a, const uint8_t *a_scales, const uint8_t *w_scales, uint8_t *out_scales, hipStream_t stream) {
    if (!gemm_mx8_supports(a) || !a_scales || !w_scales || (epi == EPI_BIAS_GELU && (!out_scales || a.ldo % MX_BK || a.ldo < a.N_pad))) return hipErrorInvalidValue;
    const dim3 grid(a.N_pad / MX_BN, (a.M_real + MX_BM - 1) / MX_BM), blk(256);
    switch (epi) {
    case EPI_BIAS: hipLaunchKernelGGL((gemm_mx8_kernel<EPI_BIAS>), grid, blk, 0, stream, a, a_scales, w_scales, out_scales); break;
    case EPI_BIAS_GELU: hipLaunchKernelGGL((gemm_mx8_kernel<EPI_BIAS_GELU>), grid, blk, 0, stream, a, a_scales, w_scales, out_scales); break;
    case EPI_BIAS_RESID: hipLaunchKernelGGL((gemm_mx8_kernel<EPI_BIAS_RESID>), grid, blk, 0, stream, a, a_scales, w_scales, out_scales); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_layernorm_mx8(const float *x, long ldx, const float *w, const float *b, uint8_t *q, uint8_t *s, int k_pad, int M, int D, float eps, hipStream_t stream) {
    if (D % 32 || k_pad < D || k_pad % MX_BK || M <= 0) return hipErrorInvalidValue;
    const dim3 grid((M + 3) / 4), blk(256);
    const bool ok = ln_for_width(D, [&](auto vec, auto nv) {
        hipLaunchKernelGGL((layernorm_mx8_kernel<vec(), nv()>), grid, blk, 0, stream, x, ldx, w, b, q, s, k_pad, M, eps);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_quantize_mx8(const float *x, int rows, int K, int k_pad, uint8_t *q, uint8_t *s, hipStream_t stream) {
    if (rows <= 0 || K <= 0 || k_pad < K || k_pad % 32) return hipErrorInvalidValue;
    const long n = (long)rows * (k_pad / 32);
    hipLaunchKernelGGL(quantize_mx8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, rows, K, k_pad, q, s);
    return hipGetLastError();
}

}  // namespace vitx
