// attention_pool_packed.hip -- the pooling pass of the attention-pooling (MAP) head on a PACK (include/vitx.h "packed batches", pool_head): images of
// different row counts end to end, image i = rows row0[i] .. row0[i + 1] - 1 of the f32 residual stream.  The arithmetic is attention_pool.hip's
//     F[t] = the final-norm row of token t (LnRow::norm);  s[h,t] = u_h . F[t];  p_h = softmax_t(s_h);  M_h = sum_t p[h,t] F[t]      -- all f32
// but both products run on the matrix pipe (v_mfma_f32_16x16x4_f32, exact f32 products, H <= 16 as one tile side) and the work is cut into chunks
// of kPoolChunkRows = 128 rows of ONE image, so a 4000-row image beside two hundred small ones is 32 work items, not one.  Two launches, no atomics.
//
// attention_pool_part_kernel: 1-D grid, one workgroup of 4 waves per (image, chunk), found by the family's scalar binary search of the workgroup
// index in chunk0 [n + 1] (the running count of ceil(N_i / 128)).  u^T goes to LDS once (zero for heads >= H).  Per step of 16 rows:
//   * wave w normalises rows 4 w .. 4 w + 3 of the step (LnRow::norm: the bits of features.hip and attention_pool.hip) and parks them as f32 in the LDS
//     tile Fs [16][D + 16]; rows past the chunk's or the image's end are never loaded: their tile rows are zeros and their P is 0;
//   * scores S [16 rows][16 heads] = Fs u^T: the K = D range is split over the waves (D / 16 MFMAs each, two accumulators), the four partial tiles are
//     summed through LDS in wave order by every wave (the same bits in all of them);
//   * online softmax per head column: lane (l15 = head, l4) holds rows l4, 4 + l4, 8 + l4, 12 + l4 -- the A fragment of P^T as it is needed next; the
//     16-row maximum and sum cross the four lane rows with v_permlane swaps (rows4_max / rows4_sum), no butterfly per row; exp = the hardware's exp2
//     of x log2 e; running (m, l) per head, replicated in every wave;
//   * acc [16 heads][D] += P^T Fs: wave w owns columns w D / 4 .. (w + 1) D / 4 - 1 as D / 64 tiles of 16, 4 MFMAs per tile and step, accumulators in
//     registers (48 per lane at D 768), rescaled by exp(m_old - m_new) first;
//   * the NEXT step's rows are loaded and normalised into registers between the score barrier and the accumulation, so their loads fly under the MFMAs.
// LDS: pitch D + 16 floats (= 16 mod 64 banks) and the column index XOR-ed with bits 2..3 of the tile row.  The accumulation reads Fs[4 kk + l4][c0 + l15]:
// banks 16 l4 + (l15 ^ 4 kk), all 64 distinct.  The scores read Fs[l15][k0 + l4] and Us[l15][k0 + l4]: banks 16 (l15 & 3) + ((k0 ^ (l15 & 12)) + l4), all 64
// distinct -- without the XOR the four rows l15, l15 + 4, .. would share a bank.  At the chunk's end (m_h, l_h, acc_h[D]) for h < H goes to the
// partial scratch [chunk][H][D + 2].
// R = 128 rows per chunk.  As hipcc reports for D 768 (VEC 4, NV 3): 195 VGPRs + 78 AGPRs, no scratch, occupancy 1 wave per SIMD; 104448 bytes of dynamic
// LDS (2 x 16 x 784 x 4 + 4096) hold one workgroup per CU as well, which is why the next step's loads are issued by hand.  D 1152 (VEC 2, NV 9): 254 + 110
// registers, 153600 bytes.  Hidden sizes above 1152 do not fit 160 KiB.  Measured: profiles/pack_map_cost.txt.
//
// attention_pool_combine_kernel: one workgroup per (image, head) walks the image's chunks in ascending order: m = max m_c, e_c = exp(m_c - m),
// L = ((l_0 e_0 + l_1 e_1) + ...), sum[d] = ((acc_0[d] e_0 + acc_1[d] e_1) + ...), M = sum / L, stored as f32 and / or RNE in the operand type.
// An image's M is a function of its own rows, N_i, D and H: chunks are cut from the image's own first row, so it has the same bits alone, at any
// position in a pack and beside any neighbours.
#include "device_common.h"
#include "ln_row.h"
#include "kernels.h"

namespace vitx {

namespace {

constexpr int kPpWaves = 4, kPpPad = 16;
constexpr int kPpLdsLimit = 160 * 1024;
constexpr int pp_lds_bytes(int D) { return (2 * 16 * (D + kPpPad) + kPpWaves * 256) * 4; }

// the image of workgroup wg: chunk0[lo] <= wg < chunk0[lo + 1], uniform addresses (scalar loads)
__device__ __forceinline__ int pp_find_image(const int *__restrict__ chunk0, int n, int wg) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk0[mid] <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

template <int VEC, int NV>
__global__ __launch_bounds__(kPpWaves * 64) void attention_pool_part_kernel(const float *__restrict__ x, const int *__restrict__ row0, const int *__restrict__ chunk0, int n,
                                                                            const float *__restrict__ w, const float *__restrict__ b, float eps, const float *__restrict__ u,
                                                                            float *__restrict__ part, int H) {
    typedef LnRow<VEC, NV> R;
    constexpr int D = 64 * VEC * NV, CPL = VEC * NV, PITCH = D + kPpPad, KW = D / kPpWaves;
    extern __shared__ __attribute__((aligned(16))) float pp_smem[];
    float *Fs = pp_smem, *Us = pp_smem + 16 * PITCH, *Sp = pp_smem + 32 * PITCH;      // [16][PITCH] | [16][PITCH] | [4][16 rows][16 heads]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l15 = lane & 15, l4 = lane >> 4;
    const int wg = blockIdx.x, img = pp_find_image(chunk0, n, wg), c = wg - chunk0[img];
    const int r_img = row0[img], N = row0[img + 1] - r_img;
    const int nrows = N - c * kPoolChunkRows < kPoolChunkRows ? N - c * kPoolChunkRows : kPoolChunkRows;      // >= 1: the host cut the chunks
    const float *xi = x + ((size_t)r_img + (size_t)c * kPoolChunkRows) * D;
    const float NEG = -__builtin_inff();

    for (int i = threadIdx.x; i < 16 * D; i += kPpWaves * 64) {
        const int h = i / D, k = i - h * D;
        Us[h * PITCH + (k ^ (h & 12))] = h < H ? u[(size_t)h * D + k] : 0.0f;
    }
    f32x4 acc[CPL];
#pragma unroll
    for (int t = 0; t < CPL; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m = NEG, l = 0.0f;             // of head l15, the same bits in every lane row and wave
    float fn[4][NV][VEC];
    // rows 4 wave .. 4 wave + 3 of step s, normalised into registers; a row past the end is zeros and is never loaded
    auto load = [&](int s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = s * 16 + wave * 4 + i;
            if (r < nrows) R::norm(xi + (size_t)r * D, w, b, eps, lane, fn[i]);
            else {
#pragma unroll
                for (int p = 0; p < NV; ++p)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) fn[i][p][e] = 0.0f;
            }
        }
    };
    load(0);
    const int steps = (nrows + 15) >> 4;
    for (int s = 0; s < steps; ++s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rt = wave * 4 + i;
#pragma unroll
            for (int p = 0; p < NV; ++p) R::put(Fs + rt * PITCH + (R::col(p, lane) ^ (rt & 12)), fn[i][p]);
        }
        __syncthreads();                  // the tile (and, in step 0, u) is in LDS
        {
            f32x4 s0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, s1 = s0;
            const float *fr = Fs + l15 * PITCH, *ur = Us + l15 * PITCH;
            const int sw = l15 & 12;
#pragma unroll 4
            for (int k0 = 0; k0 < KW; k0 += 8) {
                const int ka = (wave * KW + k0 + l4) ^ sw, kb = (wave * KW + k0 + 4 + l4) ^ sw;
                s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(fr[ka], ur[ka], s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(fr[kb], ur[kb], s1, 0, 0, 0);
            }
            const f32x4 sc = s0 + s1;
#pragma unroll
            for (int q = 0; q < 4; ++q) Sp[wave * 256 + (l4 * 4 + q) * 16 + l15] = sc[q];
        }
        __syncthreads();                  // the four partial score tiles are in LDS
        if (s + 1 < steps) load(s + 1);   // in flight under the accumulation below
        float pr[4];
        {
            float sv[4], mx = NEG;
            bool ok[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int r = 4 * kk + l4, idx = r * 16 + l15;
                sv[kk] = ((Sp[idx] + Sp[256 + idx]) + Sp[512 + idx]) + Sp[768 + idx];
                ok[kk] = s * 16 + r < nrows;
                if (ok[kk]) mx = fmaxf(mx, sv[kk]);
            }
            mx = rows4_max(mx);
            const float mn = fmaxf(m, mx);
            const float scl = mn > m ? __expf(m - mn) : 1.0f;        // exp(-inf) = 0 in the first step: the accumulators are zero anyway
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) pr[kk] = ok[kk] ? __expf(sv[kk] - mn) : 0.0f;
            l = l * scl + rows4_sum((pr[0] + pr[1]) + (pr[2] + pr[3]));
            m = mn;
            // the accumulators of this lane are heads 4 l4 + q: their factors live in lanes 4 l4 + q (lane row 0, head = lane)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float sq = __shfl(scl, l4 * 4 + q);
#pragma unroll
                for (int t = 0; t < CPL; ++t) acc[t][q] = acc[t][q] * sq;
            }
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const float *fr = Fs + (4 * kk + l4) * PITCH;
#pragma unroll
            for (int t = 0; t < CPL; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[kk], fr[(wave * KW + t * 16 + l15) ^ (4 * kk)], acc[t], 0, 0, 0);
        }
        __syncthreads();                  // every wave is done with the tile before the next step overwrites it
    }
    float *po = part + (size_t)wg * H * (D + 2);
    if (wave == 0 && l4 == 0 && l15 < H) { po[(size_t)l15 * (D + 2)] = m; po[(size_t)l15 * (D + 2) + 1] = l; }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int h = l4 * 4 + q;
        if (h < H) {
#pragma unroll
            for (int t = 0; t < CPL; ++t) po[(size_t)h * (D + 2) + 2 + wave * KW + t * 16 + l15] = acc[t][q];
        }
    }
}

template <typename T16>
__global__ __launch_bounds__(256) void attention_pool_combine_kernel(const float *__restrict__ part, const int *__restrict__ chunk0, float *__restrict__ M,
                                                                     T16 *__restrict__ m16, int D, int H) {
    const int img = blockIdx.x / H, h = blockIdx.x - img * H;
    const int c0 = chunk0[img], nc = chunk0[img + 1] - c0;
    const size_t cs = (size_t)H * (D + 2);
    const float *p0 = part + (size_t)c0 * cs + (size_t)h * (D + 2);
    const float NEG = -__builtin_inff();
    float mg = p0[0];
    for (int k = 1; k < nc; ++k) mg = fmaxf(mg, p0[k * cs]);
    float L = 0.0f;
    for (int k = 0; k < nc; ++k) {
        const float mk = p0[k * cs];
        L = L + p0[k * cs + 1] * (mk == NEG ? 0.0f : __expf(mk - mg));
    }
    const size_t off = ((size_t)img * H + h) * D;
    for (int d = threadIdx.x; d < D; d += 256) {
        float sum = 0.0f;
        for (int k = 0; k < nc; ++k) {
            const float mk = p0[k * cs];
            const float v = p0[k * cs + 2 + d] * (mk == NEG ? 0.0f : __expf(mk - mg));
            sum = k == 0 ? v : sum + v;
        }
        const float o = sum / L;
        if (M) M[off + d] = o;
        if (m16) m16[off + d] = (T16)o;
    }
}

template <typename T16>
hipError_t launch_pool_packed_t(const float *x, const int *row0, const int *chunk0, int n, int chunks, const float *w, const float *b, float eps, const float *u, float *part,
                                float *M, void *m16, int D, int H, hipStream_t stream) {
    const bool ok = ln_for_width(D, [&](auto vec, auto nv) {
        constexpr int DD = 64 * vec() * nv();
        if constexpr (pp_lds_bytes(DD) <= kPpLdsLimit)
            hipLaunchKernelGGL((attention_pool_part_kernel<vec(), nv()>), dim3(chunks), dim3(kPpWaves * 64), pp_lds_bytes(DD), stream, x, row0, chunk0, n, w, b, eps, u, part, H);
    });
    if (!ok) return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((attention_pool_combine_kernel<T16>), dim3((unsigned)n * H), dim3(256), 0, stream, part, chunk0, M, (T16 *)m16, D, H);
    return hipGetLastError();
}

}  // namespace

hipError_t prepare_attention_pool_packed() {
    hipError_t e = hipSuccess;
#define VITX_PP_PREPARE(DD, VEC, NV) \
    if constexpr (pp_lds_bytes(DD) <= kPpLdsLimit) { if (e == hipSuccess) e = hipFuncSetAttribute((const void *)attention_pool_part_kernel<VEC, NV>, hipFuncAttributeMaxDynamicSharedMemorySize, pp_lds_bytes(DD)); }
    VITX_LN_WIDTHS(VITX_PP_PREPARE)
#undef VITX_PP_PREPARE
    return e;
}

bool attention_pool_packed_fits(int D) { return D > 0 && pp_lds_bytes(D) <= kPpLdsLimit; }

bool pool_pack_chunks(const int32_t *rows, int n, int32_t *chunk0) {
    if (!rows || n <= 0) return false;
    int64_t c = 0;
    for (int i = 0; i < n; ++i) {
        if (rows[i] < 1) return false;
        if (chunk0) chunk0[i] = (int32_t)c;
        c += ((int64_t)rows[i] + kPoolChunkRows - 1) / kPoolChunkRows;
        if (c > 0x7fffffffLL) return false;
    }
    if (chunk0) chunk0[n] = (int32_t)c;
    return true;
}

hipError_t launch_attention_pool_packed(const float *x, const int *row0, const int *chunk0, int n, int chunks, const float *w, const float *b, float eps, const float *u,
                                        float *part, float *M, void *m16, int dtype, int D, int H, hipStream_t stream) {
    if (n <= 0 || chunks < n || H <= 0 || H > kPoolPackMaxHeads || !attention_pool_packed_fits(D) || (!M && !m16) || (long)n * H > 0x7fffffffL) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_pool_packed_t, x, row0, chunk0, n, chunks, w, b, eps, u, part, M, m16, D, H, stream);
}

}  // namespace vitx
