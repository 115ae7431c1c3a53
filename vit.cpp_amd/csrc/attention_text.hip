// attention_text.hip -- attention of a text tower: a short sequence (1 .. 128 tokens), any head dim that is a multiple of 8 up to 128, an optional causal mask.
#include "kernels.h"
#include "epilogue16.h"
#include "device_common.h"

namespace vitx {

// ------------------------------------------------------------------------------------------------
// The arithmetic is attention_generic_kernel's: S^T = K . Q^T by v_mfma_f32_16x16x32 over the head dim zero-padded to a multiple of 32, two
// passes over the keys (row maximum; then exp per AttnExpRt<T>, row sum of the rounded numerators, O^T = V^T . P^T), normalised after P.V,
// scores of a query in the four lanes (lane & 15, lane >> 4).  What a sequence this short allows:
//   * one workgroup per (prompt, head); its K and V rows (32-key steps, rows past N zero) are brought into LDS ONCE and shared by the four
//     waves, which take the 16-query tiles wave, wave + 4: no global re-read of K per tile and pass, one barrier, none after it;
//   * K rows carry 16 bytes of padding (16 rows of a ds_read_b128 lane group fall into different bank groups), V rows none: they are read
//     back transposed by ds_read_b64_tr_b16 exactly as the generic kernel reads its per-wave copy;
//   * causal: query tile qt needs the key tiles 0 .. qt only -- a tile wholly above the diagonal is never multiplied; in the diagonal tile
//     key j > query t is set to -inf by a select BEFORE the row maximum, so row t is exactly attention over keys 0 .. t for any FINITE later
//     rows, however large: a score of theirs that overflowed to inf or NaN is replaced, not computed with.  Their V rows are still multiplied,
//     by the weight 0, in the diagonal tile and the other half of its 32-key step -- a V element that is itself inf or NaN would make 0 . inf = NaN.
//     qkv comes from a GEMM of finite operands; an inf there has already spoiled its own rows.
// LDS: N rounded up to 32 rows of (2 DHP + 16) + 2 DHP bytes, at most 67584 (head dims above 96 at more than 124 tokens pass 64 KiB:
// prepare_attention_text raises the dynamic-LDS limit of every instantiation).
// ------------------------------------------------------------------------------------------------
template <typename T, int NK2>
__global__ __launch_bounds__(256) void attention_text_kernel(const T *__restrict__ qkv, T *__restrict__ out, int N, int D, int H, int DH, float scale, int causal) {
    constexpr int DHP = NK2 * 32, ND = DHP / 16, VROWB = DHP * 2, KROWB = VROWB + 16, C8 = DHP / 8;
    extern __shared__ __attribute__((aligned(16))) char smem_text[];
    typedef typename Elem<T>::v8 v8;
    typedef typename Pair<T>::v2 v2;
    typedef short s4 __attribute__((ext_vector_type(4)));
    typedef short s8 __attribute__((ext_vector_type(8)));
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int nt16 = (N + 15) / 16, rows = ((N + 31) / 32) * 32;
    const size_t row_el = (size_t)3 * D;
    const T *base = qkv + (size_t)b * N * row_el + (size_t)h * DH;        // q of token 0; k at + D, v at + 2 D
    const v8 zero8 = __builtin_bit_cast(v8, (int __attribute__((ext_vector_type(4)))){0, 0, 0, 0});
    char *ks = smem_text, *vs = smem_text + rows * KROWB;
    // ---- K and V of this (prompt, head) into LDS: 16-byte pieces; pieces past head_dim and rows past N are zeros
    for (int pi = tid; pi < rows * C8; pi += 256) {
        const int row = pi / C8, c8 = pi - row * C8;
        const bool live = row < N && c8 * 8 < DH;
        const T *src = base + (size_t)min(row, N - 1) * row_el + c8 * 8;
        *(v8 *)(ks + row * KROWB + c8 * 16) = live ? *(const v8 *)(src + D) : zero8;
        *(v8 *)(vs + row * VROWB + c8 * 16) = live ? *(const v8 *)(src + 2 * D) : zero8;
    }
    __syncthreads();
    const unsigned lds_v = (unsigned)(__UINTPTR_TYPE__)((__attribute__((address_space(3))) char *)vs);
    const unsigned tr_off = (4 * g4 + (l15 >> 2)) * VROWB + (l15 & 3) * 8;      // this lane's V row of a 16-key group, 4-dim piece of a 16-dim tile
    const float kk = AttnExpRt<T>::k(scale);
    for (int qt = wave; qt < nt16; qt += 4) {            // wave-uniform; no barrier below
        const int q0 = qt * 16, qrow = min(q0 + l15, N - 1);
        const int ntk = causal ? qt + 1 : nt16;          // key tiles this query tile multiplies
        const int last = causal ? qrow : N - 1;          // the last key of this lane's query
        // Q fragments (B operand): lane (l15 = query, g4) holds dims k2 * 32 + g4 * 8 .. + 7
        v8 qf[NK2];
#pragma unroll
        for (int k2 = 0; k2 < NK2; ++k2) { const int d0 = k2 * 32 + g4 * 8; qf[k2] = d0 < DH ? *(const v8 *)(base + (size_t)qrow * row_el + d0) : zero8; }
        auto score_tile = [&](int t) {                   // S^T tile t: rows = keys 16 t .., cols = queries; acc[r] = key 16 t + 4 g4 + r
            const char *kr = ks + (t * 16 + l15) * KROWB + g4 * 16;
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k2 = 0; k2 < NK2; ++k2) acc = Elem<T>::mfma16(*(const v8 *)(kr + k2 * 64), qf[k2], acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) if (t * 16 + 4 * g4 + r > last) acc[r] = -INFINITY;
            return acc;
        };
        // ---- pass 1: row maximum (key 0 is never masked: the maximum is a score)
        float mx = -INFINITY;
        for (int t = 0; t < ntk; ++t) {
            const f32x4 sc = score_tile(t);
            mx = fmaxf(fmaxf(mx, sc[0]), sc[1]); mx = fmaxf(fmaxf(mx, sc[2]), sc[3]);
        }
        mx = rows4_max(mx);
        const float nmx = -kk * mx;
        // ---- pass 2: numerators, row sum, PV
        f32x4 o[ND];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        float sum = 0.0f;
        for (int s32 = 0; s32 < (ntk + 1) / 2; ++s32) {
            const f32x4 sa = score_tile(2 * s32);
            f32x4 sb = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (2 * s32 + 1 < ntk) sb = score_tile(2 * s32 + 1);
            const v2 e0 = AttnExpRt<T>::pair(sa[0], sa[1], nmx, kk), e1 = AttnExpRt<T>::pair(sa[2], sa[3], nmx, kk);
            const v2 e2 = AttnExpRt<T>::pair(sb[0], sb[1], nmx, kk), e3 = AttnExpRt<T>::pair(sb[2], sb[3], nmx, kk);
            sum = Pair<T>::sum2(e0, sum); sum = Pair<T>::sum2(e1, sum); sum = Pair<T>::sum2(e2, sum); sum = Pair<T>::sum2(e3, sum);
            const v8 pk = v8{e0[0], e0[1], e1[0], e1[1], e2[0], e2[1], e3[0], e3[1]};
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) {
                s4 f0, f1;
                const unsigned va = lds_v + s32 * (32 * VROWB) + tr_off + dt * 32;
                asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f0) : "v"(va) : "memory");
                asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f1) : "v"(va + 16 * VROWB) : "memory");
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f0), "+v"(f1));
                const s8 both = __builtin_shufflevector(f0, f1, 0, 1, 2, 3, 4, 5, 6, 7);
                o[dt] = Elem<T>::mfma16(__builtin_bit_cast(v8, both), pk, o[dt]);
            }
        }
        const float inv = 1.0f / rows4_sum(sum);
        // lane (l15 = query, g4) holds O[query][dt * 16 + 4 g4 .. + 3]
        if (q0 + l15 < N) {
            T *orow = out + ((size_t)b * N + q0 + l15) * D + (size_t)h * DH;
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) {
                const int d0 = dt * 16 + 4 * g4;
                if (d0 < DH) {
                    const v2 lo = round_pair<T>(o[dt][0] * inv, o[dt][1] * inv), hi = round_pair<T>(o[dt][2] * inv, o[dt][3] * inv);
                    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
                    *(u32x2_t *)(orow + d0) = u32x2_t{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
                }
            }
        }
    }
}

constexpr int kTextMaxTokens = 128;
static size_t attention_text_lds(int N, int nk2) { return (size_t)((N + 31) / 32 * 32) * (size_t)(nk2 * 128 + 16); }
bool attention_text_supports(int T, int D, int H) { return T >= 1 && T <= kTextMaxTokens && attention_generic_supports(D, H); }

template <typename T>
static hipError_t launch_attention_text_t(const void *qkv, void *out, int n, int N, int D, int H, int causal, hipStream_t stream) {
    const int DH = D / H, nk2 = (DH + 31) / 32;
    const float scale = 1.0f / sqrtf((float)DH);
    const dim3 grid((unsigned)((size_t)n * H)), blk(256);
    const size_t lds = attention_text_lds(N, nk2);
    switch (nk2) {
    case 1: hipLaunchKernelGGL((attention_text_kernel<T, 1>), grid, blk, lds, stream, (const T *)qkv, (T *)out, N, D, H, DH, scale, causal); break;
    case 2: hipLaunchKernelGGL((attention_text_kernel<T, 2>), grid, blk, lds, stream, (const T *)qkv, (T *)out, N, D, H, DH, scale, causal); break;
    case 3: hipLaunchKernelGGL((attention_text_kernel<T, 3>), grid, blk, lds, stream, (const T *)qkv, (T *)out, N, D, H, DH, scale, causal); break;
    case 4: hipLaunchKernelGGL((attention_text_kernel<T, 4>), grid, blk, lds, stream, (const T *)qkv, (T *)out, N, D, H, DH, scale, causal); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
hipError_t launch_attention_text(int dtype, const void *qkv, void *out, int n, int T, int D, int H, int causal, hipStream_t stream) {
    if (n <= 0 || !attention_text_supports(T, D, H) || (size_t)n * H > 0x7fffffffu) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_attention_text_t, qkv, out, n, T, D, H, causal ? 1 : 0, stream);
}
// Only the head dims above 96 can pass 64 KiB; every instantiation gets the limit of its own largest case all the same, so a launch never depends on which ran first.
hipError_t prepare_attention_text() {
    hipError_t e = hipSuccess;
    auto set = [&](const void *fn, int nk2) { if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attention_text_lds(kTextMaxTokens, nk2)); };
    set((const void *)attention_text_kernel<_Float16, 1>, 1); set((const void *)attention_text_kernel<__bf16, 1>, 1);
    set((const void *)attention_text_kernel<_Float16, 2>, 2); set((const void *)attention_text_kernel<__bf16, 2>, 2);
    set((const void *)attention_text_kernel<_Float16, 3>, 3); set((const void *)attention_text_kernel<__bf16, 3>, 3);
    set((const void *)attention_text_kernel<_Float16, 4>, 4); set((const void *)attention_text_kernel<__bf16, 4>, 4);
    return e;
}

}  // namespace vitx
