// attention_rows.h -- the arithmetic of the generic attention for ONE wave: a 16-query tile of one (image, head) over that image's N keys.  THE
// definition for both kernels that run it: attention_generic_kernel (one token count per launch, attention_generic.hip) and
// attention_packed_kernel (a segment table, attention_packed.hip) differ only in how a workgroup finds its image, head and query block, so the
// rows of an image have the same bits through either.
// S^T = K . Q^T by v_mfma_f32_16x16x32 over the head dim zero-padded to a multiple of 32, two passes over the keys (row maximum; then exp per
// AttnExpRt<T>, row sum of the rounded numerators, O^T = V^T . P^T), scores in the four lanes (lane & 15, lane >> 4) of a query.  No workgroup
// barrier: K fragments come straight from global memory (16-byte pieces of a key's head slice; pieces past head_dim are zeros), a 32-key step
// of V goes through the wave's own 32 * DHP * 2 bytes of LDS to be read back transposed (ds_read_b64_tr_b16).
#pragma once
#include "kernels.h"
#include "epilogue16.h"
#include "device_common.h"

namespace vitx {

// base: q of the image's token 0 in this head (k at + D, v at + 2 D, rows 3 D apart); orow0: the image's output row 0 in this head (rows D apart);
// q0: the tile's first query (q0 < N); my: the wave's LDS.  Key and value rows clamp to the image's own last row N - 1; keys at and past N are
// -inf before the row maximum.  Writes rows q0 .. min(q0 + 16, N) - 1 of the head's DH columns, nothing else.
template <typename T, int NK2>
__device__ __forceinline__ void attention_rows16(const T *__restrict__ base, T *__restrict__ orow0, int N, int D, int DH, float scale, int q0, char *my) {
    constexpr int DHP = NK2 * 32, ND = DHP / 16, ROWB = DHP * 2;       // padded head dim, 16-dim output tiles, LDS row bytes
    typedef typename Elem<T>::v8 v8;
    typedef typename Pair<T>::v2 v2;
    typedef short s4 __attribute__((ext_vector_type(4)));
    typedef short s8 __attribute__((ext_vector_type(8)));
    const int lane = threadIdx.x & 63, l15 = lane & 15, g4 = lane >> 4;
    const size_t row_el = (size_t)3 * D;
    const v8 zero8 = __builtin_bit_cast(v8, (int __attribute__((ext_vector_type(4)))){0, 0, 0, 0});
    // Q fragments (B operand): lane (l15 = query, g4) holds dims k2 * 32 + g4 * 8 .. + 7
    v8 qf[NK2];
    {
        const int qrow = min(q0 + l15, N - 1);
#pragma unroll
        for (int k2 = 0; k2 < NK2; ++k2) { const int d0 = k2 * 32 + g4 * 8; qf[k2] = d0 < DH ? *(const v8 *)(base + (size_t)qrow * row_el + d0) : zero8; }
    }
    auto score_tile = [&](int t) {                   // S^T tile t: rows = keys 16 t .., cols = queries; acc[r] = key 16 t + 4 g4 + r
        const int krow = min(t * 16 + l15, N - 1);
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k2 = 0; k2 < NK2; ++k2) {
            const int d0 = k2 * 32 + g4 * 8;
            const v8 kf = d0 < DH ? *(const v8 *)(base + D + (size_t)krow * row_el + d0) : zero8;
            acc = Elem<T>::mfma16(kf, qf[k2], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) if (t * 16 + 4 * g4 + r >= N) acc[r] = -INFINITY;
        return acc;
    };
    // ---- pass 1: row maximum
    const int nt16 = (N + 15) / 16, nks = (N + 31) / 32;
    float mx = -INFINITY;
    for (int t = 0; t < nt16; ++t) {
        const f32x4 sc = score_tile(t);
        mx = fmaxf(fmaxf(mx, sc[0]), sc[1]); mx = fmaxf(fmaxf(mx, sc[2]), sc[3]);
    }
    mx = rows4_max(mx);
    const float kk = AttnExpRt<T>::k(scale), nmx = -kk * mx;
    // ---- pass 2: numerators, row sum, PV
    f32x4 o[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float sum = 0.0f;
    const unsigned lds_my = (unsigned)(__UINTPTR_TYPE__)((__attribute__((address_space(3))) char *)my);
    const unsigned tr_off = (4 * g4 + (l15 >> 2)) * ROWB + (l15 & 3) * 8;      // this lane's V row of a 16-key group, 4-dim piece of a 16-dim tile
    for (int ks = 0; ks < nks; ++ks) {
        const f32x4 sa = score_tile(2 * ks);
        f32x4 sb = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (2 * ks + 1 < nt16) sb = score_tile(2 * ks + 1);
        const v2 e0 = AttnExpRt<T>::pair(sa[0], sa[1], nmx, kk), e1 = AttnExpRt<T>::pair(sa[2], sa[3], nmx, kk);
        const v2 e2 = AttnExpRt<T>::pair(sb[0], sb[1], nmx, kk), e3 = AttnExpRt<T>::pair(sb[2], sb[3], nmx, kk);
        sum = Pair<T>::sum2(e0, sum); sum = Pair<T>::sum2(e1, sum); sum = Pair<T>::sum2(e2, sum); sum = Pair<T>::sum2(e3, sum);
        const v8 pk = v8{e0[0], e0[1], e1[0], e1[1], e2[0], e2[1], e3[0], e3[1]};
        // V rows 32 ks .. + 31 (clamped: their probabilities are zero past N) x DHP dims into the wave's LDS, row-major
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the previous step's transposed reads are done with it
#pragma unroll
        for (int i = 0; i < (32 * DHP / 8 + 63) / 64; ++i) {
            const int pi = i * 64 + lane, row = pi / (DHP / 8), c8 = pi - row * (DHP / 8);
            if (pi < 32 * DHP / 8) {
                const int vrow = min(ks * 32 + row, N - 1);
                const v8 vv = c8 * 8 < DH ? *(const v8 *)(base + 2 * D + (size_t)vrow * row_el + c8 * 8) : zero8;
                *(v8 *)(my + row * ROWB + c8 * 16) = vv;
            }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
            s4 f0, f1;
            const unsigned va = lds_my + tr_off + dt * 32;
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f0) : "v"(va) : "memory");
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f1) : "v"(va + 16 * ROWB) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f0), "+v"(f1));
            const s8 both = __builtin_shufflevector(f0, f1, 0, 1, 2, 3, 4, 5, 6, 7);
            o[dt] = Elem<T>::mfma16(__builtin_bit_cast(v8, both), pk, o[dt]);
        }
    }
    const float inv = 1.0f / rows4_sum(sum);
    // lane (l15 = query, g4) holds O[query][dt * 16 + 4 g4 .. + 3]
    const int qrow = q0 + l15;
    if (qrow < N) {
        T *orow = orow0 + (size_t)qrow * D;
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

}  // namespace vitx
