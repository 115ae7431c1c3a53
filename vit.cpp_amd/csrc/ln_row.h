// ln_row.h -- one LayerNorm row held by a wave: the statistics and THE output arithmetic F = ((x - mean) * rstd) * w + b of every kernel that
// normalises -- the stand-alone LayerNorm, the f32 pre-norm and the fix-up behind the LayerNorm-fusing GEMMs (layernorm.hip), the consumer-side
// fix of the ping-pong GEMM (gemm_pp.hip), the MX-encoding LayerNorm (gemm_mx8.hip), the feature kernel (features.hip) and the attention-pooling
// head (attention_pool.hip).  A row gets the same bits whichever of them produced it (-ffp-contract=off, as for every kernel of the library);
// the epilogue of the LayerNorm-fusing GEMM, which works from accumulators, follows the same definition in its own text (gemm_pp.hip).
#pragma once
#include "device_common.h"

namespace vitx {

// ------------------------------------------------------------------------------------------------
// LayerNorm statistics by 256-column tiles (ggml_norm, /root/reference/vit.cpp:808-812, 881-885): the ONE definition both the
// stand-alone kernel (layernorm.hip) and the LayerNorm fused into the residual GEMMs (gemm_pp.hip) follow, operation for operation,
// so that a row's result does not depend on which of them produced it (batch-size independence of the whole forward).
//   tile c (columns 256 c ..): the row's 256 values are 64 pieces of 4 consecutive columns; piece id = 16 w + 8 j + k
//     a(piece)  = (x0 + x1) + (x2 + x3)
//     s(w, k)   = a(w, 0, k) + a(w, 1, k)
//     P(w)      = ln_sum8 over k = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7))      -- a butterfly: every k holds the same bits
//     S_c       = ((P(0) + P(1)) + P(2)) + P(3);   mean_c = S_c / 256
//     M2_c      = the same tree over (x - mean_c)^2  (two passes inside the tile: no cancellation)
//   row: ln_combine() merges the tiles in index order (Chan et al.: equal counts): mean = (sum of mean_c) / NT,
//     M2 = sum of M2_c + 256 * sum of (mean_c - mean)^2, rstd = 1 / sqrt(M2 / D + eps);  y = ((x - mean) * rstd) * w + b.
// ggml's own order (double accumulation over the whole row) differs from this by f32 rounding only: within one operand ulp of
// oracle.layernorm (tests/test_gpu_kernels.py, test_gpu_parity_r02.py).
// ------------------------------------------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ float dpp_f32(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true)); }
// sum over the 8 lanes that share (lane >> 3); every one of them ends up with the same bits
__device__ __forceinline__ float ln_sum8(float v) {
    v = v + dpp_f32<0xB1>(v);       // quad_perm [1, 0, 3, 2]: k ^ 1
    v = v + dpp_f32<0x4E>(v);       // quad_perm [2, 3, 0, 1]: k ^ 2
    v = v + dpp_f32<0x141>(v);      // row_half_mirror: the other quad of the 8
    return v;
}
__device__ __forceinline__ float ln_piece_sum(f32x4 x) { return (x[0] + x[1]) + (x[2] + x[3]); }
__device__ __forceinline__ float ln_piece_sq(f32x4 x, float m) {
    const float d0 = x[0] - m, d1 = x[1] - m, d2 = x[2] - m, d3 = x[3] - m;
    return (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
}
constexpr int LN_MAX_TILES = 4;         // hidden sizes 256 .. 1024 take the tiled definition
__device__ __forceinline__ void ln_combine(const float (&mc)[LN_MAX_TILES], const float (&m2)[LN_MAX_TILES], int NT, int D, float eps, float &mean, float &rstd) {
    float sm = mc[0], q = m2[0];
#pragma unroll
    for (int c = 1; c < LN_MAX_TILES; ++c) if (c < NT) { sm = sm + mc[c]; q = q + m2[c]; }
    mean = sm / (float)NT;
    float dv = mc[0] - mean, w = dv * dv;
#pragma unroll
    for (int c = 1; c < LN_MAX_TILES; ++c) if (c < NT) { dv = mc[c] - mean; w = w + dv * dv; }
    rstd = 1.0f / sqrtf((q + 256.0f * w) / (float)D + eps);
}


// The values of one row of NT * 256 columns (v[c] = columns c * 256 + 4 lane ..) and their statistics, the tiled definition above: lane l holds
// piece l of each tile (w = l >> 4, j = (l >> 3) & 1, k = l & 7): one fully coalesced 1 KiB load per tile.
template <int NT>
__device__ __forceinline__ void ln_tiled_stats(const float *__restrict__ xr, float eps, int lane, f32x4 (&v)[NT], float &mean, float &rstd) {
    float mc[LN_MAX_TILES] = {0.0f, 0.0f, 0.0f, 0.0f}, m2[LN_MAX_TILES] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < NT; ++c) v[c] = *(const f32x4 *)(xr + c * 256 + lane * 4);
    auto tile_total = [&](float a) {       // a = this lane's piece value -> S_c (uniform)
        const float s = a + __shfl_xor(a, 8);                      // s(w, k) = a(w, 0, k) + a(w, 1, k)
        const float p = ln_sum8(s);                                // P(w), the same bits in the 16 lanes of wave column w
        const float p0 = __shfl(p, 0), p1 = __shfl(p, 16), p2 = __shfl(p, 32), p3 = __shfl(p, 48);
        return ((p0 + p1) + p2) + p3;
    };
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        mc[c] = tile_total(ln_piece_sum(v[c])) * (1.0f / 256.0f);
        m2[c] = tile_total(ln_piece_sq(v[c], mc[c]));
    }
    ln_combine(mc, m2, NT, NT * 256, eps, mean, rstd);
}

// Hidden sizes the tiled definition does not cover (launch_layernorm): lane l holds VEC consecutive columns idx = (i * 64 + l) * VEC of
// each of NV pieces; sum and sum of squared deviations over the whole wave.  Returns v[i][j] = x - mean and scale = 1 / sqrt(var + eps).
template <int VEC, int NV>
__device__ __forceinline__ void ln_flat_stats(const float *__restrict__ xr, float eps, int lane, float (&v)[NV][VEC], float &scale) {
    constexpr int D = 64 * VEC * NV;
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = (i * 64 + lane) * VEC;
        if constexpr (VEC == 4) { const float4 t = *(const float4 *)(xr + idx); v[i][0] = t.x; v[i][1] = t.y; v[i][2] = t.z; v[i][3] = t.w; }
        else if constexpr (VEC == 2) { const float2 t = *(const float2 *)(xr + idx); v[i][0] = t.x; v[i][1] = t.y; }
        else v[i][0] = xr[idx];
#pragma unroll
        for (int j = 0; j < VEC; ++j) sum += v[i][j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum / (float)D;
    float sum2 = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < VEC; ++j) { v[i][j] -= mean; sum2 += v[i][j] * v[i][j]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum2 += __shfl_xor(sum2, o);
    scale = 1.0f / sqrtf(sum2 / (float)D + eps);
}

// One row of D = 64 VEC NV columns (a row of VITX_LN_WIDTHS, kernels.h) by one wave.  Lane l holds columns c * 256 + 4 l .. + 3 of tile c (tiled
// widths: VEC 4, up to LN_MAX_TILES pieces) or (i * 64 + l) * VEC .. of piece i (flat widths): 16-, 8- or 4-byte loads and stores.
template <int VEC, int NV> struct LnRow {
    static constexpr bool kTiled = VEC == 4 && NV <= LN_MAX_TILES;
    static __device__ __forceinline__ int col(int i, int lane) { return kTiled ? i * 256 + lane * 4 : (i * 64 + lane) * VEC; }
    // THE output arithmetic, the only place it is written: sink(i, idx, o) for every piece i in turn, idx = col(i), o[j] = F at column idx + j of the
    // row xr, f32, unrounded.  The whole row is read (its statistics) before the first call, so a sink may store over xr; a sink that stores its
    // piece at once keeps one piece of F live, not the row (the widest one-wave-per-row kernels lose an occupancy step otherwise).
    template <typename S>
    static __device__ __forceinline__ void each(const float *__restrict__ xr, const float *__restrict__ w, const float *__restrict__ b, float eps, int lane, S &&sink) {
        if constexpr (kTiled) {
            f32x4 v[NV];
            float mean, rstd;
            ln_tiled_stats<NV>(xr, eps, lane, v, mean, rstd);
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const int idx = col(c, lane);
                const f32x4 ww = *(const f32x4 *)(w + idx), bb = *(const f32x4 *)(b + idx);
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) { float t = (v[c][e] - mean) * rstd; t = t * ww[e]; o[e] = t + bb[e]; }
                sink(c, idx, o);
            }
        } else {
            float v[NV][VEC];                                        // x - mean
            float scale;
            ln_flat_stats<VEC, NV>(xr, eps, lane, v, scale);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int idx = col(i, lane);
                float o[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) { float t = v[i][j] * scale; t = t * w[idx + j]; o[j] = t + b[idx + j]; }
                sink(i, idx, o);
            }
        }
    }
    // the whole row in registers: f[i][j] = F at column col(i) + j
    static __device__ __forceinline__ void norm(const float *__restrict__ xr, const float *__restrict__ w, const float *__restrict__ b, float eps, int lane, float (&f)[NV][VEC]) {
        each(xr, w, b, eps, lane, [&](int i, int, const float (&o)[VEC]) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) f[i][j] = o[j];
        });
    }
    // RNE to the operand type T (the bits of a (T) cast, two values per convert): one store per piece (put_rne), row zr of D elements (store_rne)
    template <typename T> static __device__ __forceinline__ void put_rne(T *__restrict__ p, const float (&o)[VEC]) {
        if constexpr (VEC == 4) {
            const typename Pair<T>::v2 lo = round_pair<T>(o[0], o[1]), hi = round_pair<T>(o[2], o[3]);
            *(typename Elem<T>::v4 *)p = typename Elem<T>::v4{lo[0], lo[1], hi[0], hi[1]};
        } else if constexpr (VEC == 2) *(typename Pair<T>::v2 *)p = round_pair<T>(o[0], o[1]);
        else *p = (T)o[0];
    }
    template <typename T> static __device__ __forceinline__ void store_rne(T *__restrict__ zr, int lane, const float (&f)[NV][VEC]) {
#pragma unroll
        for (int i = 0; i < NV; ++i) put_rne(zr + col(i, lane), f[i]);
    }
    // the same in f32, as it is
    static __device__ __forceinline__ void put(float *p, const float (&o)[VEC]) {
        if constexpr (VEC == 4) *(f32x4 *)p = f32x4{o[0], o[1], o[2], o[3]};
        else if constexpr (VEC == 2) *(f32x2 *)p = f32x2{o[0], o[1]};
        else *p = o[0];
    }
    static __device__ __forceinline__ void store(float *__restrict__ yr, int lane, const float (&f)[NV][VEC]) {
#pragma unroll
        for (int i = 0; i < NV; ++i) put(yr + col(i, lane), f[i]);
    }
    // VITX_FEAT_L2: f / sqrt(sum of squares), both in f32 (per-lane sums in column order, then a butterfly: the same bits in every lane);
    // an all-zero vector stays zero
    static __device__ __forceinline__ void l2(float (&f)[NV][VEC]) {
        float ss = 0.0f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int j = 0; j < VEC; ++j) ss += f[i][j] * f[i][j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
        const float nrm = sqrtf(ss);
        if (nrm > 0.0f) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int j = 0; j < VEC; ++j) f[i][j] = f[i][j] / nrm;
        }
    }
};

// One tiled row rounded to the operand type: layernorm_fixup_kernel (layernorm.hip) and the prologue of a GEMM that consumes rows a
// LayerNorm-fusing GEMM left to the fix-up (gemm_pp.hip).  The store address is spelled col(c), not the sink's idx: the same value, but with
// this spelling hipcc emits the ping-pong GEMM instruction for instruction as it did when this function held its own copy of the loop.
template <typename T, int NT>
__device__ __forceinline__ void ln_row_tiled(const float *__restrict__ xr, const float *__restrict__ w, const float *__restrict__ b, T *__restrict__ yr, float eps, int lane) {
    typedef LnRow<4, NT> R;
    R::each(xr, w, b, eps, lane, [&](int c, int, const float (&o)[4]) { R::put_rne(yr + R::col(c, lane), o); });
}

}  // namespace vitx
