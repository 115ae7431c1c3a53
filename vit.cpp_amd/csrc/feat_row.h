// feat_row.h -- one row of F = ((X - mean) * rstd) * norm.weight + norm.bias in f32, unrounded, held by a wave: the row arithmetic features.hip
// and attention_pool.hip share (the contract: include/vitx.h "image embeddings and token features").  Column ownership follows the statistics
// helpers of device_common.h: lane l holds columns c * 256 + 4 l .. + 3 of tile c (tiled widths) or (i * 64 + l) * VEC .. of piece i (flat widths).
#pragma once
#include "device_common.h"

namespace vitx {

template <int VEC, int NV> struct FeatRow {
    static constexpr bool kTiled = VEC == 4 && NV <= LN_MAX_TILES;
    static __device__ __forceinline__ int col(int i, int lane) { return kTiled ? i * 256 + lane * 4 : (i * 64 + lane) * VEC; }
    // f[i][j] = F at column col(i) + j of the row xr
    static __device__ __forceinline__ void norm(const float *__restrict__ xr, const float *__restrict__ w, const float *__restrict__ b, float eps, int lane, float (&f)[NV][VEC]) {
        if constexpr (kTiled) {
            f32x4 v[NV];
            float mean, rstd;
            ln_tiled_stats<NV>(xr, eps, lane, v, mean, rstd);
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const f32x4 ww = *(const f32x4 *)(w + col(c, lane)), bb = *(const f32x4 *)(b + col(c, lane));
#pragma unroll
                for (int e = 0; e < 4; ++e) { float t = (v[c][e] - mean) * rstd; t = t * ww[e]; f[c][e] = t + bb[e]; }
            }
        } else {
            float scale;
            ln_flat_stats<VEC, NV>(xr, eps, lane, f, scale);         // f = x - mean
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int j = 0; j < VEC; ++j) { float t = f[i][j] * scale; t = t * w[col(i, lane) + j]; f[i][j] = t + b[col(i, lane) + j]; }
        }
    }
    // RNE to the operand type T16 (the rounding layernorm_kernel applies to the same f32 value), row zr of D elements
    template <typename T16> static __device__ __forceinline__ void store_rne(T16 *__restrict__ zr, int lane, const float (&f)[NV][VEC]) {
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int j = 0; j < VEC; ++j) zr[col(i, lane) + j] = (T16)f[i][j];
    }
    static __device__ __forceinline__ void store(float *__restrict__ yr, int lane, const float (&f)[NV][VEC]) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float *p = yr + col(i, lane);
            if constexpr (VEC == 4) *(f32x4 *)p = f32x4{f[i][0], f[i][1], f[i][2], f[i][3]};
            else if constexpr (VEC == 2) *(f32x2 *)p = f32x2{f[i][0], f[i][1]};
            else *p = f[i][0];
        }
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

}  // namespace vitx
