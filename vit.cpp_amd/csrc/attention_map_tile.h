// attention_map_tile.h -- the bodies of the four attention-map kernels (attention_map.hip), as functions of ONE image's own base pointers and its
// own token count N, in the manner of dense_tile.h and depth_tile.h: the fixed-shape kernels (every image of a launch has the launch's N) and the
// packed kernels (image i of a pack has N_i = row0[i + 1] - row0[i]) run the same bodies and differ in how a workgroup finds its image and its
// piece of it, never in what it computes there.
//   map_cls_item        class-token row A_h[0][0..N) of one head: one query row against N keys, bound by reading K: VALU f32 FMAs on 16-byte loads,
//                       the raw scores parked in the output row itself;
//   map_head_mean_block mean_h A_h (or 0.5 mean_h A_h + 0.5 I, the rollout factor) for a block of 16 query rows: S = Q K^T on v_mfma_f32_16x16x32
//                       (parity mode: hi.hi + (hi.lo + lo.hi) / 2048), every score and the head mean in registers;
//   rollout_step_block  16 rows of R_l = A^_l R_(l-1) on v_mfma_f32_16x16x4_f32 (exact f32), in place over A^_l: the rows go to LDS before any is written;
//   rollout_row_image   the last factor: row 0 of A^_(L-1) R_(L-2) from the last layer's class-token maps (a GEMV).
// NT (N <= 64 NT) sizes the register tiles of the head mean and the LDS pitch of the step.  No bit depends on it: key tiles beyond N are skipped
// or masked to -inf and add exact zeros behind the row's own terms, the step's k loop ends at N rounded up to 4 (zeros in LDS, zeros for r), never at
// the pitch -- so a pack may take NT from its widest image.  All four are called by all 256 lanes of a workgroup with workgroup-uniform arguments
// (they hold barriers).  No atomics; one writer per element; nothing outside the image's own outputs is written.
#pragma once
#include <math.h>

#include "device_common.h"
#include "kernels.h"

namespace vitx {

// 8 consecutive operands -> f32 (PLANES: value = hi + lo / 2048 from the F16 parity mode's two planes, lo_off elements apart)
template <typename T, bool PLANES>
__device__ __forceinline__ void map_load8(const T *ptr, long lo_off, float (&f)[8]) {
    typedef typename Elem<T>::v8 v8;
    const v8 a = *(const v8 *)ptr;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)a[e];
    if (PLANES) {
        const v8 l = *(const v8 *)(ptr + lo_off);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = __builtin_fmaf((float)l[e], kHiLoInv, f[e]);
    }
}

// ------------------------------------------------------------------------------------------------
// Class-token map of one (image, head).  img: the image's first QKV row ([N][3 D]); o: the head's output row [N].  A row of the head's k slice is
// NP = hd / 8 pieces of 16 bytes; lanes are grouped NPP (NP rounded up to a power of two) per row, lanes p >= NP idle, 64 / NPP rows per wave and step.
//   pass 1: s_j = (q . k_j) * scale -> o[j] (by the group's lane 0), running maximum;
//   pass 2: the same lane rewrites o[j] = expf(s_j - max) and sums;  pass 3: o[j] /= sum.
// Each o[j] is written and re-read by one thread only: program order is the only ordering needed.
// ------------------------------------------------------------------------------------------------
template <typename T, int NPP, bool PLANES>
__device__ __forceinline__ void map_cls_item(const T *__restrict__ img, long lo_off, float *__restrict__ o, int N, int D, int h, int hd, int NP, float scale) {
    __shared__ float red[8];
    constexpr int G = 64 / NPP;
    const int tid = threadIdx.x, lane = tid & 63, p = lane % NPP, g = lane / NPP, wave = tid >> 6;
    const size_t row_el = (size_t)3 * D;
    const bool act = p < NP;
    const T *qp = img + (size_t)h * hd + p * 8;                                // this lane's piece of q of token 0; k at + D
    float q[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (act) map_load8<T, PLANES>(qp, lo_off, q);
    float mx = -INFINITY;
    for (int r0 = wave * G; r0 < N; r0 += 4 * G) {
        const int r = r0 + g;
        float k[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (act && r < N) map_load8<T, PLANES>(qp + D + (size_t)r * row_el, lo_off, k);
        float s = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s = __builtin_fmaf(q[e], k[e], s);
#pragma unroll
        for (int m = 1; m < NPP; m <<= 1) s += __shfl_xor(s, m);
        s *= scale;
        if (r < N) { mx = fmaxf(mx, s); if (p == 0) o[r] = s; }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.0f;
    if (p == 0)
        for (int r = wave * G + g; r < N; r += 4 * G) { const float e = expf(o[r] - mx); o[r] = e; sum += e; }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) sum += __shfl_xor(sum, m);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    sum = (red[4] + red[5]) + (red[6] + red[7]);
    if (p == 0)
        for (int r = wave * G + g; r < N; r += 4 * G) o[r] = o[r] / sum;
}

// ------------------------------------------------------------------------------------------------
// Head mean of the softmax rows of the 16 queries q0 .. q0 + 15 of one image.  img: its first QKV row; ob: its [N][N] output.  Per head: wave w
// owns the key tiles t * 4 + w (16 keys each); S tile = mfma_16x16x32(A = Q[16 queries][32 dims], B = K^T[32 dims][16 keys]) over hd / 32 dim chunks
// (dims beyond hd and keys beyond N are zeros), so lane l holds keys 16 tile + (l & 15) of queries 4 (l >> 4) + r, r = 0..3 (C/D map).
// Row maxima and sums: shuffles over the 16 lanes of a query group, then the four waves through LDS.  The f32 probabilities are added to
// per-lane accumulators that keep their (query, key) slots over all heads; out = acc / H (+ the rollout's 0.5 I when `half_identity`).
// NT = key tiles per wave (N <= 64 NT).
// ------------------------------------------------------------------------------------------------
template <typename T, int NT, bool PLANES>
__device__ __forceinline__ void map_head_mean_block(const T *__restrict__ img, long lo_off, float *__restrict__ ob, int N, int D, int H, int q0, float scale,
                                                    int half_identity) {
    typedef typename Elem<T>::v8 v8;
    __shared__ float red[2][4][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int hd = D / H, nchunk = (hd + 31) / 32;
    const size_t row_el = (size_t)3 * D;
    const v8 zero8 = {};
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int qrow = q0 + l15;                                   // the query this lane feeds into the A operand
    for (int h = 0; h < H; ++h) {
        f32x4 sc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) sc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = 0; c < nchunk; ++c) {
            const int d = c * 32 + l4 * 8;                       // this lane's 8 dims of the chunk
            const bool din = d < hd;
            const size_t col = (size_t)h * hd + d;
            v8 qh = zero8, ql = zero8;
            if (din && qrow < N) {
                qh = *(const v8 *)(img + (size_t)qrow * row_el + col);
                if (PLANES) ql = *(const v8 *)(img + (size_t)qrow * row_el + col + lo_off);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if ((t * 4 + wave) * 16 >= N) continue;           // a whole tile beyond the keys (wave-uniform): its scores stay masked
                const int key = (t * 4 + wave) * 16 + l15;
                v8 kh = zero8, kl = zero8;
                if (din && key < N) {
                    kh = *(const v8 *)(img + (size_t)key * row_el + D + col);
                    if (PLANES) kl = *(const v8 *)(img + (size_t)key * row_el + D + col + lo_off);
                }
                sc[t] = Elem<T>::mfma16(qh, kh, sc[t]);
                if (PLANES) {
                    f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
                    x = Elem<T>::mfma16(qh, kl, x);
                    x = Elem<T>::mfma16(ql, kh, x);
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[t][r] = __builtin_fmaf(x[r], kHiLoInv, sc[t][r]);
                }
            }
        }
        // scale, mask, row maxima
        float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bool kin = (t * 4 + wave) * 16 + l15 < N;
#pragma unroll
            for (int r = 0; r < 4; ++r) { sc[t][r] = kin ? sc[t][r] * scale : -INFINITY; mx[r] = fmaxf(mx[r], sc[t][r]); }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], m));
        }
        if (l15 == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) red[0][wave][l4 * 4 + r] = mx[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int qi = l4 * 4 + r; mx[r] = fmaxf(fmaxf(red[0][0][qi], red[0][1][qi]), fmaxf(red[0][2][qi], red[0][3][qi])); }
        float sm[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { sc[t][r] = expf(sc[t][r] - mx[r]); sm[r] += sc[t][r]; }     // a masked key: expf(-inf) = 0
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) sm[r] += __shfl_xor(sm[r], m);
        }
        if (l15 == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) red[1][wave][l4 * 4 + r] = sm[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int qi = l4 * 4 + r; sm[r] = (red[1][0][qi] + red[1][1][qi]) + (red[1][2][qi] + red[1][3][qi]); }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] += sc[t][r] / sm[r];
        }
        __syncthreads();                                         // red[] is rewritten by the next head
    }
    const float inv_h = 1.0f / (float)H;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int key = (t * 4 + wave) * 16 + l15;
        if (key >= N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = q0 + l4 * 4 + r;
            if (qi >= N) continue;
            float v = acc[t][r] * inv_h;
            if (half_identity) v = 0.5f * v + (qi == key ? 0.5f : 0.0f);
            ob[(size_t)qi * N + key] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Rollout step, in place, for the 16 rows i0 .. i0 + 15 of one image: ab <- ab . rb ([N][N] f32 each).  The block's 16 rows of a go to LDS first
// (zeros beyond N), then each wave computes 64-column groups of the product: four 16x16 tiles with independent accumulators on
// mfma_f32_16x16x4_f32 (A[i = l & 15][k = l >> 4] from LDS, B[k = l >> 4][j = l & 15] from r), written back over the rows it read.  No other
// workgroup touches these rows of a, and r is another buffer.  NT: N <= 64 NT, the LDS pitch.
// ------------------------------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ void rollout_step_block(float *__restrict__ ab, const float *__restrict__ rb, int N, int i0) {
    constexpr int NPAD = 64 * NT;
    __shared__ float as[16][NPAD + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    for (int e = tid; e < 16 * NPAD; e += 256) {
        const int i = e / NPAD, k = e - i * NPAD;
        as[i][k] = (i0 + i < N && k < N) ? ab[(size_t)(i0 + i) * N + k] : 0.0f;
    }
    __syncthreads();
    const int kend = (N + 3) / 4 * 4;
    for (int j0 = wave * 64; j0 < N; j0 += 256) {
        f32x4 c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int k0 = 0; k0 < kend; k0 += 4) {
            const int k = k0 + l4;
            const float av = as[l15][k];
            const float *rr = rb + (size_t)k * N;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u * 16 + l15;
                const float bv = (k < N && j < N) ? rr[j] : 0.0f;
                c[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, c[u], 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * 16 + l15;
            if (j >= N) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + l4 * 4 + q;
                if (i < N) ab[(size_t)i * N + j] = c[u][q];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Last rollout factor of one image: ob[k] = sum_j w_j rb[j][k] with w_j = 0.5 mean_h cb[h][j] + 0.5 [j == 0] (row 0 of A^_(L-1)); rb == nullptr
// (a one-layer model): ob = w.  w in LDS (N <= 1024), thread k walks column k (coalesced rows of r).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rollout_row_image(const float *__restrict__ cb, const float *__restrict__ rb, float *__restrict__ ob, int N, int H) {
    __shared__ float w[1024];
    const float inv_h = 1.0f / (float)H;
    for (int j = threadIdx.x; j < N; j += 256) {
        float s = 0.0f;
        for (int h = 0; h < H; ++h) s += cb[(size_t)h * N + j];
        w[j] = 0.5f * (s * inv_h) + (j == 0 ? 0.5f : 0.0f);
    }
    __syncthreads();
    if (!rb) { for (int k = threadIdx.x; k < N; k += 256) ob[k] = w[k]; return; }
    for (int k = threadIdx.x; k < N; k += 256) {
        float s = 0.0f;
        for (int j = 0; j < N; ++j) s = __builtin_fmaf(w[j], rb[(size_t)j * N + k], s);
        ob[k] = s;
    }
}

// The image of workgroup `wg` in a running block count blk0 [n + 1] (blk0[lo] <= wg < blk0[lo + 1]): every load has a uniform address and is a
// scalar load (attention_packed.hip's search)
__device__ __forceinline__ int map_find_image(const int *__restrict__ blk0, int n, int wg) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk0[mid] <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace vitx
