// attention_map.hip -- attention maps and attention rollout (vitx_attn_enable, vitx_op_attention_map).
//
// Opt-in outputs of the forward: what the model looked at.  The kernels only READ the QKV scratch a layer's qkv projection wrote
// ([n_img * N][3 D] in the operand type; q of head h at column h * hd, k at D + h * hd) and write buffers of their own, so the
// forward's own results do not change.  Semantics (include/vitx.h): the maps are f32 softmaxes of the context's own q, k --
// s = (q . k) / sqrt(hd) in f32, A = expf(s - max) / sum -- not the rounded numerators the attention kernels multiply v with.
//   attn_cls_map_kernel    class-token row A_h[0][0..N) of every head: one query row against N keys, bound by reading K: VALU f32 FMAs on
//                          16-byte loads, one workgroup per (image, head), the raw scores parked in the output row itself;
//   attn_head_mean_kernel  mean_h A_h (or 0.5 mean_h A_h + 0.5 I, the rollout factor) for a block of 16 query rows: S = Q K^T on
//                          v_mfma_f32_16x16x32 (parity mode: hi.hi + (hi.lo + lo.hi) / 2048), every score and the head mean in registers;
//   attn_rollout_step_kernel  R_l = A^_l R_(l-1) on v_mfma_f32_16x16x4_f32 (exact f32), in place over A^_l: a workgroup owns a block of
//                          16 rows of A^_l and reads all of them into LDS before it writes any of them;
//   attn_rollout_row_kernel   the last factor: row 0 of A^_(L-1) R_(L-2) from the last layer's class-token maps (a GEMV).
#include <hip/hip_runtime.h>
#include <math.h>

#include "device_common.h"
#include "kernels.h"

namespace vitx {
namespace {

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
// Class-token map.  One workgroup of four waves per (image, head).  A row of the head's k slice is NP = hd / 8 pieces of 16 bytes; lanes are
// grouped NPP (NP rounded up to a power of two) per row, lanes p >= NP idle, 64 / NPP rows per wave and step.
//   pass 1: s_j = (q . k_j) * scale -> out[j] (by the group's lane 0), running maximum;
//   pass 2: the same lane rewrites out[j] = expf(s_j - max) and sums;  pass 3: out[j] /= sum.
// Each out[j] is written and re-read by one thread only: program order is the only ordering needed.
// out row of head h of image b: out + b * img_stride + h * N.
// ------------------------------------------------------------------------------------------------
template <typename T, int NPP, bool PLANES>
__global__ __launch_bounds__(256) void attn_cls_map_kernel(const T *__restrict__ qkv, long lo_off, float *__restrict__ out, long img_stride,
                                                          int N, int D, int H, int NP, float scale) {
    __shared__ float red[8];
    constexpr int G = 64 / NPP;
    const int tid = threadIdx.x, lane = tid & 63, p = lane % NPP, g = lane / NPP, wave = tid >> 6;
    const int item = blockIdx.x, b = item / H, h = item - b * H;
    const int hd = D / H;
    const size_t row_el = (size_t)3 * D;
    const bool act = p < NP;
    const T *qp = qkv + (size_t)b * N * row_el + (size_t)h * hd + p * 8;      // this lane's piece of q of token 0; k at + D
    float *o = out + (size_t)b * img_stride + (size_t)h * N;
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
// Head mean of the softmax rows of 16 queries.  One workgroup of four waves per (image, 16-row query block).  Per head: wave w owns the
// key tiles t * 4 + w (16 keys each); S tile = mfma_16x16x32(A = Q[16 queries][32 dims], B = K^T[32 dims][16 keys]) over hd / 32 dim chunks
// (dims beyond hd and keys beyond N are zeros), so lane l holds keys 16 tile + (l & 15) of queries 4 (l >> 4) + r, r = 0..3 (C/D map).
// Row maxima and sums: shuffles over the 16 lanes of a query group, then the four waves through LDS.  The f32 probabilities are added to
// per-lane accumulators that keep their (query, key) slots over all heads; out = acc / H (+ the rollout's 0.5 I when `half_identity`).
// NT = key tiles per wave (N <= 64 NT).
// ------------------------------------------------------------------------------------------------
template <typename T, int NT, bool PLANES>
__global__ __launch_bounds__(256) void attn_head_mean_kernel(const T *__restrict__ qkv, long lo_off, float *__restrict__ out, int N, int D, int H,
                                                            float scale, int half_identity) {
    typedef typename Elem<T>::v8 v8;
    __shared__ float red[2][4][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int qblocks = (N + 15) / 16;
    const int b = blockIdx.x / qblocks, q0 = (blockIdx.x - b * qblocks) * 16;
    const int hd = D / H, nchunk = (hd + 31) / 32;
    const size_t row_el = (size_t)3 * D;
    const T *img = qkv + (size_t)b * N * row_el;
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
    float *ob = out + (size_t)b * N * N;
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
// Rollout step, in place: a[b] <- a[b] . r[b] ([N][N] f32 each).  One workgroup of four waves per (image, 16-row block of a).  The block's
// 16 rows of a go to LDS first (zeros beyond N), then each wave computes 64-column groups of the product: four 16x16 tiles with independent
// accumulators on mfma_f32_16x16x4_f32 (A[i = l & 15][k = l >> 4] from LDS, B[k = l >> 4][j = l & 15] from r), written back over the rows
// it read.  No other workgroup touches these rows of a, and r is another buffer.  NT: N <= 64 NT.
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(256) void attn_rollout_step_kernel(float *__restrict__ a, const float *__restrict__ r, int N) {
    constexpr int NPAD = 64 * NT;
    __shared__ float as[16][NPAD + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int rblocks = (N + 15) / 16;
    const int b = blockIdx.x / rblocks, i0 = (blockIdx.x - b * rblocks) * 16;
    float *ab = a + (size_t)b * N * N;
    const float *rb = r + (size_t)b * N * N;
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
// Last rollout factor: out[b][k] = sum_j w_j r[b][j][k] with w_j = 0.5 mean_h cls[b][h][j] + 0.5 [j == 0] (row 0 of A^_(L-1)); r == nullptr
// (a one-layer model): out = w.  One workgroup per image; w in LDS (N <= 1024), thread k walks column k (coalesced rows of r).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_rollout_row_kernel(const float *__restrict__ cls, long cls_stride, const float *__restrict__ r,
                                                              float *__restrict__ out, long out_stride, int N, int H) {
    __shared__ float w[1024];
    const int b = blockIdx.x;
    const float *cb = cls + (size_t)b * cls_stride;
    const float inv_h = 1.0f / (float)H;
    for (int j = threadIdx.x; j < N; j += 256) {
        float s = 0.0f;
        for (int h = 0; h < H; ++h) s += cb[(size_t)h * N + j];
        w[j] = 0.5f * (s * inv_h) + (j == 0 ? 0.5f : 0.0f);
    }
    __syncthreads();
    float *ob = out + (size_t)b * out_stride;
    if (!r) { for (int k = threadIdx.x; k < N; k += 256) ob[k] = w[k]; return; }
    const float *rb = r + (size_t)b * N * N;
    for (int k = threadIdx.x; k < N; k += 256) {
        float s = 0.0f;
        for (int j = 0; j < N; ++j) s = __builtin_fmaf(w[j], rb[(size_t)j * N + k], s);
        ob[k] = s;
    }
}

template <typename T, bool PLANES>
hipError_t launch_cls_map_t(const void *qkv, long lo_off, float *out, long img_stride, int n_img, int N, int D, int H, hipStream_t st) {
    const int np = D / H / 8;
    const float scale = 1.0f / sqrtf((float)(D / H));
    const dim3 grid((unsigned)((size_t)n_img * H)), blk(256);
#define VITX_MAPC(NPP) hipLaunchKernelGGL((attn_cls_map_kernel<T, NPP, PLANES>), grid, blk, 0, st, (const T *)qkv, lo_off, out, img_stride, N, D, H, np, scale)
    if (np <= 1) VITX_MAPC(1);
    else if (np <= 2) VITX_MAPC(2);
    else if (np <= 4) VITX_MAPC(4);
    else if (np <= 8) VITX_MAPC(8);
    else VITX_MAPC(16);
#undef VITX_MAPC
    return hipGetLastError();
}

template <typename T, bool PLANES>
hipError_t launch_head_mean_t(const void *qkv, long lo_off, float *out, int n_img, int N, int D, int H, bool half_identity, hipStream_t st) {
    const float scale = 1.0f / sqrtf((float)(D / H));
    const dim3 grid((unsigned)((size_t)n_img * ((N + 15) / 16))), blk(256);
    const int nt = (N + 63) / 64;
#define VITX_MAPM(NT) hipLaunchKernelGGL((attn_head_mean_kernel<T, NT, PLANES>), grid, blk, 0, st, (const T *)qkv, lo_off, out, N, D, H, scale, half_identity ? 1 : 0)
    if (nt <= 1) VITX_MAPM(1);
    else if (nt <= 2) VITX_MAPM(2);
    else if (nt <= 4) VITX_MAPM(4);
    else if (nt <= 8) VITX_MAPM(8);
    else VITX_MAPM(16);
#undef VITX_MAPM
    return hipGetLastError();
}

}  // namespace

bool attention_map_supports(int N, int D, int H) { return H > 0 && D % H == 0 && (D / H) % 8 == 0 && D / H <= 128 && N > 0; }
bool attention_mean_supports(int N, int D, int H) { return attention_map_supports(N, D, H) && N <= kAttnMeanMaxTokens; }

hipError_t launch_attention_cls_map(int dtype, const void *qkv, long lo_off, float *out, long img_stride, int n_img, int N, int D, int H, hipStream_t st) {
    if (!attention_map_supports(N, D, H) || n_img <= 0 || (lo_off && dtype != DT_F16)) return hipErrorInvalidValue;
    if (dtype == DT_F16) return lo_off ? launch_cls_map_t<_Float16, true>(qkv, lo_off, out, img_stride, n_img, N, D, H, st)
                                       : launch_cls_map_t<_Float16, false>(qkv, 0, out, img_stride, n_img, N, D, H, st);
    return launch_cls_map_t<__bf16, false>(qkv, 0, out, img_stride, n_img, N, D, H, st);
}

hipError_t launch_attention_head_mean(int dtype, const void *qkv, long lo_off, float *out, int n_img, int N, int D, int H, bool half_identity, hipStream_t st) {
    if (!attention_mean_supports(N, D, H) || n_img <= 0 || (lo_off && dtype != DT_F16)) return hipErrorInvalidValue;
    if (dtype == DT_F16) return lo_off ? launch_head_mean_t<_Float16, true>(qkv, lo_off, out, n_img, N, D, H, half_identity, st)
                                       : launch_head_mean_t<_Float16, false>(qkv, 0, out, n_img, N, D, H, half_identity, st);
    return launch_head_mean_t<__bf16, false>(qkv, 0, out, n_img, N, D, H, half_identity, st);
}

hipError_t launch_rollout_step(float *a, const float *r, int n_img, int N, hipStream_t st) {
    if (n_img <= 0 || N <= 0 || N > kAttnMeanMaxTokens) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((size_t)n_img * ((N + 15) / 16))), blk(256);
    const int nt = (N + 63) / 64;
    if (nt <= 1) hipLaunchKernelGGL((attn_rollout_step_kernel<1>), grid, blk, 0, st, a, r, N);
    else if (nt <= 2) hipLaunchKernelGGL((attn_rollout_step_kernel<2>), grid, blk, 0, st, a, r, N);
    else if (nt <= 4) hipLaunchKernelGGL((attn_rollout_step_kernel<4>), grid, blk, 0, st, a, r, N);
    else if (nt <= 8) hipLaunchKernelGGL((attn_rollout_step_kernel<8>), grid, blk, 0, st, a, r, N);
    else hipLaunchKernelGGL((attn_rollout_step_kernel<16>), grid, blk, 0, st, a, r, N);
    return hipGetLastError();
}

hipError_t launch_rollout_row(const float *cls, long cls_stride, const float *r, float *out, long out_stride, int n_img, int N, int H, hipStream_t st) {
    if (n_img <= 0 || N <= 0 || N > kAttnMeanMaxTokens || H <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attn_rollout_row_kernel, dim3((unsigned)n_img), dim3(256), 0, st, cls, cls_stride, r, out, out_stride, N, H);
    return hipGetLastError();
}

}  // namespace vitx
