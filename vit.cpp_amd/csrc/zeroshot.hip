// zeroshot.hip -- zero-shot classification against a bank of class (text) embeddings (vitx_zeroshot_set, vitx_op_zeroshot; the contract:
// include/vitx.h "zero-shot classification").  Two small kernels around the bank GEMM, which is the GEMM dispatcher's (gemm.hip):
//   zs_embed_kernel   z [n][E] f32 (row stride given) -> a [M_pad][E] in the operand type: a = RNE(z / sqrt(sum z^2)), an all-zero row stays zero,
//                     rows n .. M_pad are written as zeros (the GEMM multiplies whole row tiles);
//   zs_score_kernel   acc [n][ld] f32 (the GEMM's output, columns K .. ld never read) -> logits = acc * scale + bias, probs = softmax over
//                     the K classes or the sigmoid of every logit.
// No atomics, nothing depends on the batch: an image's bits are a function of its own row, E, K and the bank only.  Division and square root
// are IEEE, nothing is contracted (-ffp-contract=off, as for every kernel of the library).
#include "device_common.h"
#include "kernels.h"

namespace vitx {

namespace {

// One wave per row, four rows per workgroup.  Lane l owns the 16-byte pieces l, l + 64, ... of the row: the sum of squares is taken per lane in
// ascending column order, then over the lanes by a butterfly (the same bits in every lane) -- an order that depends on E only.  The rule is
// VITX_FEAT_L2's (LnRow::l2, ln_row.h); that one walks the LayerNorm tables' column ownership and exists only for their widths, this one
// takes any E that is a multiple of 64 (a CLIP projection width need not be a hidden size), so the two stay separate functions.
// (T16 = float: the same rule with the quotient stored as it is -- VITX_TEXT_L2 of a text context, launch_zs_embed_f32)
template <typename T16> struct ZsVec { typedef typename Elem<T16>::v4 v4; };
template <> struct ZsVec<float> { typedef f32x4 v4; };
// (Tin = the type z is read in: float, or -- launch_zs_embed_operand -- an operand type, every element widened to f32 as it is loaded)
template <typename Tin> __device__ __forceinline__ f32x4 zs_load4(const Tin *p) {
    if constexpr (std::is_same<Tin, float>::value) return *(const f32x4 *)p;
    else { const typename Elem<Tin>::v4 x = *(const typename Elem<Tin>::v4 *)p; return f32x4{(float)x[0], (float)x[1], (float)x[2], (float)x[3]}; }
}
template <typename T16, typename Tin = float>
__global__ __launch_bounds__(256) void zs_embed_kernel(const Tin *__restrict__ z, long z_stride, T16 *__restrict__ a, int n, int m_pad, int E) {
    typedef typename ZsVec<T16>::v4 v4;
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m_pad) return;
    T16 *ar = a + (size_t)row * E;
    const int nv = E >> 2;
    if (row >= n) {
        for (int v = lane; v < nv; v += 64) *(v4 *)(ar + 4 * v) = v4{(T16)0.0f, (T16)0.0f, (T16)0.0f, (T16)0.0f};
        return;
    }
    const Tin *zr = z + (size_t)row * z_stride;
    float ss = 0.0f;
    for (int v = lane; v < nv; v += 64) {
        const f32x4 x = zs_load4(zr + 4 * v);
#pragma unroll
        for (int e = 0; e < 4; ++e) ss += x[e] * x[e];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float nrm = sqrtf(ss);
    for (int v = lane; v < nv; v += 64) {
        f32x4 x = zs_load4(zr + 4 * v);       // the row again: it is a few KiB and still in the cache
        if (nrm > 0.0f) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = x[e] / nrm;
        }
        *(v4 *)(ar + 4 * v) = v4{(T16)x[0], (T16)x[1], (T16)x[2], (T16)x[3]};
    }
}

// the workgroup's maximum / sum of one value per thread: a butterfly inside every wave, then the four waves' results in wave order
__device__ __forceinline__ float zs_block_max(float v, float *red, int lane, int wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();                       // the previous reduction's reads of red[] are over
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float zs_block_sum(float v, float *red, int lane, int wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per image; thread t owns the classes t, t + 256, ... (a thread only ever re-reads what it wrote itself).
//   every kind:  l_k = acc_k * scale + bias (one multiply, one add) -> logits
//   softmax:     two reduction passes over the row -- the maximum, then e_k = expf(l_k - max) and its sum (per thread in ascending class order, then
//                zs_block_sum: an order that depends on K only) -- and the normalising write p_k = e_k / sum
//   sigmoid:     p = 1 / (1 + expf(-l)) for l <= 0, 1 - 1 / (1 + expf(l)) for l > 0: the same function; the second form keeps the bits just below 1
//                that the first loses when 1 + expf(-l) rounds to 1
__global__ __launch_bounds__(256) void zs_score_kernel(const float *__restrict__ acc, int ld, float *__restrict__ probs, float *__restrict__ logits, long out_img_stride,
                                                       int K, int kind, float scale, float bias) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *c = acc + (size_t)blockIdx.x * ld;
    float *p = probs + (size_t)blockIdx.x * out_img_stride, *lg = logits + (size_t)blockIdx.x * out_img_stride;
    if (kind == VITX_ZS_SIGMOID) {
        for (int k = tid; k < K; k += 256) {
            float l = c[k] * scale; l = l + bias;
            lg[k] = l;
            p[k] = l > 0.0f ? 1.0f - 1.0f / (1.0f + expf(l)) : 1.0f / (1.0f + expf(-l));
        }
        return;
    }
    float mx = -INFINITY;
    for (int k = tid; k < K; k += 256) {
        float l = c[k] * scale; l = l + bias;
        lg[k] = l;
        mx = fmaxf(mx, l);
    }
    mx = zs_block_max(mx, red, lane, wave);
    float sum = 0.0f;
    for (int k = tid; k < K; k += 256) { const float e = expf(lg[k] - mx); p[k] = e; sum += e; }
    sum = zs_block_sum(sum, red, lane, wave);
    for (int k = tid; k < K; k += 256) p[k] = p[k] / sum;
}

}  // namespace

hipError_t launch_zs_embed(int dtype, const float *z, long z_stride, void *a, int n, int m_pad, int E, hipStream_t stream) {
    if (n <= 0 || m_pad < n || E <= 0 || E % 64 || z_stride < E || z_stride % 4) return hipErrorInvalidValue;
    const dim3 grid((m_pad + 3) / 4), blk(256);
    if (dtype == DT_F16) hipLaunchKernelGGL(zs_embed_kernel<_Float16>, grid, blk, 0, stream, z, z_stride, (_Float16 *)a, n, m_pad, E);
    else hipLaunchKernelGGL(zs_embed_kernel<__bf16>, grid, blk, 0, stream, z, z_stride, (__bf16 *)a, n, m_pad, E);
    return hipGetLastError();
}

hipError_t launch_zs_embed_operand(int dtype, const void *z, long z_stride, void *a, int n, int m_pad, int E, hipStream_t stream) {
    if (n <= 0 || m_pad < n || E <= 0 || E % 64 || z_stride < E || z_stride % 4 || z == a) return hipErrorInvalidValue;
    const dim3 grid((m_pad + 3) / 4), blk(256);
    if (dtype == DT_F16) hipLaunchKernelGGL((zs_embed_kernel<_Float16, _Float16>), grid, blk, 0, stream, (const _Float16 *)z, z_stride, (_Float16 *)a, n, m_pad, E);
    else hipLaunchKernelGGL((zs_embed_kernel<__bf16, __bf16>), grid, blk, 0, stream, (const __bf16 *)z, z_stride, (__bf16 *)a, n, m_pad, E);
    return hipGetLastError();
}

hipError_t launch_zs_embed_f32(const float *z, long z_stride, float *a, int n, int E, hipStream_t stream) {
    if (n <= 0 || E <= 0 || E % 64 || z_stride < E || z_stride % 4 || (const void *)z == (const void *)a) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zs_embed_kernel<float>, dim3((n + 3) / 4), dim3(256), 0, stream, z, z_stride, a, n, n, E);
    return hipGetLastError();
}

hipError_t launch_zs_score(const float *acc, int ld, float *probs, float *logits, long out_img_stride, int n, int K, int kind, float scale, float bias, hipStream_t stream) {
    if (n <= 0 || K <= 0 || ld < K || out_img_stride < K || (kind != VITX_ZS_SOFTMAX && kind != VITX_ZS_SIGMOID)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zs_score_kernel, dim3(n), dim3(256), 0, stream, acc, ld, probs, logits, out_img_stride, K, kind, scale, bias);
    return hipGetLastError();
}

}  // namespace vitx
