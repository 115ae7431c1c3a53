// softmax_topk.hip -- class softmax and device top-k of the probability rows.
#include "kernels.h"
#include "epilogue16.h"
#include "device_common.h"
#include "topk_rank.h"

namespace vitx {

// ------------------------------------------------------------------------------------------------
// Class softmax (ggml_soft_max, vit.cpp:931): max, e_i = round(expf(round(x_i - max))), p = e * (1/sum).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void softmax_kernel(const float *__restrict__ logits, float *__restrict__ probs, int cols, int ld) {
    __shared__ float red[4];
    const float *x = logits + (size_t)blockIdx.x * ld;
    float *p = probs + (size_t)blockIdx.x * cols;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float mx = -INFINITY;
    for (int i = tid; i < cols; i += 256) mx = fmaxf(mx, x[i]);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.0f;
    for (int i = tid; i < cols; i += 256) { const float e = rnd<T>(expf(rnd<T>(x[i] - mx))); p[i] = e; sum += e; }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) red[wv] = sum;
    __syncthreads();
    const float inv = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
    for (int i = tid; i < cols; i += 256) p[i] *= inv;
}
hipError_t launch_softmax(int dtype, const float *logits, float *probs, int rows, int cols, int ld, hipStream_t stream) {
    if (dtype == DT_F16) hipLaunchKernelGGL(softmax_kernel<_Float16>, dim3(rows), dim3(256), 0, stream, logits, probs, cols, ld);
    else hipLaunchKernelGGL(softmax_kernel<__bf16>, dim3(rows), dim3(256), 0, stream, logits, probs, cols, ld);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Top-k of every probability row (vit_predict's sort, vit.cpp:1043-1057): one wave per row, k selection passes; pass i takes the
// largest entry that comes after pass i - 1's in the order -- no scratch, no ties lost.
// The order is vitx_topk's (model_file.cpp): entries that are not NaN first, by probability descending then class index ascending
// (+0 and -0 tie), NaN entries last by class index ascending.  It is TOTAL: a value maps to a 32-bit rank that grows with it (0 for
// a NaN, below -inf's) and an entry to rank << 32 | ~index, so with k <= cols every pass finds an entry and every class written lies
// in [0, cols) and is written once -- also for a row of NaNs, which float comparisons alone would answer with no entry at all.
// ------------------------------------------------------------------------------------------------
// (topk_rank: topk_rank.h, shared with nn_select.hip)
__global__ __launch_bounds__(256) void topk_kernel(const float *__restrict__ probs, int rows, int cols, int k, float *__restrict__ out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *p = probs + (size_t)row * cols;
    unsigned long long prev = ~0ull;                                     // above every entry (no value has rank 0xffffffff)
    for (int it = 0; it < k; ++it) {
        unsigned long long best = 0; float bv = 0.0f;                    // 0 = none yet: an entry's low word is ~index >= 0x80000000
        for (int i = lane; i < cols; i += 64) {
            const float v = p[i];
            const unsigned long long e = ((unsigned long long)topk_rank(v) << 32) | (unsigned)~i;
            if (e < prev && e > best) { best = e; bv = v; }              // not yet taken, and ahead of this lane's best
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long oe = __shfl_xor(best, o);
            if (oe > best) best = oe;
        }
        const int bi = (int)~(unsigned)best;
        bv = __shfl(bv, bi & 63);                                        // the value as stored (sign of a zero, bits of a NaN): lane bi % 64 read it
        if (lane == 0) { out[((size_t)row * k + it) * 2] = bv; ((int *)out)[((size_t)row * k + it) * 2 + 1] = bi; }
        prev = best;
    }
}

hipError_t launch_topk(const float *probs, int rows, int cols, int k, void *out_pairs, hipStream_t stream) {
    if (rows <= 0 || cols <= 0 || k <= 0 || k > cols) return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, probs, rows, cols, k, (float *)out_pairs);
    return hipGetLastError();
}

}  // namespace vitx
