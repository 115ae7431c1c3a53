// attention_packed.hip -- attention over a PACK of images of different token counts laid end to end (include/vitx.h "packed batches"):
// qkv [rows][3 D] -> out [rows][D], image i = rows row0[i] .. row0[i + 1] - 1, any N_i = row0[i + 1] - row0[i] >= 1.
// The arithmetic is attention_generic_kernel's, operation for operation (attention_rows16, attention_rows.h): image i's rows have exactly the
// bits launch_attention_generic(.., qkv + row0[i] * 3 D, .., n_img = 1, N_i, ..) writes.  New is the work distribution: a work item is
// (image, head, block of 64 queries) and the grid is H * sum_i ceil(N_i / 64) workgroups, so a pack of one 4000-token image and two hundred
// 50-token images balances itself.  A workgroup finds its item by a wave-uniform binary search of blockIdx.x in qb0 [n + 1], the running
// count of query blocks (image i owns workgroups H qb0[i] .. H qb0[i + 1] - 1, heads outermost, as the generic kernel orders them): every
// load of the search has a uniform address and is a scalar load.  Key and value rows clamp to the image's own last row, never to a
// neighbour's.  No atomics, one writer per output element, nothing written outside rows row0[0] .. row0[n] - 1.  32 * DHP * 2 bytes of LDS
// per wave (at most 32 KiB per workgroup): no dynamic-LDS attribute, no prepare_*.
// K and V are NOT staged in LDS for the four waves of a workgroup (attention_text.hip does, for its short sequences): profiles/pack_cost.txt.
#include "attention_rows.h"

namespace vitx {

template <typename T, int NK2>
__global__ __launch_bounds__(256) void attention_packed_kernel(const T *__restrict__ qkv, T *__restrict__ out, const int *__restrict__ row0, const int *__restrict__ qb0, int n,
                                                               int D, int H, int DH, float scale) {
    constexpr int ROWB = NK2 * 32 * 2;                // LDS row bytes of the padded head dim
    __shared__ __attribute__((aligned(16))) char smem[4 * 32 * ROWB];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wg = blockIdx.x;
    int lo = 0, hi = n;                               // the image: H qb0[lo] <= wg < H qb0[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (H * qb0[mid] <= wg) lo = mid; else hi = mid;
    }
    const int r0 = row0[lo], N = row0[lo + 1] - r0, qblocks = qb0[lo + 1] - qb0[lo];
    const int item = wg - H * qb0[lo], h = item / qblocks, qb = item - h * qblocks;
    const int q0 = (qb * 4 + wave) * 16;
    if (q0 >= N) return;                              // no barrier in this kernel: a wave without queries simply leaves
    attention_rows16<T, NK2>(qkv + (size_t)r0 * 3 * D + (size_t)h * DH, out + (size_t)r0 * D + (size_t)h * DH, N, D, DH, scale, q0, smem + wave * (32 * ROWB));
}

bool attention_packed_supports(int D, int H) { return attention_generic_supports(D, H); }

template <typename T>
static hipError_t launch_attention_packed_t(const void *qkv, void *out, const int *row0, const int *qb0, int n, long qblocks, int D, int H, hipStream_t stream) {
    const int DH = D / H, nk2 = (DH + 31) / 32;
    const float scale = 1.0f / sqrtf((float)DH);
    const dim3 grid((unsigned)(qblocks * H)), blk(256);
    switch (nk2) {
    case 1: hipLaunchKernelGGL((attention_packed_kernel<T, 1>), grid, blk, 0, stream, (const T *)qkv, (T *)out, row0, qb0, n, D, H, DH, scale); break;
    case 2: hipLaunchKernelGGL((attention_packed_kernel<T, 2>), grid, blk, 0, stream, (const T *)qkv, (T *)out, row0, qb0, n, D, H, DH, scale); break;
    case 3: hipLaunchKernelGGL((attention_packed_kernel<T, 3>), grid, blk, 0, stream, (const T *)qkv, (T *)out, row0, qb0, n, D, H, DH, scale); break;
    case 4: hipLaunchKernelGGL((attention_packed_kernel<T, 4>), grid, blk, 0, stream, (const T *)qkv, (T *)out, row0, qb0, n, D, H, DH, scale); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
// qblocks = qb0[n] on the host: the caller built the table
hipError_t launch_attention_packed(int dtype, const void *qkv, void *out, const int *row0, const int *qb0, int n, long qblocks, int D, int H, hipStream_t stream) {
    if (!attention_packed_supports(D, H) || n <= 0 || qblocks < n || qblocks * H > 0x7fffffffL) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_attention_packed_t, qkv, out, row0, qb0, n, qblocks, D, H, stream);
}

}  // namespace vitx
