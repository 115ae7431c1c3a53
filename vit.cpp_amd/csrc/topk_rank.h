// topk_rank.h -- the total order of vitx_topk (model_file.cpp) as one 64-bit key, shared by the device top-k of the probability rows
// (softmax_topk.hip) and the streaming nearest-neighbour selection (nn_select.hip).
// Entries that are not NaN come first, by value descending then index ascending (+0 and -0 tie); NaN entries last, by index ascending.  A value maps
// to a 32-bit rank that grows with it (0 for a NaN, below -inf's), an entry to rank << 32 | ~index: a LARGER key is an EARLIER entry.  The low
// word of an entry with index < 2^31 is at least 0x80000000, so no entry has the key 0.
#pragma once
#include <hip/hip_runtime.h>

namespace vitx {

__device__ __forceinline__ unsigned topk_rank(float v) {
    if (v != v) return 0u;
    const unsigned b = __builtin_bit_cast(unsigned, v + 0.0f);            // -0 + 0 = +0: the two zeros share a rank
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long topk_key(float v, unsigned index) { return ((unsigned long long)topk_rank(v) << 32) | (unsigned)~index; }
// The value a rank stands for: the canonical quiet NaN for rank 0, +0 for either zero, every other value as it was.
__device__ __forceinline__ float topk_rank_value(unsigned r) {
    if (r == 0u) return __builtin_bit_cast(float, 0x7fc00000u);
    return __builtin_bit_cast(float, (r & 0x80000000u) ? (r ^ 0x80000000u) : ~r);
}

}  // namespace vitx
