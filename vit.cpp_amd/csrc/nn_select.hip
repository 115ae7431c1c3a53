// nn_select.hip -- streaming top-k of a query's scores against a gallery that passes by in chunks (vitx_nn_set, vitx_op_nn*; the contract:
// include/vitx.h "nearest neighbours in a gallery").  Two kernels:
//   nn_select_kernel   scores [n][ld] f32, `cols` real columns of one chunk, gallery index of column 0 = base_index -> merged into the running state;
//   nn_finish_kernel   the state -> out [n][k] {f32 score, i32 index} best first and, with labels, the temperature-weighted vote [n][n_labels].
// An entry is the 64-bit key of topk_rank.h (rank << 32 | ~index; larger = earlier in vitx_topk's order); keys of distinct gallery rows are distinct,
// so "the k largest keys" is ONE set whatever the order the entries are met in: the result does not depend on the chunk size or on the cut below.
// One wave owns one (query row, column segment) pair: a chunk's columns are cut into kNnSegs segments (whole 16-byte groups), segment s of every
// chunk goes to list s of the row, state [n][kNnSegs][k] keys.  A wave holds its list sorted across lanes (lane j = the j-th best, 0 = no entry),
// its k-th key is the threshold; it reads 4 scores per lane and iteration, compares them with the threshold, and inserts the few that pass one by
// one: a ballot names them, a lane shift makes room.  No atomics, no flags, no wave reads another's list before the final launch.
#include "device_common.h"
#include "kernels.h"
#include "topk_rank.h"

namespace vitx {

namespace {

typedef unsigned long long u64;

// lane l's value in every lane, as a scalar (l is wave-uniform)
__device__ __forceinline__ u64 nn_lane(u64 v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}
// The candidates `key` of the lanes with `valid` that beat the threshold enter the sorted list `mine` (one entry per lane, descending), in lane
// order; thr = the list's k-th entry after each.  Everything but `mine`, `key` and `valid` is wave-uniform.
__device__ __forceinline__ void nn_offer(u64 &mine, u64 &thr, u64 key, bool valid, int lane, int k) {
    u64 m = __ballot(valid && key > thr);
    while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        const u64 c = nn_lane(key, l);
        if (c > thr) {                                   // the threshold may have risen since the ballot
            const int pos = __popcll(__ballot(mine > c));
            const u64 up = __shfl_up(mine, 1);
            mine = lane < pos ? mine : (lane == pos ? c : up);
            thr = nn_lane(mine, k - 1);
        }
    }
}

// 4 scores of columns c .. c + 3 of a row (columns at or past c1 read as 0 and are never offered); one 16-byte load where the row allows it
__device__ __forceinline__ f32x4 nn_load4(const float *__restrict__ p, long c, long c1, bool vec) {
    if (vec && c + 4 <= c1) return *(const f32x4 *)(p + c);
    f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int e = 0; e < 4; ++e) if (c + e < c1) x[e] = p[c + e];
    return x;
}

__global__ __launch_bounds__(256) void nn_select_kernel(const float *__restrict__ scores, long ld, int n, int cols, int seg, long base_index,
                                                        u64 *__restrict__ state, int k, int first) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int row = (int)(w / kNnSegs), s = (int)(w % kNnSegs);
    if (row >= n) return;
    u64 *st = state + ((size_t)row * kNnSegs + s) * k;
    u64 mine = (!first && lane < k) ? st[lane] : 0;
    u64 thr = nn_lane(mine, k - 1);
    const long c0 = (long)s * seg < cols ? (long)s * seg : cols, c1 = c0 + seg < cols ? c0 + seg : cols;
    const float *p = scores + (size_t)row * ld;
    const bool vec = ((uintptr_t)p & 15) == 0;           // seg is a multiple of 4: every lane's group then starts on a 16-byte boundary
    f32x4 x = nn_load4(p, c0 + 4 * lane, c1, vec);
    for (long t = c0; t < c1; t += 256) {
        const long c = t + 4 * lane;
        const f32x4 nx = nn_load4(p, c + 256, c1, vec);  // the next iteration's scores are in flight while this one's are inserted
#pragma unroll
        for (int e = 0; e < 4; ++e) nn_offer(mine, thr, topk_key(x[e], (unsigned)(base_index + c + e)), c + e < c1, lane, k);
        x = nx;
    }
    if (lane < k) st[lane] = mine;
}

// One wave per query row: the kNnSegs lists of the row merged by the same insertion, then lane j writes entry j.  The vote (labels != nullptr):
// w_j = expf((score_j - score_0) / T), W = the sum over j in rank order, vote[c] = (the sum of w_j over the entries labelled c, in rank order) / W;
// lane l owns the classes l, l + 64, ...: one writer per element.
__global__ __launch_bounds__(256) void nn_finish_kernel(const u64 *__restrict__ state, int n, int k, const int *__restrict__ labels, int n_labels, float T,
                                                        float *__restrict__ pairs, float *__restrict__ vote) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    u64 mine = 0, thr = 0;
    for (int s = 0; s < kNnSegs; ++s) {
        const u64 key = lane < k ? state[((size_t)row * kNnSegs + s) * k + lane] : 0;
        nn_offer(mine, thr, key, lane < k, lane, k);     // an empty slot (key 0) never beats a threshold
    }
    const bool have = lane < k && mine != 0;
    const float score = have ? topk_rank_value((unsigned)(mine >> 32)) : __builtin_bit_cast(float, 0x7fc00000u);
    const int idx = have ? (int)~(unsigned)mine : -1;
    if (lane < k) { pairs[((size_t)row * k + lane) * 2] = score; ((int *)pairs)[((size_t)row * k + lane) * 2 + 1] = idx; }
    if (!labels) return;
    const float s0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, score), 0));
    const float wj = have ? expf((score - s0) / T) : 0.0f;
    const int lj = have ? labels[idx] : -1;
    float W = 0.0f;
    for (int j = 0; j < k; ++j) W += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wj), j));
    for (int cb = 0; cb < n_labels; cb += 64) {
        const int c = cb + lane;
        float acc = 0.0f;
        for (int j = 0; j < k; ++j) {
            const float w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wj), j));
            if (__builtin_amdgcn_readlane(lj, j) == c) acc += w;
        }
        if (c < n_labels) vote[(size_t)row * n_labels + c] = acc / W;
    }
}

}  // namespace

size_t nn_state_bytes(int n, int k) { return n > 0 && k > 0 ? (size_t)n * kNnSegs * k * sizeof(u64) : 0; }

hipError_t launch_nn_select(const float *scores, long ld, int n, int cols, long base_index, void *state, int k, bool first, hipStream_t stream) {
    if (n <= 0 || cols <= 0 || ld < cols || k < 1 || k > kNnMaxK || base_index < 0 || base_index + cols > 0x7fffffffL) return hipErrorInvalidValue;
    const int seg = ((cols + kNnSegs - 1) / kNnSegs + 3) / 4 * 4;
    const long waves = (long)n * kNnSegs;
    hipLaunchKernelGGL(nn_select_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, scores, ld, n, cols, seg, base_index, (u64 *)state, k, first ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_nn_finish(const void *state, int n, int k, const int *labels, int n_labels, float temperature, void *pairs, float *vote, hipStream_t stream) {
    if (n <= 0 || k < 1 || k > kNnMaxK || (labels && (n_labels < 1 || !vote || !(temperature > 0.0f) || temperature - temperature != 0.0f))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_finish_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, (const u64 *)state, n, k, labels, n_labels, temperature, (float *)pairs, labels ? vote : nullptr);
    return hipGetLastError();
}

}  // namespace vitx
