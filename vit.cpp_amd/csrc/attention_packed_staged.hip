// attention_packed_staged.hip -- attention_packed.hip's kernel for head dim 64 with K and V staged in LDS for the four waves of a workgroup.
// Same contract (include/vitx.h "packed batches"): qkv [rows][3 D] -> out [rows][D], image i = rows row0[i] .. row0[i + 1] - 1, any N_i >= 1, the same
// row0 / qb0 tables, the same grid of H * qb0[n] workgroups of 256 threads found by the same wave-uniform binary search, wave w on the 16-query tile
// 64 qb + 16 w.  The arithmetic is attention_rows16<T, 2>'s, operation for operation (the pieces of Rows16, attention_rows.h: same 32-key steps in the
// same order, same masks, same rounding points), so image i's rows have the bits of attention_packed_kernel and of launch_attention_generic on that
// image alone -- with ONE exception: keys at and past N_i of the last 32-key step.  The generic kernel reads the image's last row there and multiplies it
// by a probability of exactly 0; this kernel reads zeros.  0 . NaN = NaN (and a NaN in v[N_i - 1] reaches the row through its own key anyway), but
// 0 . Inf = NaN where 0 . 0 = 0: the bits differ only where v[N_i - 1] of an (image, head) holds +-Inf and N_i % 32 != 0.
// New is the data movement:
//   * keys stream through LDS in chunks of 64: 8 KiB K + 8 KiB V of the head's 128-byte slices, double buffered in 32 KiB of STATIC LDS (no
//     dynamic-LDS attribute, no prepare_*), filled by LDS-DMA (buffer_load ... lds, 16 bytes per lane, as attention_flow.hip issues it): no staging
//     registers, no VALU work, and each key row is fetched once per workgroup instead of once per wave;
//   * the buffer descriptor starts at the image's row 0 in this head's column block and ENDS at the image's last row: keys past N_i of the last chunk
//     arrive as the zeros an out-of-range buffer load returns, whatever the next image or the memory behind the pack holds;
//   * the DMA lays the lanes of a wave out contiguously, so the bank swizzle of K is applied on the source side -- which (key, 16-byte slot) a lane
//     fetches (swz_inv) -- and a K fragment is one conflict-free ds_read_b128 per lane (swz_byte).  V lands row-major: the ds_read_b64_tr_b16 pattern
//     of Rows16::pv_step (ROWB = 128) yields attention_rows16's fragments;
//   * pass 1 streams K only (the true row maximum), pass 2 K and V; the DMA of chunk c + 1 flies under the compute of chunk c, one vmcnt wait and one
//     workgroup barrier per chunk; the last chunk of pass 1 prefetches chunk 0 of pass 2 (with V).  An image of one chunk (N_i <= 64) stages K and V
//     once and runs both passes on it without a barrier in between;
//   * a wave whose tile starts at or past N_i still stages its share and takes part in every barrier; it computes and writes nothing.
// The per-chunk wait is vmcnt(0), not a counted one: after the wait in front of the first barrier (which also covers the Q loads) a wave has nothing
// in flight but the DMA of the next chunk, so a count would wait for the same loads.  The XCD placement of attention_flow.hip was not tried.
// Two properties rest on how the hardware treats a raw buffer load, as attention_flow.hip's do: (1) the range check of the descriptor includes the
// scalar offset (the chunk's first key), not only the lane's offset -- exercised by every image of more than one chunk whose last chunk is partial
// (tests: N = 65, 129, 130, 193, 260, 577); (2) an out-of-range LDS-DMA lane WRITES zeros to LDS instead of leaving the stale bytes -- a test can see
// that only where the stale bytes are not finite (the poison test, when a workgroup of a NaN image left its chunks in the LDS a clean image's
// workgroup gets next: likely, not certain); a finite stale V row times a probability of exactly 0 is invisible, and stale K only meets the mask.  Built without packed-fp32 instructions (vit.cpp_amd/Makefile says why).
// No atomics, one writer per output element, nothing written outside rows row0[0] .. row0[n] - 1.  Numbers: profiles/pack_staged_cost.txt.
#include "attention_rows.h"

namespace vitx {

template <typename T>
__global__ __launch_bounds__(256, 4) void attention_packed_staged_kernel(const T *__restrict__ qkv, T *__restrict__ out, const int *__restrict__ row0, const int *__restrict__ qb0,
                                                                         int n, int D, int H, float scale) {
    typedef Rows16<T, 2> R;
    typedef typename R::v8 v8;
    constexpr int DH = 64, CK = 64, KBYTES = CK * 128, BUF = 2 * KBYTES;      // a chunk buffer: K image, then V image
    static_assert(R::ROWB == 128 && R::ND == 4, "head dim 64");
    __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wg = blockIdx.x;
    int lo = 0, hi = n;                               // the image: H qb0[lo] <= wg < H qb0[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (H * qb0[mid] <= wg) lo = mid; else hi = mid;
    }
    const int r0 = row0[lo], N = row0[lo + 1] - r0, qblocks = qb0[lo + 1] - qb0[lo];
    const int item = wg - H * qb0[lo], h = item / qblocks, qb = item - h * qblocks;
    const int q0 = (qb * 4 + wave) * 16;
    const bool live = q0 < N;                         // wave-uniform; a wave without queries only stages and meets the barriers
    const T *base = qkv + (size_t)r0 * 3 * D + (size_t)h * DH;
    const int nch = (N + CK - 1) / CK, nt16 = (N + 15) / 16;
    const int row_bytes = 3 * D * 2;

    v8 qf[2];
    R::q_frags(base, N, D, DH, live ? q0 : 0, qf);

    // ---- LDS-DMA: physical 16-B piece p = it * 256 + tid of a chunk image <-> (key row, 16-B slot) of the K / V column block
    const unsigned remaining = (unsigned)min((size_t)0xf0000000u, ((size_t)N * 3 * D - (size_t)h * DH) * 2);      // from this head's column block to the end of the IMAGE
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)remaining, 0x00020000);
    int koff[2], voff[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int p = it * 256 + tid;
        int rr, sl; swz_inv(p, rr, sl);
        koff[it] = rr * row_bytes + D * 2 + sl * 16;
        voff[it] = (p >> 3) * row_bytes + 2 * D * 2 + (p & 7) * 16;           // V image: row-major
    }
    auto stage = [&](char *buf, int key0, bool with_v) {
        char *dst = buf + wave * 1024;
        const int so = (int)((unsigned)key0 * (unsigned)row_bytes);
#pragma unroll
        for (int it = 0; it < 2; ++it) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(dst + it * 4096), 16, koff[it], so, 0, 0);
        if (with_v) {
#pragma unroll
            for (int it = 0; it < 2; ++it) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(dst + KBYTES + it * 4096), 16, voff[it], so, 0, 0);
        }
    };
    // K fragment of the chunk's 16-key tile tl: key 16 tl + l15, 16-B slot k2 * 4 + g4.  swz_byte's line term of an odd tile flips bit 7.
    int krd[2];
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) krd[k2] = swz_byte(l15, k2 * 4 + g4);
    auto score_tile = [&](const char *cur, int c, int tl) {
        return R::score_tile(qf, c * 4 + tl, N, [&](int k2) { return *(const v8 *)(cur + tl * 2048 + (krd[k2] ^ ((tl & 1) << 7))); });
    };

    stage(smem, 0, nch == 1);
    __builtin_amdgcn_s_waitcnt(0x0f70);       // vmcnt(0)
    __syncthreads();

    // ---- pass 1: row maximum.  Chunk c is computed out of buffer c & 1 while the DMA of chunk c + 1 fills the other one; after the last chunk comes
    // chunk 0 of pass 2 (with V).  One chunk: K and V are there already.
    float mx = -INFINITY;
    for (int c = 0; c < nch; ++c) {
        const int key0 = c * CK;
        const char *cur = smem + (c & 1) * BUF;
        const bool last = c + 1 == nch;
        if (nch > 1) stage(smem + ((c + 1) & 1) * BUF, last ? 0 : key0 + CK, last);
        if (live) {
            const int nt = min(4, nt16 - c * 4);
            for (int tl = 0; tl < nt; ++tl) mx = R::tile_max(score_tile(cur, c, tl), mx);
        }
        if (nch > 1) { __builtin_amdgcn_s_waitcnt(0x0f70); __syncthreads(); }
    }
    mx = rows4_max(mx);
    const float kk = AttnExpRt<T>::k(scale), nmx = -kk * mx;

    // ---- pass 2: numerators, row sum, PV.  Pass 1's last stage filled buffer nch & 1 (one chunk: buffer 0): chunk c lives in buffer (nch + c) & 1.
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float sum = 0.0f;
    const int buf0 = nch > 1 ? nch : 0;
    const unsigned va0 = (unsigned)(__UINTPTR_TYPE__)((__attribute__((address_space(3))) char *)smem) + KBYTES + R::tr_off();
    for (int c = 0; c < nch; ++c) {
        const int key0 = c * CK, b = (buf0 + c) & 1;
        const char *cur = smem + b * BUF;
        const bool last = c + 1 == nch;
        if (!last) stage(smem + (b ^ 1) * BUF, key0 + CK, true);
        if (live) {
            const int ns = min(2, (N - key0 + 31) / 32);
            for (int s = 0; s < ns; ++s) {
                const f32x4 sa = score_tile(cur, c, 2 * s);
                f32x4 sb = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                if (c * 4 + 2 * s + 1 < nt16) sb = score_tile(cur, c, 2 * s + 1);
                const v8 pk = R::exp_step(sa, sb, nmx, kk, sum);
                R::pv_step(va0 + b * BUF + s * (32 * 128), pk, o);
            }
        }
        if (!last) { __builtin_amdgcn_s_waitcnt(0x0f70); __syncthreads(); }
    }
    if (live) R::store(out + (size_t)r0 * D + (size_t)h * DH, N, D, DH, q0, o, sum);
}

bool attention_packed_staged_supports(int D, int H) { return H > 0 && D > 0 && D % H == 0 && D / H == 64; }

template <typename T>
static hipError_t launch_attention_packed_staged_t(const void *qkv, void *out, const int *row0, const int *qb0, int n, long qblocks, int D, int H, hipStream_t stream) {
    hipLaunchKernelGGL((attention_packed_staged_kernel<T>), dim3((unsigned)(qblocks * H)), dim3(256), 0, stream, (const T *)qkv, (T *)out, row0, qb0, n, D, H, 1.0f / sqrtf(64.0f));
    return hipGetLastError();
}
// qblocks = qb0[n] on the host: the caller built the table
hipError_t launch_attention_packed_staged(int dtype, const void *qkv, void *out, const int *row0, const int *qb0, int n, long qblocks, int D, int H, hipStream_t stream) {
    if (!attention_packed_staged_supports(D, H) || n <= 0 || qblocks < n || qblocks * H > 0x7fffffffL) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_attention_packed_staged_t, qkv, out, row0, qb0, n, qblocks, D, H, stream);
}

}  // namespace vitx
