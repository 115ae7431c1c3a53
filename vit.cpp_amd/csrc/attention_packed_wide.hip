// attention_packed_wide.hip -- attention_packed.hip's kernel for head dims 72, 80, .., 128 with K and V staged in LDS for the four waves of a workgroup:
// attention_packed_staged.hip's contract and work distribution with attention_wide.hip's data movement.
// Contract (include/vitx.h "packed batches"): qkv [rows][3 D] -> out [rows][D], image i = rows row0[i] .. row0[i + 1] - 1, any N_i >= 1, the same
// row0 / qb0 tables, the same 1-D grid of H * qb0[n] workgroups of 256 threads found by the same wave-uniform binary search, wave w on the 16-query
// tile 64 qb + 16 w.  The arithmetic is attention_rows16<T, NK2>'s, operation for operation, with NK2 = 3 up to head dim 96 and 4 above (the pieces of
// Rows16<T, NK2, ROWB, NDV>, attention_rows.h: same 32-key steps in the same order, same masks, same rounding points), so image i's rows have the bits
// of attention_packed_kernel and of launch_attention_generic on that image alone -- with the ONE exception of the staged kernels: keys at and past N_i
// of the last 32-key step are zeros here and the image's last row there, both times a probability of exactly 0, so the bits differ only where
// v[N_i - 1] of an (image, head) holds +-Inf and N_i % 32 != 0.
// What depends on the image comes from the table row, per workgroup: N = row0[i + 1] - row0[i], and from it the chunk count nch, the tile count nt16,
// the descriptor length and the bases of qkv and out (row0[i] rows in).  The descriptor starts at the image's row 0 in this head's column block and is
// `remaining` = (N_i * 3 D - h * DH) * 2 bytes long: the rows of THIS image, not the rest of the pack, less the h * DH columns in front of the base
// (clamped at 0xf0000000 as the head-dim-64 kernel clamps it).  The highest byte a lane asks for that lies inside it is V's last piece of key N_i - 1:
// it ends ((N_i - 1) * 3 D + 2 D + DH) * 2 bytes behind the base, <= remaining with equality at h = H - 1; a piece of a key r >= N_i starts
// (r * 3 D + D) * 2 bytes or more behind the base, past remaining <= N_i * 3 D * 2, and comes back as zeros, whatever the next image or the memory
// behind the pack holds.  No offset is formed from another image's N: koff / voff address keys 0 .. 63 of a chunk, the chunk's first key
// (c * 64 < N_i) is the scalar offset.
// The data movement (DH = head dim, P = DH / 8 pieces of 16 bytes in a head's row slice; WideShape, attention_wide_shape.h):
//   * keys stream through LDS in chunks of 64: a K image and a V image of 64 * DH * 2 bytes each, UNPADDED rows, double buffered in 512 DH (+ 16)
//     bytes of STATIC LDS (no dynamic-LDS attribute, no prepare_*).  An image is exactly P wave-wide LDS-DMA instructions (buffer_load ... lds, 16 bytes
//     per lane), dealt round-robin to the four waves; each key row is fetched once per workgroup instead of once per wave;
//   * K: key r's piece s lives at piece r P + (s + j(r)) mod P, j(r) = ((r & 15) * gcd(P, 16)) >> 4, applied on the source side (which piece a DMA
//     lane fetches): a K fragment is one conflict-free ds_read_b128 per lane (attention_wide.hip has the argument);
//   * the K dimension of the score product is zero-padded to 96 / 128 by a PREDICATE on the fragment read (pieces s >= P are the constant zero): the
//     pad never holds a neighbouring head's bytes;
//   * V lands row-major with ROWB = DH * 2 for Rows16::pv_step, ceil(DH / 16) output tiles.  At head dims 72, 88, 104, 120 the last tile is half
//     live: its upper 8 dims read the first 16 bytes of the next key row of the same (image, head) in LDS (16 spare bytes behind the last buffer) and
//     feed output dims >= DH only, which Rows16::store does not write;
//   * pass 1 streams K only (the true row maximum), pass 2 K and V; the DMA of chunk c + 1 flies under the compute of chunk c, one vmcnt(0) and one
//     workgroup barrier per chunk; the last chunk of pass 1 prefetches chunk 0 of pass 2 (with V).  An image of N_i <= 64 stages K and V once for both
//     passes.  nch is uniform over the workgroup (one image per workgroup), so every wave meets the same barriers;
//   * a wave whose tile starts at or past N_i still stages its share and takes part in every barrier; it computes and writes nothing.
// The two hardware properties attention_packed_staged.hip names hold this kernel up too: the descriptor's range check includes the scalar offset, and
// an out-of-range LDS-DMA lane writes zeros.  Built without packed-fp32 instructions (vit.cpp_amd/Makefile says why).  No atomics, one writer per
// output element, nothing written outside rows row0[0] .. row0[n] - 1.
// Compiler (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, the sixteen instantiations; F16 / bf16 where they differ), no scratch and no AGPRs
// anywhere -- column for column attention_wide_kernel's table, which was compiled again beside it and is what its header says:
//   head dim          72      80      88      96     104     112     120     128
//   VGPRs             70      70      74   77/78      84      86      88   95/96
//   static LDS     36880   40960   45072   49152   53264   57344   61456   65536   bytes
//   waves / SIMD       4       4       3       3       3       2       2       2   = workgroups per CU, bound by LDS (the VGPRs would allow 5)
// Numbers: profiles/pack_wide_cost.txt.
#include "attention_rows.h"
#include "attention_wide_shape.h"

namespace vitx {

template <typename T, int DH>
__global__ __launch_bounds__(256, WideShape<DH>::WAVES) void attention_packed_wide_kernel(const T *__restrict__ qkv, T *__restrict__ out, const int *__restrict__ row0,
                                                                                          const int *__restrict__ qb0, int n, int D, int H, float scale) {
    typedef WideShape<DH> S;
    typedef Rows16<T, S::NK2, S::ROWB, S::NDV> R;
    typedef typename R::v8 v8;
    constexpr int P = S::P, NK2 = S::NK2, CK = S::CK, KBYTES = S::KBYTES, BUF = S::BUF, TILEB = 16 * S::ROWB;
    __shared__ __attribute__((aligned(16))) char smem[S::LDS];
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

    v8 qf[NK2];
    R::q_frags(base, N, D, DH, live ? q0 : 0, qf);

    // ---- LDS-DMA: instruction i = wave + 4 it of an image moves its physical 16-B pieces 64 i .. 64 i + 63
    const unsigned remaining = (unsigned)min((size_t)0xf0000000u, ((size_t)N * 3 * D - (size_t)h * DH) * 2);      // from this head's column block to the end of the IMAGE
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)remaining, 0x00020000);
    int koff[4], voff[4];       // at most 4 instructions per wave and image; the size is a literal on purpose (attention_wide.hip says why)
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int p = (wave + 4 * it) * 64 + lane, r = p / P, sp = p - r * P;
        int s = sp - S::rot(r);
        if (s < 0) s += P;
        koff[it] = r * row_bytes + D * 2 + s * 16;
        voff[it] = r * row_bytes + 2 * D * 2 + sp * 16;                          // V image: row-major
    }
    auto stage = [&](char *buf, int key0, bool with_v) {
        const int so = (int)((unsigned)key0 * (unsigned)row_bytes);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int i = wave + 4 * it;
            if (i < P) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(buf + i * 1024), 16, koff[it], so, 0, 0);
                if (with_v) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(buf + KBYTES + i * 1024), 16, voff[it], so, 0, 0);
            }
        }
    };
    // K fragment of the chunk's 16-key tile tl: key 16 tl + l15, piece k2 * 4 + g4 -- the constant zero where that piece is past the head dim
    int krd[NK2];
#pragma unroll
    for (int k2 = 0; k2 < NK2; ++k2) krd[k2] = (l15 * P + (k2 * 4 + g4 + S::rot(l15)) % P) * 16;
    const v8 zero8 = R::zero8();
    auto score_tile = [&](const char *cur, int c, int tl) {
        return R::score_tile(qf, c * 4 + tl, N, [&](int k2) { return k2 * 4 + g4 < P ? *(const v8 *)(cur + tl * TILEB + krd[k2]) : zero8; });
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
    f32x4 o[R::ND];
#pragma unroll
    for (int dt = 0; dt < R::ND; ++dt) o[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float sum = 0.0f;
    const int buf0 = nch > 1 ? nch : 0;
    const unsigned va0 = (unsigned)(__UINTPTR_TYPE__)((__attribute__((address_space(3))) char *)smem) + KBYTES + R::tr_off();
    for (int c = 0; c < nch; ++c) {
        const int key0 = c * CK, bb = (buf0 + c) & 1;
        const char *cur = smem + bb * BUF;
        const bool last = c + 1 == nch;
        if (!last) stage(smem + (bb ^ 1) * BUF, key0 + CK, true);
        if (live) {
            const int ns = min(2, (N - key0 + 31) / 32);
            for (int s = 0; s < ns; ++s) {
                const f32x4 sa = score_tile(cur, c, 2 * s);
                f32x4 sb = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                if (c * 4 + 2 * s + 1 < nt16) sb = score_tile(cur, c, 2 * s + 1);
                const v8 pk = R::exp_step(sa, sb, nmx, kk, sum);
                R::pv_step(va0 + bb * BUF + s * (32 * S::ROWB), pk, o);
            }
        }
        if (!last) { __builtin_amdgcn_s_waitcnt(0x0f70); __syncthreads(); }
    }
    if (live) R::store(out + (size_t)r0 * D + (size_t)h * DH, N, D, DH, q0, o, sum);
}

bool attention_packed_wide_supports(int D, int H) {
    if (H <= 0 || D <= 0 || D % H != 0) return false;
    const int DH = D / H;
    return DH % 8 == 0 && DH >= 72 && DH <= 128;
}

template <typename T, int DH>
static hipError_t launch_attention_packed_wide_dh(const void *qkv, void *out, const int *row0, const int *qb0, int n, long qblocks, int D, int H, hipStream_t stream) {
    hipLaunchKernelGGL((attention_packed_wide_kernel<T, DH>), dim3((unsigned)(qblocks * H)), dim3(256), 0, stream, (const T *)qkv, (T *)out, row0, qb0, n, D, H, 1.0f / sqrtf((float)DH));
    return hipGetLastError();
}
template <typename T>
static hipError_t launch_attention_packed_wide_t(const void *qkv, void *out, const int *row0, const int *qb0, int n, long qblocks, int D, int H, hipStream_t stream) {
    switch (D / H) {
    case 72: return launch_attention_packed_wide_dh<T, 72>(qkv, out, row0, qb0, n, qblocks, D, H, stream);
    case 80: return launch_attention_packed_wide_dh<T, 80>(qkv, out, row0, qb0, n, qblocks, D, H, stream);
    case 88: return launch_attention_packed_wide_dh<T, 88>(qkv, out, row0, qb0, n, qblocks, D, H, stream);
    case 96: return launch_attention_packed_wide_dh<T, 96>(qkv, out, row0, qb0, n, qblocks, D, H, stream);
    case 104: return launch_attention_packed_wide_dh<T, 104>(qkv, out, row0, qb0, n, qblocks, D, H, stream);
    case 112: return launch_attention_packed_wide_dh<T, 112>(qkv, out, row0, qb0, n, qblocks, D, H, stream);
    case 120: return launch_attention_packed_wide_dh<T, 120>(qkv, out, row0, qb0, n, qblocks, D, H, stream);
    case 128: return launch_attention_packed_wide_dh<T, 128>(qkv, out, row0, qb0, n, qblocks, D, H, stream);
    default: return hipErrorInvalidValue;
    }
}
// qblocks = qb0[n] on the host: the caller built the table
hipError_t launch_attention_packed_wide(int dtype, const void *qkv, void *out, const int *row0, const int *qb0, int n, long qblocks, int D, int H, hipStream_t stream) {
    if (!attention_packed_wide_supports(D, H) || n <= 0 || qblocks < n || qblocks * H > 0x7fffffffL) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_attention_packed_wide_t, qkv, out, row0, qb0, n, qblocks, D, H, stream);
}

}  // namespace vitx
