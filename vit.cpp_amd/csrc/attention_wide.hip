// attention_wide.hip -- image-context attention for head dims 72, 80, .., 128 with K and V staged in LDS for the four waves of a workgroup.
// Contract: launch_attention_generic's.  qkv [n_img N][3 D] -> out [n_img N][D], one token count N >= 1 per launch, the same grid (n_img * H * ceil(N / 64)
// workgroups of 256 threads, wave w on the 16-query tile 64 qb + 16 w).  The arithmetic is attention_rows16<T, NK2>'s, operation for operation, with
// NK2 = 3 up to head dim 96 and 4 above (the pieces of Rows16, attention_rows.h: same 32-key steps in the same order, same masks, same rounding
// points), so an (image, head)'s rows have the generic kernel's bits -- with the ONE exception attention_packed_staged.hip documents: keys at and past
// N of the last 32-key step are zeros here and the image's last row there, both times a probability of exactly 0, so the bits differ only where
// v[N - 1] of an (image, head) holds +-Inf and N % 32 != 0.
// The data movement (DH = head dim, P = DH / 8 pieces of 16 bytes in a head's row slice, 9 .. 16):
//   * keys stream through LDS in chunks of 64: a K image and a V image of 64 * DH * 2 bytes each, UNPADDED rows, double buffered in 512 DH bytes of
//     STATIC LDS (36 KiB at head dim 72 .. 64 KiB at 128: no dynamic-LDS attribute, no prepare_*).  64 keys make an image exactly P wave-wide LDS-DMA
//     instructions (buffer_load ... lds, 16 bytes per lane, 1 KiB per instruction), dealt round-robin to the four waves; 32-key chunks would halve the LDS
//     but leave half-instructions at odd P.  Each key row is fetched once per workgroup instead of once per wave;
//   * the buffer descriptor starts at the image's row 0 in this head's column block and ENDS at the image's last row: keys past N of the last chunk
//     arrive as the zeros an out-of-range buffer load returns, whatever the next image holds;
//   * K: key r's piece s lives at piece r P + (s + j(r)) mod P, j(r) = ((r & 15) * g) >> 4, g = gcd(P, 16) -- a rotation inside the row, applied on
//     the source side (which piece a DMA lane fetches).  A K fragment is one ds_read_b128 per lane; its lane group is 16 keys r = 16 t .. + 15 at one s,
//     and the 16-byte bank slot of a lane is (r P + (s + j) mod P) mod 16.  r P mod 16 runs over the 16 / g multiples of g, the g keys that share one
//     have j = 0 .. g - 1, and g | P makes (s + j) mod P distinct mod g: 16 distinct slots, conflict-free at every P.  Odd P (head dims 72, 88, 104,
//     120) has g = 1: plain row-major is already conflict-free; P = 16 is a full rotation.
//   * the K dimension of the score product is zero-padded to 96 / 128 by a PREDICATE on the fragment read (pieces s >= P are the constant zero, as in
//     the generic kernel): the pad never holds a neighbouring head's bytes, LDS holds none of it;
//   * V lands row-major with ROWB = DH * 2 for Rows16::pv_step's ds_read_b64_tr_b16 pattern, ceil(DH / 16) output tiles.  At head dims 72, 88, 104,
//     120 the last tile is half live: its upper 8 dims read the first 16 bytes of the NEXT key row of the same (image, head) (16 spare bytes behind the
//     last buffer keep the last row's read inside the array).  They feed rows 8 .. 15 of that tile's V^T operand only, i.e. output dims >= DH, which
//     Rows16::store does not write.  What conflict remains: the transposed reads of a half wave cover 8 key rows x 32 bytes, ROWB apart -- 2-way at
//     144-byte rows, none at 176 / 208 / 240, 8-way at 256 (head dim 128, as the generic kernel's own LDS image has there).  Not swizzled here;
//   * pass 1 streams K only (the true row maximum), pass 2 K and V; the DMA of chunk c + 1 flies under the compute of chunk c, one vmcnt wait and one
//     workgroup barrier per chunk; the last chunk of pass 1 prefetches chunk 0 of pass 2 (with V).  N <= 64 stages K and V once for both passes;
//   * a wave whose tile starts at or past N still stages its share and takes part in every barrier; it computes and writes nothing.
// The two hardware properties attention_packed_staged.hip names hold this kernel up too: the descriptor's range check includes the scalar offset, and
// an out-of-range LDS-DMA lane writes zeros.  Built without packed-fp32 instructions (vit.cpp_amd/Makefile says why).  No atomics, one writer per
// output element, nothing written outside out's n_img * N rows.
// Compiler (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; F16 and bf16 agree but for one VGPR at 96 and 128), no scratch anywhere:
//   head dim          72      80      88      96     104     112     120     128
//   VGPRs             70      70      74   77/78      84      86      88   95/96
//   static LDS     36880   40960   45072   49152   53264   57344   61456   65536   bytes
//   waves / SIMD       4       4       3       3       3       2       2       2   = workgroups per CU, bound by LDS (the VGPRs would allow 5)
// Numbers: profiles/wide_attn_cost.txt.
#include "attention_rows.h"
#include "attention_wide_shape.h"

namespace vitx {

template <typename T, int DH>
__global__ __launch_bounds__(256, WideShape<DH>::WAVES) void attention_wide_kernel(const T *__restrict__ qkv, T *__restrict__ out, int N, int D, int H, float scale, int qblocks) {
    typedef WideShape<DH> S;
    typedef Rows16<T, S::NK2, S::ROWB, S::NDV> R;
    typedef typename R::v8 v8;
    constexpr int P = S::P, NK2 = S::NK2, CK = S::CK, KBYTES = S::KBYTES, BUF = S::BUF, TILEB = 16 * S::ROWB;
    __shared__ __attribute__((aligned(16))) char smem[S::LDS];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int item = blockIdx.x / qblocks, qb = blockIdx.x - item * qblocks;
    const int b = item / H, h = item - b * H;
    const int q0 = (qb * 4 + wave) * 16;
    const bool live = q0 < N;                         // wave-uniform; a wave without queries only stages and meets the barriers
    const T *base = qkv + (size_t)b * N * 3 * D + (size_t)h * DH;
    const int nch = (N + CK - 1) / CK, nt16 = (N + 15) / 16;
    const int row_bytes = 3 * D * 2;

    v8 qf[NK2];
    R::q_frags(base, N, D, DH, live ? q0 : 0, qf);

    // ---- LDS-DMA: instruction i = wave + 4 it of an image moves its physical 16-B pieces 64 i .. 64 i + 63
    const unsigned remaining = (unsigned)(((size_t)N * 3 * D - (size_t)h * DH) * 2);      // from this head's column block to the end of the IMAGE (launcher: below 0xf0000000)
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)remaining, 0x00020000);
    int koff[4], voff[4];       // at most 4 instructions per wave and image.  The size is a literal on purpose: with an array of dependent type among the DMA
                                // builtin's arguments the HOST pass silently drops the kernel's launch stub (an undefined symbol at link time)
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
    if (live) R::store(out + (size_t)b * N * D + (size_t)h * DH, N, D, DH, q0, o, sum);
}

// head dim 72, 80, .., 128; an image's qkv rows within the 32-bit range of a buffer descriptor
bool attention_wide_supports(int N, int D, int H) {
    if (H <= 0 || D <= 0 || D % H != 0 || N <= 0) return false;
    const int DH = D / H;
    return DH % 8 == 0 && DH >= 72 && DH <= 128 && (size_t)N * 3 * D * 2 < 0xf0000000u;
}

template <typename T, int DH>
static hipError_t launch_attention_wide_dh(const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream) {
    const int qblocks = (N + 63) / 64;
    hipLaunchKernelGGL((attention_wide_kernel<T, DH>), dim3((unsigned)((size_t)n_img * H * qblocks)), dim3(256), 0, stream, (const T *)qkv, (T *)out, N, D, H, 1.0f / sqrtf((float)DH), qblocks);
    return hipGetLastError();
}
template <typename T>
static hipError_t launch_attention_wide_t(const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream) {
    switch (D / H) {
    case 72: return launch_attention_wide_dh<T, 72>(qkv, out, n_img, N, D, H, stream);
    case 80: return launch_attention_wide_dh<T, 80>(qkv, out, n_img, N, D, H, stream);
    case 88: return launch_attention_wide_dh<T, 88>(qkv, out, n_img, N, D, H, stream);
    case 96: return launch_attention_wide_dh<T, 96>(qkv, out, n_img, N, D, H, stream);
    case 104: return launch_attention_wide_dh<T, 104>(qkv, out, n_img, N, D, H, stream);
    case 112: return launch_attention_wide_dh<T, 112>(qkv, out, n_img, N, D, H, stream);
    case 120: return launch_attention_wide_dh<T, 120>(qkv, out, n_img, N, D, H, stream);
    case 128: return launch_attention_wide_dh<T, 128>(qkv, out, n_img, N, D, H, stream);
    default: return hipErrorInvalidValue;
    }
}
hipError_t launch_attention_wide(int dtype, const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream) {
    if (!attention_wide_supports(N, D, H) || n_img <= 0 || (size_t)n_img * H * ((N + 63) / 64) > 0x7fffffffu) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_attention_wide_t, qkv, out, n_img, N, D, H, stream);
}

}  // namespace vitx
