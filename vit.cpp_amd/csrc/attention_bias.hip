// attention_bias.hip -- attention with a learned relative position bias inside the fused softmax (BEiT, BEiT v2; include/vitx.h
// "relative position bias"): qkv [n_img * N][3 D] -> out [n_img * N][D], N = gh gw + 1 tokens (class token first), head dim 64, and per head a table of
// (2 gh - 1)(2 gw - 1) + 3 floats.  The softmax exponent of (query q, key k) is scale . (q . k) + table[index(q, k)], index() being timm's
// gen_relative_position_index: patch -> patch by the offset (qy - ky, qx - kx), and one entry each for class -> patch, patch -> class, class -> class.
// The arithmetic is attention_rows16<T, 2>'s (attention_rows.h: S^T = K . Q^T on v_mfma_f32_16x16x32, two passes over the keys, AttnExpRt, the rounded-
// numerator row sum, O^T = V^T . P^T) with ONE more step: between the matrix product and the -inf mask of keys >= N, each accumulator element gets
// + table[index] . sqrt(dh) in f32.  The unscaled score then still meets the exponent's own scale . (..): the fold of `scale` into AttnExpRt stays, and
// sqrt(64) = 8 is exact, so the exponent is the f32 sum the formula names.  An all-zero table adds +0 everywhere: the bits of launch_attention_generic.
// A dense [H][N][N] bias never exists.  A workgroup owns one (image, head, 64-query block) -- wave w the 16-query tile 64 qb + 16 w -- and keeps in LDS
//   * the head's table, multiplied by 8 ONCE per entry as it is written, row-major as the file has it.  No padding or swizzle: the row stride 2 gw - 1 is
//     odd, the 16 queries of a lane group at one key read consecutive words (a grid-row wrap moves the run by gw - 1 words), and the four lane groups
//     of a tile sit 4 keys apart, so their runs overlap in the SAME words, which the LDS broadcasts; what conflicts remain are two-way, at row wraps;
//   * koff[j] = ky (2 gw - 1) + kx of key j (0 for the class key and for the padding keys of the last chunk, so every gather stays inside the table).
// A lane's query gives base_q = (qy + gh - 1)(2 gw - 1) + (qx + gw - 1) once; per score tile it reads the koff of its four keys as one ds_read_b128
// and gathers table[base_q - koff[key]]: one v_sub and one ds_read_b32 per score, in both passes (nothing of size N^2 is kept between them: 4 floats
// per 16 x 16 tile would be 13 tiles x 4 VGPRs at N = 197 and does not scale to 577).  The three class entries are held in registers and SELECTED:
// the patch -> class / class -> class value replaces element 0 of lane group 0 in the image's first tile only (a wave-uniform branch), and the
// class -> patch value replaces the gathered ones in the lane of query 0, which only the wave of tile 0 has (wave-uniform again): the other fifteen
// sixteenths of the waves pay no select.
// K and V move as attention_packed_staged.hip moves them at this head dim -- 64-key chunks, 8 KiB K (bank swizzle applied on the source side of the
// LDS-DMA, one conflict-free ds_read_b128 per fragment) + 8 KiB V (row-major, read back by ds_read_b64_tr_b16), double buffered, pass 1 K only, the
// DMA of chunk c + 1 under the compute of chunk c, one vmcnt wait and one barrier per chunk; the descriptor ends at the image's last row, so keys
// past N arrive as zeros -- with the tables filled by plain loads WHILE the first chunk's DMA flies: the barrier that publishes chunk 0 publishes them.
// LDS is dynamic: 32 KiB of chunks + the table rounded up to 16 bytes + koff for the padded key count: 35.9 KiB at a 14 x 14 grid (four workgroups per
// CU), 43.1 KiB at 24 x 24 (three), 51.8 KiB at 32 x 32 (the largest grid a test runs).  prepare_attention_bias raises the kernel's dynamic-LDS limit to
// 64 KiB at device bring-up; above that the launcher refuses (a 41 x 41 grid is the first square one).  Compiler, gfx950, both types: 75 VGPRs, no scratch.
// No atomics, one writer per output element; an image's rows depend on that image's q, k, v and the table alone.  Numbers: profiles/relbias_cost.txt.
#include "attention_rows.h"

namespace vitx {

namespace {
constexpr int kBiasChunks = 2 * 2 * 64 * 128;        // two chunk buffers of K image + V image
inline size_t attention_bias_lds(int gh, int gw) {
    const size_t len = (size_t)(2 * gh - 1) * (2 * gw - 1) + 3, nk = ((size_t)gh * gw + 1 + 63) / 64 * 64;
    return kBiasChunks + (len + 3) / 4 * 16 + nk * 4;
}
}  // namespace

template <typename T>
__global__ __launch_bounds__(256, 4) void attention_bias_kernel(const T *__restrict__ qkv, const float *__restrict__ table, T *__restrict__ out, int gh, int gw, int D, int H,
                                                                int qblocks) {
    typedef Rows16<T, 2> R;
    typedef typename R::v8 v8;
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    constexpr int DH = 64, CK = 64, KBYTES = CK * 128, BUF = 2 * KBYTES;      // a chunk buffer: K image, then V image
    static_assert(R::ROWB == 128 && R::ND == 4, "head dim 64");
    extern __shared__ __attribute__((aligned(16))) char smem_bias[];
    char *smem = smem_bias;
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int item = blockIdx.x / qblocks, qb = blockIdx.x - item * qblocks;
    const int b = item / H, h = item - b * H;
    const int N = gh * gw + 1, W = 2 * gw - 1, len = (2 * gh - 1) * W + 3;
    const int q0 = (qb * 4 + wave) * 16;
    const bool live = q0 < N;                         // wave-uniform; a wave without queries only stages and meets the barriers
    const T *base = qkv + (size_t)b * N * 3 * D + (size_t)h * DH;
    const int nch = (N + CK - 1) / CK, nt16 = (N + 15) / 16;
    const int row_bytes = 3 * D * 2;
    float *tab = (float *)(smem + 2 * BUF);
    int *kofs = (int *)(tab + (len + 3) / 4 * 4);

    v8 qf[2];
    R::q_frags(base, N, D, DH, live ? q0 : 0, qf);

    // ---- LDS-DMA: physical 16-B piece p = it * 256 + tid of a chunk image <-> (key row, 16-B slot) of the K / V column block
    const unsigned remaining = (unsigned)(((size_t)N * 3 * D - (size_t)h * DH) * 2);      // from this head's column block to the end of the IMAGE (the launcher bounds it)
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
    stage(smem, 0, nch == 1);

    // ---- the two tables, under the first chunk's DMA: the head's entries times sqrt(dh) = 8; the per-key offsets (class and padding keys: 0)
    const float *src = table + (size_t)h * len;
    for (int i = tid; i < len; i += 256) tab[i] = src[i] * 8.0f;
    for (int j = tid; j < nch * CK; j += 256) {
        const int p = j - 1, ky = p / gw;
        kofs[j] = (j >= 1 && j < N) ? ky * W + (p - ky * gw) : 0;
    }
    // this lane's query: a class query and the padding lanes of the last tile gather as patch 0 / the last patch do; the class lane's values are replaced
    const int qi = min(q0 + l15, N - 1), qp = max(qi - 1, 0), qy = qp / gw;
    const int base_q = (qy + gh - 1) * W + (qp - qy * gw) + gw - 1;
    const bool qcls = q0 + l15 == 0;
    const bool cls_wave = q0 == 0;                    // wave-uniform: the wave that holds query 0

    // K fragment of the chunk's 16-key tile tl: key 16 tl + l15, 16-B slot k2 * 4 + g4.  swz_byte's line term of an odd tile flips bit 7.
    int krd[2];
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) krd[k2] = swz_byte(l15, k2 * 4 + g4);

    __builtin_amdgcn_s_waitcnt(0x0f70);       // vmcnt(0)
    __syncthreads();
    const float c_row = tab[len - 3];                                   // class -> patch
    const float c_k0 = qcls ? tab[len - 1] : tab[len - 2];              // class -> class, patch -> class

    // S^T tile tl of chunk c: the product, + the bias of (this lane's query, its four keys), then the mask of keys >= N
    auto score_tile = [&](const char *cur, int c, int tl) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) acc = Elem<T>::mfma16(*(const v8 *)(cur + tl * 2048 + (krd[k2] ^ ((tl & 1) << 7))), qf[k2], acc);
        const int key0 = c * CK + tl * 16 + 4 * g4;
        const i32x4 ko = *(const i32x4 *)(kofs + key0);
        f32x4 bs = {tab[base_q - ko[0]], tab[base_q - ko[1]], tab[base_q - ko[2]], tab[base_q - ko[3]]};
        if (cls_wave) {
#pragma unroll
            for (int r = 0; r < 4; ++r) bs[r] = qcls ? c_row : bs[r];
        }
        if (c == 0 && tl == 0) bs[0] = g4 == 0 ? c_k0 : bs[0];          // key 0 is the class token
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += bs[r];
#pragma unroll
        for (int r = 0; r < 4; ++r) if (key0 + r >= N) acc[r] = -INFINITY;
        return acc;
    };

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
    const float kk = AttnExpRt<T>::k(0.125f), nmx = -kk * mx;

    // ---- pass 2: numerators, row sum, PV.  Pass 1's last stage filled buffer nch & 1 (one chunk: buffer 0): chunk c lives in buffer (nch + c) & 1.
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float sum = 0.0f;
    const int buf0 = nch > 1 ? nch : 0;
    const unsigned va0 = (unsigned)(__UINTPTR_TYPE__)((__attribute__((address_space(3))) char *)smem) + KBYTES + R::tr_off();
    for (int c = 0; c < nch; ++c) {
        const int key0 = c * CK, bi = (buf0 + c) & 1;
        const char *cur = smem + bi * BUF;
        const bool last = c + 1 == nch;
        if (!last) stage(smem + (bi ^ 1) * BUF, key0 + CK, true);
        if (live) {
            const int ns = min(2, (N - key0 + 31) / 32);
            for (int s = 0; s < ns; ++s) {
                const f32x4 sa = score_tile(cur, c, 2 * s);
                f32x4 sb = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                if (c * 4 + 2 * s + 1 < nt16) sb = score_tile(cur, c, 2 * s + 1);
                const v8 pk = R::exp_step(sa, sb, nmx, kk, sum);
                R::pv_step(va0 + bi * BUF + s * (32 * 128), pk, o);
            }
        }
        if (!last) { __builtin_amdgcn_s_waitcnt(0x0f70); __syncthreads(); }
    }
    if (live) R::store(out + (size_t)b * N * D + (size_t)h * DH, N, D, DH, q0, o, sum);
}

// head dim 64, N = gh gw + 1 >= 2, an image's qkv rows below 0xf0000000 bytes (the buffer descriptor), chunks + both tables within 64 KiB of LDS
bool attention_bias_supports(int gh, int gw, int D, int H) {
    if (gh <= 0 || gw <= 0 || H <= 0 || D <= 0 || D % H || D / H != 64 || gh > 4096 || gw > 4096) return false;
    return ((size_t)gh * gw + 1) * 3 * D * 2 < 0xf0000000u && attention_bias_lds(gh, gw) <= 65536;
}

// device bring-up (prepare_attention): the chunks and tables of a large grid take up to 64 KiB of dynamic LDS
hipError_t prepare_attention_bias() {
    const hipError_t e = hipFuncSetAttribute((const void *)attention_bias_kernel<_Float16>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    return e != hipSuccess ? e : hipFuncSetAttribute((const void *)attention_bias_kernel<__bf16>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
}

template <typename T>
static hipError_t launch_attention_bias_t(const void *qkv, const float *table, void *out, int n_img, int gh, int gw, int D, int H, hipStream_t stream) {
    const int qblocks = (gh * gw + 1 + 63) / 64;
    hipLaunchKernelGGL((attention_bias_kernel<T>), dim3((unsigned)((size_t)n_img * H * qblocks)), dim3(256), attention_bias_lds(gh, gw), stream, (const T *)qkv, table, (T *)out, gh, gw,
                       D, H, qblocks);
    return hipGetLastError();
}
hipError_t launch_attention_bias(int dtype, const void *qkv, const float *table, void *out, int n_img, int gh, int gw, int D, int H, hipStream_t stream) {
    if (!attention_bias_supports(gh, gw, D, H) || n_img <= 0 || (size_t)n_img * H * ((gh * gw + 1 + 63) / 64) > 0x7fffffffu) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_attention_bias_t, qkv, table, out, n_img, gh, gw, D, H, stream);
}

}  // namespace vitx
