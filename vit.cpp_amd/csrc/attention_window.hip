// attention_window.hip -- windowed attention with a decomposed relative position term (the ViTDet / Segment-Anything image encoder; include/vitx.h
// "windowed attention and decomposed relative position"): qkv [n_img * gh gw][3 D] -> out [n_img * gh gw][D], class-less tokens in raster order, head
// dim 64.  One launch is one layer: the grid is cut into windows of wh x ww tokens (the last window of a row / column reaches past the grid: its
// missing tokens are PAD tokens), and a query attends to the wh ww slots of its own window.  (wh, ww) = (gh, gw) is a global layer: one window, no pads.
// The exponent of (query q at window position (qy, qx), key slot j at (ky, kx) = (j / ww, j % ww)) is
//     scale . (q . k_j) + q . Rh[qy - ky + wh - 1] + q . Rw[qx - kx + ww - 1]          (q unscaled; Rh [2 wh - 1][64], Rw [2 ww - 1][64] in the operand type)
// and a pad slot is a real key whose k, v are RNE(qkv bias): what the qkv GEMM gives for the zero row that the model pads with behind norm1.
// The arithmetic is attention_rows16<T, 2>'s (attention_rows.h) with the step attention_bias.hip added: between the matrix product and the -inf mask
// of slots >= wh ww each f32 accumulator gets + 8 Bh[q][ky] + 8 Bw[q][kx]; sqrt(64) = 8 is exact and the exponent's folded `scale` then applies to
// the sum.  Zero tables add +0 twice: a global launch has launch_attention_generic's bits at N = gh gw, a window of a grid without pads the bits of
// the generic kernel on that window's rows gathered as an image.
// A workgroup owns (image, window, head, 64-query block of the window's slots), wave w the 16-query tile 64 qb + 16 w; a tile without a real query
// only stages and meets the barriers, pad queries store nothing.
//   * Bias panels, per wave, once, under the first chunk's DMA: Bh [ky][16 q] and Bw [kx][16 q] f32.  The table is the A operand of
//     v_mfma_f32_16x16x32 (16 table rows r0 .. r0 + 15, as 16 keys are for S^T), the wave's q fragments the B operand, so a lane holds (table row
//     r0 + 4 g4 + i, query l15) and writes 8 x it to row ky = qy + wh - 1 - r of the panel where 0 <= ky < wh.  Only table rows qy_min .. qy_max + wh - 1
//     of the tile's queries are multiplied (5 tiles of 16 rows at 64 x 64 global, not 8).  2 wh - 1 columns per query are never kept.
//   * Per score, both passes: one ds_read_b32 from each panel and two adds.  There is NO per-slot (ky, kx) table: at 64 x 64 global the chunks and
//     the panels fill the 64 KiB to the byte.  (ky, kx) of the tile's first key is wave-uniform and is kept on the scalar unit, chunk by chunk; a
//     lane adds its four keys' constant offsets (divmod(4 g4 + i, ww), once) and wraps kx at most once.  Rows of the Bw panel 4 apart share their
//     banks, so the four lane groups of a tile conflict there where ww > 4: not cured (a padded row would not fit at 64 x 64).
//   * K and V move as attention_packed_staged.hip moves them: 64-slot chunks, 8 KiB K (bank swizzle on the source side of the LDS-DMA, one
//     ds_read_b128 per fragment) + 8 KiB V (row-major, ds_read_b64_tr_b16), double buffered, pass 1 K only, the DMA of chunk c + 1 under the compute
//     of chunk c, one vmcnt wait and one barrier per chunk.  A lane's DMA offset is its slot's grid row (the rows of a window are not contiguous);
//     the descriptor ends at the image's last row; pad slots and slots >= wh ww get an offset past it and arrive as zeros.  The lane that fetched a
//     16-byte piece of a PAD slot then overwrites it with its piece of RNE(bias_k) / RNE(bias_v) (one piece each in registers: the 16-byte slot of a
//     lane is the same in every chunk) by a plain ds_write behind its own vmcnt(0) and in front of the chunk's barrier.
// LDS is dynamic: 32 KiB of chunks + 4 waves x 64 bytes x (ceil(64 nch / ww) + ww) panel rows, nch = ceil(wh ww / 64): 35.5 KiB at a 14 x 14 window
// (four workgroups per CU), 64 KiB at 64 x 64 (two).  prepare_attention_window raises the limit to 64 KiB; wh or ww above 64 is refused.
// Compiler, gfx950, both types: 121 VGPRs, 76 SGPRs, no scratch, occupancy 4 waves per SIMD by registers (the LDS of four workgroups at 14 x 14 asks no more).
// No atomics, one writer per output element; an image's rows depend on that image's q, k, v, the tables and the bias alone.  Numbers: profiles/window_cost.txt.
#include "attention_rows.h"

namespace vitx {

namespace {
constexpr int kWinChunks = 2 * 2 * 64 * 128;         // two chunk buffers of K image + V image
inline int window_panel_rows(int wh, int ww) { return (((wh * ww + 63) / 64) * 64 + ww - 1) / ww + ww; }      // Bh rows (every slot of the last chunk has one) + Bw rows
inline size_t attention_window_lds(int wh, int ww) { return kWinChunks + (size_t)4 * 64 * window_panel_rows(wh, ww); }
}  // namespace

template <typename T>
__global__ __launch_bounds__(256, 2) void attention_window_kernel(const T *__restrict__ qkv, const T *__restrict__ rel_h, const T *__restrict__ rel_w, const float *__restrict__ qkv_bias,
                                                                  T *__restrict__ out, int gh, int gw, int wh, int ww, int D, int H, int nwx, int nwin, int qblocks) {
    typedef Rows16<T, 2> R;
    typedef typename R::v8 v8;
    typedef typename Pair<T>::v2 v2;
    constexpr int DH = 64, CK = 64, KBYTES = CK * 128, BUF = 2 * KBYTES;      // a chunk buffer: K image, then V image
    static_assert(R::ROWB == 128 && R::ND == 4, "head dim 64");
    extern __shared__ __attribute__((aligned(16))) char smem_window[];
    char *smem = smem_window;
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int item = blockIdx.x / qblocks;
    const int qb = blockIdx.x - item * qblocks;
    const int h = item % H; item /= H;
    const int win = item % nwin, b = item / nwin;
    const int wy0 = (win / nwx) * wh, wx0 = (win % nwx) * ww;
    const int G = gh * gw, Nw = wh * ww;
    const int nch = (Nw + CK - 1) / CK, nt16 = (Nw + 15) / 16;
    const int row_bytes = 3 * D * 2;
    const T *base = qkv + (size_t)b * G * 3 * D + (size_t)h * DH;
    const int rows_h = (nch * CK + ww - 1) / ww;
    float *pan_h = (float *)(smem + 2 * BUF) + wave * 16 * (rows_h + ww), *pan_w = pan_h + 16 * rows_h;

    // ---- this lane's query: slot q0 + l15 of the window.  A pad or missing query computes as the window's first token (always real) and stores nothing
    // (its panel column is filled only where its own (qyl, qxl) allow, the rest is stale LDS: such a lane computes on garbage, alone -- the lanes of a
    // query share nothing with another query's -- and nothing of it is stored)
    const int q0 = (qb * 4 + wave) * 16;
    const int sq = q0 + l15, qyl = sq / ww, qxl = sq - qyl * ww;
    const bool real = sq < Nw && wy0 + qyl < gh && wx0 + qxl < gw;
    const bool live = __builtin_amdgcn_ballot_w64(real) != 0;      // wave-uniform; a tile without a real query only stages and meets the barriers
    const int qtok = real ? (wy0 + qyl) * gw + wx0 + qxl : wy0 * gw + wx0;
    v8 qf[2];
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) qf[k2] = *(const v8 *)(base + (size_t)qtok * 3 * D + k2 * 32 + g4 * 8);

    // ---- LDS-DMA: physical 16-B piece p = it * 256 + tid of a chunk image <-> (slot row, 16-B slot) of the K / V column block; it = 1 is 32 rows on
    const unsigned remaining = (unsigned)(((size_t)G * 3 * D - (size_t)h * DH) * 2);      // from this head's column block to the end of the IMAGE (the launcher bounds it)
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)remaining, 0x00020000);
    int krow, ksl; swz_inv(tid, krow, ksl);
    const int vrow = tid >> 3, vsl = tid & 7;
    const int kcol = D * 2 + ksl * 16, vcol = 2 * D * 2 + vsl * 16;
    // the pad key of this head, this lane's 16-byte pieces: RNE of the f32 bias
    v8 kpad, vpad;
#pragma unroll
    for (int e = 0; e < 8; ++e) { kpad[e] = (T)qkv_bias[D + h * DH + ksl * 8 + e]; vpad[e] = (T)qkv_bias[2 * D + h * DH + vsl * 8 + e]; }
    // offset of slot j's grid row, or one past every descriptor; pad: a slot of the window that lies outside the grid
    auto slot_off = [&](int j, int col, bool &pad) {
        const int ky = j / ww, kx = j - ky * ww, Y = wy0 + ky, X = wx0 + kx;
        const bool in = j < Nw, on = in && Y < gh && X < gw;
        pad = in && !on;
        return (int)(on ? (unsigned)(Y * gw + X) * (unsigned)row_bytes + (unsigned)col : 0xf0000000u);
    };
    // returns the lane's pad pieces: bit it = K piece it, bit 2 + it = V piece it
    auto stage = [&](char *buf, int key0, bool with_v) {
        char *dst = buf + wave * 1024;
        unsigned pads = 0;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            bool pad;
            const int off = slot_off(key0 + it * 32 + krow, kcol, pad);
            pads |= (unsigned)pad << it;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(dst + it * 4096), 16, off, 0, 0, 0);
        }
        if (with_v) {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                bool pad;
                const int off = slot_off(key0 + it * 32 + vrow, vcol, pad);
                pads |= (unsigned)pad << (2 + it);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(dst + KBYTES + it * 4096), 16, off, 0, 0, 0);
            }
        }
        return pads;
    };
    // the chunk is there: the lane's own DMA has landed, its pad pieces are written over the zeros, then the workgroup's barrier
    auto publish = [&](char *buf, unsigned pads) {
        __builtin_amdgcn_s_waitcnt(0x0f70);       // vmcnt(0)
        if (pads) {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                if (pads & (1u << it)) *(v8 *)(buf + it * 4096 + tid * 16) = kpad;
                if (pads & (4u << it)) *(v8 *)(buf + KBYTES + it * 4096 + tid * 16) = vpad;
            }
        }
        __syncthreads();
    };
    const unsigned pads0 = stage(smem, 0, nch == 1);

    // ---- the bias panels, under the first chunk's DMA: 8 q . R[r] for table rows r0 .. r0 + 15 per product, kept where the key index is in range
    if (live) {
        const int qlast = min(q0 + 15, Nw - 1), qa = q0 / ww, qe = qlast / ww;          // wave-uniform: the tile's window rows
        const int xa = qa == qe ? q0 - qa * ww : 0, xe = qa == qe ? qlast - qa * ww : ww - 1;
        auto panel = [&](const T *__restrict__ rel, float *pan, int w, int ql, int ra, int re) {
            for (int r0 = ra & ~15; r0 <= re; r0 += 16) {
                const int row = min(r0 + l15, 2 * w - 2);
                f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int k2 = 0; k2 < 2; ++k2) acc = Elem<T>::mfma16(*(const v8 *)(rel + (size_t)row * DH + k2 * 32 + g4 * 8), qf[k2], acc);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = ql + w - 1 - (r0 + 4 * g4 + i);
                    if ((unsigned)k < (unsigned)w) pan[k * 16 + l15] = acc[i] * 8.0f;
                }
            }
        };
        panel(rel_h, pan_h, wh, qyl, qa, qe + wh - 1);
        panel(rel_w, pan_w, ww, qxl, xa, xe + ww - 1);
    }
    // this lane's four keys of a tile: divmod(4 g4 + i, ww), as panel rows
    int dyo[4], dxo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int o = 4 * g4 + i; dyo[i] = o / ww; dxo[i] = o - dyo[i] * ww; }
    const float *ph = pan_h + l15, *pw = pan_w + l15;
    const int d16 = 16 / ww, m16 = 16 - d16 * ww, d64 = CK / ww, m64 = CK - d64 * ww;

    // K fragment of the chunk's 16-key tile tl: key 16 tl + l15, 16-B slot k2 * 4 + g4.  swz_byte's line term of an odd tile flips bit 7.
    int krd[2];
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) krd[k2] = swz_byte(l15, k2 * 4 + g4);

    publish(smem, pads0);

    // S^T tile tl of chunk c, whose first slot is (kyc, kxc): the product, + the two bias terms of (this lane's query, its four keys), then the mask
    auto score_tile = [&](const char *cur, int c, int tl, int kyc, int kxc) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) acc = Elem<T>::mfma16(*(const v8 *)(cur + tl * 2048 + (krd[k2] ^ ((tl & 1) << 7))), qf[k2], acc);
        int kyt = kyc + tl * d16, kxt = kxc + tl * m16;                 // scalar: the tile's first slot; tl m16 < 3 ww + .. wraps at most three times
#pragma unroll
        for (int w3 = 0; w3 < 3; ++w3) if (kxt >= ww) { kxt -= ww; ++kyt; }
        const int key0 = c * CK + tl * 16 + 4 * g4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int kx = kxt + dxo[r], ky = kyt + dyo[r];
            if (kx >= ww) { kx -= ww; ++ky; }
            acc[r] += ph[ky * 16];
            acc[r] += pw[kx * 16];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) if (key0 + r >= Nw) acc[r] = -INFINITY;
        return acc;
    };
    // the next chunk's first slot
    auto advance = [&](int &kyc, int &kxc) { kyc += d64; kxc += m64; if (kxc >= ww) { kxc -= ww; ++kyc; } };

    // ---- pass 1: row maximum.  Chunk c is computed out of buffer c & 1 while the DMA of chunk c + 1 fills the other one; after the last chunk comes
    // chunk 0 of pass 2 (with V).  One chunk: K and V are there already.
    float mx = -INFINITY;
    for (int c = 0, kyc = 0, kxc = 0; c < nch; ++c, advance(kyc, kxc)) {
        const int key0 = c * CK;
        const char *cur = smem + (c & 1) * BUF;
        const bool last = c + 1 == nch;
        unsigned pads = 0;
        if (nch > 1) pads = stage(smem + ((c + 1) & 1) * BUF, last ? 0 : key0 + CK, last);
        if (live) {
            const int nt = min(4, nt16 - c * 4);
            for (int tl = 0; tl < nt; ++tl) mx = R::tile_max(score_tile(cur, c, tl, kyc, kxc), mx);
        }
        if (nch > 1) publish(smem + ((c + 1) & 1) * BUF, pads);
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
    for (int c = 0, kyc = 0, kxc = 0; c < nch; ++c, advance(kyc, kxc)) {
        const int key0 = c * CK, bi = (buf0 + c) & 1;
        const char *cur = smem + bi * BUF;
        const bool last = c + 1 == nch;
        unsigned pads = 0;
        if (!last) pads = stage(smem + (bi ^ 1) * BUF, key0 + CK, true);
        if (live) {
            const int ns = min(2, (Nw - key0 + 31) / 32);
            for (int s = 0; s < ns; ++s) {
                const f32x4 sa = score_tile(cur, c, 2 * s, kyc, kxc);
                f32x4 sb = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                if (c * 4 + 2 * s + 1 < nt16) sb = score_tile(cur, c, 2 * s + 1, kyc, kxc);
                const v8 pk = R::exp_step(sa, sb, nmx, kk, sum);
                R::pv_step(va0 + bi * BUF + s * (32 * 128), pk, o);
            }
        }
        if (!last) publish(smem + (bi ^ 1) * BUF, pads);
    }
    // Rows16::store's arithmetic, the row being the query's grid token: lane (l15 = query, g4) holds O[query][dt * 16 + 4 g4 .. + 3]
    if (live) {
        const float inv = 1.0f / rows4_sum(sum);
        if (real) {
            T *orow = out + ((size_t)b * G + qtok) * D + (size_t)h * DH;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const v2 lo = round_pair<T>(o[dt][0] * inv, o[dt][1] * inv), hi = round_pair<T>(o[dt][2] * inv, o[dt][3] * inv);
                typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
                *(u32x2_t *)(orow + dt * 16 + 4 * g4) = u32x2_t{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
            }
        }
    }
}

// head dim 64, windows of 1 .. 64 slots a side (chunks + panels within 64 KiB of LDS), an image's qkv rows below 0xf0000000 bytes (the buffer descriptor)
bool attention_window_supports(int gh, int gw, int wh, int ww, int D, int H) {
    if (gh <= 0 || gw <= 0 || wh <= 0 || ww <= 0 || H <= 0 || D <= 0 || D % H || D / H != 64 || gh > 4096 || gw > 4096 || wh > 64 || ww > 64) return false;
    return (size_t)gh * gw * 3 * D * 2 < 0xf0000000u && attention_window_lds(wh, ww) <= 65536;
}

// device bring-up (prepare_attention): the chunks and panels of a large window take up to 64 KiB of dynamic LDS
hipError_t prepare_attention_window() {
    const hipError_t e = hipFuncSetAttribute((const void *)attention_window_kernel<_Float16>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    return e != hipSuccess ? e : hipFuncSetAttribute((const void *)attention_window_kernel<__bf16>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
}

template <typename T>
static hipError_t launch_attention_window_t(const void *qkv, const void *rel_h, const void *rel_w, const float *qkv_bias, void *out, int n_img, int gh, int gw, int wh, int ww, int D, int H,
                                            hipStream_t stream) {
    const int nwy = (gh + wh - 1) / wh, nwx = (gw + ww - 1) / ww, qblocks = (wh * ww + 63) / 64;
    hipLaunchKernelGGL((attention_window_kernel<T>), dim3((unsigned)((size_t)n_img * nwy * nwx * H * qblocks)), dim3(256), attention_window_lds(wh, ww), stream, (const T *)qkv,
                       (const T *)rel_h, (const T *)rel_w, qkv_bias, (T *)out, gh, gw, wh, ww, D, H, nwx, nwy * nwx, qblocks);
    return hipGetLastError();
}
hipError_t launch_attention_window(int dtype, const void *qkv, const void *rel_h, const void *rel_w, const float *qkv_bias, void *out, int n_img, int gh, int gw, int wh, int ww, int D, int H,
                                   hipStream_t stream) {
    if (!attention_window_supports(gh, gw, wh, ww, D, H) || n_img <= 0) return hipErrorInvalidValue;
    const size_t wgs = (size_t)n_img * ((gh + wh - 1) / wh) * ((gw + ww - 1) / ww) * H * ((wh * ww + 63) / 64);
    if (wgs > 0x7fffffffu) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_attention_window_t, qkv, rel_h, rel_w, qkv_bias, out, n_img, gh, gw, wh, ww, D, H, stream);
}

}  // namespace vitx
