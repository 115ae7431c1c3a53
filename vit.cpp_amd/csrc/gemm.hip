// gemm.hip -- the v1 128 x 128 GEMM (today: its q4_0 form) and the GEMM dispatcher that picks a kernel family for a shape;
// device bring-up of every GEMM family (prepare_gemm).
#include <algorithm>

#include "kernels.h"
#include "epilogue16.h"
#include "device_common.h"
#include "ln_row.h"      // LN_MAX_TILES: the widths the LayerNorm-fusing GEMM takes

namespace vitx {

// ------------------------------------------------------------------------------------------------
// GEMM  C[M][N] = A[M][K] . W[N][K]^T  (ggml_mul_mat, vit.cpp:820,868,889,896,927 and the im2col GEMM
// of ggml_conv_2d_sk_p0, vit.cpp:772) with the bias / GELU / residual / pos-embed epilogues fused.
// 128x128x64 tile, 4 waves (2x2), each wave 64x64 = 4x4 tiles of MFMA 16x16x32, LDS double buffer filled
// by global_load_lds dwordx4 (one K-tile ahead).
// ------------------------------------------------------------------------------------------------
constexpr int GBM = 128, GBN = 128, GBK = 64;
constexpr int G_TILE_BYTES = GBM * GBK * 2;            // 16 KiB per operand tile
constexpr int G_STAGE_BYTES = 2 * G_TILE_BYTES;        // A + W
constexpr int G_LDS_BYTES = 2 * G_STAGE_BYTES;         // double buffer: 64 KiB

// Q4 = true: W stays in ggml q4_0 block form in HBM (GemmArgs::W = nibble plane, ::Wscale = f16 block scales, 4.5 bits per weight) and
// is expanded in the LDS-fill path: every thread loads ONE block (16 B of nibbles + its scale) of the next K-tile into registers
// while the current K-tile is multiplied, then writes (q - 8) * d, rounded once to the operand type exactly as the host-side
// expansion does (HostTensor::decode_f32 + RNE), into the same swizzled LDS image the LDS-DMA path produces.  The reference keeps
// quantised weights through compute the same way (ggml_mul_mat on a q4_0 src0: /root/reference/vit.cpp:645-678, 820).
typedef unsigned q4_u32x4 __attribute__((ext_vector_type(4)));
template <typename T, int EPI, bool Q4 = false>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g4 = lane >> 4;

    // XCD-aware tile order: blocks b, b+8, b+16, ... (same XCD, co-resident) get consecutive tile ids,
    // which share the same A row panel (n fastest).  Bijective for any grid size.
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const int tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    const int ntn = g.N_pad / GBN;
    const int m0 = (tile / ntn) * GBM, n0 = (tile % ntn) * GBN;

    const T *A = (const T *)g.A, *W = (const T *)g.W;
    // per-thread source offsets of the 4+4 16-byte pieces this thread DMA-loads per K tile
    int aoff[4], woff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int row, slot; swz_inv(i * 256 + tid, row, slot);
        aoff[i] = (m0 + row) * g.lda + slot * 8;
        woff[i] = (n0 + row) * g.ldw + slot * 8;
    }
    auto stage = [&](int buf, int k0) {
        char *base = smem + buf * G_STAGE_BYTES + wave * 1024;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds(GPTR(A + aoff[i] + k0), LPTR(base + i * 4096), 16, 0, 0);
            if constexpr (!Q4) __builtin_amdgcn_global_load_lds(GPTR(W + woff[i] + k0), LPTR(base + G_TILE_BYTES + i * 4096), 16, 0, 0);
        }
    };
    // q4_0 path: thread -> (tile row tid / 2, block tid % 2 of the 64-deep K-tile)
    const int q_row = tid >> 1, q_kb = tid & 1;
    const int q_nbk = g.K >> 5;
    const unsigned char *q_qs = (const unsigned char *)g.W + (size_t)(n0 + q_row) * q_nbk * 16;
    const uint16_t *q_d = g.Wscale + (size_t)(n0 + q_row) * q_nbk;
    q4_u32x4 q_regs = {0, 0, 0, 0}; uint16_t q_scale = 0;
    auto load_q4 = [&](int kt) {
        const int b = kt * 2 + q_kb;
        q_regs = *(const q4_u32x4 *)(q_qs + (size_t)b * 16);
        q_scale = q_d[b];
    };
    auto write_q4 = [&](int buf) {
        const float d = (float)__builtin_bit_cast(_Float16, q_scale);
        char *wt = smem + buf * G_STAGE_BYTES + G_TILE_BYTES;
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) {        // block elements 8 sl .. 8 sl + 7: low nibbles of bytes 0-15 first, then the high nibbles (block_q4_0)
            typename Elem<T>::v8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int byte = (sl & 1) * 8 + e;
                const unsigned w = q_regs[byte >> 2] >> ((byte & 3) * 8);
                const int nib = (sl < 2) ? (int)(w & 15u) : (int)((w >> 4) & 15u);
                v[e] = (T)((float)(nib - 8) * d);
            }
            *(typename Elem<T>::v8 *)(wt + swz_byte(q_row, q_kb * 4 + sl)) = v;
        }
    };

    const int wm = wave >> 1, wn = wave & 1;
    f32x4 acc[4][4];                                  // the wave's 64 x 64 block as 4 x 4 tiles of v_mfma_f32_16x16x32 (epilogue16.h)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[t][u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // fragment read addresses: row = w*64 + t*16 + l15, 16-byte slot = k2*4 + g4 (k-step k2 = 32 of the K-tile's 64)
    int a_rd[4][2], w_rd[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            a_rd[t][k2] = swz_byte(wm * 64 + t * 16 + l15, k2 * 4 + g4);
            w_rd[t][k2] = G_TILE_BYTES + swz_byte(wn * 64 + t * 16 + l15, k2 * 4 + g4);
        }

    const int nk = g.K / GBK;
    stage(0, 0);
    if constexpr (Q4) { load_q4(0); write_q4(0); }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) { stage(cur ^ 1, (kt + 1) * GBK); if constexpr (Q4) load_q4(kt + 1); }
        const char *sb = smem + cur * G_STAGE_BYTES;
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            typename Elem<T>::v8 af[4], wf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = *(const typename Elem<T>::v8 *)(sb + a_rd[t][k2]);
                wf[t] = *(const typename Elem<T>::v8 *)(sb + w_rd[t][k2]);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[t][u] = Elem<T>::mfma16(wf[u], af[t], acc[t][u]);
        }
        if constexpr (Q4) { if (kt + 1 < nk) write_q4(cur ^ 1); }     // the other buffer: every wave finished reading it before the previous barrier
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // every wave is past the last K-tile's barrier: the staging buffers are free, each wave takes 4 KiB as its epilogue patch
    const bool full = (m0 + GBM <= g.M_real) && (n0 + GBN <= g.N);
    epilogue16_tile<T, EPI, 2>(g, acc, full, m0, n0, wm * 64, wn * 64, smem + wave * 4096, lane);
}

int gemm_tile_m() { return 256; }   // row padding of every activation buffer (ring kernel tile height)
int gemm_tile_n() { return GBN; }

template <typename T, bool Q4 = false>
static hipError_t launch_gemm_t(int epi, const GemmArgs &a, hipStream_t stream, bool prepare) {
    const int grid = prepare ? 1 : (a.M / GBM) * (a.N_pad / GBN);
    const dim3 blk(256);
#define VITX_GEMM_CASE(E)                                                                                   \
    case E: {                                                                                               \
        if (prepare) return hipFuncSetAttribute((const void *)gemm_nt_kernel<T, E, Q4>, hipFuncAttributeMaxDynamicSharedMemorySize, G_LDS_BYTES); \
        hipLaunchKernelGGL((gemm_nt_kernel<T, E, Q4>), dim3(grid), blk, G_LDS_BYTES, stream, a);            \
    } break;
    switch (epi) {
        VITX_GEMM_CASE(EPI_BIAS)
        VITX_GEMM_CASE(EPI_BIAS_GELU)
        VITX_GEMM_CASE(EPI_BIAS_RESID)
        VITX_GEMM_CASE(EPI_BIAS_F32)
        VITX_GEMM_CASE(EPI_PATCH)
        VITX_GEMM_CASE(EPI_BIAS_HILO)
        VITX_GEMM_CASE(EPI_BIAS_GELU_ERF)
        VITX_GEMM_CASE(EPI_BIAS_QGELU)
    default: return hipErrorInvalidValue;
    }
#undef VITX_GEMM_CASE
    return hipGetLastError();
}

// Kernel selection (t.gemm_cfg: an explicit family, set by vitx_op_gemm_ex for the parity tests).
//   * >= 128 tiles of 256x256 and K % 128 == 0: the ping-pong persistent kernel (gemm_pp.hip);
//   * otherwise 128x256 ring tiles, or the skinny 64x128 ring kernel when those would leave half of the CUs idle
//     (a handful of images: same K order per element, so results stay bit-identical across batch sizes);
//   * a column count that is a multiple of 128 but not of 256: the skinny ring tiles at any row count.
static int wide_ring_cfg(const GemmArgs &a) { return gemm_ring_supports(a, 945) ? 945 : 445; }

// Persistent grid of the ping-pong kernel.  Tiles are dealt round-robin, so with one workgroup per CU a partial last round
// (e.g. 339 tiles = 256 + 83) leaves most of the chip idle while the first round ran at the power-capped clock.  Balanced:
// rounds = ceil(tiles / CUs), grid = ceil(tiles / rounds) rounded up to the 8 XCDs -- every workgroup walks the same number
// of tiles, fewer CUs are lit at a higher clock (the GEMM is energy-bound: half the CUs deliver 76 % of the throughput),
// and the CUs left free take the other sub-batch's kernels.
static int pp_grid(const Tuning &t, const GemmArgs &a) {
    int cap = t.n_cu & ~7;
    if (cap <= 0) cap = 256;
    const long ntiles = (long)(a.M / 256) * (a.N_pad / 256);
    if (!t.gemm_balance || ntiles <= cap) return cap;
    const long rounds = (ntiles + cap - 1) / cap;
    const long g = ((ntiles + rounds - 1) / rounds + 7) & ~7L;
    return (int)(g < cap ? g : cap);
}

static bool is_wide(const GemmArgs &a) {
    const long t256 = (long)(a.M / 256) * (a.N_pad / 256);
    return a.M % 256 == 0 && a.N_pad % 256 == 0 && t256 >= 128 && (gemm_pp_supports(a) || gemm_ring_supports(a, 445));
}
int gemm_pp_ln_grid(int n_cu, int M, int N);      // gemm_pp.hip
int gemm_ln_grid(int n_cu, int M, int N) { return gemm_pp_ln_grid(n_cu, M, N); }
bool gemm_ln_fusable(const Tuning &t, const GemmArgs &a) {
    // the peer mapping of pp_epilogue_ln (bid & 7 = XCD, whole row blocks per XCD) is built for the 8 XCDs of an MI355X in SPX mode: any
    // other partitioning (CPX / a different part) takes the stand-alone LayerNorm -- same bits, no spinning on peers that are elsewhere
    return t.n_xcd == 8 && t.n_cu % 8 == 0 && t.gemm_cfg < 0 && !t.gemm_split && !t.pp_flags && a.M > 0 && is_wide(a) && gemm_pp_supports(a) && a.N == a.ldo && a.N == a.N_pad && a.N % 256 == 0 &&
           a.N / 256 <= LN_MAX_TILES && (size_t)a.M * a.ldo * 4 < 0xf0000000u;
}
bool gemm_fix_capable(const Tuning &t, const GemmArgs &a) {
    return t.gemm_cfg < 0 && !t.gemm_split && !t.pp_flags && a.M > 0 && is_wide(a) && gemm_pp_supports(a) && a.K == a.lda && a.K % 256 == 0 && a.K / 256 <= LN_MAX_TILES;
}
static hipError_t launch_wide(const Tuning &t, int dtype, int epi, const GemmArgs &a0, hipStream_t stream) {
    GemmArgs a = a0; a.group_m = t.group_m;
    // Raster of the qkv / fc1 launches (r05, profiles/r05/raster_sweep.txt): an XCD walks groups of group_m row blocks x all column tiles.  While the
    // whole weight matrix fits beside the A panels in the XCD's 4 MiB L2 (+ a little: ViT-B qkv 3.4 MiB, fc1 4.5 MiB), group_m = 1 -- every CU of the
    // XCD on the same few row blocks, W resident, A streamed once -- is 0.4-0.7 % of the ViT-B forward faster than 8 (two independent A/Bs, same
    // bits); with ViT-L's matrices (6 / 8 MiB) it is 0.6 % slower, so they keep the A-resident groups of 8.
    if (!a.group_m && !a.ln && (epi == EPI_BIAS || epi == EPI_BIAS_HILO || epi_is_act(epi))) a.group_m = ((size_t)a.N_pad * a.K * 2 <= ((size_t)5 << 20)) ? 1 : 8;
    if (a.ln) return (epi == EPI_BIAS_RESID && gemm_ln_fusable(t, a)) ? launch_gemm_pp(dtype, epi, a, t.n_cu, stream, 0) : hipErrorInvalidValue;
    if (gemm_pp_supports(a)) return launch_gemm_pp(dtype, epi, a, pp_grid(t, a), stream, t.pp_flags);
    return launch_gemm_ring(t, dtype, epi, a, wide_ring_cfg(a), stream);
}

// The ring tiling of a shape that is not wide (0: none): 128 x 256 tiles, or the skinny 64 x 128 ones when those would leave half of the CUs idle.
// A column count that is a multiple of 128 but not of 256 takes the 64 x 128 tiles at any row count (the v1 128 x 128 kernel used to take
// these; it now exists only in its q4_0 form, launch_gemm_q4).  launch_gemm's rule, stated once: a text context pins it per GEMM (text_forward.cpp).
int gemm_ring_cfg(const Tuning &t, const GemmArgs &a) {
    int cfg = 245;
    if ((long)(a.M / 128) * (a.N_pad / 256) < t.skinny_tiles && gemm_ring_supports(a, 122)) cfg = 122;
    if (gemm_ring_supports(a, cfg)) return cfg;
    return gemm_ring_supports(a, 122) ? 122 : 0;
}

hipError_t launch_gemm(const Tuning &t, int dtype, int epi, const GemmArgs &a, hipStream_t stream) {
    if (a.M <= 0) return hipErrorInvalidValue;
    if (a.ln && !gemm_ln_fusable(t, a)) return hipErrorInvalidValue;      // the caller asks gemm_ln_fusable first
    if (a.fix && !gemm_fix_capable(t, a)) return hipErrorInvalidValue;     // ... and gemm_fix_capable
    int cfg = t.gemm_cfg;
    if (cfg == 1) return launch_gemm_pp(dtype, epi, a, pp_grid(t, a), stream, t.pp_flags);
    if (cfg > 1) return gemm_ring_supports(a, cfg) ? launch_gemm_ring(t, dtype, epi, a, cfg, stream) : hipErrorInvalidValue;
    if (is_wide(a)) {
        // Tail split (t.gemm_split; off: with the persistent kernel the second launch costs 5 % of the step, profiles/r02_forward_sweeps.txt,
        // re-measured with the 16x16x32 kernels in r02f): rows that fill whole rounds keep 256x256 tiles, the remaining rows are re-tiled
        // 128x256 (half-cost tiles) in a second launch.  Kept reachable through vitx_op_gemm_ex(kernel 2) so the path stays tested.
        const int ntm = a.M / 256, ntn = a.N_pad / 256;
        const long tiles = (long)ntm * ntn, rounds = tiles / t.n_cu, rem = tiles % t.n_cu;
        if (t.gemm_split && epi != EPI_PATCH && rounds >= 1 && rem > 0 && rem <= t.n_cu * 6 / 10) {
            const int m_main = (int)((rounds * t.n_cu) / ntn);                 // m-tiles that fit in whole rounds
            const int rows_main = m_main * 256;
            GemmArgs head = a, tail = a;
            head.M = rows_main; head.M_real = std::min(a.M_real, rows_main);
            tail.A = (const char *)a.A + (size_t)rows_main * a.lda * 2;
            tail.out = (char *)a.out + (size_t)rows_main * a.ldo * epi_out_bytes(epi);
            tail.M = a.M - rows_main; tail.M_real = a.M_real - rows_main;
            if (m_main >= 1 && rows_main < a.M && gemm_ring_supports(tail, 245)) {
                hipError_t e = launch_wide(t, dtype, epi, head, stream);
                if (e != hipSuccess) return e;
                if (tail.M_real <= 0) return hipSuccess;
                return launch_gemm_ring(t, dtype, epi, tail, 245, stream);
            }
        }
        return launch_wide(t, dtype, epi, a, stream);
    }
    cfg = gemm_ring_cfg(t, a);
    return cfg ? launch_gemm_ring(t, dtype, epi, a, cfg, stream) : hipErrorInvalidValue;
}

bool gemm_q4_supports(const GemmArgs &a) { return a.Wscale && a.M > 0 && a.M % GBM == 0 && a.N_pad % GBN == 0 && a.K % GBK == 0; }
hipError_t launch_gemm_q4(int dtype, int epi, const GemmArgs &a, hipStream_t stream) {
    if (!gemm_q4_supports(a)) return hipErrorInvalidValue;
    return VITX_BY_DTYPE2(dtype, launch_gemm_t, true, epi, a, stream, false);
}

// Device bring-up of every GEMM instantiation: the families enumerate theirs through their own dispatch switches (`prepare`)
hipError_t prepare_gemm(const Tuning &t) {
    GemmArgs none{};
    hipError_t e;
    for (int dt = 0; dt < 2; ++dt) {
        for (int epi = 0; epi < EPI_COUNT; ++epi) {
            for (int cfg : {945, 445, 245, 122}) if ((e = launch_gemm_ring(t, dt, epi, none, cfg, nullptr, true)) != hipSuccess) return e;
            if ((e = launch_gemm_pp(dt, epi, none, t.n_cu, nullptr, 0, true)) != hipSuccess) return e;
#ifdef VITX_LAB
            for (int nw : {4, 8}) if ((epi == EPI_BIAS || epi == EPI_BIAS_GELU) && (e = launch_gemm_w4(dt, epi, none, t.n_cu, nullptr, 0, true, nw)) != hipSuccess) return e;
#endif
            if ((e = VITX_BY_DTYPE2(dt, launch_gemm_t, true, epi, none, nullptr, true)) != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace vitx
