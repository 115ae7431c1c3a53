// attention_flow.hip -- pipelined two-pass attention (bf16: one pass, running maximum), head dim 64, any token count.
#include <type_traits>

#include "kernels.h"
#include "epilogue16.h"
#include "device_common.h"

namespace vitx {

// ------------------------------------------------------------------------------------------------
// Pipelined two-pass attention (vit.cpp:826-866), any token count.  Same arithmetic as the single-pass kernel of attention_single.hip (same products,
// rounding points and summation order: bit-identical results), laid out for latency hiding instead of register residency:
//   * a workgroup = 4 waves = 4 query tiles of one (image, head); the query blocks of one (image, head) share an XCD (L2 hits
//     on the re-streamed K/V);
//   * keys stream through LDS in chunks of 64 (8 KiB K + 8 KiB V), double buffered, by LDS-DMA (buffer_load ... lds): no
//     staging registers and no VALU work -- the softmax's exp/convert instructions are what bounds this kernel.  K lands in the
//     swizzled row image (swizzle applied on the source side), V lands ROW-major and the V^T fragments of O^T = V^T P^T come
//     out of ds_read_b64_tr_b16 (a 16-lane group reads a [4 keys][16 dims] block and receives it transposed: lane i gets dim
//     i of keys 0..3, which is the k-slot order of the P registers -- tools/tr_probe.hip prints the mapping);
//   * 32 KiB of LDS and <= 128 VGPRs: four workgroups = 16 waves per CU, so the MFMA work of one wave runs under the VALU work
//     of the others (the single-pass kernel holds every score in registers: one wave per SIMD at 577 tokens).
// Pass 1 streams K for the row maxima, pass 2 streams K and V.  Keys past N inside the last chunk are never fetched: the buffer
// descriptor of the K / V DMA ends at the last row of the item's image, so they arrive as the zeros a buffer load returns out of range,
// whatever the next image holds (their scores are masked to -inf and their probabilities are exactly 0, but 0 . NaN and 0 . Inf are NaN
// in the PV product: tests/test_gpu_poison.py).
// ------------------------------------------------------------------------------------------------
// ONLINE (r04, bf16 only): ONE pass.  The reference's softmax goes through fp16 tables relative to the TRUE row maximum, which is why the F16
// builds take the maximum first; bf16 has no rounding point of the reference to reproduce there, and softmax is invariant under the per-row
// constant that is subtracted, so the bf16 build keeps a RUNNING maximum instead and never streams K a second time (64 images x 16 heads x 577
// tokens: 211 -> 160 us; ViT-L/16-384 forward +3.5 %, profiles/r04/ab_online_softmax.txt).  The constant is only moved when some row's tile maximum
// exceeds it by more than kTau (2^8 in the exponent: numerators stay <= 256, exact in bf16's range and harmless in the f32 sums) -- in practice
// during the first chunks only -- and then the accumulators and the running sum of every lane are rescaled by exp2 of its own shift.
// Rounding: P is rounded to bf16 at whatever scale it has (a relative rounding), O / sum once at the end, as before.
template <typename T, int FLAGS, bool ONLINE = false>      // FLAGS: ablation builds of tools/attn_bench.py (1 no re-staging, 2 no barriers, 4 no exp/convert, 8 no PV, 16 no pass 1); 0 = product
__global__ __launch_bounds__(256, 4) void attention_flow_kernel(const T *__restrict__ qkv, T *__restrict__ out, int N, int D, int H, int qblocks, int items) {
    static_assert(!ONLINE || std::is_same<T, __bf16>::value, "the running-maximum schedule is the bf16 build's");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int CK = 64, KBYTES = CK * 128, VBYTES = CK * 128, BUF = KBYTES + VBYTES;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // blockIdx -> (item, query block): blocks whose index is equal mod 8 run on one XCD; an item's query blocks are consecutive there
    const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
    const int item = (jb / qblocks) * 8 + xcd, qb = jb % qblocks;
    if (item >= items) return;
    const int b = item / H, h = item % H;
    const T *base = qkv + (size_t)b * N * 3 * D + h * 64;
    typedef typename Elem<T>::v8 v8;
    typedef short s4 __attribute__((ext_vector_type(4)));
    const int nch = (N + CK - 1) / CK;
    const int row_bytes = 3 * D * 2;

    const int qrow = (qb * 4 + wave) * 32 + l31;
    const bool qvalid = qrow < N;
    const bool wave_live = (qb * 4 + wave) * 32 < N;          // a wave past the last query tile only takes part in the barriers
    v8 qf[4];
    {
        const int qr = min(qrow, N - 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const v8 *)(base + (size_t)qr * 3 * D + ks * 16 + hh * 8);
    }

    // ---- LDS-DMA: physical 16-B piece p = it*256 + tid of a chunk image <-> (key row, 16-B slot) of the K / V column block
    const unsigned remaining = (unsigned)min((size_t)0xf0000000u, ((size_t)N * 3 * D - h * 64) * 2);      // from this head's column block to the end of the IMAGE
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)remaining, 0x00020000);
    int koff[2], voff[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int p = it * 256 + tid;
        int rr, sl; swz_inv(p, rr, sl);
        koff[it] = rr * row_bytes + D * 2 + sl * 16;
        const int vr = p >> 3, vs = (p & 7) ^ (((vr >> 1) & 1) << 2);          // V image: 16-B slot ^ 4 on rows 2, 3 (mod 4)
        voff[it] = vr * row_bytes + 2 * D * 2 + vs * 16;
    }
    auto stage = [&](char *buf, int key0, bool with_v) {
        char *dst = buf + wave * 1024;
        const int so = key0 * row_bytes;
#pragma unroll
        for (int it = 0; it < 2; ++it) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(dst + it * 4096), 16, koff[it], so, 0, 0);
        if (with_v) {
#pragma unroll
            for (int it = 0; it < 2; ++it) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(dst + KBYTES + it * 4096), 16, voff[it], so, 0, 0);
        }
    };
    // V^T fragment addresses: lane of a 16-lane group g = (lane >> 4) & 1 (dims 16g..16g+15 of the 32-dim tile) supplies the
    // address of key row (lane & 15) >> 2 (+ 4 hh), dims 4 (lane & 3)..+3; the tile's dt bit and the row's swizzle bit share bit 6
    int vrd[2];
    {
        const int r = 4 * hh + ((lane & 15) >> 2), rb = (r >> 1) & 1;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) vrd[dt] = KBYTES + r * 128 + ((dt ^ rb) << 6) + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
    }
    // K fragment addresses inside a chunk image: tile kt adds kt * 4096 (the swizzle term depends on l31 only)
    int krd[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) krd[ks] = swz_byte(l31, ks * 2 + hh);
    auto qk_tile = [&](const char *cur, int kt, f32x16 &s) {             // S^T tile = K tile . Q^T (4 MFMAs)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) s = Elem<T>::mfma(*(const v8 *)(cur + krd[ks] + kt * 4096), qf[ks], s);
    };
    auto mask_tile = [&](int kt, int key0, f32x16 &s) {                   // keys >= N of the last chunk: -inf
        if (key0 + kt * 32 + 32 > N) {
#pragma unroll
            for (int r = 0; r < 16; ++r) if (key0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh >= N) s[r] = -INFINITY;
        }
    };
    auto max_tile = [&](const f32x16 &s, float &m) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) m = fmaxf(fmaxf(s[r], s[r + 1]), m);        // v_max3_f32
    };

    stage(smem, 0, ONLINE);
    __builtin_amdgcn_s_waitcnt(0x0f70);       // vmcnt(0)
    __syncthreads();

    // ---- pass 1: global row maximum of the raw scores.  Chunk c is computed out of buffer c & 1 while the DMA of chunk c + 1
    // fills the other one; after the last chunk comes chunk 0 of pass 2 (with V).
    float mxs = -INFINITY;
    for (int c = 0; c < nch && !ONLINE; ++c) {
        const int key0 = c * CK;
        const char *cur = smem + (c & 1) * BUF;
        char *nxt = smem + ((c + 1) & 1) * BUF;
        const bool last = c + 1 == nch;
        if (!(FLAGS & 1) || last) stage(nxt, last ? 0 : key0 + CK, last);
        if (wave_live && !(FLAGS & 16)) {
            const int nt = min(2, (N - key0 + 31) / 32);
            for (int kt = 0; kt < nt; ++kt) {
                f32x16 s; qk_tile(cur, kt, s);
                if (last) mask_tile(kt, key0, s);
                max_tile(s, mxs);
            }
        }
        __builtin_amdgcn_s_waitcnt(0x0f70);
        if (!(FLAGS & 2) || last) __syncthreads();
    }
    if constexpr (!ONLINE) mxs = fmaxf(mxs, __shfl_xor(mxs, 32));

    // ---- pass 2: exponentials against the global maximum (ONLINE: the running one), row sum of the ROUNDED values, O^T = V^T P^T
    float sum = 0.0f;
    float nmx = -AttnExp<T>::kScale * mxs;            // ONLINE: mxs = -inf here, nmx is set by the first tile's rescale
    f32x16 o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.0f;
    auto exp_tile = [&](const f32x16 &s, v8 (&p)[2]) {      // e = round(exp(round(s/8 - max/8))) per ggml_soft_max, row sum of the rounded values
        if constexpr (FLAGS & 4) {
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const typename Pair<T>::v2 eh = round_pair<T>(s[r], s[r + 1]);
                p[r >> 3][r & 7] = eh[0]; p[r >> 3][(r & 7) + 1] = eh[1];
            }
            sum += s[0];
        } else {
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const typename Pair<T>::v2 eh = AttnExp<T>::pair(s[r], s[r + 1], nmx);
                sum = Pair<T>::sum2(eh, sum);
                p[r >> 3][r & 7] = eh[0]; p[r >> 3][(r & 7) + 1] = eh[1];
            }
        }
    };
    // The V^T fragments are read with inline asm: behind the builtin hipcc puts `s_waitcnt vmcnt(0)` in front of every transposed
    // read (it cannot tell the read from the in-flight LDS-DMA of the NEXT chunk), which exposed the whole DMA latency per chunk.
    // "=v" results + one wait statement that owns them keeps the MFMAs below the wait.
    const unsigned lds0 = (unsigned)(__UINTPTR_TYPE__)((__attribute__((address_space(3))) char *)smem);
    auto pv_tile = [&](const char *cur, int kt, const v8 (&p)[2]) {      // O^T += V^T tile . P^T tile (4 MFMAs, 8 transposed reads)
        if constexpr (FLAGS & 8) { o[0][0] += (float)p[0][0] + (float)p[1][0]; } else {
            const unsigned cb = lds0 + (unsigned)(cur - smem) + kt * 32 * 128;
            s4 f[2][2][2];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const unsigned va = cb + vrd[dt];
                asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f[dt][0][0]) : "v"(va));
                asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(f[dt][0][1]) : "v"(va));
                asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(f[dt][1][0]) : "v"(va));
                asm volatile("ds_read_b64_tr_b16 %0, %1 offset:3072" : "=v"(f[dt][1][1]) : "v"(va));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0][0][0]), "+v"(f[0][0][1]), "+v"(f[0][1][0]), "+v"(f[0][1][1]),
                                                  "+v"(f[1][0][0]), "+v"(f[1][0][1]), "+v"(f[1][1][0]), "+v"(f[1][1][1]));
            typedef short s8 __attribute__((ext_vector_type(8)));
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const s8 both = __builtin_shufflevector(f[dt][half][0], f[dt][half][1], 0, 1, 2, 3, 4, 5, 6, 7);
                    o[dt] = Elem<T>::mfma(__builtin_bit_cast(v8, both), p[half], o[dt]);
                }
        }
    };
    const int buf0 = ONLINE ? 0 : nch;                // pass 1's last stage filled buffer nch & 1: pass 2's chunk c lives in buffer (nch + c) & 1
    for (int c = 0; c < nch; ++c) {
        const int key0 = c * CK;
        const char *cur = smem + ((buf0 + c) & 1) * BUF;
        char *nxt = smem + ((buf0 + c + 1) & 1) * BUF;
        const bool last = c + 1 == nch;
        if (!last && !(FLAGS & 1)) stage(nxt, key0 + CK, true);
        if (wave_live) {
            const int nt = min(2, (N - key0 + 31) / 32);
            for (int kt = 0; kt < nt; ++kt) {
                f32x16 s; v8 p[2];
                qk_tile(cur, kt, s);
                if (last) mask_tile(kt, key0, s);
                if constexpr (ONLINE) {
                    // a processed tile holds at least one real key, so its maximum is finite; the two lanes of a query (key halves hh = 0, 1) see
                    // the same tile maximum and the same running one, hence the same shift
                    constexpr float kTau = 8.0f / AttnExp<T>::kScale;
                    float tm = -INFINITY, u, v;
                    max_tile(s, tm);
                    rows_swap32(tm, u, v); tm = fmaxf(u, v);
                    if (__builtin_amdgcn_ballot_w64(tm > mxs + kTau) != 0) {          // wave-uniform; first tile: mxs = -inf
                        const float mnew = fmaxf(mxs, tm);
                        const float sc = __builtin_amdgcn_exp2f((mxs - mnew) * AttnExp<T>::kScale);      // exp2(-inf) = 0 on the first tile
                        mxs = mnew; nmx = -AttnExp<T>::kScale * mnew;
                        sum *= sc;
#pragma unroll
                        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                            for (int r = 0; r < 16; ++r) o[dt][r] *= sc;
                    }
                }
                exp_tile(s, p); pv_tile(cur, kt, p);
            }
        }
        if (!last) { __builtin_amdgcn_s_waitcnt(0x0f70); if (!(FLAGS & 2)) __syncthreads(); }
    }
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    if (qvalid) {
        T *orow = out + ((size_t)b * N + qrow) * D + h * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                typename Elem<T>::v4 w4;
#pragma unroll
                for (int e = 0; e < 4; ++e) w4[e] = (T)(o[dt][r4 * 4 + e] * inv);
                *(typename Elem<T>::v4 *)(orow + dt * 32 + r4 * 8 + hh * 4) = w4;
            }
    }
}
template <typename T, int FLAGS>
static hipError_t launch_attention_flow_inst(const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream, bool prepare) {
    constexpr int lds = 2 * (64 * 128 + 64 * 128);        // two (8 KiB K + 8 KiB V) chunk buffers
    constexpr bool ONLINE = std::is_same<T, __bf16>::value && FLAGS == 0;
    if (prepare) return hipFuncSetAttribute((const void *)attention_flow_kernel<T, FLAGS, ONLINE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);   // device bring-up
    const int qblocks = ((N + 31) / 32 + 3) / 4, items = n_img * H;
    const int grid = ((items + 7) / 8) * 8 * qblocks;
    hipLaunchKernelGGL((attention_flow_kernel<T, FLAGS, ONLINE>), dim3(grid), dim3(256), lds, stream, (const T *)qkv, (T *)out, N, D, H, qblocks, items);
    return hipGetLastError();
}
template <typename T>
static hipError_t launch_attention_flow_t(const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream, int flags, bool prepare) {
    switch (flags) {
    case 0: return launch_attention_flow_inst<T, 0>(qkv, out, n_img, N, D, H, stream, prepare);
#ifdef VITX_LAB      // ablation builds of tools/attn_bench.py (results are garbage by design)
    case 1: return launch_attention_flow_inst<T, 1>(qkv, out, n_img, N, D, H, stream, prepare);
    case 2: return launch_attention_flow_inst<T, 2>(qkv, out, n_img, N, D, H, stream, prepare);
    case 4: return launch_attention_flow_inst<T, 4>(qkv, out, n_img, N, D, H, stream, prepare);
    case 8: return launch_attention_flow_inst<T, 8>(qkv, out, n_img, N, D, H, stream, prepare);
    case 16: return launch_attention_flow_inst<T, 16>(qkv, out, n_img, N, D, H, stream, prepare);
#endif
    default: return hipErrorInvalidValue;
    }
}
hipError_t launch_attention_flow(int dtype, const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream, int flags) {
    return VITX_BY_DTYPE(dtype, launch_attention_flow_t, qkv, out, n_img, N, D, H, stream, flags, false);
}
hipError_t prepare_attention_flow() {       // the product build of both types; the ablation builds fit the default 64 KiB
    for (int dt = 0; dt < 2; ++dt) {
        const hipError_t e = VITX_BY_DTYPE(dt, launch_attention_flow_t, nullptr, nullptr, 0, 64, 64, 1, nullptr, 0, true);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace vitx
