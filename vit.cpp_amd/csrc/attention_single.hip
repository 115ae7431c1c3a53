// attention_single.hip -- single-pass attention, head dim 64: every score of a query tile stays in registers (up to 608 tokens).
#include "kernels.h"
#include "epilogue16.h"
#include "device_common.h"

namespace vitx {

// ------------------------------------------------------------------------------------------------
// Fused attention for one (image, head) per workgroup (vit.cpp:826-866): S = K Q^T * 1/8, softmax
// over keys, O = P V, heads merged on store.  head_dim is 64 for every model the reference converts.
//   * K [Nk][64] is staged in LDS in the swizzled row image above, V is staged TRANSPOSED
//     ([64][Nk+8], keys permuted inside each group of 16 so that the MFMA k-slot order of the P
//     registers needs no shuffle).
//   * "swapped" products: S^T = K . Q^T puts a whole score column (one query) in one lane pair, so the
//     softmax max/sum are in-register reductions plus one cross-half shuffle; O^T = V^T . P^T then
//     takes the probabilities straight from the accumulator registers as its B operand.
//   * each wave owns 32 queries; all NKT key tiles are kept in registers (single pass, no online
//     rescale), which fits N <= 608 tokens.
// exp follows ggml_soft_max: e = round(exp(round(s - max))) in the operand type (fp16 LUT in ggml).
// ------------------------------------------------------------------------------------------------
template <typename T, int NKT, int NWAVES>
__global__ __launch_bounds__(NWAVES * 64, (NKT <= 9 && NWAVES <= 4) ? 2 : 1) void attention_kernel(const T *__restrict__ qkv, T *__restrict__ out, int N, int D, int H) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = NWAVES * 64;
    constexpr int NK = NKT * 32;          // padded key count
    constexpr int VLD = NK + 8;           // V^T row stride (elements); (VLD/8) odd -> conflict-free b128 reads
    char *Ks = smem;
    T *VT = (T *)(smem + NK * 128);
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const T *base = qkv + (size_t)b * N * 3 * D + h * 64;
    typedef typename Elem<T>::v8 v8;

    // ---- this wave's first query fragments: issued first so their latency hides under the K/V staging
    auto load_q = [&](int qt, v8 (&qf)[4]) {
        const int qrow = min(qt * 32 + l31, N - 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const v8 *)(base + (size_t)qrow * 3 * D + ks * 16 + hh * 8);
    };
    constexpr bool QPREF = NKT <= 9;      // longer sequences have no registers to spare for a prefetched Q tile
    v8 qf[4];
    if (QPREF && wave < NKT) load_q(wave, qf);

    // ---- stage K: 16-B pieces in row order (coalesced 128-B rows), all loads issued before the LDS writes
    {
        constexpr int IT = (NK * 8 + NT - 1) / NT;
        v8 kv[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = it * NT + tid, key = c >> 3, sl = c & 7;
#pragma unroll
            for (int j = 0; j < 8; ++j) kv[it][j] = (T)0.0f;
            if (c < NK * 8 && key < N) kv[it] = *(const v8 *)(base + (size_t)key * 3 * D + D + sl * 8);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = it * NT + tid;
            if (c < NK * 8) *(v8 *)(Ks + swz_byte(c >> 3, c & 7)) = kv[it];
        }
    }
    // ---- stage V^T: one work item = (key pair, 8 head dims).  Consecutive lanes take consecutive key pairs, so
    // each of the 8 transposed stores is a 4-byte (two keys) write to consecutive dwords of one V^T row (no bank
    // conflicts); keys 4-7 <-> 8-11 of every 16 are swapped (MFMA k-slot order of the P registers).
    {
        constexpr int NP = NK / 2, ITEMS = NP * 8, IT = (ITEMS + NT - 1) / NT;
        v8 va[IT], vb[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = it * NT + tid, pr = c % NP, sl = c / NP, key = 2 * pr;
#pragma unroll
            for (int j = 0; j < 8; ++j) { va[it][j] = (T)0.0f; vb[it][j] = (T)0.0f; }
            if (c < ITEMS && key < N) va[it] = *(const v8 *)(base + (size_t)key * 3 * D + 2 * D + sl * 8);
            if (c < ITEMS && key + 1 < N) vb[it] = *(const v8 *)(base + (size_t)(key + 1) * 3 * D + 2 * D + sl * 8);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = it * NT + tid, pr = c % NP, sl = c / NP, key = 2 * pr;
            if (c >= ITEMS) continue;
            const int a = key & 15, q4 = a >> 2, q4s = (q4 == 1) ? 2 : (q4 == 2) ? 1 : q4;
            const int pos = (key & ~15) | (q4s << 2) | (a & 3);
            typedef T v2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int j = 0; j < 8; ++j) *(v2 *)(VT + (sl * 8 + j) * VLD + pos) = v2{va[it][j], vb[it][j]};
        }
    }
    __syncthreads();

#pragma unroll 1
    for (int qt = wave; qt < NKT; qt += NWAVES) {
        int lds_off = 0;
        asm volatile("" : "+v"(lds_off));   // opaque zero: keeps the (query-independent) K / V^T fragment reads inside the loop instead of hoisted into ~220 live registers
        const int qrow = qt * 32 + l31;
        const bool qvalid = qrow < N;
        if (!QPREF) load_q(qt, qf);

        // S^T tiles: rows = keys, cols = queries
        f32x16 s[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kt][r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const v8 kf = *(const v8 *)(Ks + lds_off + swz_byte(kt * 32 + l31, ks * 2 + hh));
                s[kt] = Elem<T>::mfma(kf, qf[ks], s[kt]);
            }
        }
        if (QPREF && qt + NWAVES < NKT) load_q(qt + NWAVES, qf);       // next query tile of this wave: in flight during softmax + PV
        // mask padded keys, max of the raw scores; the 2^-3 scale is exact, so fma(s, 1/8, -max/8) == s/8 - max/8
        float mxs = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (kt == NKT - 1) {       // only the last key tile can hold padded keys
                    const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                    if (key >= N) s[kt][r] = -INFINITY;
                }
                mxs = fmaxf(mxs, s[kt][r]);
            }
        mxs = fmaxf(mxs, __shfl_xor(mxs, 32));
        const float nmx = -AttnExp<T>::kScale * mxs;
        // e = round(exp(round(s/8 - max))) per ggml_soft_max, two keys per packed convert; exp(-inf) = 0 for padded keys.
        // The row sum adds the ROUNDED values (as ggml does) with one v_dot2c per pair.
        float sum = 0.0f;
        v8 p[NKT][2];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const typename Pair<T>::v2 eh = AttnExp<T>::pair(s[kt][r], s[kt][r + 1], nmx);
                sum = Pair<T>::sum2(eh, sum);
                p[kt][r >> 3][r & 7] = eh[0]; p[kt][r >> 3][(r & 7) + 1] = eh[1];
            }
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;

        // O^T = V^T . P^T : rows = head dims (2 tiles of 32), cols = queries
        f32x16 o[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] = 0.0f;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const v8 vf = *(const v8 *)((const char *)(VT + (dt * 32 + l31) * VLD + kt * 32 + half * 16 + hh * 8) + lds_off);
                    o[dt] = Elem<T>::mfma(vf, p[kt][half], o[dt]);
                }
        }
        if (qvalid) {
            T *orow = out + ((size_t)b * N + qrow) * D + h * 64;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    typename Elem<T>::v4 w4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) w4[j] = (T)(o[dt][r4 * 4 + j] * inv);
                    *(typename Elem<T>::v4 *)(orow + dt * 32 + r4 * 8 + hh * 4) = w4;
                }
        }
    }
}

template <typename T, int NKT, int NWAVES>
static hipError_t launch_attention_inst(const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream, bool prepare) {
    constexpr int lds = NKT * 32 * 128 + 64 * (NKT * 32 + 8) * 2;
    if (prepare) return hipFuncSetAttribute((const void *)attention_kernel<T, NKT, NWAVES>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);   // device bring-up
    hipLaunchKernelGGL((attention_kernel<T, NKT, NWAVES>), dim3(n_img * H), dim3(NWAVES * 64), lds, stream, (const T *)qkv, (T *)out, N, D, H);
    return hipGetLastError();
}
template <typename T>
static hipError_t launch_attention_t(const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream, bool prepare) {
    const int nkt = (N + 31) / 32;
    switch (nkt) {
    case 1: return launch_attention_inst<T, 1, 1>(qkv, out, n_img, N, D, H, stream, prepare);
    case 2: return launch_attention_inst<T, 2, 2>(qkv, out, n_img, N, D, H, stream, prepare);
    case 3: return launch_attention_inst<T, 3, 3>(qkv, out, n_img, N, D, H, stream, prepare);
    case 4: return launch_attention_inst<T, 4, 4>(qkv, out, n_img, N, D, H, stream, prepare);
    case 5: return launch_attention_inst<T, 5, 4>(qkv, out, n_img, N, D, H, stream, prepare);
    case 6: return launch_attention_inst<T, 6, 4>(qkv, out, n_img, N, D, H, stream, prepare);
    // 197 tokens (224/16): 4 waves x 2 query tiles, two workgroups per CU (one stages K/V while the other computes): 109 us vs 124 us for
    // one 7-wave workgroup per CU on 256 x 12 heads (r01)
    case 7: return launch_attention_inst<T, 7, 4>(qkv, out, n_img, N, D, H, stream, prepare);
    case 9: return launch_attention_inst<T, 9, 4>(qkv, out, n_img, N, D, H, stream, prepare);      // 257 tokens (224/14)
    case 19: return launch_attention_inst<T, 19, 4>(qkv, out, n_img, N, D, H, stream, prepare);    // 577 tokens (384/16)
    default: return hipErrorInvalidValue;
    }
}

static const int kAttnNkt[] = {1, 2, 3, 4, 5, 6, 7, 9, 19};      // instantiated key-tile counts (tokens = 32 * nkt, rounded up)
bool attention_single_pass_supports(int N) {
    const int nkt = (N + 31) / 32;
    for (int k : kAttnNkt) if (k == nkt) return true;
    return false;
}
hipError_t launch_attention_single(int dtype, const void *qkv, void *out, int n_img, int N, int D, int H, hipStream_t stream) {
    return VITX_BY_DTYPE(dtype, launch_attention_t, qkv, out, n_img, N, D, H, stream, false);
}
hipError_t prepare_attention_single() {
    for (int dt = 0; dt < 2; ++dt)
        for (int nkt : kAttnNkt) {
            const hipError_t e = VITX_BY_DTYPE(dt, launch_attention_t, nullptr, nullptr, 0, nkt * 32, 64, 1, nullptr, true);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

}  // namespace vitx
