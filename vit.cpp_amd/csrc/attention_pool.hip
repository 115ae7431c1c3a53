// attention_pool.hip -- the pooling pass of the attention-pooling (MAP) head of a SigLIP-class model (the contract: include/vitx.h "no class
// token and the attention-pooling head").
//
// The probe of the head is a constant of the model, so its K projection folds into one vector per head, u_h = Wk_h^T q_h / sqrt(d) (host, at
// context creation), and -- because the softmax weights sum to 1 -- the V projection commutes with the weighted sum.  What is left per image is
// one pass over the f32 residual stream:
//     F[t]   = the final-norm row of token t (LnRow::norm, ln_row.h: the row of features.hip, unrounded)
//     s[h,t] = u_h . F[t];   p_h = softmax_t(s_h);   M_h = sum_t p[h,t] F[t]            -- all f32, M is [H][D]
//
// One workgroup of 4 waves per (image, head group): heads go in groups of HG, HG x D / 64 accumulators per lane within kPoolAcc registers, and the
// groups of an image run as workgroups of their own (grid.y), each walking the image's rows -- the first read comes from HBM, the others hit
// L2.  Measured on ViT-B/16 at batch 256 (profiles/map_head_cost.txt): all 12 heads in one workgroup (144 accumulators, one wave per SIMD at
// 350 registers) 254 us per launch; groups of 4 heads (48 accumulators, 168 registers, 3 waves per SIMD) 186 us: the pass is bound by its
// dependent cross-lane and LDS round trips, not by memory, and more resident waves hide them.  Per workgroup:
//   * u of the group is staged in LDS once;
//   * wave w takes rows w, w + 4, ... in ascending order, two at a time up to 1024 columns (both rows' loads are issued before either is used
//     and one read of u from LDS serves both).  Per row and head: the lane's partial dot in column order, a 6-step butterfly (the same bits in
//     every lane; the exchanges of all heads go together), then the online softmax (exp = the hardware's exp2 of x log2 e): a running maximum m,
//     the sum l (wave-uniform: kept in LDS) and the accumulators are rescaled by exp(m - m') when m grows;
//   * the 4 waves' (m, l, acc) are combined in wave order: the group maximum, every wave's exp(m_w - m), L = ((l_0' + l_1') + ...), and the
//     rescaled accumulators added into one LDS block in wave order; M = block / L.
// An image's M is a function of its own rows, N, D and H only: nothing depends on the batch or on the position in it, and there are no atomics.
// p (optional): the raw scores are parked in the output during the pass and turned into exp(s - m) / L by the workgroup once m and L are known.
#include "device_common.h"
#include "ln_row.h"
#include "kernels.h"

namespace vitx {

namespace {

constexpr int kPoolWaves = 4;
constexpr int kPoolAcc = 48;          // accumulator registers per lane of one head group (24: 253 us, 48: 186 us, 144: 254 us at ViT-B, batch 256)
// heads per group
constexpr int pool_group(int cpl) { return kPoolAcc / cpl < 1 ? 1 : (kPoolAcc / cpl > 12 ? 12 : kPoolAcc / cpl); }      // at most 12: the scores of a step are registers too

template <int VEC, int NV, typename T16>
__global__ __launch_bounds__(kPoolWaves * 64) void attention_pool_kernel(const float *__restrict__ x, long row_stride, long img_stride, const float *__restrict__ w,
                                                                         const float *__restrict__ b, float eps, const float *__restrict__ u, float *__restrict__ M,
                                                                         T16 *__restrict__ m16, float *__restrict__ p, int N, int H) {
    typedef LnRow<VEC, NV> R;
    constexpr int D = 64 * VEC * NV, CPL = VEC * NV, HG = pool_group(CPL), W = kPoolWaves;
    constexpr int U = D <= 1024 ? 2 : 1;          // rows per step of a wave
    __shared__ __attribute__((aligned(16))) float blk[HG * D];      // u of the group during the pass, then the combined accumulators
    __shared__ float stat[W][HG][2];                                 // every wave's running (m, l): wave-uniform, so they live here, not in registers
    __shared__ float fin[HG][2];                                     // the group's (m, L)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *xi = x + (size_t)blockIdx.x * img_stride;
    const size_t img = blockIdx.x;
    const float NEG = -__builtin_inff();
    volatile float *st = &stat[wave][0][0];

    {
        const int h0 = blockIdx.y * HG;           // one workgroup per (image, head group)
        const int hg = H - h0 < HG ? H - h0 : HG;
        for (int i = threadIdx.x; i < hg * D; i += W * 64) blk[i] = u[(size_t)h0 * D + i];
        if (lane < HG) { st[2 * lane] = NEG; st[2 * lane + 1] = 0.0f; }
        __syncthreads();
        float acc[HG][NV][VEC];
#pragma unroll
        for (int j = 0; j < HG; ++j)
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[j][i][e] = 0.0f;
        float f[U][NV][VEC];
#pragma unroll
        for (int r = 0; r < U; ++r)
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int e = 0; e < VEC; ++e) f[r][i][e] = 0.0f;
        for (int t = wave; t < N; t += U * W) {
#pragma unroll
            for (int r = 0; r < U; ++r)
                if (t + r * W < N) R::norm(xi + (size_t)(t + r * W) * row_stride, w, b, eps, lane, f[r]);
            const bool two = U > 1 && t + W < N;
            // the scores of all heads of the group first: the partial dots, then ONE butterfly over all of them (6 steps of independent exchanges,
            // not a dependent chain per head: with one wave per SIMD nothing else hides a cross-lane round trip)
            float s[HG][U];
#pragma unroll
            for (int j = 0; j < HG; ++j) {
#pragma unroll
                for (int r = 0; r < U; ++r) s[j][r] = 0.0f;
                if (j < hg) {
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        const float *up = blk + j * D + R::col(i, lane);
                        float uv[VEC];
                        if constexpr (VEC == 4) { const f32x4 q = *(const f32x4 *)up; uv[0] = q[0]; uv[1] = q[1]; uv[2] = q[2]; uv[3] = q[3]; }
                        else if constexpr (VEC == 2) { const f32x2 q = *(const f32x2 *)up; uv[0] = q[0]; uv[1] = q[1]; }
                        else uv[0] = up[0];
#pragma unroll
                        for (int e = 0; e < VEC; ++e)
#pragma unroll
                            for (int r = 0; r < U; ++r) s[j][r] += uv[e] * f[r][i][e];
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
#pragma unroll
                for (int j = 0; j < HG; ++j)
#pragma unroll
                    for (int r = 0; r < U; ++r) s[j][r] += __shfl_xor(s[j][r], o);
#pragma unroll
            for (int j = 0; j < HG; ++j) {
                if (j < hg) {
                    if (p && lane == 0) {
                        float *pr = p + (img * H + h0 + j) * (size_t)N;
                        pr[t] = s[j][0];
                        if (two) pr[t + W] = s[j][U - 1];
                    }
                    const float mo = st[2 * j];
                    float lj = st[2 * j + 1];
                    float mn = fmaxf(mo, s[j][0]);
                    if (two) mn = fmaxf(mn, s[j][U - 1]);
                    if (mn > mo) {                // uniform: s is the same in every lane
                        const float sc = __expf(mo - mn);     // exp(-inf) = 0 on the first row: the accumulators are zero anyway
                        lj = lj * sc;
#pragma unroll
                        for (int i = 0; i < NV; ++i)
#pragma unroll
                            for (int e = 0; e < VEC; ++e) acc[j][i][e] = acc[j][i][e] * sc;
                    }
#pragma unroll
                    for (int r = 0; r < U; ++r) {
                        if (r > 0 && !two) continue;
                        const float pe = __expf(s[j][r] - mn);
                        lj = lj + pe;
#pragma unroll
                        for (int i = 0; i < NV; ++i)
#pragma unroll
                            for (int e = 0; e < VEC; ++e) acc[j][i][e] = acc[j][i][e] + pe * f[r][i][e];
                    }
                    if (lane == 0) { st[2 * j] = mn; st[2 * j + 1] = lj; }
                }
            }
        }
        __syncthreads();                          // every wave's (m, l) is in stat, and every wave is done reading u from blk
        // the group's maximum and L = ((l_0 e_0 + l_1 e_1) + ...) in wave order, e_k = exp(m_k - m); a wave without rows contributes nothing
        if ((int)threadIdx.x < hg) {
            const int j = threadIdx.x;
            float mg = stat[0][j][0];
            for (int k = 1; k < W; ++k) mg = fmaxf(mg, stat[k][j][0]);
            float L = 0.0f;
            for (int k = 0; k < W; ++k) {
                const float mk = stat[k][j][0];
                L = L + stat[k][j][1] * (mk == NEG ? 0.0f : __expf(mk - mg));
            }
            fin[j][0] = mg; fin[j][1] = L;
        }
        __syncthreads();
        for (int k = 0; k < W; ++k) {
            if (wave == k) {
#pragma unroll
                for (int j = 0; j < HG; ++j) {
                    if (j < hg) {
                        const float mk = st[2 * j];
                        const float sk = mk == NEG ? 0.0f : __expf(mk - fin[j][0]);
#pragma unroll
                        for (int i = 0; i < NV; ++i)
#pragma unroll
                            for (int e = 0; e < VEC; ++e) {
                                float *q = blk + j * D + R::col(i, lane) + e;
                                const float v = acc[j][i][e] * sk;
                                *q = k == 0 ? v : *q + v;
                            }
                    }
                }
            }
            __syncthreads();
        }
        // M = block / L: head j of the group by wave j % W
        for (int j = wave; j < hg; j += W) {
            const float L = fin[j][1];
            float o[NV][VEC];
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int e = 0; e < VEC; ++e) o[i][e] = blk[j * D + R::col(i, lane) + e] / L;
            const size_t off = (img * H + h0 + j) * (size_t)D;
            if (M) R::store(M + off, lane, o);
            if (m16) R::store_rne(m16 + off, lane, o);
        }
        if (p) {                                  // the parked scores -> probabilities (the stores above are visible to the workgroup past the barriers)
            for (int j = 0; j < hg; ++j) {
                float *pr = p + (img * H + h0 + j) * (size_t)N;
                const float mg = fin[j][0], L = fin[j][1];
                for (int t = threadIdx.x; t < N; t += W * 64) pr[t] = __expf(pr[t] - mg) / L;
            }
        }
    }
}

template <int VEC, int NV, typename T16>
__global__ __launch_bounds__(64) void pool_embed_kernel(const float *__restrict__ e, T16 *__restrict__ z, float *__restrict__ cls, long out_img_stride, int l2) {
    typedef LnRow<VEC, NV> R;
    constexpr int D = 64 * VEC * NV;
    const int lane = threadIdx.x;
    const float *er = e + (size_t)blockIdx.x * D;
    float f[NV][VEC];
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < VEC; ++j) f[i][j] = er[R::col(i, lane) + j];
    if (z) R::store_rne(z + (size_t)blockIdx.x * D, lane, f);
    if (!cls) return;
    if (l2) R::l2(f);
    R::store(cls + (size_t)blockIdx.x * out_img_stride, lane, f);
}

template <typename T16>
hipError_t launch_attention_pool_t(const float *x, long row_stride, long img_stride, const float *w, const float *b, float eps, const float *u, float *M, void *m16, float *p,
                                   int n_img, int N, int D, int H, hipStream_t stream) {
    const bool ok = ln_for_width(D, [&](auto vec, auto nv) {
        constexpr int HG = pool_group(vec() * nv());
        hipLaunchKernelGGL((attention_pool_kernel<vec(), nv(), T16>), dim3(n_img, (H + HG - 1) / HG), dim3(kPoolWaves * 64), 0, stream, x, row_stride, img_stride, w, b, eps, u, M,
                           (T16 *)m16, p, N, H);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

template <typename T16>
hipError_t launch_pool_embed_t(const float *e, void *z, float *cls, long out_img_stride, bool l2, int n_img, int D, hipStream_t stream) {
    const bool ok = ln_for_width(D, [&](auto vec, auto nv) {
        hipLaunchKernelGGL((pool_embed_kernel<vec(), nv(), T16>), dim3(n_img), dim3(64), 0, stream, e, (T16 *)z, cls, out_img_stride, l2 ? 1 : 0);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_attention_pool(const float *x, long row_stride, long img_stride, const float *w, const float *b, float eps, const float *u, float *M, void *m16, int dtype,
                                 float *p, int n_img, int N, int D, int H, hipStream_t stream) {
    if (n_img <= 0 || N <= 0 || H <= 0 || H > kPoolMaxHeads || (!M && !m16)) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_attention_pool_t, x, row_stride, img_stride, w, b, eps, u, M, m16, p, n_img, N, D, H, stream);
}

hipError_t launch_pool_embed(const float *e, void *z, int dtype, float *cls, long out_img_stride, bool l2, int n_img, int D, hipStream_t stream) {
    if (n_img <= 0 || (!z && !cls)) return hipErrorInvalidValue;
    return VITX_BY_DTYPE(dtype, launch_pool_embed_t, e, z, cls, out_img_stride, l2, n_img, D, stream);
}

}  // namespace vitx
