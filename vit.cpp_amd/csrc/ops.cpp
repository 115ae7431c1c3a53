// ops.cpp -- single-kernel entry points (vitx_op_*, vitx_preprocess_u8_device): one launcher each, on the caller's buffers, for the
// parity tests and the kernel benchmarks.  None takes a context.
#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "context.h"
#include "preproc_resample.h"
#include "dense_resample.h"
#include "depth_bins.h"

// A launcher's hipError_t -> the entry point's return code, with "<name>: <hip string>" as the error text.  `invalid`: the code that
// hipErrorInvalidValue (the launchers' "no instantiation for this shape") maps to -- each entry point keeps the mapping it always had
static int op_rc(const char *name, hipError_t e, int invalid = VITX_ERR_HIP) {
    if (e == hipSuccess) return VITX_OK;
    set_error("%s: %s", name, hipGetErrorString(e));
    return e == hipErrorInvalidValue ? invalid : VITX_ERR_HIP;
}
// The lo plane of the F16 parity mode behind d_qkv (vitx_op_attention_cls, vitx_op_attention_map): VITX_F16 only, past the hi plane's rows
static bool lo_plane_ok(const char *name, int dtype, long lo_off, long hi_elems) {
    if (!lo_off || (dtype == VITX_F16 && lo_off >= hi_elems && lo_off % 8 == 0)) return true;
    set_error("%s: a lo plane needs VITX_F16 and lo_off %ld a multiple of 8 elements, at least n_img * N * 3 * D = %ld", name, lo_off, hi_elems);
    return false;
}

extern "C" {

// ---- single-kernel entry points --------------------------------------------------------------
int vitx_op_layernorm(int dtype, const void *x, const void *w, const void *b, void *y, int M, int D, float eps, void *stream) {
    if (!x || !w || !b || !y || M <= 0) return VITX_ERR_ARG;
    return op_rc("vitx_op_layernorm", launch_layernorm(dtype, (const float *)x, D, (const float *)w, (const float *)b, y, D, M, D, eps, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
int vitx_op_layernorm_f32(const void *x, const void *w, const void *b, void *y, int M, int D, float eps, void *stream) {
    if (!x || !w || !b || !y || M <= 0) return VITX_ERR_ARG;
    return op_rc("vitx_op_layernorm_f32", launch_layernorm_f32((const float *)x, (const float *)w, (const float *)b, (float *)y, M, D, eps, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
static int op_gemm_impl(int dtype, int epi, int kernel, const void *a, const void *w, const void *bias, void *out, const void *pos, int M, int M_real, int N, int n_pad, int K, int tpi, void *stream) {
    if (!a || !w || !out || !bias || epi < 0 || epi >= EPI_COUNT || M_real <= 0 || M_real > M || (epi == EPI_PATCH && (!pos || tpi <= 0))) { set_error("vitx_op_gemm_ex: invalid argument"); return VITX_ERR_ARG; }
    if (M % 128 || N % 4 || K % 64) { set_error("vitx_op_gemm: M %% 128, N %% 4, K %% 64 must be 0"); return VITX_ERR_ARG; }
    const Tuning *t0 = tuning_for_device(-1);
    if (!t0) { set_error("vitx_op_gemm: kernel bring-up failed"); return VITX_ERR_HIP; }
    Tuning t = *t0;
    if (kernel == 2) t.gemm_split = 1;
    else if (kernel == 1) t.gemm_cfg = 1;                  // ping-pong persistent kernel
    else if (kernel != 0) t.gemm_cfg = kernel;
    // W (and bias) must hold n_pad rows; rows beyond N are never stored
    GemmArgs g = dense_gemm(a, w, (const float *)bias, out, M, M_real, N, n_pad, K);
    g.pos = (const float *)pos; g.tpi = tpi;
    g.hilo_off = epi == EPI_BIAS_HILO ? (long)M * N : 0;          // the lo plane follows the [M][N] hi plane
    hipError_t e = launch_gemm(t, dtype, epi, g, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) { set_error("vitx_op_gemm: kernel %d cannot tile M %d N %d K %d", kernel, M, N, K); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_gemm", e);
}
int vitx_op_gemm_ex(int dtype, int epi, int kernel, const void *a, const void *w, const void *bias, void *out, const void *pos, int M, int M_real, int N, int K, int tpi, void *stream) {
    return op_gemm_impl(dtype, epi, kernel, a, w, bias, out, pos, M, M_real, N, round_up(N, 256), K, tpi, stream);     // W and bias hold N rounded up to 256 rows
}
int vitx_op_gemm(int dtype, int epi, const void *a, const void *w, const void *bias, void *out, int M, int N, int K, void *stream) {
    if (epi < 0 || (epi > 3 && !epi_is_act(epi)) || N % 64) { set_error("vitx_op_gemm: epi 0..3, 6 or 7, N %% 64 == 0"); return VITX_ERR_ARG; }
    return op_gemm_impl(dtype, epi, 0, a, w, bias, out, nullptr, M, M, N, round_up(N, gemm_tile_n()), K, 0, stream);   // W and bias hold N rounded up to 128 rows
}
// x[M][N] f32 += A[M][K] . W[N][K]^T + bias, then y[M][N] (dtype) = LayerNorm(x) * ln_w + ln_b computed by the GEMM's own epilogue
// (GemmLn) + the fix-up launch.  `test`: GemmLn::test (forced time-outs).  Synchronous; *fallbacks = tiles that took the fix-up path.
int vitx_op_gemm_ln(int dtype, const void *a, const void *w, const void *bias, void *x, const void *ln_w, const void *ln_b, void *y, int M, int N, int K, float eps,
                    int test, int timeout_us, int *fallbacks, void *stream) {
    if (!a || !w || !bias || !x || !ln_w || !ln_b || !y || M <= 0 || timeout_us < 0) { set_error("vitx_op_gemm_ln: invalid argument"); return VITX_ERR_ARG; }
    const Tuning *t0 = tuning_for_device(-1);
    if (!t0) { set_error("vitx_op_gemm_ln: kernel bring-up failed"); return VITX_ERR_HIP; }
    GemmArgs g = dense_gemm(a, w, (const float *)bias, x, M, M, N, N, K);
    if (!gemm_ln_fusable(*t0, g)) { set_error("vitx_op_gemm_ln: M %d N %d K %d does not take the LayerNorm-fusing kernel (M %% 256, N in {256,512,768,1024}, >= 128 tiles, K %% 128)", M, N, K); return VITX_ERR_UNSUPPORTED; }
    static unsigned epoch = 0x40000000u;       // its own tag range (the scratch is private to the call anyway)
    const size_t nb = (size_t)M / 256, sync_bytes = nb * (N / 256) * 256 * 2 * sizeof(unsigned long long);
    unsigned long long *sync = nullptr; unsigned *todo = nullptr;
    HIP_TRY(hipMalloc((void **)&sync, sync_bytes));
    const DevMem sync_own(sync);
    if (hipMalloc((void **)&todo, (nb + 1) * 4) != hipSuccess) return VITX_ERR_NOMEM;
    const DevMem todo_own(todo);
    hipStream_t st = (hipStream_t)stream;
    GemmLn ln{};
    ln.w = (const float *)ln_w; ln.b = (const float *)ln_b; ln.out = y; ln.eps = eps; ln.sync = sync; ln.todo = todo; ln.fallbacks = todo + nb;
    ln.epoch = ++epoch; ln.timeout = (unsigned)timeout_us * 100u; ln.test = test;
    g.ln = &ln;
    hipError_t e = hipMemsetAsync(sync, 0, sync_bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(todo, 0, (nb + 1) * 4, st);
    if (e == hipSuccess) e = launch_gemm(*t0, dtype, EPI_BIAS_RESID, g, st);
    if (e == hipSuccess) e = launch_layernorm_fixup(dtype, (const float *)x, ln.w, ln.b, y, M, N, eps, todo, ln.epoch, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    unsigned fb = 0;
    if (e == hipSuccess) e = hipMemcpy(&fb, todo + nb, 4, hipMemcpyDeviceToHost);
    if (fallbacks) *fallbacks = (int)fb;
    return op_rc("vitx_op_gemm_ln", e);
}
// quantised-weight kernels (quant.hip, gemm_nt_kernel<.., Q4>): blocks in the FILE's byte layout for every type except q4_0, whose
// nibble plane / scale plane split is done here the way the context does it at upload
int vitx_op_dequant(int dtype, int qtype, const void *blocks, const void *scales, void *out, int N, int n_pad, int K, void *stream) {
    if (!blocks || !out || N <= 0 || n_pad < N || K <= 0 || K % 32 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_dequant: invalid argument"); return VITX_ERR_ARG; }
    DequantJob j{blocks, scales, out, N, n_pad, K / 32};
    return op_rc("vitx_op_dequant", launch_dequant(dtype, qtype, &j, 1, (hipStream_t)stream), VITX_ERR_ARG);
}
// launch_dequant as the forward calls it (SliceForward::expand, forward.cpp): up to four matrices of one block type in ONE launch
int vitx_op_dequant_jobs(int dtype, int qtype, int njobs, const void *const *blocks, const void *const *scales, void *const *out, const int *N, const int *n_pad, const int *K, void *stream) {
    if (njobs < 1 || njobs > 4 || !blocks || !out || !N || !n_pad || !K || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_dequant_jobs: invalid argument"); return VITX_ERR_ARG; }
    DequantJob jobs[4];
    for (int j = 0; j < njobs; ++j) {
        if (!blocks[j] || !out[j] || N[j] <= 0 || n_pad[j] < N[j] || K[j] <= 0 || K[j] % 32) { set_error("vitx_op_dequant_jobs: invalid argument in job %d", j); return VITX_ERR_ARG; }
        jobs[j] = DequantJob{blocks[j], scales ? scales[j] : nullptr, out[j], N[j], n_pad[j], K[j] / 32};
    }
    return op_rc("vitx_op_dequant_jobs", launch_dequant(dtype, qtype, jobs, njobs, (hipStream_t)stream), VITX_ERR_ARG);
}
int vitx_op_gemm_q4(int dtype, int epi, const void *a, const void *qs, const void *scales, const void *bias, void *out, int M, int M_real, int N, int K, void *stream) {
    if (!a || !qs || !scales || !bias || !out || epi < 0 || (epi > EPI_BIAS_F32 && !epi_is_act(epi)) || M_real <= 0 || M_real > M) { set_error("vitx_op_gemm_q4: invalid argument"); return VITX_ERR_ARG; }
    if (!tuning_for_device(-1)) { set_error("vitx_op_gemm_q4: kernel bring-up failed"); return VITX_ERR_HIP; }
    GemmArgs g = dense_gemm(a, qs, (const float *)bias, out, M, M_real, N, round_up(N, 128), K);
    g.Wscale = (const uint16_t *)scales;
    hipError_t e = launch_gemm_q4(dtype, epi, g, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) { set_error("vitx_op_gemm_q4: M %% 128, K %% 64 must be 0 (M %d N %d K %d)", M, N, K); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_gemm_q4", e);
}
// ---- MXFP8 single-kernel entry points (include/vitx.h) ----
int vitx_op_quantize_mxfp8(const void *x, int rows, int K, int k_pad, void *q, void *scales, void *stream) {
    if (!x || !q || !scales || rows <= 0 || K <= 0 || k_pad < K || k_pad % kMxBlock) { set_error("vitx_op_quantize_mxfp8: invalid argument"); return VITX_ERR_ARG; }
    return op_rc("vitx_op_quantize_mxfp8", launch_quantize_mx8((const float *)x, rows, K, k_pad, (uint8_t *)q, (uint8_t *)scales, (hipStream_t)stream));
}
int vitx_op_layernorm_mxfp8(const void *x, const void *w, const void *b, void *q, void *scales, int M, int D, float eps, void *stream) {
    if (!x || !w || !b || !q || !scales || M <= 0 || D <= 0) { set_error("vitx_op_layernorm_mxfp8: invalid argument"); return VITX_ERR_ARG; }
    if (D % kMxBlock || !layernorm_supports(D)) { set_error("vitx_op_layernorm_mxfp8: hidden size %d has no MX LayerNorm instantiation", D); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_layernorm_mxfp8", launch_layernorm_mx8((const float *)x, D, (const float *)w, (const float *)b, (uint8_t *)q, (uint8_t *)scales, mx_k_pad(D), M, D, eps, (hipStream_t)stream));
}
int vitx_op_gemm_mxfp8(int epi, const void *a, const void *a_scales, const void *w, const void *w_scales, const void *bias, void *out, void *out_scales,
                       int M, int N, int K, void *stream) {
    if (!a || !a_scales || !w || !w_scales || !bias || !out || M <= 0 || N <= 0 || K <= 0 || (epi != EPI_BIAS && epi != EPI_BIAS_GELU && epi != EPI_BIAS_RESID) ||
        (epi == EPI_BIAS_GELU && !out_scales)) { set_error("vitx_op_gemm_mxfp8: invalid argument"); return VITX_ERR_ARG; }
    if (!tuning_for_device(-1)) { set_error("vitx_op_gemm_mxfp8: kernel bring-up failed"); return VITX_ERR_HIP; }
    const GemmArgs g = dense_gemm(a, w, (const float *)bias, out, M, M, N, round_up(N, 128), mx_k_pad(K), epi == EPI_BIAS_GELU ? mx_k_pad(N) : N);
    const hipError_t e = launch_gemm_mx8(epi, g, (const uint8_t *)a_scales, (const uint8_t *)w_scales, (uint8_t *)out_scales, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) { set_error("vitx_op_gemm_mxfp8: the kernel cannot tile M %d N %d K %d", M, N, K); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_gemm_mxfp8", e);
}

int vitx_op_attention_ex(int dtype, int kernel, const void *qkv, void *out, int n_img, int N, int D, int H, void *stream) {
    if (!qkv || !out || n_img <= 0 || kernel < 0) return VITX_ERR_ARG;
    const Tuning *t0 = tuning_for_device(-1);
    if (!t0) { set_error("vitx_op_attention: kernel bring-up failed"); return VITX_ERR_HIP; }
    Tuning t = *t0;
#ifdef VITX_LAB
    t.attn_flags = kernel >> 4; kernel &= 15;                // bits 4+: ablation build of the pipelined kernel (tools/attn_bench.py only)
#endif
    if (kernel == ATTN_PERSIST) {                            // persistent single-pass kernel (193..224 tokens)
        if (N <= 192 || N > 224) { set_error("vitx_op_attention: the persistent kernel takes 193..224 tokens, not %d", N); return VITX_ERR_UNSUPPORTED; }
    } else if (kernel == ATTN_SINGLE) {                      // single-pass kernel, also where the automatic choice prefers the pipelined one
        if (!attention_single_pass_supports(N)) { set_error("vitx_op_attention: no single-pass instantiation for %d tokens", N); return VITX_ERR_UNSUPPORTED; }
    } else if (kernel == ATTN_STREAM) {                      // streaming two-pass kernel (attention_stream.hip), head dim 64
        if (!attention_stream_supports(n_img, N, D, H)) { set_error("vitx_op_attention: the streaming kernel needs head_dim 64"); return VITX_ERR_UNSUPPORTED; }
    } else if (kernel != ATTN_AUTO && kernel != ATTN_FLOW) { set_error("vitx_op_attention: unknown kernel id %d", kernel); return VITX_ERR_ARG; }
    t.attn_kernel = kernel;
    return op_rc("vitx_op_attention", launch_attention(t, dtype, qkv, out, n_img, N, D, H, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
int vitx_op_attention(int dtype, const void *qkv, void *out, int n_img, int N, int D, int H, void *stream) { return vitx_op_attention_ex(dtype, 0, qkv, out, n_img, N, D, H, stream); }
// The precise kernel on planes that are already split (what the QKV GEMM's epilogue 5 emits): d_hi [n_img * N][3 D] fp16, the lo plane lo_off
// ELEMENTS behind it.  Only enqueues on `stream`.
int vitx_op_attention_planes(const void *d_hi, long lo_off, void *out, int n_img, int N, int D, int H, void *stream) {
    if (!d_hi || !out || n_img <= 0 || N <= 0 || D <= 0 || H <= 0) { set_error("vitx_op_attention_planes: invalid argument"); return VITX_ERR_ARG; }
    // the lo plane lies a whole number of 4-element groups behind the hi plane's rows and inside the 32-bit byte window the kernels address
    if (lo_off < (long)n_img * N * 3 * D || lo_off % 4 != 0 || (size_t)lo_off * 2 + (size_t)n_img * N * 3 * D * 2 > 0xf0000000u) {
        set_error("vitx_op_attention_planes: lo_off %ld must be a multiple of 4 elements, at least n_img * N * 3 * D = %ld, and keep both planes below 0xf0000000 bytes", lo_off, (long)n_img * N * 3 * D);
        return VITX_ERR_ARG;
    }
    if (!tuning_for_device(-1)) { set_error("vitx_op_attention_planes: kernel bring-up failed"); return VITX_ERR_HIP; }
    if (!attention_stream_supports(n_img, N, D, H)) { set_error("vitx_op_attention_planes: head_dim must be 64"); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_attention_planes", launch_attention_stream(DT_F16, true, d_hi, out, n_img, N, D, H, lo_off, (hipStream_t)stream));
}
// Attention of token 0 of every image (the row the last layer of a classifier keeps, vit.cpp:910-911): out[n_img][D] (dtype).  lo_off != 0: the two
// fp16 planes of the F16 parity mode (VITX_F16 only), as vitx_op_attention_planes takes them.  Only enqueues on `stream`.
int vitx_op_attention_cls(int dtype, const void *d_qkv, long lo_off, void *out, int n_img, int N, int D, int H, void *stream) {
    if (!d_qkv || !out || n_img <= 0 || N <= 0 || D <= 0 || H <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_attention_cls: invalid argument"); return VITX_ERR_ARG; }
    if (!lo_plane_ok("vitx_op_attention_cls", dtype, lo_off, (long)n_img * N * 3 * D)) return VITX_ERR_ARG;
    if (!attention_cls_supports(N, D, H)) { set_error("vitx_op_attention_cls: head_dim must be 8, 16, 32, 64 or 128 and N at most 15360 (head_dim %d, N %d)", D / H, N); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_attention_cls", launch_attention_cls(dtype, d_qkv, lo_off, out, nullptr, nullptr, n_img, N, D, H, (hipStream_t)stream));
}
// Rotary position embeddings in place on d_qkv (rope.hip; include/vitx.h "rotary position embeddings").  Every check comes before the launch; only enqueues.
int vitx_op_rope(int dtype, void *d_qkv, long lo_off, const void *d_cos, const void *d_sin, int n_img, int N, int prefix, int D, int H, void *stream) {
    if (!d_qkv || !d_cos || !d_sin || n_img <= 0 || N <= 0 || D <= 0 || H <= 0 || prefix < 0 || prefix > N || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_rope: invalid argument (0 <= prefix <= N)"); return VITX_ERR_ARG; }
    if ((size_t)n_img * N * 3 * D >= ((size_t)1 << 40)) { set_error("vitx_op_rope: n_img * N * 3 * D is out of range"); return VITX_ERR_ARG; }
    if (!lo_plane_ok("vitx_op_rope", dtype, lo_off, (long)n_img * N * 3 * D)) return VITX_ERR_ARG;
    if (lo_off && (size_t)lo_off * 2 + (size_t)n_img * N * 3 * D * 2 > 0xf0000000u) { set_error("vitx_op_rope: both planes must lie below 0xf0000000 bytes"); return VITX_ERR_ARG; }
    if ((uintptr_t)d_qkv % 2 || (uintptr_t)d_cos % 4 || (uintptr_t)d_sin % 4) { set_error("vitx_op_rope: misaligned pointer"); return VITX_ERR_ARG; }
    if (!rope_supports(D, H)) { set_error("vitx_op_rope: D must be a multiple of H and the head dim even (D %d, H %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_rope", launch_rope(dtype, d_qkv, lo_off, (const float *)d_cos, (const float *)d_sin, n_img, N, prefix, D, H, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
// The gate of a gated MLP (swiglu.hip; include/vitx.h "gated MLP").  Every check comes before the launch; only enqueues.
int vitx_op_swiglu(int dtype, const void *d_in, long ld_in, void *d_out, long ld_out, long rows, int F, void *stream) {
    if (!d_in || !d_out || rows <= 0 || F <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_swiglu: invalid argument"); return VITX_ERR_ARG; }
    if (F % 8 || ld_in % 8 || ld_out % 8 || ld_in < 2L * F || ld_out < F || (uintptr_t)d_in % 16 || (uintptr_t)d_out % 16) {
        set_error("vitx_op_swiglu: F, ld_in and ld_out must be multiples of 8, ld_in >= 2 F, ld_out >= F and both pointers on 16-byte boundaries (F %d, ld_in %ld, ld_out %ld)", F, ld_in, ld_out);
        return VITX_ERR_ARG;
    }
    return op_rc("vitx_op_swiglu", launch_swiglu(dtype, d_in, ld_in, d_out, ld_out, rows, F, (hipStream_t)stream), VITX_ERR_ARG);
}
// The two packed kernels on the caller's buffers (include/vitx.h "packed batches").  TEST entry points: they read the device tables back (a
// synchronous copy) to check them -- a table that lies would send the kernel out of bounds -- and, the attention, to build the count of query blocks.
static int read_row0(const char *name, const void *d_row0, int n, int min_rows, std::vector<int32_t> &row0) {
    row0.resize((size_t)n + 1);
    HIP_TRY(hipMemcpy(row0.data(), d_row0, row0.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i)
        if (row0[0] < 0 || (long)row0[i + 1] - row0[i] < min_rows) { set_error("%s: d_row0 must start at 0 or above and give every image at least %d rows (image %d)", name, min_rows, i); return VITX_ERR_ARG; }
    return VITX_OK;
}
int vitx_op_attention_packed(int dtype, const void *d_qkv, void *d_out, const void *d_row0, int n, int D, int H, void *stream) {
    if (!d_qkv || !d_out || !d_row0 || n <= 0 || D <= 0 || H <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_attention_packed: invalid argument"); return VITX_ERR_ARG; }
    if (!attention_packed_supports(D, H)) { set_error("vitx_op_attention_packed: head_dim must be a multiple of 8 up to 128 (D %d, H %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    std::vector<int32_t> row0, qb0((size_t)n + 1);
    if (const int rc = read_row0("vitx_op_attention_packed", d_row0, n, 1, row0)) return rc;
    long qblocks = 0;
    for (int i = 0; i < n; ++i) { qb0[i] = (int32_t)qblocks; qblocks += (row0[i + 1] - row0[i] + 63) / 64; }
    qb0[n] = (int32_t)qblocks;
    int *d_qb0 = nullptr;
    HIP_TRY(hipMalloc((void **)&d_qb0, qb0.size() * 4));
    const DevMem qb_own(d_qb0);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpy(d_qb0, qb0.data(), qb0.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_attention_packed(dtype, d_qkv, d_out, (const int *)d_row0, d_qb0, n, qblocks, D, H, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);       // d_qb0 is freed on return
    return op_rc("vitx_op_attention_packed", e, VITX_ERR_UNSUPPORTED);
}
// The same launch on tables the caller has built and vouches for (d_qb0 [n + 1]: the running count of 64-query blocks; qblocks = d_qb0[n]): only
// enqueues, reads nothing back -- what a packed context does per layer, and what tools/pack_cost.py times.
int vitx_op_attention_packed_tables(int dtype, const void *d_qkv, void *d_out, const void *d_row0, const void *d_qb0, int n, long qblocks, int D, int H, void *stream) {
    if (!d_qkv || !d_out || !d_row0 || !d_qb0 || n <= 0 || qblocks < n || D <= 0 || H <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_attention_packed_tables: invalid argument"); return VITX_ERR_ARG; }
    return op_rc("vitx_op_attention_packed_tables", launch_attention_packed(dtype, d_qkv, d_out, (const int *)d_row0, (const int *)d_qb0, n, qblocks, D, H, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
int vitx_op_rope_packed(int dtype, void *d_qkv, long lo_off, const void *d_cos, const void *d_sin, const void *d_row0, const void *d_table_off, int n, int prefix, int D, int H, void *stream) {
    if (!d_qkv || !d_cos || !d_sin || !d_row0 || !d_table_off || n <= 0 || D <= 0 || H <= 0 || prefix < 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_rope_packed: invalid argument"); return VITX_ERR_ARG; }
    if (lo_off) { set_error("vitx_op_rope_packed: a pack has one operand plane (lo_off must be 0)"); return VITX_ERR_ARG; }
    if ((uintptr_t)d_qkv % 2 || (uintptr_t)d_cos % 4 || (uintptr_t)d_sin % 4) { set_error("vitx_op_rope_packed: misaligned pointer"); return VITX_ERR_ARG; }
    if (!rope_supports(D, H)) { set_error("vitx_op_rope_packed: D must be a multiple of H and the head dim even (D %d, H %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    std::vector<int32_t> row0, toff((size_t)n);
    if (const int rc = read_row0("vitx_op_rope_packed", d_row0, n, std::max(prefix, 1), row0)) return rc;
    HIP_TRY(hipMemcpy(toff.data(), d_table_off, toff.size() * 4, hipMemcpyDeviceToHost));
    bool aligned = true;
    for (int i = 0; i < n; ++i) {
        if (toff[i] < 0) { set_error("vitx_op_rope_packed: d_table_off[%d] is negative", i); return VITX_ERR_ARG; }
        aligned = aligned && toff[i] % 4 == 0;
    }
    return op_rc("vitx_op_rope_packed", launch_rope_packed(dtype, d_qkv, (const float *)d_cos, (const float *)d_sin, (const int *)d_row0, (const int *)d_table_off, n,
                                                           (long)row0[n] - row0[0] - (long)n * prefix, aligned, prefix, D, H, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
// The parity mode's attention on f32 q, k, v (what the reference multiplies, vit.cpp:848,858): splits the rows into the two fp16 planes the
// QKV GEMM's EPI_BIAS_HILO epilogue emits, then runs the precise streaming kernel.  Synchronous (allocates its own scratch).
int vitx_op_attention_f32(const float *qkv_f32, void *out, int n_img, int N, int D, int H, void *stream) {
    if (!qkv_f32 || !out || n_img <= 0 || N <= 0 || D <= 0 || H <= 0) { set_error("vitx_op_attention_f32: invalid argument"); return VITX_ERR_ARG; }
    if (!tuning_for_device(-1)) { set_error("vitx_op_attention_f32: kernel bring-up failed"); return VITX_ERR_HIP; }
    if (!attention_stream_supports(n_img, N, D, H)) { set_error("vitx_op_attention_f32: head_dim must be 64"); return VITX_ERR_UNSUPPORTED; }
    const size_t n = (size_t)n_img * N * 3 * D;
    void *planes = nullptr;
    HIP_TRY(hipMalloc(&planes, n * 2 * 2 + 64));
    const DevMem planes_own(planes);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = launch_split_hilo(DT_F16, qkv_f32, planes, (char *)planes + n * 2, n, st);
    if (e == hipSuccess) e = launch_attention_stream(DT_F16, true, planes, out, n_img, N, D, H, (long)n, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return op_rc("vitx_op_attention_f32", e);
}
int vitx_op_softmax_dt(int dtype, const void *logits, void *probs, int rows, int cols, int ld, void *stream) {
    if (!logits || !probs || rows <= 0 || cols <= 0 || ld < cols || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_softmax: invalid argument"); return VITX_ERR_ARG; }
    return op_rc("vitx_op_softmax", launch_softmax(dtype, (const float *)logits, (float *)probs, rows, cols, ld, (hipStream_t)stream));
}
int vitx_op_softmax(const void *logits, void *probs, int rows, int cols, int ld, void *stream) { return vitx_op_softmax_dt(VITX_F16, logits, probs, rows, cols, ld, stream); }
// launch_topk as the sharded forward calls it (sharded.cpp): pairs {f32 probability, i32 class} of every row
int vitx_op_topk(const void *probs, int rows, int cols, int k, void *pairs, void *stream) {
    if (!probs || !pairs || rows <= 0 || cols <= 0 || k <= 0 || k > cols) { set_error("vitx_op_topk: invalid argument"); return VITX_ERR_ARG; }
    return op_rc("vitx_op_topk", launch_topk((const float *)probs, rows, cols, k, pairs, (hipStream_t)stream));
}

// The feature kernel on its own.  Every argument check comes before the first device call.  `name`: the entry point that was called; `ex`:
// it is vitx_op_features_ex, whose texts also tell `first`.  vitx_op_features is first = 1 and no head operand (so d_z never counts as its output).
static int op_features(const char *name, bool ex, const void *d_x, long row_stride, long img_stride, const void *d_w, const void *d_b, void *d_cls, void *d_mean,
                       void *d_tokens, long out_img_stride, int n_img, int N, int first, int D, float eps, int l2, void *d_z, int dtype, void *stream) {
    if (!d_x || !d_w || !d_b || (!d_cls && !d_mean && !d_tokens && !d_z) || n_img <= 0 || N <= 0 || D <= 0 || first < 0 || first > N || (!ex && first < 1)) { set_error("%s: invalid argument", name); return VITX_ERR_ARG; }
    if (first == 0 && (d_cls || d_z)) { set_error("vitx_op_features_ex: first = 0 means no class row: d_cls and d_z cannot be asked for"); return VITX_ERR_ARG; }
    if (first == N && (d_mean || d_tokens || d_z)) {
        if (ex) set_error("vitx_op_features_ex: the mean and the tokens need at least one patch row (N %d, first %d)", N, first);
        else set_error("vitx_op_features: the mean and the tokens need at least one patch row (N %d)", N);
        return VITX_ERR_ARG;
    }
    if (d_z && dtype != VITX_F16 && dtype != VITX_BF16) { set_error("%s: the head operand is VITX_F16 or VITX_BF16", name); return VITX_ERR_ARG; }
    for (const void *p : {d_x, d_w, d_b, (const void *)d_cls, (const void *)d_mean, (const void *)d_tokens, (const void *)d_z})
        if ((uintptr_t)p % 16) { set_error("%s: pointers must be 16-byte aligned", name); return VITX_ERR_ARG; }
    if (row_stride % 4 || img_stride % 4 || out_img_stride % 4) { set_error("%s: strides must be multiples of 4 floats", name); return VITX_ERR_ARG; }
    if (!layernorm_supports(D)) { set_error("%s: hidden size %d has no LayerNorm instantiation", name, D); return VITX_ERR_UNSUPPORTED; }
    return op_rc(name, launch_features((const float *)d_x, row_stride, img_stride, (const float *)d_w, (const float *)d_b, (float *)d_cls, (float *)d_mean, (float *)d_tokens,
                                       out_img_stride, n_img, N, D, eps, l2 != 0, (hipStream_t)stream, first, d_z, dtype));
}
int vitx_op_features(const void *d_x, long row_stride, long img_stride, const void *d_w, const void *d_b, void *d_cls, void *d_mean, void *d_tokens, long out_img_stride,
                     int n_img, int N, int D, float eps, int l2, void *stream) {
    return op_features("vitx_op_features", false, d_x, row_stride, img_stride, d_w, d_b, d_cls, d_mean, d_tokens, out_img_stride, n_img, N, 1, D, eps, l2, nullptr, VITX_F16, stream);
}
int vitx_op_features_ex(const void *d_x, long row_stride, long img_stride, const void *d_w, const void *d_b, void *d_cls, void *d_mean, void *d_tokens, long out_img_stride,
                        int n_img, int N, int first, int D, float eps, int l2, void *d_z, int dtype, void *stream) {
    return op_features("vitx_op_features_ex", true, d_x, row_stride, img_stride, d_w, d_b, d_cls, d_mean, d_tokens, out_img_stride, n_img, N, first, D, eps, l2, d_z, dtype, stream);
}
// The product's patch-embedding kernel on its own (TEST ONLY: allocates, uploads and synchronises).  d_w: the f32 kernel [D][Cin * P * P] in the
// file's order (channel-major); it is rounded (RNE) to the operand type, K-permuted and padded exactly as the context does at upload.
// vitx_op_patch_embed_rect: the same on [n][img_h][img_w][Cin] images (one body; the square entry point passes S twice).
static int op_patch_embed(const char *name, int dtype, const void *d_img, const void *d_w, const void *d_bias, const void *d_pos, const void *d_cls, const void *d_reg, int R, void *d_X,
                          int n_img, int img_h, int img_w, int P, int Cin, int D, void *stream) {
    if (!d_img || !d_w || !d_bias || !d_pos || (!d_cls && R != 0) || !d_X || R < 0 || (R > 0 && !d_reg) || n_img <= 0 || img_h <= 0 || img_w <= 0 || P <= 0 || img_h % P || img_w % P ||
        Cin <= 0 || D <= 0 || D % 4 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("%s: invalid argument", name); return VITX_ERR_ARG; }
    if (!tuning_for_device(-1)) { set_error("%s: kernel bring-up failed", name); return VITX_ERR_HIP; }
    const int K = Cin * P * P, k_pad = round_up(K, 64), n_pad = round_up(D, gemm_tile_n());
    std::vector<float> wf((size_t)D * K);
    HIP_TRY(hipMemcpy(wf.data(), d_w, wf.size() * 4, hipMemcpyDeviceToHost));
    const std::vector<uint16_t> hp = operand_matrix_host(dtype, wf.data(), nullptr, D, K, n_pad, k_pad, P, Cin);
    void *w_perm = nullptr; float *bias = nullptr;
    HIP_TRY(hipMalloc(&w_perm, hp.size() * 2));
    const DevMem w_own(w_perm);
    if (hipMalloc((void **)&bias, (size_t)n_pad * 4) != hipSuccess) return VITX_ERR_NOMEM;
    const DevMem bias_own(bias);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpy(w_perm, hp.data(), hp.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(bias, 0, (size_t)n_pad * 4);
    if (e == hipSuccess) e = hipMemcpy(bias, d_bias, (size_t)D * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = launch_patch_embed(dtype, (const float *)d_img, w_perm, bias, (const float *)d_pos, (const float *)d_cls, (const float *)d_reg, R,
                                                (float *)d_X, n_img, img_h, img_w, P, Cin, D, n_pad, k_pad, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return op_rc(name, e, VITX_ERR_UNSUPPORTED);
}
int vitx_op_patch_embed(int dtype, const void *d_img, const void *d_w, const void *d_bias, const void *d_pos, const void *d_cls, const void *d_reg, int R, void *d_X,
                        int n_img, int S, int P, int Cin, int D, void *stream) {
    return op_patch_embed("vitx_op_patch_embed", dtype, d_img, d_w, d_bias, d_pos, d_cls, d_reg, R, d_X, n_img, S, S, P, Cin, D, stream);
}
int vitx_op_patch_embed_rect(int dtype, const void *d_img, const void *d_w, const void *d_bias, const void *d_pos, const void *d_cls, const void *d_reg, int R,
                             int n_img, int img_h, int img_w, int P, int Cin, int D, void *d_X) {
    return op_patch_embed("vitx_op_patch_embed_rect", dtype, d_img, d_w, d_bias, d_pos, d_cls, d_reg, R, d_X, n_img, img_h, img_w, P, Cin, D, nullptr);
}
// The pooling kernel of the attention-pooling head on its own.  Every argument check comes before the first device call.
int vitx_op_attention_pool(const void *d_x, long row_stride, long img_stride, const void *d_ln_w, const void *d_ln_b, float eps, const void *d_u, void *d_M, void *d_p,
                           int n_img, int N, int D, int H, void *stream) {
    if (!d_x || !d_ln_w || !d_ln_b || !d_u || !d_M || n_img <= 0 || N <= 0 || D <= 0 || H <= 0 || H > kPoolMaxHeads) { set_error("vitx_op_attention_pool: invalid argument (1 <= H <= %d)", kPoolMaxHeads); return VITX_ERR_ARG; }
    for (const void *p : {d_x, d_ln_w, d_ln_b, d_u, (const void *)d_M, (const void *)d_p})
        if ((uintptr_t)p % 16) { set_error("vitx_op_attention_pool: pointers must be 16-byte aligned"); return VITX_ERR_ARG; }
    if (row_stride % 4 || img_stride % 4) { set_error("vitx_op_attention_pool: strides must be multiples of 4 floats"); return VITX_ERR_ARG; }
    if (!layernorm_supports(D)) { set_error("vitx_op_attention_pool: hidden size %d has no LayerNorm instantiation", D); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_attention_pool", launch_attention_pool((const float *)d_x, row_stride, img_stride, (const float *)d_ln_w, (const float *)d_ln_b, eps, (const float *)d_u,
                                                                 (float *)d_M, nullptr, DT_F16, (float *)d_p, n_img, N, D, H, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
// The map kernels on their own (the parity tests): d_cls [n_img][H][N] class-token rows, d_mean [n_img][N][N] mean_h A_h (either may be NULL).
int vitx_op_attention_map(int dtype, const void *d_qkv, long lo_off, void *d_cls, void *d_mean, int n_img, int N, int D, int H, void *stream) {
    if (!d_qkv || (!d_cls && !d_mean) || n_img <= 0 || N <= 0 || D <= 0 || H <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_attention_map: invalid argument"); return VITX_ERR_ARG; }
    if (!lo_plane_ok("vitx_op_attention_map", dtype, lo_off, (long)n_img * N * 3 * D)) return VITX_ERR_ARG;
    if (!attention_map_supports(N, D, H)) { set_error("vitx_op_attention_map: head_dim must be a multiple of 8 up to 128 (D %d, H %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    if (d_mean && !attention_mean_supports(N, D, H)) { set_error("vitx_op_attention_map: the head mean takes at most %d tokens (N %d)", kAttnMeanMaxTokens, N); return VITX_ERR_UNSUPPORTED; }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (d_cls) e = launch_attention_cls_map(dtype, d_qkv, lo_off, (float *)d_cls, (long)H * N, n_img, N, D, H, st);
    if (e == hipSuccess && d_mean) e = launch_attention_head_mean(dtype, d_qkv, lo_off, (float *)d_mean, n_img, N, D, H, false, st);
    return op_rc("vitx_op_attention_map", e);
}
// The rollout kernels on their own (include/vitx.h).  Every argument check comes before the launch; all three only enqueue.
// The rollout factor A^ = 0.5 mean_h A_h + 0.5 I: the head-mean kernel in its half_identity form, under vitx_op_attention_map's own checks.
int vitx_op_rollout_factor(int dtype, const void *d_qkv, long lo_off, void *d_out, int n_img, int N, int D, int H, void *stream) {
    if (!d_qkv || !d_out || n_img <= 0 || N <= 0 || D <= 0 || H <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_rollout_factor: invalid argument"); return VITX_ERR_ARG; }
    if (!lo_plane_ok("vitx_op_rollout_factor", dtype, lo_off, (long)n_img * N * 3 * D)) return VITX_ERR_ARG;
    if (!attention_map_supports(N, D, H)) { set_error("vitx_op_rollout_factor: head_dim must be a multiple of 8 up to 128 (D %d, H %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    if (!attention_mean_supports(N, D, H)) { set_error("vitx_op_rollout_factor: the head mean takes at most %d tokens (N %d)", kAttnMeanMaxTokens, N); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_rollout_factor", launch_attention_head_mean(dtype, d_qkv, lo_off, (float *)d_out, n_img, N, D, H, true, (hipStream_t)stream));
}
// d_a <- d_a . d_r per image.  The kernel reads r while it overwrites a: ranges that overlap are refused.
int vitx_op_rollout_step(void *d_a, const void *d_r, int n_img, int N, void *stream) {
    if (!d_a || !d_r || n_img <= 0 || N <= 0) { set_error("vitx_op_rollout_step: invalid argument"); return VITX_ERR_ARG; }
    if (N > kAttnMeanMaxTokens) { set_error("vitx_op_rollout_step: rollout takes at most %d tokens (N %d)", kAttnMeanMaxTokens, N); return VITX_ERR_UNSUPPORTED; }
    const uintptr_t a0 = (uintptr_t)d_a, r0 = (uintptr_t)d_r, bytes = (uintptr_t)n_img * N * N * sizeof(float);
    if (a0 < r0 + bytes && r0 < a0 + bytes) { set_error("vitx_op_rollout_step: d_a and d_r overlap (the step is in place over d_a and reads all of d_r)"); return VITX_ERR_ARG; }
    return op_rc("vitx_op_rollout_step", launch_rollout_step((float *)d_a, (const float *)d_r, n_img, N, (hipStream_t)stream));
}
int vitx_op_rollout_row(const void *d_cls, long cls_stride, const void *d_r, void *d_out, long out_stride, int n_img, int N, int H, void *stream) {
    if (!d_cls || !d_out || n_img <= 0 || N <= 0 || H <= 0) { set_error("vitx_op_rollout_row: invalid argument"); return VITX_ERR_ARG; }
    if (cls_stride < (long)H * N || out_stride < N) { set_error("vitx_op_rollout_row: cls_stride %ld must be at least H * N = %ld and out_stride %ld at least N = %d", cls_stride, (long)H * N, out_stride, N); return VITX_ERR_ARG; }
    if (N > kAttnMeanMaxTokens) { set_error("vitx_op_rollout_row: rollout takes at most %d tokens (N %d)", kAttnMeanMaxTokens, N); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_rollout_row", launch_rollout_row((const float *)d_cls, cls_stride, (const float *)d_r, (float *)d_out, out_stride, n_img, N, H, (hipStream_t)stream));
}

// The map kernels on a pack (include/vitx.h "packed batches"): TEST entry points.  row0 is a HOST table; each call builds rblk0 and sq0
// (attn_pack_tables), uploads the three tables, launches on the null stream, waits and frees them.  Every argument check comes before the first device call.
namespace {
struct PackMapTables {
    std::vector<int32_t> host;           // row0 [n + 1] | rblk0 [n + 1] | sq0 [n + 1]
    int n = 0, n_max = 0;
    int *dev = nullptr;
    ~PackMapTables() { (void)hipFree(dev); }
    const int *row0() const { return dev; }
    const int *rblk0() const { return dev + n + 1; }
    const int *sq0() const { return dev + 2 * (n + 1); }
    int blocks() const { return host[2 * (n + 1) - 1]; }
    size_t sq_floats() const { return (size_t)host[3 * (n + 1) - 1]; }
    // the checks of the table (need_mean: every image within the rollout kernels' token bound)
    int check(const char *name, const int32_t *row0, int n_, bool need_mean) {
        if (!row0 || n_ <= 0 || row0[0] < 0) { set_error("%s: invalid argument", name); return VITX_ERR_ARG; }
        for (int i = 0; i < n_; ++i) {
            if (row0[i + 1] <= row0[i]) { set_error("%s: image %d: row0 must ascend (an image has at least one token)", name, i); return VITX_ERR_ARG; }
            if (need_mean && row0[i + 1] - row0[i] > kAttnMeanMaxTokens) {
                set_error("%s: image %d: rollout takes at most %d tokens (N %d)", name, i, kAttnMeanMaxTokens, row0[i + 1] - row0[i]);
                return VITX_ERR_UNSUPPORTED;
            }
        }
        n = n_;
        host.assign((size_t)3 * (n + 1), 0);
        std::copy(row0, row0 + n + 1, host.begin());
        if (!attn_pack_tables(row0, n, host.data() + n + 1, host.data() + 2 * (n + 1), &n_max)) { set_error("%s: the sum of N_i^2 leaves 31 bits", name); return VITX_ERR_ARG; }
        return VITX_OK;
    }
    hipError_t upload() {
        hipError_t e = hipMalloc((void **)&dev, host.size() * 4);
        if (e == hipSuccess) e = hipMemcpy(dev, host.data(), host.size() * 4, hipMemcpyHostToDevice);
        return e;
    }
};
}  // namespace
// d_cls: image i's [H][N_i] class-token maps at float row0[i] * H; d_mean: its [N_i][N_i] head mean (half_identity: the rollout factor) at float sq0[i]
int vitx_op_attention_map_packed(int dtype, const void *d_qkv, void *d_cls, void *d_mean, const int32_t *row0, int n, int D, int H, int half_identity) {
    if (!d_qkv || (!d_cls && !d_mean) || D <= 0 || H <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_attention_map_packed: invalid argument"); return VITX_ERR_ARG; }
    if (!attention_map_supports(1, D, H)) { set_error("vitx_op_attention_map_packed: head_dim must be a multiple of 8 up to 128 (D %d, H %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    PackMapTables t;
    if (const int rc = t.check("vitx_op_attention_map_packed", row0, n, d_mean != nullptr)) return rc;
    hipError_t e = t.upload();
    if (e == hipSuccess && d_cls) e = launch_attention_cls_map_packed(dtype, d_qkv, (float *)d_cls, H, 0, t.row0(), n, D, H, nullptr);
    if (e == hipSuccess && d_mean) e = launch_attention_head_mean_packed(dtype, d_qkv, (float *)d_mean, t.row0(), t.rblk0(), t.sq0(), n, t.blocks(), t.n_max, D, H, half_identity != 0, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return op_rc("vitx_op_attention_map_packed", e);
}
// d_a <- d_a . d_r per image, image i's matrices at float sq0[i] of both
int vitx_op_rollout_step_packed(void *d_a, const void *d_r, const int32_t *row0, int n) {
    if (!d_a || !d_r) { set_error("vitx_op_rollout_step_packed: invalid argument"); return VITX_ERR_ARG; }
    PackMapTables t;
    if (const int rc = t.check("vitx_op_rollout_step_packed", row0, n, true)) return rc;
    const uintptr_t a0 = (uintptr_t)d_a, r0 = (uintptr_t)d_r, bytes = (uintptr_t)t.sq_floats() * sizeof(float);
    if (a0 < r0 + bytes && r0 < a0 + bytes) { set_error("vitx_op_rollout_step_packed: d_a and d_r overlap (the step is in place over d_a and reads all of d_r)"); return VITX_ERR_ARG; }
    hipError_t e = t.upload();
    if (e == hipSuccess) e = launch_rollout_step_packed((float *)d_a, (const float *)d_r, t.row0(), t.rblk0(), t.sq0(), n, t.blocks(), t.n_max, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return op_rc("vitx_op_rollout_step_packed", e);
}
// d_cls as vitx_op_attention_map_packed writes it; d_r: image i's matrix at float sq0[i], or NULL; d_out: image i's row [N_i] at float row0[i]
int vitx_op_rollout_row_packed(const void *d_cls, const void *d_r, void *d_out, const int32_t *row0, int n, int H) {
    if (!d_cls || !d_out || H <= 0) { set_error("vitx_op_rollout_row_packed: invalid argument"); return VITX_ERR_ARG; }
    PackMapTables t;
    if (const int rc = t.check("vitx_op_rollout_row_packed", row0, n, true)) return rc;
    hipError_t e = t.upload();
    if (e == hipSuccess) e = launch_rollout_row_packed((const float *)d_cls, H, 0, (const float *)d_r, (float *)d_out, 1, 0, t.row0(), t.sq0(), n, t.n_max, H, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return op_rc("vitx_op_rollout_row_packed", e);
}

// Zero-shot classification on the caller's buffers: the sequence the forward of a context with a bank runs (head_zeroshot, heads.cpp).  Every
// argument check comes before the first device call.  The GEMM's bias is the row of zeros the call writes behind the accumulator rows
// (d_acc_scratch holds round_up(n, 256) + 1 rows of K_pad floats).
int vitx_zeroshot_max_classes(int E) {
    if (E <= 0 || E % 64) return 0;
    return (int)std::min<size_t>((size_t)0xf0000000u / ((size_t)E * 2) / gemm_tile_n() * gemm_tile_n(), (size_t)0x7fffff80);
}
int vitx_op_zeroshot(int dtype, const void *d_z, long z_stride, const void *d_bank, void *d_a_scratch, void *d_acc_scratch, void *d_probs, void *d_logits,
                     int n, int K, int E, int kind, float scale, float bias, void *stream) {
    if (!d_z || !d_bank || !d_a_scratch || !d_acc_scratch || !d_probs || !d_logits || n <= 0 || K <= 0 || E <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_zeroshot: invalid argument"); return VITX_ERR_ARG; }
    if (kind != VITX_ZS_SOFTMAX && kind != VITX_ZS_SIGMOID) { set_error("vitx_op_zeroshot: unknown kind %d (0 softmax, 1 sigmoid)", kind); return VITX_ERR_ARG; }
    if (!std::isfinite(scale) || !std::isfinite(bias)) { set_error("vitx_op_zeroshot: scale and bias must be finite"); return VITX_ERR_ARG; }
    if (z_stride < E || z_stride % 4) { set_error("vitx_op_zeroshot: z_stride %ld must be at least E = %d and a multiple of 4 floats", z_stride, E); return VITX_ERR_ARG; }
    for (const void *p : {d_z, d_bank, (const void *)d_a_scratch, (const void *)d_acc_scratch})
        if ((uintptr_t)p % 16) { set_error("vitx_op_zeroshot: d_z, d_bank and the scratch buffers must be 16-byte aligned"); return VITX_ERR_ARG; }
    if (E % 64) { set_error("vitx_op_zeroshot: E = %d is not a multiple of 64 (the GEMMs' K step)", E); return VITX_ERR_UNSUPPORTED; }
    if (K > vitx_zeroshot_max_classes(E)) { set_error("vitx_op_zeroshot: %d classes of width %d exceed the bank GEMM's 32-bit window (at most %d)", K, E, vitx_zeroshot_max_classes(E)); return VITX_ERR_UNSUPPORTED; }
    const Tuning *t = tuning_for_device(-1);
    if (!t) { set_error("vitx_op_zeroshot: kernel bring-up failed"); return VITX_ERR_HIP; }
    const int Kpad = round_up(K, gemm_tile_n()), M = round_up(n, gemm_tile_m());
    hipStream_t st = (hipStream_t)stream;
    float *acc = (float *)d_acc_scratch, *zero = acc + (size_t)M * Kpad;
    hipError_t e = hipMemsetAsync(zero, 0, (size_t)Kpad * 4, st);
    if (e == hipSuccess) e = head_zeroshot(HeadLaunch{*t, dtype, st, nullptr}, (const float *)d_z, z_stride, d_a_scratch, d_bank, zero, acc, (float *)d_probs, (float *)d_logits, K, n, K, E, kind, scale, bias);
    return op_rc("vitx_op_zeroshot", e, VITX_ERR_UNSUPPORTED);
}

// Nearest neighbours on the caller's buffers (include/vitx.h "nearest neighbours in a gallery").  Every argument check comes before the first device
// call; all of them only enqueue.
size_t vitx_op_nn_state_bytes(int n, int k) { return nn_state_bytes(n, k); }
int vitx_op_nn_select(const void *d_scores, long ld, int n, int cols, long base_index, void *d_state, int k, int first, void *stream) {
    if (!d_scores || !d_state || n <= 0 || cols <= 0 || ld < cols || k < 1 || base_index < 0 || (uintptr_t)d_scores % 4 || (uintptr_t)d_state % 8) { set_error("vitx_op_nn_select: invalid argument"); return VITX_ERR_ARG; }
    if (k > kNnMaxK) { set_error("vitx_op_nn_select: k = %d above %d", k, kNnMaxK); return VITX_ERR_UNSUPPORTED; }
    if (base_index + cols > 0x7fffffffL) { set_error("vitx_op_nn_select: gallery indices are 31 bits (base_index %ld + %d columns)", base_index, cols); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_nn_select", launch_nn_select((const float *)d_scores, ld, n, cols, base_index, d_state, k, first != 0, (hipStream_t)stream), VITX_ERR_ARG);
}
int vitx_op_nn_finish(const void *d_state, int n, int k, const void *d_labels, int n_labels, float temperature, void *d_pairs, void *d_vote, void *stream) {
    if (!d_state || !d_pairs || n <= 0 || k < 1 || (uintptr_t)d_state % 8 || (uintptr_t)d_pairs % 4) { set_error("vitx_op_nn_finish: invalid argument"); return VITX_ERR_ARG; }
    if (d_labels && (n_labels < 1 || !d_vote || !(std::isfinite(temperature) && temperature > 0.0f))) { set_error("vitx_op_nn_finish: labels need n_labels >= 1, d_vote and a finite positive temperature"); return VITX_ERR_ARG; }
    if (k > kNnMaxK) { set_error("vitx_op_nn_finish: k = %d above %d", k, kNnMaxK); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_nn_finish", launch_nn_finish(d_state, n, k, (const int *)d_labels, n_labels, temperature, d_pairs, (float *)d_vote, (hipStream_t)stream), VITX_ERR_ARG);
}
// The sequence the forward of a context with a gallery runs (head_nearest, heads.cpp), without the vote.  The GEMMs' bias is the row of zeros the
// call writes behind the score rows.
int vitx_op_nn(int dtype, const void *d_z, long z_stride, int z_is_operand, int n, const void *d_gallery, long G, int E, int k, int chunk,
               void *d_a_scratch, void *d_acc_scratch, void *d_state, void *d_pairs, void *stream) {
    if (!d_z || !d_gallery || !d_a_scratch || !d_acc_scratch || !d_state || !d_pairs || n <= 0 || G <= 0 || E <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_nn: invalid argument"); return VITX_ERR_ARG; }
    if (k < 1 || k > G) { set_error("vitx_op_nn: k = %d outside 1 .. G = %ld", k, G); return VITX_ERR_ARG; }
    if (chunk <= 0 || chunk % gemm_tile_n()) { set_error("vitx_op_nn: chunk = %d is not a positive multiple of %d", chunk, gemm_tile_n()); return VITX_ERR_ARG; }
    if (z_stride < E || z_stride % 4) { set_error("vitx_op_nn: z_stride %ld must be at least E = %d and a multiple of 4 elements", z_stride, E); return VITX_ERR_ARG; }
    for (const void *p : {d_z, d_gallery, (const void *)d_a_scratch, (const void *)d_acc_scratch, (const void *)d_state})
        if ((uintptr_t)p % 16) { set_error("vitx_op_nn: d_z, d_gallery, the scratch buffers and the state must be 16-byte aligned"); return VITX_ERR_ARG; }
    if (k > kNnMaxK) { set_error("vitx_op_nn: k = %d above %d", k, kNnMaxK); return VITX_ERR_UNSUPPORTED; }
    if (E % 64) { set_error("vitx_op_nn: E = %d is not a multiple of 64 (the GEMMs' K step)", E); return VITX_ERR_UNSUPPORTED; }
    if (G >= 0x7fffffffL - 127) { set_error("vitx_op_nn: %ld gallery rows: indices are 31 bits", G); return VITX_ERR_UNSUPPORTED; }
    if ((size_t)chunk * E * 2 > 0xf0000000u) { set_error("vitx_op_nn: a chunk of %d rows of width %d exceeds the GEMM's 32-bit operand window", chunk, E); return VITX_ERR_UNSUPPORTED; }
    const Tuning *t = tuning_for_device(-1);
    if (!t) { set_error("vitx_op_nn: kernel bring-up failed"); return VITX_ERR_HIP; }
    const int M = round_up(n, gemm_tile_m());
    hipStream_t st = (hipStream_t)stream;
    float *acc = (float *)d_acc_scratch, *zero = acc + (size_t)M * chunk;
    hipError_t e = hipMemsetAsync(zero, 0, (size_t)chunk * 4, st);
    if (e == hipSuccess) e = head_nearest(HeadLaunch{*t, dtype, st, nullptr}, d_z, z_stride, z_is_operand != 0, d_a_scratch, d_gallery, zero, acc, d_state, G, E, k, chunk, nullptr, 0, 0.0f, d_pairs, nullptr, n);
    return op_rc("vitx_op_nn", e, VITX_ERR_UNSUPPORTED);
}

// The dense head on the caller's buffers (include/vitx.h "dense prediction").  dense_label_args: the checks the device entry point and its host twin
// share -- none needs a device.
static int dense_label_args(const char *name, const void *logits, long ld, int n, int gh, int gw, int K, int out_h, int out_w, const void *labels) {
    if (!logits || !labels || n < 1 || gh < 1 || gw < 1 || K < 1) { set_error("%s: invalid argument", name); return VITX_ERR_ARG; }
    if (ld < ((K + 3) & ~3) || ld % 4) { set_error("%s: ld = %ld must be a multiple of 4 and at least K = %d rounded up to 4", name, ld, K); return VITX_ERR_ARG; }
    if (K > kDenseMaxK) { set_error("%s: K = %d classes above %d (labels are bytes)", name, K, kDenseMaxK); return VITX_ERR_UNSUPPORTED; }
    if (out_h < gh || out_w < gw || out_h > kDenseMaxOut || out_w > kDenseMaxOut) { set_error("%s: output %d x %d outside the grid %d x %d .. %d (upsampling only)", name, out_h, out_w, gh, gw, kDenseMaxOut); return VITX_ERR_UNSUPPORTED; }
    if (n > 65535 || (size_t)n * gh * gw > 0x7fffffffu) { set_error("%s: %d images of %d x %d patches in one launch", name, n, gh, gw); return VITX_ERR_UNSUPPORTED; }
    return VITX_OK;
}
int vitx_op_dense_labels(const void *d_logits, long ld, int n, int gh, int gw, int K, int out_h, int out_w, void *d_labels, void *d_score, void *stream) {
    if (const int rc = dense_label_args("vitx_op_dense_labels", d_logits, ld, n, gh, gw, K, out_h, out_w, d_labels)) return rc;
    if ((uintptr_t)d_logits % 16 || (uintptr_t)d_score % 4) { set_error("vitx_op_dense_labels: d_logits must be 16-byte, d_score 4-byte aligned"); return VITX_ERR_ARG; }
    return op_rc("vitx_op_dense_labels", launch_dense_labels((const float *)d_logits, ld, n, gh, gw, K, out_h, out_w, (uint8_t *)d_labels, (float *)d_score, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
// The label kernel on a pack (include/vitx.h "packed batches"): vitx_op_dense_labels's checks image by image, the tables built by the one host
// function (dense_pack_tables) and uploaded in one copy -- tile0 [n + 1] | seg [n][kDenseSegInts] -- then the launch.  A test entry point: it waits
// for the launch before it frees the tables.
int vitx_op_dense_labels_packed(const void *d_logits, long ld, const int32_t *grids, const int32_t *outs, const int32_t *lrow, int n, int K, void *d_labels, void *d_score,
                                void *stream) {
    const char *name = "vitx_op_dense_labels_packed";
    if (!grids || !outs || !lrow || n < 1) { set_error("%s: invalid argument", name); return VITX_ERR_ARG; }
    for (int i = 0; i < n; ++i) {
        if (const int rc = dense_label_args(name, d_logits, ld, 1, grids[2 * i], grids[2 * i + 1], K, outs[2 * i], outs[2 * i + 1], d_labels)) return rc;
        if (lrow[i] < 0 || (size_t)lrow[i] + (size_t)grids[2 * i] * grids[2 * i + 1] > 0x7fffffffu) { set_error("%s: image %d: first logit row %d", name, i, lrow[i]); return VITX_ERR_ARG; }
    }
    if ((uintptr_t)d_logits % 16 || (uintptr_t)d_score % 4) { set_error("%s: d_logits must be 16-byte, d_score 4-byte aligned", name); return VITX_ERR_ARG; }
    std::vector<int64_t> pix0((size_t)n + 1);
    std::vector<int32_t> tab((size_t)n + 1 + (size_t)n * kDenseSegInts);
    int cells = 0;
    if (!dense_pack_tables(grids, outs, n, pix0.data(), tab.data(), &cells)) { set_error("%s: the outputs hold more than 2^31 - 1 tiles", name); return VITX_ERR_UNSUPPORTED; }
    dense_pack_seg(grids, outs, lrow, pix0.data(), n, tab.data() + n + 1);
    int *d_tab = nullptr;
    HIP_TRY(hipMalloc((void **)&d_tab, tab.size() * 4));
    const DevMem own(d_tab);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    const hipError_t e = launch_dense_labels_packed((const float *)d_logits, ld, d_tab, d_tab + n + 1, n, tab[n], cells, K, (uint8_t *)d_labels, (float *)d_score, st);
    const hipError_t es = hipStreamSynchronize(st);      // the tables are freed, and the staging vector goes, when this returns
    if (e == hipSuccess && es != hipSuccess) return op_rc(name, es);
    return op_rc(name, e, VITX_ERR_UNSUPPORTED);
}
// The two halves of the above for callers that keep the tables (tools/pack_dense_cost.py times the launch alone): the host builder -- tab =
// tile0 [n + 1] | seg [n][kDenseSegInts], *tiles = tile0[n], *cells = the widest window -- and the launch on such a table uploaded by the caller.
int vitx_dense_pack_tables(const int32_t *grids, const int32_t *outs, const int32_t *lrow, int n, int32_t *tab, int *tiles, int *cells) {
    if (!grids || !outs || !lrow || !tab || !tiles || !cells || n < 1) { set_error("vitx_dense_pack_tables: invalid argument"); return VITX_ERR_ARG; }
    std::vector<int64_t> pix0((size_t)n + 1);
    if (!dense_pack_tables(grids, outs, n, pix0.data(), tab, cells)) { set_error("vitx_dense_pack_tables: an output outside its grid .. %d, or more than 2^31 - 1 tiles", kDenseMaxOut); return VITX_ERR_UNSUPPORTED; }
    dense_pack_seg(grids, outs, lrow, pix0.data(), n, tab + n + 1);
    *tiles = tab[n];
    return VITX_OK;
}
int vitx_op_dense_labels_packed_tables(const void *d_logits, long ld, const void *d_tab, int n, int tiles, int cells, int K, void *d_labels, void *d_score, void *stream) {
    if (!d_logits || !d_tab || !d_labels || (uintptr_t)d_logits % 16 || (uintptr_t)d_score % 4 || (uintptr_t)d_tab % 4) { set_error("vitx_op_dense_labels_packed_tables: invalid argument"); return VITX_ERR_ARG; }
    return op_rc("vitx_op_dense_labels_packed_tables", launch_dense_labels_packed((const float *)d_logits, ld, (const int *)d_tab, (const int *)d_tab + n + 1, n, tiles, cells, K,
                                                                                     (uint8_t *)d_labels, (float *)d_score, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
// The host twin: dense_resample.h's arithmetic in plain loops, the classes of a pixel walked upwards.  No device call.
int vitx_dense_labels_host(const float *logits, long ld, int n, int gh, int gw, int K, int out_h, int out_w, uint8_t *labels, float *score) {
    if (const int rc = dense_label_args("vitx_dense_labels_host", logits, ld, n, gh, gw, K, out_h, out_w, labels)) return rc;
    const float sy = dense_scale(gh, out_h), sx = dense_scale(gw, out_w);
    std::vector<DenseAxis> axs(out_w);
    for (int x = 0; x < out_w; ++x) axs[x] = dense_axis(gw, sx, x);
    for (int i = 0; i < n; ++i) {
        const float *lg = logits + (size_t)i * gh * gw * ld;
        for (int y = 0; y < out_h; ++y) {
            const DenseAxis ay = dense_axis(gh, sy, y);
            for (int x = 0; x < out_w; ++x) {
                const DenseAxis &ax = axs[x];
                const float *a = lg + ((size_t)ay.i0 * gw + ax.i0) * ld, *b = lg + ((size_t)ay.i0 * gw + ax.i1) * ld;
                const float *c = lg + ((size_t)ay.i1 * gw + ax.i0) * ld, *d = lg + ((size_t)ay.i1 * gw + ax.i1) * ld;
                DenseBest best = dense_best_init();
                for (int k = 0; k < K; ++k) dense_offer(best, dense_value(ax.h, ax.l, ay.h, ay.l, a[k], b[k], c[k], d[k]), k);
                const size_t pix = ((size_t)i * out_h + y) * out_w + x;
                labels[pix] = (uint8_t)best.cls;
                if (score) score[pix] = dense_score(best);
            }
        }
    }
    return VITX_OK;
}
// The sequence the forward of a context with a dense head runs after its operand rows are written (head_dense, heads.cpp).
int vitx_op_dense(int dtype, void *d_a, const void *d_w, const void *d_bias, void *d_logits, int n, int gh, int gw, int K, int Dc, int out_h, int out_w,
                  void *d_labels, void *d_score, void *stream) {
    if (!d_a || !d_w || !d_bias || Dc < 1 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_dense: invalid argument"); return VITX_ERR_ARG; }
    const int Kpad = K > 0 ? round_up(K, gemm_tile_n()) : 0;
    if (const int rc = dense_label_args("vitx_op_dense", d_logits, Kpad, n, gh, gw, K, out_h, out_w, d_labels)) return rc;
    for (const void *p : {(const void *)d_a, d_w, d_bias, (const void *)d_logits, (const void *)d_score})
        if ((uintptr_t)p % 16) { set_error("vitx_op_dense: every pointer but d_labels must be 16-byte aligned"); return VITX_ERR_ARG; }
    if (Dc % 64) { set_error("vitx_op_dense: Dc = %d is not a multiple of 64 (the GEMMs' K step)", Dc); return VITX_ERR_UNSUPPORTED; }
    const int rows = n * gh * gw, M = round_up(rows, gemm_tile_m());
    if ((size_t)M * Dc * 2 > 0xf0000000u || (size_t)M * Kpad * 4 > 0xf0000000u || (size_t)Kpad * Dc * 2 > 0xf0000000u) { set_error("vitx_op_dense: %d rows of width %d leave the GEMM's 32-bit byte window", M, Dc); return VITX_ERR_UNSUPPORTED; }
    const Tuning *t = tuning_for_device(-1);
    if (!t) { set_error("vitx_op_dense: kernel bring-up failed"); return VITX_ERR_HIP; }
    return op_rc("vitx_op_dense", head_dense(HeadLaunch{*t, dtype, (hipStream_t)stream, nullptr}, d_a, d_w, (const float *)d_bias, (float *)d_logits, n, gh, gw, K, Dc, out_h, out_w,
                                             (uint8_t *)d_labels, (float *)d_score, nullptr), VITX_ERR_UNSUPPORTED);
}

// The depth head on the caller's buffers (include/vitx.h "depth estimation"); depth_fine_args / depth_resize_args: heads.h, depth_host.cpp.
int vitx_op_depth_fine(const void *d_logits, long ld, const void *d_offsets, const void *d_bins, int n, int gh, int gw, int K, int upsample, void *d_fine, void *stream) {
    if (const int rc = depth_fine_args("vitx_op_depth_fine", d_logits, ld, d_bins, n, gh, gw, K, upsample, d_fine)) return rc;
    if ((uintptr_t)d_logits % 16 || (uintptr_t)d_offsets % 16 || (uintptr_t)d_bins % 4 || (uintptr_t)d_fine % 4) { set_error("vitx_op_depth_fine: d_logits and d_offsets must be 16-byte, d_bins and d_fine 4-byte aligned"); return VITX_ERR_ARG; }
    return op_rc("vitx_op_depth_fine", launch_depth_fine((const float *)d_logits, ld, (const float *)d_offsets, ld, (const float *)d_bins, n, gh, gw, K, upsample, (float *)d_fine, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
int vitx_op_depth_resize(const void *d_fine, int n, int fh, int fw, int out_h, int out_w, float min_depth, float max_depth, void *d_out, void *stream) {
    if (const int rc = depth_resize_args("vitx_op_depth_resize", d_fine, n, fh, fw, out_h, out_w, min_depth, max_depth, d_out)) return rc;
    if ((uintptr_t)d_fine % 4 || (uintptr_t)d_out % 4) { set_error("vitx_op_depth_resize: d_fine and d_out must be 4-byte aligned"); return VITX_ERR_ARG; }
    return op_rc("vitx_op_depth_resize", launch_depth_resize((const float *)d_fine, n, fh, fw, out_h, out_w, min_depth, max_depth, (float *)d_out, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
// The two depth kernels on a pack (include/vitx.h "packed batches"): vitx_op_depth_fine's / vitx_op_depth_resize's checks image by image, the tables
// built by the one host function (depth_pack_tables) and uploaded in one copy -- ftile0 [n + 1] | otile0 [n + 1] | seg [n][kDepthSegInts] -- then the
// launch.  Test entry points: they wait for the launch before they free the tables.  Image i's offsets are row orow[i] of d_offsets, rows ld floats apart.
static int depth_packed_run(const char *name, const int32_t *grids, const int32_t *outs, const int32_t *lrow, const int32_t *orow, int n, int u, hipStream_t st,
                            hipError_t (*launch)(const int *d_tab, int n, int ftiles, int otiles, int cells, void *arg, hipStream_t st), void *arg) {
    std::vector<int64_t> pix0((size_t)n + 1), fine0((size_t)n + 1);
    std::vector<int32_t> tab((size_t)2 * (n + 1) + (size_t)n * kDepthSegInts);
    int cells = 0;
    if (!depth_pack_tables(grids, outs, n, u, pix0.data(), fine0.data(), tab.data(), tab.data() + n + 1, &cells)) { set_error("%s: the planes hold more than 2^31 - 1 tiles", name); return VITX_ERR_UNSUPPORTED; }
    depth_pack_seg(grids, outs, lrow, orow, fine0.data(), pix0.data(), n, u, tab.data() + 2 * (n + 1));
    int *d_tab = nullptr;
    HIP_TRY(hipMalloc((void **)&d_tab, tab.size() * 4));
    const DevMem own(d_tab);
    HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    const hipError_t e = launch(d_tab, n, tab[n], tab[2 * n + 1], cells, arg, st);
    const hipError_t es = hipStreamSynchronize(st);      // the tables are freed, and the staging vector goes, when this returns
    if (e == hipSuccess && es != hipSuccess) return op_rc(name, es);
    return op_rc(name, e, VITX_ERR_UNSUPPORTED);
}
int vitx_op_depth_fine_packed(const void *d_logits, long ld, const void *d_offsets, const void *d_bins, const int32_t *grids, const int32_t *lrow, const int32_t *orow, int n, int K,
                              int upsample, void *d_fine, void *stream) {
    const char *name = "vitx_op_depth_fine_packed";
    if (!grids || !lrow || (d_offsets && !orow) || n < 1) { set_error("%s: invalid argument", name); return VITX_ERR_ARG; }
    std::vector<int32_t> outs((size_t)2 * n), zero((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        if (const int rc = depth_fine_args(name, d_logits, ld, d_bins, 1, grids[2 * i], grids[2 * i + 1], K, upsample, d_fine)) return rc;
        if (lrow[i] < 0 || (size_t)lrow[i] + (size_t)grids[2 * i] * grids[2 * i + 1] > 0x7fffffffu) { set_error("%s: image %d: first logit row %d", name, i, lrow[i]); return VITX_ERR_ARG; }
        if (d_offsets && orow[i] < 0) { set_error("%s: image %d: offsets row %d", name, i, orow[i]); return VITX_ERR_ARG; }
        outs[2 * i] = upsample * grids[2 * i]; outs[2 * i + 1] = upsample * grids[2 * i + 1];
    }
    if ((uintptr_t)d_logits % 16 || (uintptr_t)d_offsets % 16 || (uintptr_t)d_bins % 4 || (uintptr_t)d_fine % 4) { set_error("%s: d_logits and d_offsets must be 16-byte, d_bins and d_fine 4-byte aligned", name); return VITX_ERR_ARG; }
    struct Arg { const float *lg; long ld; const float *off, *bins; int K; float *fine; } a{(const float *)d_logits, ld, (const float *)d_offsets, (const float *)d_bins, K, (float *)d_fine};
    return depth_packed_run(name, grids, outs.data(), lrow, d_offsets ? orow : zero.data(), n, upsample, (hipStream_t)stream,
                            [](const int *t, int n_, int ftiles, int, int cells, void *v, hipStream_t st) {
                                const Arg &g = *(const Arg *)v;
                                return launch_depth_fine_packed(g.lg, g.ld, g.off, g.ld, g.bins, t, t + 2 * (n_ + 1), n_, ftiles, cells, g.K, g.fine, st);
                            }, &a);
}
int vitx_op_depth_resize_packed(const void *d_fine, const int32_t *fines, const int32_t *outs, int n, float min_depth, float max_depth, void *d_out, void *stream) {
    const char *name = "vitx_op_depth_resize_packed";
    if (!fines || !outs || n < 1) { set_error("%s: invalid argument", name); return VITX_ERR_ARG; }
    for (int i = 0; i < n; ++i)
        if (const int rc = depth_resize_args(name, d_fine, 1, fines[2 * i], fines[2 * i + 1], outs[2 * i], outs[2 * i + 1], min_depth, max_depth, d_out)) return rc;
    if ((uintptr_t)d_fine % 4 || (uintptr_t)d_out % 4) { set_error("%s: d_fine and d_out must be 4-byte aligned", name); return VITX_ERR_ARG; }
    struct Arg { const float *fine; float lo, hi; float *out; } a{(const float *)d_fine, min_depth, max_depth, (float *)d_out};
    const std::vector<int32_t> zero((size_t)n, 0);
    // the fine planes stand in for the grids of the table (u = 1): the resize reads the fine shape, the output shape and the two base offsets
    return depth_packed_run(name, fines, outs, zero.data(), zero.data(), n, 1, (hipStream_t)stream,
                            [](const int *t, int n_, int, int otiles, int, void *v, hipStream_t st) {
                                const Arg &g = *(const Arg *)v;
                                return launch_depth_resize_packed(g.fine, t + n_ + 1, t + 2 * (n_ + 1), n_, otiles, g.lo, g.hi, g.out, st);
                            }, &a);
}
// The halves of the above for callers that keep the tables (tools/pack_depth_cost.py times the launches alone): the host builder -- tab = ftile0 [n + 1] |
// otile0 [n + 1] | seg [n][kDepthSegInts], *ftiles = ftile0[n], *otiles = otile0[n], *cells = the widest window -- and the launches on such a table
// uploaded by the caller.
int vitx_depth_pack_tables(const int32_t *grids, const int32_t *outs, const int32_t *lrow, const int32_t *orow, int n, int upsample, int32_t *tab, int *ftiles, int *otiles, int *cells) {
    if (!grids || !outs || !lrow || !orow || !tab || !ftiles || !otiles || !cells || n < 1) { set_error("vitx_depth_pack_tables: invalid argument"); return VITX_ERR_ARG; }
    std::vector<int64_t> pix0((size_t)n + 1), fine0((size_t)n + 1);
    if (!depth_pack_tables(grids, outs, n, upsample, pix0.data(), fine0.data(), tab, tab + n + 1, cells)) {
        set_error("vitx_depth_pack_tables: upsample not 1, 2 or 4, an output outside its fine plane .. %d, or more than 2^31 - 1 tiles", kDepthMaxOut);
        return VITX_ERR_UNSUPPORTED;
    }
    depth_pack_seg(grids, outs, lrow, orow, fine0.data(), pix0.data(), n, upsample, tab + 2 * (n + 1));
    *ftiles = tab[n]; *otiles = tab[2 * n + 1];
    return VITX_OK;
}
int vitx_op_depth_fine_packed_tables(const void *d_logits, long ld, const void *d_offsets, long ldo, const void *d_bins, const void *d_tab, int n, int tiles, int cells, int K,
                                     void *d_fine, void *stream) {
    if (!d_logits || !d_bins || !d_tab || !d_fine || (uintptr_t)d_logits % 16 || (uintptr_t)d_offsets % 16 || (uintptr_t)d_bins % 4 || (uintptr_t)d_fine % 4 || (uintptr_t)d_tab % 4) {
        set_error("vitx_op_depth_fine_packed_tables: invalid argument");
        return VITX_ERR_ARG;
    }
    return op_rc("vitx_op_depth_fine_packed_tables", launch_depth_fine_packed((const float *)d_logits, ld, (const float *)d_offsets, ldo, (const float *)d_bins, (const int *)d_tab,
                                                                              (const int *)d_tab + 2 * (n + 1), n, tiles, cells, K, (float *)d_fine, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
int vitx_op_depth_resize_packed_tables(const void *d_fine, const void *d_tab, int n, int tiles, float min_depth, float max_depth, void *d_out, void *stream) {
    if (!d_fine || !d_tab || !d_out || (uintptr_t)d_fine % 4 || (uintptr_t)d_out % 4 || (uintptr_t)d_tab % 4) { set_error("vitx_op_depth_resize_packed_tables: invalid argument"); return VITX_ERR_ARG; }
    return op_rc("vitx_op_depth_resize_packed_tables", launch_depth_resize_packed((const float *)d_fine, (const int *)d_tab + n + 1, (const int *)d_tab + 2 * (n + 1), n, tiles, min_depth,
                                                                                  max_depth, (float *)d_out, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}
// The sequence the forward of a context with a depth head runs after its operand rows are written (head_depth, heads.cpp).  The patch GEMM's zero
// bias is the row of zeros the call writes behind the logit rows.
int vitx_op_depth(int dtype, void *d_a, const void *d_wp, void *d_acls, const void *d_wc, const void *d_bias, const void *d_bins, void *d_logits, void *d_offsets,
                  int n, int gh, int gw, int K, int Dc, int upsample, int out_h, int out_w, float min_depth, float max_depth, void *d_fine, void *d_depth, void *stream) {
    if (!d_a || !d_wp || !d_bias || Dc < 1 || (dtype != VITX_F16 && dtype != VITX_BF16) || (!d_wc) != (!d_acls) || (d_wc && !d_offsets)) { set_error("vitx_op_depth: invalid argument"); return VITX_ERR_ARG; }
    const int Kpad = K > 0 ? round_up(K, gemm_tile_n()) : 0;
    if (const int rc = depth_fine_args("vitx_op_depth", d_logits, Kpad, d_bins, n, gh, gw, K, upsample, d_fine)) return rc;
    const int fh = upsample * gh, fw = upsample * gw;
    if (const int rc = depth_resize_args("vitx_op_depth", d_fine, n, fh, fw, out_h, out_w, min_depth, max_depth, d_depth)) return rc;
    for (const void *p : {(const void *)d_a, d_wp, (const void *)d_acls, d_wc, d_bias, d_bins, (const void *)d_logits, (const void *)d_offsets, (const void *)d_fine})
        if ((uintptr_t)p % 16) { set_error("vitx_op_depth: every pointer but d_depth must be 16-byte aligned"); return VITX_ERR_ARG; }
    if ((uintptr_t)d_depth % 4) { set_error("vitx_op_depth: d_depth must be 4-byte aligned"); return VITX_ERR_ARG; }
    if (Dc % 64) { set_error("vitx_op_depth: Dc = %d is not a multiple of 64 (the GEMMs' K step)", Dc); return VITX_ERR_UNSUPPORTED; }
    const int rows = n * gh * gw, M = round_up(rows, gemm_tile_m());
    if ((size_t)M * Dc * 2 > 0xf0000000u || (size_t)(M + 1) * Kpad * 4 > 0xf0000000u || (size_t)Kpad * Dc * 2 > 0xf0000000u) { set_error("vitx_op_depth: %d rows of width %d leave the GEMM's 32-bit byte window", M, Dc); return VITX_ERR_UNSUPPORTED; }
    const Tuning *t = tuning_for_device(-1);
    if (!t) { set_error("vitx_op_depth: kernel bring-up failed"); return VITX_ERR_HIP; }
    hipStream_t st = (hipStream_t)stream;
    float *acc = (float *)d_logits, *zero = acc + (size_t)M * Kpad;
    hipError_t e = hipMemsetAsync(zero, 0, (size_t)Kpad * 4, st);
    if (e == hipSuccess) e = head_depth(HeadLaunch{*t, dtype, st, nullptr}, d_a, d_wp, zero, acc, d_acls, d_wc, (const float *)d_bias, (float *)d_offsets, (const float *)d_bins,
                                        n, gh, gw, K, Dc, upsample, out_h, out_w, min_depth, max_depth, (float *)d_fine, (float *)d_depth, nullptr, nullptr);
    return op_rc("vitx_op_depth", e, VITX_ERR_UNSUPPORTED);
}
// The raw operand rows on their own: y[row][0 .. D) (dtype, row stride ldy elements) = RNE(x[row][0 .. D)) (f32, row stride ldx floats)
int vitx_op_depth_rows(int dtype, const void *d_x, long ldx, void *d_y, long ldy, int rows, int D, void *stream) {
    if (!d_x || !d_y || rows < 1 || D < 1 || ldx < D || ldy < D || (dtype != VITX_F16 && dtype != VITX_BF16) || (uintptr_t)d_x % 16 || (uintptr_t)d_y % 16) { set_error("vitx_op_depth_rows: invalid argument"); return VITX_ERR_ARG; }
    if (D % 8 || ldx % 4 || ldy % 8) { set_error("vitx_op_depth_rows: D %% 8, ldx %% 4 and ldy %% 8 must be 0"); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_depth_rows", launch_depth_rows(dtype, (const float *)d_x, ldx, d_y, ldy, rows, D, (hipStream_t)stream), VITX_ERR_UNSUPPORTED);
}

// The text tower's three kernels on their own (include/vitx.h "the text tower").  Every argument check comes before the first device call.
int vitx_op_text_embed(int table_f16, const void *d_tok, const void *d_pos, const void *d_ids, void *d_x, int n, int T, int D, void *stream) {
    if (!d_tok || !d_pos || !d_ids || !d_x || n <= 0 || T <= 0 || D <= 0 || D % 8) { set_error("vitx_op_text_embed: invalid argument (D %% 8 == 0)"); return VITX_ERR_ARG; }
    for (const void *p : {d_tok, d_pos, (const void *)d_x})
        if ((uintptr_t)p % 16) { set_error("vitx_op_text_embed: pointers must be 16-byte aligned"); return VITX_ERR_ARG; }
    return op_rc("vitx_op_text_embed", launch_text_embed(table_f16 != 0, d_tok, (const float *)d_pos, (const int *)d_ids, (float *)d_x, n, T, D, (hipStream_t)stream), VITX_ERR_ARG);
}
int vitx_op_text_pool(int dtype, const void *d_x, const void *d_pooled, const void *d_w, const void *d_b, void *d_z, int n, int T, int D, float eps, void *stream) {
    if (!d_x || !d_pooled || !d_w || !d_b || !d_z || n <= 0 || T <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_text_pool: invalid argument"); return VITX_ERR_ARG; }
    if (!layernorm_supports(D)) { set_error("vitx_op_text_pool: hidden size %d has no LayerNorm instantiation", D); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_text_pool", launch_text_pool(dtype, (const float *)d_x, (const int *)d_pooled, (const float *)d_w, (const float *)d_b, d_z, n, n, T, D, eps, (hipStream_t)stream));
}
// The generic head-dim kernel at ANY head dim, 64 included (where the dispatcher prefers the tuned families): tools/text_cost.py measures the text
// attention against it.  Only enqueues.
int vitx_op_attention_generic(int dtype, const void *d_qkv, void *d_out, int n_img, int N, int D, int H, void *stream) {
    if (!d_qkv || !d_out || n_img <= 0 || N <= 0 || D <= 0 || H <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_attention_generic: invalid argument"); return VITX_ERR_ARG; }
    if (!attention_generic_supports(D, H)) { set_error("vitx_op_attention_generic: head_dim must be a multiple of 8 up to 128 (D %d, H %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    return op_rc("vitx_op_attention_generic", launch_attention_generic(dtype, d_qkv, d_out, n_img, N, D, H, (hipStream_t)stream));
}
int vitx_op_attention_text(int dtype, const void *d_qkv, void *d_out, int n, int T, int D, int H, int causal, void *stream) {
    if (!d_qkv || !d_out || n <= 0 || T <= 0 || D <= 0 || H <= 0 || (dtype != VITX_F16 && dtype != VITX_BF16)) { set_error("vitx_op_attention_text: invalid argument"); return VITX_ERR_ARG; }
    if (!attention_text_supports(T, D, H)) { set_error("vitx_op_attention_text: 1 <= T <= %d and a head dim that is a multiple of 8 up to 128 (T %d, D %d, H %d)", VITX_TEXT_MAX_TOKENS, T, D, H); return VITX_ERR_UNSUPPORTED; }
    if (!tuning_for_device(-1)) { set_error("vitx_op_attention_text: kernel bring-up failed"); return VITX_ERR_HIP; }
    return op_rc("vitx_op_attention_text", launch_attention_text(dtype, d_qkv, d_out, n, T, D, H, causal, (hipStream_t)stream));
}

int vitx_preprocess_ex_device_supports(const vitx_preproc *pp, int nx, int ny) { return pp && preprocess_ex_supports(*pp, nx, ny) ? 1 : 0; }
int vitx_preprocess_ex_device(const vitx_preproc *pp, const void *d_hwc, int n, int nx, int ny, void *d_out, void *stream) {
    if (!pp || !d_hwc || !d_out || n <= 0) { set_error("vitx_preprocess_ex_device: invalid argument"); return VITX_ERR_ARG; }
    PpGeom g;
    const char *bad = pp_check(*pp);
    if (!bad) bad = pp_geometry(*pp, nx, ny, g);
    if (bad) { set_error("vitx_preprocess_ex_device: %s", bad); return VITX_ERR_ARG; }
    if (!preprocess_ex_supports(*pp, nx, ny)) {
        set_error("vitx_preprocess_ex_device: a %d x %d source resized to %d x %d needs more than 64 KiB of LDS per tile (use vitx_preprocess_ex)", nx, ny, g.W, g.H);
        return VITX_ERR_UNSUPPORTED;
    }
    return op_rc("vitx_preprocess_ex_device", launch_preprocess_ex(*pp, d_hwc, (float *)d_out, n, nx, ny, (hipStream_t)stream));
}
int vitx_preprocess_rect_device_supports(const vitx_preproc *pp, int nx, int ny, int out_w, int out_h) { return pp && preprocess_rect_supports(*pp, nx, ny, out_w, out_h) ? 1 : 0; }
int vitx_preprocess_rect_device(const vitx_preproc *pp, const void *d_hwc, int n, int nx, int ny, int out_w, int out_h, void *d_out, void *stream) {
    if (!pp || !d_hwc || !d_out || n <= 0) { set_error("vitx_preprocess_rect_device: invalid argument"); return VITX_ERR_ARG; }
    PpGeom g;
    const char *bad = pp_check(*pp);
    if (!bad) bad = pp_geometry_rect(nx, ny, out_w, out_h, g);
    if (bad) { set_error("vitx_preprocess_rect_device: %s", bad); return VITX_ERR_ARG; }
    if (!pp_filter_is_pil(pp->filter)) { set_error("vitx_preprocess_rect_device: the reference's filters resize to squares only (use a PIL filter)"); return VITX_ERR_UNSUPPORTED; }
    if (!preprocess_rect_supports(*pp, nx, ny, out_w, out_h)) {
        set_error("vitx_preprocess_rect_device: a %d x %d source resized to %d x %d needs more than 64 KiB of LDS per tile (use vitx_preprocess_rect)", nx, ny, out_w, out_h);
        return VITX_ERR_UNSUPPORTED;
    }
    return op_rc("vitx_preprocess_rect_device", launch_preprocess_rect(*pp, d_hwc, (float *)d_out, n, nx, ny, out_w, out_h, (hipStream_t)stream));
}
// The PIL kernel on a pack (include/vitx.h "packed batches", u8 sources): the tables built by the one host function (pp_pack_tables: its refusals) and
// uploaded in one copy -- tile0 [n + 1] | seg [n][kPpSegInts] -- then the launch, on the null stream.  A test entry point: it waits for the launch
// before it frees the tables.
int vitx_op_preprocess_pack(const vitx_preproc *pp, const void *d_srcs, const int32_t *src_shapes, const int32_t *out_shapes, int n, void *d_out) {
    const char *name = "vitx_op_preprocess_pack";
    if (!pp || !d_srcs || !src_shapes || !out_shapes || !d_out || n < 1) { set_error("%s: invalid argument", name); return VITX_ERR_ARG; }
    if ((uintptr_t)d_srcs % 4 || (uintptr_t)d_out % 4) { set_error("%s: d_srcs and d_out must be 4-byte aligned", name); return VITX_ERR_ARG; }
    std::vector<int32_t> tab((size_t)n + 1 + (size_t)n * kPpSegInts);
    int lds = 0;
    if (const int rc = pp_pack_tables(name, *pp, src_shapes, out_shapes, n, nullptr, nullptr, tab.data(), tab.data() + n + 1, &lds)) return rc;
    int *d_tab = nullptr;
    HIP_TRY(hipMalloc((void **)&d_tab, tab.size() * 4));
    const DevMem own(d_tab);
    HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, nullptr));
    const hipError_t e = launch_preprocess_pack(*pp, d_srcs, (float *)d_out, d_tab, d_tab + n + 1, n, tab[n], lds, nullptr);
    const hipError_t es = hipStreamSynchronize(nullptr);      // the tables are freed, and the staging vector goes, when this returns
    if (e == hipSuccess && es != hipSuccess) return op_rc(name, es);
    return op_rc(name, e);
}
int vitx_preprocess_u8_device(const void *d_hwc, int n, int nx, int ny, int img_size, int interp, void *d_out, void *stream) {
    if (!d_hwc || !d_out || n <= 0 || nx <= 0 || ny <= 0 || img_size <= 0) { set_error("vitx_preprocess_u8_device: invalid argument"); return VITX_ERR_ARG; }
    if (interp != VITX_BICUBIC && interp != VITX_BILINEAR) { set_error("vitx_preprocess_u8_device: interpolation mode %d is not supported", interp); return VITX_ERR_ARG; }
    return op_rc("vitx_preprocess_u8_device", launch_preprocess(d_hwc, (float *)d_out, n, nx, ny, img_size, interp == VITX_BICUBIC, (hipStream_t)stream));
}

}  // extern "C"
