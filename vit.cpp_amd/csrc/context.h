// context.h -- the execution context (struct vitx_ctx) as context.cpp, forward.cpp, outputs.cpp, heads.cpp and ops.cpp share it: what a forward
// uses.  The weights it reads are a WeightSet (weights.h), its opt-in outputs the structs of heads.h.  Internal: nothing outside those five files
// includes it (depth_host.cpp shares its argument checks with ops.cpp through heads.h); callers see the opaque vitx_ctx of include/vitx.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "heads.h"
#include "weights.h"

namespace vitx {

enum ProfClass {
    PC_GEMM_PATCH = 0, PC_LAYERNORM, PC_GEMM_QKV, PC_ATTENTION, PC_GEMM_PROJ, PC_GEMM_FC1, PC_GEMM_FC2,
    PC_GEMM_HEAD, PC_SOFTMAX, PC_DEQUANT, PC_ATTENTION_CLS, PC_GEMM_TAIL, PC_ATTN_MAP, PC_FEATURES, PC_HEAD_POOL, PC_ZEROSHOT, PC_ROPE, PC_SWIGLU, PC_NN, PC_DENSE, PC_DEPTH, PC_COUNT
};
inline const char *const kProfNames[PC_COUNT] = {"patch_embed", "layernorm", "gemm_qkv_bias", "attention", "gemm_proj_resid",
                                    "gemm_fc1_gelu", "gemm_fc2_resid", "gemm_head", "softmax", "dequant_weights", "attention_cls", "gemm_cls_tail", "attention_map",
                                    "features", "head_pool", "zeroshot", "rope", "swiglu", "nn", "dense", "depth"};
static_assert(PC_COUNT <= VITX_PROF_MAX_CLASSES, "vitx_profile_read callers size their arrays by VITX_PROF_MAX_CLASSES");

static_assert(VITX_F16 == DT_F16 && VITX_BF16 == DT_BF16, "the API's dtype values are handed to the launchers as they are");
}  // namespace vitx
using namespace vitx;

struct vitx_ctx {
    const vitx_model *model = nullptr;
    vitx_hparams hp{};
    int device = 0, dtype = VITX_F16, max_batch = 0;   // dtype: the type of every bf16 / f16 kernel (VITX_BF16 in an MXFP8 context)
    bool mx = false;                     // VITX_MXFP8: qkv, fc1 and fc2 take MX operands (norm1, norm2 and the fc1 output are encoded)
    int D = 0, L = 0, H = 0, C = 0, P = 0, N = 0, Kpe = 0, Kpe_pad = 0, C_pad = 0;
    // geometry of THIS context (include/vitx.h "rectangular contexts"): images are [Sh][Sw][Cin], the patch grid is gh x gw, x fastest; a context of
    // vitx_ctx_create_ex has Sh == Sw.  S = the side of a square context, 0 for any other (vitx_ctx_img_size): nothing sizes a buffer with it
    int Sh = 0, Sw = 0, gh = 0, gw = 0, S = 0;
    size_t img_floats() const { return (size_t)Sh * Sw * Cin; }      // one input image
    int Cin = 3;                         // input channels: 3 (RGB classifier) or 1 (ViTSTR, grey)
    int R = 1;                           // probability rows per image: 1 (cls token) or 25 (ViTSTR: tokens 0..24, vitstr.cpp:864-904)
    // Token layout of an image (include/vitx.h "Register tokens and the pooled head"): row 0 = class token, rows 1 .. nreg = register tokens,
    // rows Tp .. N - 1 = patches in raster order; N = gh * gw + Tp
    int nreg = 0, Tp = 1;                // register tokens of the model (reg_token), prefix tokens 1 + nreg (0 for a VITX_POOL_MAP model: no class token)
    int fc1_epi = EPI_BIAS_GELU;         // the fc1 epilogue of the model's activation (vitx_model_activation), taken once at creation; EPI_BIAS in a `glu` context
    // The MLP widths of the blocks: F = the hidden width, fc2's K; F1 = fc1's N.  4 D both, or -- a file with `glu` (include/vitx.h "gated MLP") --
    // the file's F and 2 F: fc1 writes gate | up into Hbuf [Mpad][2 F], the gate kernel (swiglu.hip) the compact Hg [Mpad][F] that fc2 reads
    int F = 0, F1 = 0;
    bool glu = false;
    bool pool = false;                   // VITX_POOL_CLS_MEAN: the head reads concat(cls, mean of the patch tokens) of the final norm, K = 2 D
    bool map = false;                    // VITX_POOL_MAP: no class token; the head reads the attention-pooled embedding e (SliceForward::pooled_tail)
    int tm = 128, tn = 128;
    const Tuning *tune = nullptr;        // per-device launch parameters (CU count, kernel selection), immutable
    int split_first = 0;                 // vitx_ctx_options::split_first: images of the first of two sub-batches (0 = the tile-round model)
#ifdef VITX_LAB
    int skip = 0;                        // VITX_SKIP (upper-bound experiments; results are garbage): 1 = no attention, 2 = no per-layer LayerNorm
#endif
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;          // scratch of THIS context
    // weights: the device copies, shared by every context of the same loaded model, device, requested dtype and block mode (weights.h)
    std::shared_ptr<WeightSet> wset;     // never null once the context exists
    const float *pos = nullptr;          // [1 + gh * gw][D] position table the patch embedding adds: wset->pos, or pos_own when the grid differs from the file's
    float *pos_own = nullptr;            // the table resampled to this context's grid (vitx_ctx_options::img_size, pos_interp); in `allocs`
    // rotary position embeddings of a file with `rope` (include/vitx.h): cos and sin [gh * gw][hd / 2] f32 for THIS context's grid, one allocation in
    // `allocs` (the table depends on the context's size, not on the weights); nullptr for every other file: nothing is allocated or launched
    float *rope_cos = nullptr, *rope_sin = nullptr;
    bool weights_shared = false;         // this context found the set already uploaded (vitx_ctx_shares_weights)
    // quantised files: vitx_ctx_options::quant_on_host restores the r01 behaviour (expand once on the host at upload, 16 bits per weight in HBM)
    bool quant_on_device = true;
    // q4_0 GEMMs with at most this many rows expand the blocks inside the GEMM's LDS-fill path (vitx_ctx_options::q4_fused_rows).  0 = never:
    // measured on ViT-B (profiles/r02c_quant.txt) the 128x128-tile fused kernel loses to "expand the layer just in time, then the skinny ring
    // kernels" at every batch size (batch 1: 1.75 vs 1.06 ms, batch 8: 2.15 vs 1.33 ms), so it is an option, not the default.
    int q4_fused_rows = 0;
    // LayerNorm fused into the residual GEMMs (GemmLn, kernels.h): norm2 rides in proj, the next layer's norm1 in fc2, wherever those GEMMs
    // run on the wide persistent kernel.  vitx_ctx_options::no_ln_fusion turns it off (every LayerNorm its own launch; same bits).
    // F16 = the parity mode: q, k, v stay f32-grade into the attention products, as the reference's do (vit.cpp:826-858).  The QKV GEMM then
    // emits two fp16 planes (EPI_BIAS_HILO) and the precise streaming kernel multiplies hi.hi + (hi.lo + lo.hi) / 2048 (attention_stream.hip).
    // Head dim 64 only (the generic head-dim kernel keeps fp16 q, k, v).
    bool prec_attn = false;
    // Last layer of a classifier: vit.cpp:910-911 reads row 0 of its output and nothing else, and rows meet each other only inside the attention
    // (through k and v).  So after the last qkv projection only the class token's row is carried on: its attention (attention_cls_kernel), then the
    // output projection, norm2 and the MLP on ONE row per image (Slice::Xc).  Same results; 0.76 of one layer's work is never asked for
    // (ViT-B: 6.3 % of the forward's flops).  vitx_ctx_options::last_layer_all_rows computes every row as the reference graph does (bench.py's headline does).
    // Not taken by ViTSTR contexts (25 rows per image feed the head) or while a residual-stream trace is on (the trace shows every row).
    bool cls_tail = true;
    bool ln_fuse = true;
    unsigned ln_epoch = 0;               // tag of the next fused launch (unique per launch; 0 is never used)
    unsigned ln_timeout = 20000;         // 200 us of the 100 MHz wall clock before a workgroup leaves its tile to the fix-up
    int ln_test = 0;                     // vitx_ctx_options::ln_test (parity tests: forced time-outs, GemmLn::test)
    int call_limit = 0;                  // images ONE pass of the kernels takes (32-bit byte offsets into the largest per-slice buffer); larger batches run as several passes
    int pass_cap() const { return std::min(max_batch, call_limit); }    // images a slice, the map buffers and the feature buffer hold
    // Fall-back budget (r03 advisor): a fused tile whose peers do not answer stalls up to ln_timeout per polled peer before it leaves its row block to
    // the consumer -- correct, but a throughput cliff when the peers' CUs are held by someone else (a second context, another process).  Every
    // forward copies the slices' fall-back counters to pinned host memory (asynchronously: the values read here are one forward old); more than
    // kLnBudget tiles per forward on average over a window of kLnWindow forwards switches the fusion off for this context (same bits either way).
    unsigned *ln_fb_host = nullptr;      // [nslices] pinned
    unsigned long long ln_fb_base = 0;   // counter total at the start of the current window
    int ln_fb_forwards = 0;
    bool ln_fuse_disabled = false;       // the budget tripped (vitx_ctx_ln_fusion_active)
    // ... and is re-armed after a cool-down (r04 advisor: one burst of contention -- another context warming up -- must not cost the fused path
    // for the rest of the context's life): the fusion is tried again after ln_cool_len forwards; every further trip doubles the cool-down (cap 2^16)
    int ln_cool_left = 0, ln_cool_len = 256;
    // activations: the batch is cut into `nslices` contiguous sub-batches, each with its own scratch and HIP stream,
    // so that the tail round / launch gaps / epilogues of one sub-batch's kernels are filled by the other's
    // (measured +10 % images/s at batch 256, tools/two_stream_probe.py).  Sub-batches are independent images.
    struct Slice {
        int cap = 0;                 // images this slice can hold
        float *X = nullptr;          // [Mpad][D] f32 residual stream
        void *U = nullptr;           // [Mpad][D] norm1 output / attention output
        void *U2 = nullptr;          // [Mpad][D] norm2 output (its own buffer: proj reads U while its epilogue writes the normalised rows)
        unsigned long long *ln_sync = nullptr;   // [Mpad / 256][D / 256][256][2] statistics granules of the fused LayerNorm
        unsigned *ln_todo = nullptr;             // [ln_blocks] row blocks left to the fix-up launch; [ln_blocks] = the fallback counter
        int ln_blocks = 0;                       // Mpad / 256 of the slice's capacity
        void *QKV = nullptr;         // [Mpad][3D]; the parity mode's lo plane follows at qkv_lo_off elements
        long qkv_lo_off = 0;
        void *Hbuf = nullptr;        // [Mpad][F1]: the fc1 output (4 D columns, or gate | up of a `glu` context)
        void *Hg = nullptr;          // `glu` contexts only: [Mpad][F] = silu(gate) . up, the A operand of fc2 (nullptr otherwise: nothing is allocated)
        float *Xc = nullptr;         // [Bpad][D] f32 class-token rows of the residual stream through the last layer's tail (cls_tail)
        void *Z = nullptr;           // [Bpad][D] final-LN output of the cls rows; pooled head: [Bpad][2 D] = RNE(cls) ‖ RNE(mean of the patch rows); MAP head: RNE(e)
        void *Mp = nullptr;          // VITX_POOL_MAP: [Bpad][H][D] RNE(M), the A operand of the value projection (Xc holds a, then e, in f32)
        // VITX_MXFP8: norm1 and norm2 outputs [Mpad][k_pad(D)] + scales; the fc1 output [Mpad][4D] + scales lives in Hbuf
        uint8_t *Umx = nullptr, *Umx_s = nullptr, *U2mx = nullptr, *U2mx_s = nullptr, *Hmx = nullptr, *Hmx_s = nullptr;
        void *Wq[W_PER_LAYER] = {nullptr, nullptr, nullptr, nullptr};   // just-in-time expansion of the current layer's quantised matrices
        void *Wq_head = nullptr;
        float *logits = nullptr;     // [Bpad][C_pad]
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
    };
    int nslices = 1;
    std::vector<Slice> slices;
    hipEvent_t fork = nullptr;
    std::vector<hipStream_t> probed_streams;   // caller streams the internal streams were already checked against (ensure_concurrent): never re-probed
    int stream_retries = 0;               // internal streams re-created because they did not run beside the caller's stream
    hipEvent_t probe_a = nullptr, probe_b = nullptr;
    float *img = nullptr;        // [max_batch][Sh][Sw][Cin] staging for the host entry point
    float *probs = nullptr;      // [max_batch][C]
    float *logits_all = nullptr; // [max_batch][C] staging for the host entry point
    // residual-stream trace (vitx_trace_enable)
    std::vector<int> trace_ids;
    float *trace_buf = nullptr;  // [L + 1][n_ids][N][D]
    // The opt-in outputs (heads.h), each built by its vitx_*_enable / vitx_*_set (outputs.cpp).  nullptr: off -- nothing is allocated or launched;
    // dropping the object frees its buffers.  They are released after ~vitx_ctx's body, with the context's device still current.
    std::unique_ptr<AttnMaps> attn;
    std::unique_ptr<Features> feat;
    std::unique_ptr<ZeroShot> zs;
    std::unique_ptr<Gallery> nn;
    std::unique_ptr<DenseHead> dense;
    std::unique_ptr<DepthHead> depth;
    // f(Output &) for every output that is set, in the order above
    template <typename F> void each_output(F &&f) const {
        Output *const all[] = {attn.get(), feat.get(), zs.get(), nn.get(), dense.get(), depth.get()};
        for (Output *o : all) if (o) f(*o);
    }
    bool any_output() const { bool any = false; each_output([&](Output &) { any = true; }); return any; }
    bool outputs_need_last_rows() const { bool need = false; each_output([&](Output &o) { need |= o.last_all_rows; }); return need; }
    // The widths a bank and a gallery must have are the context's own: they are asked for before either exists (vitx_nn_width)
    int zs_width() const { return map ? D : C; }      // E: the pooled embedding e, or the head GEMM's logits row (CLIP: image_embeds)
    int nn_width(int source) const {       // E of a source: the logits row, or the head GEMM's operand row Z
        if (source == VITX_NN_LOGITS) return C;
        return source == VITX_NN_EMBED ? (pool ? 2 * D : D) : 0;
    }
    // hipGraph cache of the single-stream (small-batch) forward, opt-in (vitx_ctx_options::graph).  Key = (images, batch, outputs): the graph
    // bakes the pointers in.  An entry is captured the second time in a row its key is seen (one-off calls are never captured).
    // Measured (profiles/r02f/hipgraph_small_batch.txt): replaying the ~100 dependent launches as a graph takes the enqueue work off
    // the host thread but does not shorten the forward -- ViT-B batch 1: 0.874 vs 0.867 ms, batch 8: 1.141 vs 1.136 ms.  The chain is
    // bound by the GPU-side cost of ~100 dependent 5-12 us kernels, not by the host's launch rate, so it is not the default.
    struct GraphEntry { const void *imgs; void *probs, *logits; int n; hipGraphExec_t exec; };
    std::vector<GraphEntry> graphs;
    GraphEntry graph_last{nullptr, nullptr, nullptr, 0, nullptr};
    bool graphs_on = false;
    long long graph_launches = 0;        // forwards enqueued as a cached graph (vitx_ctx_graph_launches)
    // profiling
    bool prof_on = false;
    hipEvent_t prof_base = nullptr;
    struct Rec { int cls; hipEvent_t a, b; double flops, bytes; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;

    ~vitx_ctx() {
        (void)hipSetDevice(device);
        for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
        for (auto &ge : graphs) (void)hipGraphExecDestroy(ge.exec);
        for (auto &sl : slices) { if (sl.stream) (void)hipStreamDestroy(sl.stream); if (sl.done) (void)hipEventDestroy(sl.done); }
        if (fork) (void)hipEventDestroy(fork);
        if (probe_a) (void)hipEventDestroy(probe_a);
        if (probe_b) (void)hipEventDestroy(probe_b);
        if (prof_base) (void)hipEventDestroy(prof_base);
        if (ln_fb_host) (void)hipHostFree(ln_fb_host);
        if (trace_buf) (void)hipFree(trace_buf);
        for (void *p : allocs) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
    int dmalloc(void **p, size_t bytes, bool zero) {
        HIP_TRY(hipMalloc(p, bytes ? bytes : 16));
        allocs.push_back(*p);
        if (zero) HIP_TRY(hipMemset(*p, 0, bytes ? bytes : 16));
        return VITX_OK;
    }
    hipEvent_t next_event() {
        if (ev_used == ev_pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); ev_pool.push_back(e); }
        return ev_pool[ev_used++];
    }
};

// The profile record around one launch on stream s.  A null context (a vitx_op_* call through heads.cpp) records nothing.
struct ProfScope {
    vitx_ctx *c; hipStream_t s; size_t idx = 0; bool on;
    ProfScope(vitx_ctx *c_, hipStream_t s_, int cls, double flops, double bytes) : c(c_), s(s_), on(c_ && c_->prof_on) {
        if (!on) return;
        vitx_ctx::Rec r{cls, c->next_event(), c->next_event(), flops, bytes};
        idx = c->recs.size(); c->recs.push_back(r);
        (void)hipEventRecord(r.a, s);
    }
    ~ProfScope() { if (on) (void)hipEventRecord(c->recs[idx].b, s); }
};
