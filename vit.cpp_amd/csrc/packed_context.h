// packed_context.h -- the packed context (struct vitx_pack); include/vitx.h "packed batches": n images, each with its own h_i x w_i, their
// tokens end to end in one [sum N_i][D] residual stream, one forward.  Modelled on the text context (text_context.h): its own scratch, one
// stream, no sub-batches, no graph cache, no LayerNorm fusion.  Three units stand on it, split like the image context's: packed_context.cpp
// (creation, counters, the table cache), packed_forward.cpp (the checks of a call, the forward), packed_outputs.cpp (features, the dense and the depth head, attention maps)
// and packed_input.cpp (u8 sources).
// Internal: callers see the opaque vitx_pack of include/vitx.h.
#pragma once
#include <memory>

#include "heads.h"

using namespace vitx;

// The segment tables of a call, in ints into vitx_pack::tab / host (cap = max_images): row0 [cap + 1] | qb0 [cap + 1] | toff [cap] and, while a
// dense head is set, behind them tile0 [cap + 1] | seg [cap][kDenseSegInts] and, while a depth head is set, behind those ftile0 [cap + 1] |
// otile0 [cap + 1] | dseg [cap][kDepthSegInts] and, while u8 sources are on (vitx_pack_u8_set), behind those ptile0 [cap + 1] | pseg [cap][kPpSegInts]
// (kernels.h) and, while attention rollout is on (vitx_pack_attn_enable), behind those rblk0 [cap + 1] | sq0 [cap + 1] (kernels.h attn_pack_tables).
// One buffer, one upload; a new table goes in here.
struct PackLayout {
    size_t cap;
    bool dense, depth;                   // the heads whose tables the buffer holds
    bool u8 = false;                     // the u8 preprocessing's tables too
    bool rollout = false;                // the attention rollout's tables too
    size_t row0() const { return 0; }
    size_t qb0() const { return row0() + cap + 1; }
    size_t toff() const { return qb0() + cap + 1; }
    size_t tile0() const { return toff() + cap; }
    size_t seg() const { return tile0() + cap + 1; }
    size_t ftile0() const { return dense ? seg() + cap * kDenseSegInts : tile0(); }
    size_t otile0() const { return ftile0() + cap + 1; }
    size_t dseg() const { return otile0() + cap + 1; }
    size_t ptile0() const { return depth ? dseg() + cap * kDepthSegInts : ftile0(); }
    size_t pseg() const { return ptile0() + cap + 1; }
    size_t rblk0() const { return u8 ? pseg() + cap * kPpSegInts : ptile0(); }
    size_t sq0() const { return rblk0() + cap + 1; }
    size_t ints() const { return rollout ? sq0() + cap + 1 : rblk0(); }
};

// What the host-only checks of a forward call (packed_forward.cpp check_call) give the forward: made once per call, before its first device call
struct PackCall {
    std::vector<int32_t> row0;           // [n + 1]: image i's rows of the pack are row0[i] .. row0[i + 1] - 1
    std::vector<uint64_t> want;          // the distinct grids, in order of first appearance, as (gh << 32 | gw)
    std::vector<int32_t> grids, outs;    // with a dense head set: [n][2] each, the patch grids and the output shapes
    std::vector<int64_t> pix0;           // [n + 1], the running pixel count of the outputs
    std::vector<int32_t> tile0;          // [n + 1], the running tile count of the label launch
    int cells = 0;                       // the widest tile window (kernels.h dense_pack_tables)
    // with a depth head set (kernels.h depth_pack_tables): the grids again, the depth maps' shapes, the running pixel counts of the maps and of the
    // fine planes, the running tile counts of the fine and the resize launch, the widest fine-tile window
    std::vector<int32_t> dgrids, douts;
    std::vector<int64_t> dpix0, dfine0;
    std::vector<int32_t> ftile0, otile0;
    int dcells = 0;
    // with u8 sources declared for the call (kernels.h pp_pack_tables): the running tile count of the preprocessing launch, its table rows, its LDS
    // and the bytes of the sources
    bool u8 = false;
    std::vector<int32_t> ptile0, pseg;
    int plds = 0;
    int64_t src_bytes = 0;
    // with attention rollout on (kernels.h attn_pack_tables): the running counts of 16-row blocks and of N_i^2, the widest image of the call
    std::vector<int32_t> rblk0, sq0;
    int n_max = 0;
};

// Attention maps (vitx_pack_attn_enable): the image context's AttnMaps per image of a pack.  Image i's floats of `out` start at row0[i] * fpt: the
// selected layers in ascending order, each [H][N_i], then the rollout row [N_i]
struct PackAttn {
    uint64_t mask = 0;
    int flags = 0;
    int fpt = 0;                         // floats per token: popcount(mask) * H (+ 1 with VITX_ATTN_ROLLOUT)
    long max_sq = 0;                     // rollout: the floats of one matrix arena, the bound on a call's sum of N_i^2
    DevMem out;                          // [max_tokens][fpt] f32
    DevMem roll[2];                      // rollout: [max_sq] f32 x 2, A^_l written into one, the product R_l in place of it (ping-pong)
    DevMem cls_last;                     // rollout without the last layer in the mask: its class-token maps, [max_tokens][H] f32
    size_t bytes = 0;                    // what the enable added to vitx_pack_scratch_bytes besides the tables
    int n = 0;                           // images of the last forward with maps on (0: none)
    std::vector<int32_t> rblk0, sq0;     // of that forward (rollout)
    int n_max = 0;
    bool rollout() const { return (flags & VITX_ATTN_ROLLOUT) != 0; }
    bool selects(int il) const { return (mask >> il) & 1; }
};

// u8 sources (vitx_pack_u8_set): the description, the device staging of the host entry point and the declaration of the next call
struct PackU8 {
    vitx_preproc pp;
    size_t max_src_bytes = 0;
    DevMem src;                          // max_src_bytes rounded up to 4: the sources of vitx_pack_forward_u8 on the device
    bool own_img = false;                // vitx_pack::img was allocated by the set (else by an earlier vitx_pack_forward: it stays when u8 goes off)
    size_t bytes = 0;                    // what the set added to vitx_pack_scratch_bytes besides the tables
    bool declared = false;               // vitx_pack_u8_sources: the next forward call's d_imgs are u8 sources of next_src [n][2] = (ny, nx)
    std::vector<int32_t> next_src;
};

// One grid of the table cache: the position table resampled to gh x gw and the grid's place in the rotary arenas
struct PackGrid {
    int gh = 0, gw = 0;
    float *pos = nullptr;                // [1 + gh gw][D] f32; the weight set's own table (own == false) at the file's grid
    bool own = false;
    size_t pos_bytes = 0;                // bytes allocated behind an own table (a reused one may be larger than the grid needs)
    long rope_off = 0;                   // floats into rope_cos / rope_sin: the grid's [gh gw][hd / 2] table (files with `rope`)
    uint64_t used = 0;                   // the call (vitx_pack::tick) that named the grid last
};

struct vitx_pack {
    const vitx_model *model = nullptr;
    int device = 0, dtype = VITX_F16;
    int D = 0, L = 0, H = 0, C = 0, C_pad = 0, P = 0, Tp = 1, nreg = 0, g_in = 0, Kpe_pad = 0;
    int F = 0, F1 = 0;                   // MLP widths: fc2's K and fc1's N (4 D both, or F and 2 F of a `glu` file)
    bool glu = false, rope = false;
    int fc1_epi = EPI_BIAS_GELU;
    float eps = 1e-6f;
    int tm = 256, tn = 128;
    int max_tokens = 0, max_images = 0, max_grids = 32, pos_interp = 0;
    const Tuning *tune = nullptr;        // per-device launch parameters, immutable: the GEMMs go through launch_gemm with the device's own tuning
    std::shared_ptr<WeightSet> wset;
    bool weights_shared = false;
    hipStream_t stream = nullptr;        // of vitx_pack_forward (the host entry point)
    std::vector<void *> allocs;
    float *X = nullptr;                  // [Mpad][D] f32 residual stream, Mpad = max_tokens rounded up to the GEMMs' row tile
    void *U = nullptr, *QKV = nullptr, *Hbuf = nullptr, *Hg = nullptr;      // [Mpad][D], [Mpad][3 D], [Mpad][F1], [Mpad][F] (glu) operand type
    void *Z = nullptr;                   // [Bpad][D] operand type: the class rows through the final norm, Bpad = max_images rounded up
    float *logits = nullptr, *probs = nullptr;      // [Bpad][C_pad], [max_images][C] f32
    float *logits_out = nullptr;         // [max_images][C] f32: the dense logits of the host entry point
    float *img = nullptr;                // the host entry point's pixels on the device (allocated by its first call, or by vitx_pack_u8_set: the u8
                                         // preprocessing writes them there)
    int *tab = nullptr;                  // the segment tables of a call (PackLayout)
    std::vector<int> host;               // the same on the host: the staging buffer of the upload
    std::vector<int32_t> row0;           // PackCall::row0 of the last call that passed its checks (vitx_pack_feat_read, vitx_pack_dense_read)
    hipEvent_t uploaded = nullptr;       // recorded behind the upload of a call: the next call waits for it before it overwrites `host`
    bool uploaded_pending = false;
    hipEvent_t done = nullptr;           // recorded behind the last forward: a table is evicted or overwritten only after it
    bool done_pending = false;
    std::vector<PackGrid> grids;         // the table cache, at most max_grids entries
    uint64_t tick = 0;
    float *rope_cos = nullptr, *rope_sin = nullptr;      // the rotary arenas, rope_cap floats each; rope_top: the first free float
    long rope_cap = 0, rope_top = 0;
    float *rope_host = nullptr;          // pinned mirror of both arenas, [2][rope_cap]: the staging of the asynchronous table uploads (a piece is
                                         // rewritten only when the arena restarts, after the forwards that were fed from it)
    struct Retired { float *pos; size_t bytes; };
    std::vector<Retired> retired;        // own position tables of dropped grids, kept for the next grid they hold: hipFree would wait for the whole
                                         // device, and a call that drops a table must not wait for the caller's stream (oldest first)
    int feat_flags = 0;                  // vitx_pack_feat_enable
    float *feat = nullptr;               // [max_tokens][D] f32 final-norm rows of the last forward (allocated by vitx_pack_feat_enable)
    int feat_n = 0;                      // images of the last forward with features on (0: none)
    std::unique_ptr<PackDense> dense;    // vitx_pack_dense_set (null: off); its device memory is its own
    std::unique_ptr<PackDepth> depth;    // vitx_pack_depth_set (null: off); its device memory is its own
    std::unique_ptr<PackU8> u8;          // vitx_pack_u8_set (null: off)
    std::unique_ptr<PackAttn> attn;      // vitx_pack_attn_enable (null: off); its device memory is its own
    bool rollout() const { return attn && attn->rollout(); }
    int launches = 0, pe_launches = 0;   // kernel launches of the last forward, and how many of them were patch embeddings
    size_t scratch_bytes = 0;            // device bytes of activation scratch and tables held now
    PackLayout layout() const { return PackLayout{(size_t)max_images, (bool)dense, (bool)depth, (bool)u8, rollout()}; }
    // image i of the last call that passed its checks: its patch rows, and where they start in an output that holds every image's patch rows end to end
    size_t patch_rows(int i) const { return (size_t)(row0[i + 1] - row0[i] - Tp); }
    size_t patch_at(int i) const { return (size_t)(row0[i] - i * Tp); }
    ~vitx_pack() {
        (void)hipSetDevice(device);
        for (void *p : allocs) (void)hipFree(p);
        for (PackGrid &g : grids) if (g.own) (void)hipFree(g.pos);
        for (Retired &r : retired) (void)hipFree(r.pos);
        if (rope_host) (void)hipHostFree(rope_host);
        if (img) (void)hipFree(img);
        if (feat) (void)hipFree(feat);
        if (uploaded) (void)hipEventDestroy(uploaded);
        if (done) (void)hipEventDestroy(done);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// The table cache (packed_context.cpp).  find_grid: the cached grid, or nullptr.  wait_done: before a table is freed or overwritten, the last forward
// of this context, which may still read it on another stream, is waited for.  resolve_grids: the tables of every grid a call names, on its stream.
PackGrid *find_grid(vitx_pack *p, int gh, int gw);
int wait_done(vitx_pack *p);
int resolve_grids(vitx_pack *p, const std::vector<uint64_t> &want, hipStream_t st);
// Before buffers and tables change hands (the set calls): nothing of this context is in flight.  resize_tables: the segment tables with the parts
// that will be set behind them (PackLayout), a fresh zeroed buffer in place of the old one.
int pack_quiesce(vitx_pack *p);
int resize_tables(vitx_pack *p, const char *api, bool dense, bool depth, bool u8, bool rollout);
// Attention maps (packed_forward.cpp): what vitx_pack_attn_enable and vitx_pack_attn_check refuse in their arguments, host only
int pack_attn_args(const char *api, int L, uint64_t layer_mask, int flags, long max_sq_tokens);
