// packed_context.h -- the packed context (struct vitx_pack); include/vitx.h "packed batches": n images, each with its own h_i x w_i, their
// tokens end to end in one [sum N_i][D] residual stream, one forward.  Modelled on the text context (text_context.h): its own scratch, one
// stream, no sub-batches, no graph cache, no LayerNorm fusion.  Three units stand on it, split like the image context's: packed_context.cpp
// (creation, counters, the table cache), packed_forward.cpp (the checks of a call, the forward), packed_outputs.cpp (features, the dense and the depth head).
// Internal: callers see the opaque vitx_pack of include/vitx.h.
#pragma once
#include <memory>

#include "heads.h"

using namespace vitx;

// The segment tables of a call, in ints into vitx_pack::tab / host (cap = max_images): row0 [cap + 1] | qb0 [cap + 1] | toff [cap] and, while a
// dense head is set, behind them tile0 [cap + 1] | seg [cap][kDenseSegInts] and, while a depth head is set, behind those ftile0 [cap + 1] |
// otile0 [cap + 1] | dseg [cap][kDepthSegInts] (kernels.h).  One buffer, one upload; a new table goes in here.
struct PackLayout {
    size_t cap;
    bool dense, depth;                   // the heads whose tables the buffer holds
    size_t row0() const { return 0; }
    size_t qb0() const { return row0() + cap + 1; }
    size_t toff() const { return qb0() + cap + 1; }
    size_t tile0() const { return toff() + cap; }
    size_t seg() const { return tile0() + cap + 1; }
    size_t ftile0() const { return dense ? seg() + cap * kDenseSegInts : tile0(); }
    size_t otile0() const { return ftile0() + cap + 1; }
    size_t dseg() const { return otile0() + cap + 1; }
    size_t ints() const { return depth ? dseg() + cap * kDepthSegInts : ftile0(); }
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
    float *img = nullptr;                // the host entry point's pixels on the device (allocated by its first call)
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
    int launches = 0, pe_launches = 0;   // kernel launches of the last forward, and how many of them were patch embeddings
    size_t scratch_bytes = 0;            // device bytes of activation scratch and tables held now
    PackLayout layout() const { return PackLayout{(size_t)max_images, (bool)dense, (bool)depth}; }
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
