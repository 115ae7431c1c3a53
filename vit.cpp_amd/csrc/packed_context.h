// packed_context.h -- the packed context (struct vitx_pack); include/vitx.h "packed batches": n images, each with its own h_i x w_i, their
// tokens end to end in one [sum N_i][D] residual stream, one forward.  Modelled on the text context (text_context.h): its own scratch, one
// stream, no sub-batches, no graph cache, no LayerNorm fusion.  Four units stand on it: packed_context.cpp (creation, counters, the table
// cache, what the set calls share), packed_forward.cpp (the checks of a call, the forward, the entry points), packed_outputs.cpp (features,
// attention maps, the dense and the depth head) and packed_input.cpp (u8 sources).
// Four opt-in PARTS bring segment tables and state of a call with them: the dense head, the depth head, u8 sources, attention rollout.  Each is
// one bit (PackPart), one or two lines of kPackTables, one struct of what its check gives a call (PackDenseCall, PackDepthCall in heads.h,
// PackU8Call, PackRolloutCall here) and one struct of what its set call holds (PackDense, PackDepth in heads.h, PackU8, PackAttn here).
// DESIGN.md ("Packed batches", Parts) lists the places a new part is added in.
// Internal: callers see the opaque vitx_pack of include/vitx.h.
#pragma once
#include <memory>

#include "heads.h"

using namespace vitx;

enum PackPart : unsigned { kDense = 1u << 0, kDepth = 1u << 1, kU8 = 1u << 2, kRollout = 1u << 3 };

// The segment tables of a call, in their order in vitx_pack::tab / host: `per_image` ints per image the context holds (cap = max_images) and `plus`
// more.  A table of part 0 is always there, another while its part is on.  One buffer, one upload; a new table goes at the end of this list.
struct PackTable { unsigned part; int per_image, plus; };
constexpr PackTable kPackTables[] = {
    {0, 1, 1}, {0, 1, 1}, {0, 1, 0},                                 // row0 [cap + 1] | qb0 [cap + 1] | toff [cap]
    {kDense, 1, 1}, {kDense, kDenseSegInts, 0},                      // tile0 [cap + 1] | seg [cap][kDenseSegInts]               (kernels.h dense_pack_tables)
    {kDepth, 1, 1}, {kDepth, 1, 1}, {kDepth, kDepthSegInts, 0},      // ftile0 [cap + 1] | otile0 [cap + 1] | dseg [cap][kDepthSegInts]  (depth_pack_tables)
    {kU8, 1, 1}, {kU8, kPpSegInts, 0},                               // ptile0 [cap + 1] | pseg [cap][kPpSegInts]                (pp_pack_tables)
    {kRollout, 1, 1}, {kRollout, 1, 1},                              // rblk0 [cap + 1] | sq0 [cap + 1]                          (attn_pack_tables)
};

struct PackLayout {
    size_t cap;
    unsigned parts;                      // PackPart bits: the parts whose tables the buffer holds
    enum Table { kRow0, kQb0, kToff, kTile0, kSeg, kFtile0, kOtile0, kDseg, kPtile0, kPseg, kRblk0, kSq0, kTables };
    static_assert(sizeof(kPackTables) / sizeof(kPackTables[0]) == kTables, "one name per table");
    // the ints in front of table t: the tables before it whose part is on (a table of a part that is off is placed as if that part alone were on too)
    size_t at(int t) const {
        const unsigned on = parts | (t < kTables ? kPackTables[t].part : 0);
        size_t o = 0;
        for (int k = 0; k < t; ++k) if (!kPackTables[k].part || (on & kPackTables[k].part)) o += cap * kPackTables[k].per_image + kPackTables[k].plus;
        return o;
    }
    size_t row0() const { return at(kRow0); }
    size_t qb0() const { return at(kQb0); }
    size_t toff() const { return at(kToff); }
    size_t tile0() const { return at(kTile0); }
    size_t seg() const { return at(kSeg); }
    size_t ftile0() const { return at(kFtile0); }
    size_t otile0() const { return at(kOtile0); }
    size_t dseg() const { return at(kDseg); }
    size_t ptile0() const { return at(kPtile0); }
    size_t pseg() const { return at(kPseg); }
    size_t rblk0() const { return at(kRblk0); }
    size_t sq0() const { return at(kSq0); }
    size_t ints() const { return at(kTables); }
};

// What check_u8 gives a call whose d_imgs are u8 sources (kernels.h pp_pack_tables): the running tile count of the preprocessing launch [n + 1], its
// table rows, its LDS and the bytes of the sources
struct PackU8Call {
    bool on = false;
    std::vector<int32_t> tile0, seg;
    int lds = 0;
    int64_t src_bytes = 0;
};
// What check_attn gives a call while attention rollout is on (kernels.h attn_pack_tables): the running counts of 16-row blocks and of N_i^2 [n + 1]
// each, the widest image of the call
struct PackRolloutCall {
    std::vector<int32_t> rblk0, sq0;
    int n_max = 0;
};

// What the host-only checks of a forward call (packed_forward.cpp check_call) give the forward: made once per call, before its first device call.
// pack_forward takes a part's struct over as that part's `last` with one swap.
struct PackCall {
    std::vector<int32_t> row0;           // [n + 1]: image i's rows of the pack are row0[i] .. row0[i + 1] - 1
    std::vector<uint64_t> want;          // the distinct grids, in order of first appearance, as (gh << 32 | gw)
    PackDenseCall dense;                 // with a dense head set
    PackDepthCall depth;                 // with a depth head set
    PackU8Call u8;                       // with u8 sources declared for the call
    PackRolloutCall roll;                // with attention rollout on
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
    size_t bytes = 0;                    // device bytes of everything above: what the enable adds to vitx_pack_scratch_bytes besides the tables
    int n = 0;                           // images of the last forward with maps on (0: none)
    PackRolloutCall last;                // of that forward (rollout)
    bool rollout() const { return (flags & VITX_ATTN_ROLLOUT) != 0; }
    bool selects(int il) const { return (mask >> il) & 1; }
};

// u8 sources (vitx_pack_u8_set): the description, the device staging of the host entry point and the declaration of the next call
struct PackU8 {
    vitx_preproc pp;
    size_t max_src_bytes = 0;
    DevMem src;                          // max_src_bytes rounded up to 4: the sources of vitx_pack_forward_u8 on the device
    bool own_img = false;                // vitx_pack::img was allocated by the set (else by an earlier vitx_pack_forward: it stays when u8 goes off)
    size_t bytes = 0;                    // device bytes the set allocated: what it adds to vitx_pack_scratch_bytes besides the tables
    std::vector<int32_t> next_src;       // vitx_pack_u8_sources: the next forward call's d_imgs are u8 sources of these shapes [n][2] = (ny, nx) (empty: f32 pixels)
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
    DevMem img;                          // the host entry point's f32 pixels on the device (allocated by its first call, or by vitx_pack_u8_set: the u8
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
    DevMem feat;                         // [max_tokens][D] f32 final-norm rows of the last forward (allocated by vitx_pack_feat_enable)
    int feat_n = 0;                      // images of the last forward with features on (0: none)
    std::unique_ptr<PackDense> dense;    // vitx_pack_dense_set (null: off); its device memory is its own
    std::unique_ptr<PackDepth> depth;    // vitx_pack_depth_set (null: off); its device memory is its own
    std::unique_ptr<PackU8> u8;          // vitx_pack_u8_set (null: off)
    std::unique_ptr<PackAttn> attn;      // vitx_pack_attn_enable (null: off); its device memory is its own
    bool rollout() const { return attn && attn->rollout(); }         // the rollout tables are there; class maps alone add no table
    int launches = 0, pe_launches = 0;   // kernel launches of the last forward, and how many of them were patch embeddings
    size_t scratch_bytes = 0;            // device bytes of activation scratch and tables held now
    unsigned parts() const { return (dense ? kDense : 0u) | (depth ? kDepth : 0u) | (u8 ? kU8 : 0u) | (rollout() ? kRollout : 0u); }
    PackLayout layout() const { return PackLayout{(size_t)max_images, parts()}; }
    // image i of the last call that passed its checks: its patch rows, and where they start in an output that holds every image's patch rows end to end
    size_t patch_rows(int i) const { return (size_t)(row0[i + 1] - row0[i] - Tp); }
    size_t patch_at(int i) const { return (size_t)(row0[i] - i * Tp); }
    ~vitx_pack() {
        (void)hipSetDevice(device);
        for (void *p : allocs) (void)hipFree(p);
        for (PackGrid &g : grids) if (g.own) (void)hipFree(g.pos);
        for (Retired &r : retired) (void)hipFree(r.pos);
        if (rope_host) (void)hipHostFree(rope_host);
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
// What the set calls share (packed_context.cpp).  pack_quiesce: before buffers and tables change hands, nothing of this context is in flight.
// resize_tables: the segment tables for the parts that will be set (PackLayout), a fresh zeroed buffer in place of the old one.  pack_commit:
// the end of a set call whose new state is built -- the tables for `parts`, then the old state's bytes leave vitx_pack_scratch_bytes and the new
// state's enter; the caller moves the new state in behind it.  alloc_counted: one device allocation of a part, added to the count it is given, so
// that what a part adds to vitx_pack_scratch_bytes is what it allocated; false when the device has no room (DevMem::alloc).
int pack_quiesce(vitx_pack *p);
int resize_tables(vitx_pack *p, const char *api, unsigned parts);
int pack_commit(vitx_pack *p, const char *api, unsigned parts, size_t old_bytes, size_t new_bytes);
inline bool alloc_counted(DevMem &m, size_t bytes, size_t *count) {
    if (!m.alloc(bytes)) return false;
    *count += bytes;
    return true;
}
// vitx_pack_dense_out, vitx_pack_depth_out, vitx_pack_u8_sources: the shapes [n][2] a part declares for the next forward call (NULL or n = 0: none)
int pack_next_shapes(const vitx_pack *p, const char *api, const int32_t *shapes, int n, std::vector<int32_t> *next);
// Attention maps (packed_forward.cpp): what vitx_pack_attn_enable and vitx_pack_attn_check refuse in their arguments, host only
int pack_attn_args(const char *api, int L, uint64_t layer_mask, int flags, long max_sq_tokens);
