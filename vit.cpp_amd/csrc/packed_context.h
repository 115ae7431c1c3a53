// packed_context.h -- the packed context (struct vitx_pack) of packed_forward.cpp; include/vitx.h "packed batches": n images, each with its own
// h_i x w_i, their tokens end to end in one [sum N_i][D] residual stream, one forward.  Modelled on the text context (text_context.h): its own
// scratch, one stream, no sub-batches, no graph cache, no LayerNorm fusion.  Internal: callers see the opaque vitx_pack of include/vitx.h.
#pragma once
#include <memory>

#include "heads.h"

using namespace vitx;

// One grid of the table cache: the position table resampled to gh x gw and the grid's place in the rotary arenas
struct PackGrid {
    int gh = 0, gw = 0;
    float *pos = nullptr;                // [1 + gh gw][D] f32; the weight set's own table (own == false) at the file's grid
    bool own = false;
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
    // the segment tables of a call: row0 [cap + 1] | qb0 [cap + 1] | toff [cap] (cap = max_images) and, while a dense head is set, behind them
    // tile0 [cap + 1] | seg [cap][kDenseSegInts] (kernels.h): one buffer, one upload
    int *tab = nullptr;
    std::vector<int> host;               // the same on the host: the staging buffer of the upload
    std::vector<int32_t> chk, row0;      // [cap + 1] each: the rows of the call being checked; of the last call that passed its checks (vitx_pack_feat_read)
    hipEvent_t uploaded = nullptr;       // recorded behind the upload of a call: the next call waits for it before it overwrites `host`
    bool uploaded_pending = false;
    hipEvent_t done = nullptr;           // recorded behind the last forward: a table is evicted or overwritten only after it
    bool done_pending = false;
    std::vector<PackGrid> grids;         // the table cache, at most max_grids entries
    uint64_t tick = 0;
    float *rope_cos = nullptr, *rope_sin = nullptr;      // the rotary arenas, rope_cap floats each; rope_top: the first free float
    long rope_cap = 0, rope_top = 0;
    int feat_flags = 0;                  // vitx_pack_feat_enable
    float *feat = nullptr;               // [max_tokens][D] f32 final-norm rows of the last forward (allocated by vitx_pack_feat_enable)
    int feat_n = 0;                      // images of the last forward with features on (0: none)
    std::unique_ptr<PackDense> dense;    // vitx_pack_dense_set (null: off); its device memory is its own
    int launches = 0, pe_launches = 0;   // kernel launches of the last forward, and how many of them were patch embeddings
    size_t scratch_bytes = 0;            // device bytes of activation scratch and tables held now
    ~vitx_pack() {
        (void)hipSetDevice(device);
        for (void *p : allocs) (void)hipFree(p);
        for (PackGrid &g : grids) if (g.own) (void)hipFree(g.pos);
        if (img) (void)hipFree(img);
        if (feat) (void)hipFree(feat);
        if (uploaded) (void)hipEventDestroy(uploaded);
        if (done) (void)hipEventDestroy(done);
        if (stream) (void)hipStreamDestroy(stream);
    }
};
