// text_context.h -- the text context (struct vitx_text) of text_forward.cpp; include/vitx.h "the text tower".  One stream, no sub-batches, no graph
// cache, no LayerNorm fusion.  Internal: callers see the opaque vitx_text of include/vitx.h.
#pragma once
#include "weights.h"

using namespace vitx;

struct vitx_text {
    const vitx_model *model = nullptr;
    int device = 0, dtype = VITX_F16;
    int D = 0, L = 0, H = 0;
    int tm = 128, tn = 128;
    const Tuning *tune = nullptr;        // per-device launch parameters, immutable
    std::shared_ptr<WeightSet> wset;     // never null once the context exists (weights.h: shared with every text context of the model, device and dtype)
    bool weights_shared = false;         // this context found the set already uploaded (vitx_text_shares_weights)
    int V = 0, T = 0, E = 0, E_pad = 0, causal = 0, eos = -1, max_prompts = 0;
    int fc1_epi = EPI_BIAS_GELU;
    float eps = 1e-6f;
    Tuning tune_qkv, tune_proj, tune_fc1, tune_fc2, tune_head;      // the device's tuning with ONE ring family pinned per GEMM, chosen at creation from max_prompts * T rows
    hipStream_t stream = nullptr;        // of vitx_text_embed (the host entry point)
    std::vector<void *> allocs;
    int *pooled = nullptr, *ids = nullptr;      // [max_prompts] pooled positions, then [max_prompts][T] ids: one buffer, one upload of its front
    std::vector<int> host;               // the same on the host: the staging buffer of the upload
    std::vector<int32_t> pooled_host;    // the positions of the call being checked (stage_ids), before they may enter `host`
    hipEvent_t uploaded = nullptr;       // recorded behind the upload of a call: the next call waits for it before it overwrites `host`
    bool uploaded_pending = false;
    float *X = nullptr;                  // [Mpad][D] f32 residual stream
    void *U = nullptr, *QKV = nullptr, *Hbuf = nullptr, *Z = nullptr;      // [Mpad][D], [Mpad][3 D], [Mpad][4 D], [Bpad][D] operand type
    float *out = nullptr;                // [Bpad][E] f32 embeddings of the host entry point
    float *raw = nullptr;                // [Bpad][E] f32: the head's output in front of VITX_TEXT_L2
    ~vitx_text() {
        (void)hipSetDevice(device);
        for (void *p : allocs) (void)hipFree(p);
        if (uploaded) (void)hipEventDestroy(uploaded);
        if (stream) (void)hipStreamDestroy(stream);
    }
};
