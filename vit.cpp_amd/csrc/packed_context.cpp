// packed_context.cpp -- the life of a packed context (packed_context.h; include/vitx.h "packed batches"): creation with every refusal before the
// first device call, the counters, the table cache -- per grid the resampled position table and, for `rope` files, a piece of the rotary arenas --
// and what the set calls of the opt-in parts share: the wait for the context, the segment tables resized for a set of parts, the commit, the
// declaration of shapes for the next call.
// One stream, no sub-batch split, no hipGraph cache; block matrices are expanded at upload, as in the text context (text_forward.cpp).
#include <algorithm>
#include <new>

#include "packed_context.h"

PackGrid *find_grid(vitx_pack *p, int gh, int gw) {
    for (PackGrid &g : p->grids) if (g.gh == gh && g.gw == gw) return &g;
    return nullptr;
}

int wait_done(vitx_pack *p) {
    if (p->done_pending) { HIP_TRY(hipEventSynchronize(p->done)); p->done_pending = false; }
    return VITX_OK;
}

// The caller has waited for the last forward (wait_done): nothing reads the table any more.  It is not freed -- hipFree waits for everything
// enqueued on the device, the caller's own stream included -- but retired for the next grid it can hold; only beyond 2 max_grids retired
// tables is the oldest really freed.  scratch_bytes counts the tables of cached grids, not the retired ones.
static void drop_grid(vitx_pack *p, size_t k) {
    PackGrid &g = p->grids[k];
    if (g.own) {
        p->retired.push_back(vitx_pack::Retired{g.pos, g.pos_bytes});
        p->scratch_bytes -= ((size_t)g.gh * g.gw + 1) * p->D * 4;
        if (p->retired.size() > 2 * (size_t)p->max_grids) { (void)hipFree(p->retired.front().pos); p->retired.erase(p->retired.begin()); }
    }
    p->grids.erase(p->grids.begin() + k);
}
// An own position table of at least `bytes`: the smallest retired one that holds it, else a new allocation
static hipError_t take_table(vitx_pack *p, size_t bytes, float **pos, size_t *cap) {
    size_t best = p->retired.size();
    for (size_t k = 0; k < p->retired.size(); ++k)
        if (p->retired[k].bytes >= bytes && (best == p->retired.size() || p->retired[k].bytes < p->retired[best].bytes)) best = k;
    if (best < p->retired.size()) {
        *pos = p->retired[best].pos; *cap = p->retired[best].bytes;
        p->retired.erase(p->retired.begin() + best);
        return hipSuccess;
    }
    *cap = bytes;
    return hipMalloc((void **)pos, bytes);
}
static void give_back(vitx_pack *p, PackGrid &g) {
    if (!g.own) return;
    p->retired.push_back(vitx_pack::Retired{g.pos, g.pos_bytes});
    p->scratch_bytes -= ((size_t)g.gh * g.gw + 1) * p->D * 4;
}

// The tables of every grid the call names, built the first time a call names them: the position table by launch_pos_resample on the call's
// stream, the rotary table on the host (vitx_model_rope_table) and uploaded.  The cache holds max_grids grids; the least recently used grid
// the call does not name goes first.  A rotary table takes the next free piece of the arenas; when they are full the cache starts over.
int resolve_grids(vitx_pack *p, const std::vector<uint64_t> &want, hipStream_t st) {
    const int half = p->D / p->H / 2;
    ++p->tick;
    size_t missing = 0; long rope_need = 0;
    for (uint64_t k : want) {
        const int gh = (int)(k >> 32), gw = (int)(uint32_t)k;
        if (PackGrid *g = find_grid(p, gh, gw)) g->used = p->tick;
        else { ++missing; rope_need += (long)gh * gw * half; }
    }
    if (!missing) return VITX_OK;
    int rc;
    if (p->rope && p->rope_top + rope_need > p->rope_cap) {          // the arenas are full: every grid of the call is built again from their start
        if ((rc = wait_done(p))) return rc;
        while (!p->grids.empty()) drop_grid(p, p->grids.size() - 1);
        p->rope_top = 0;
    }
    while (p->grids.size() + missing > (size_t)p->max_grids) {       // (a call names at most max_grids grids: there is always one it does not name)
        size_t lru = p->grids.size();
        for (size_t k = 0; k < p->grids.size(); ++k)
            if (p->grids[k].used != p->tick && (lru == p->grids.size() || p->grids[k].used < p->grids[lru].used)) lru = k;
        if (lru == p->grids.size()) break;
        if ((rc = wait_done(p))) return rc;
        drop_grid(p, lru);
    }
    for (uint64_t k : want) {
        const int gh = (int)(k >> 32), gw = (int)(uint32_t)k;
        if (find_grid(p, gh, gw)) continue;
        PackGrid g;
        g.gh = gh; g.gw = gw; g.used = p->tick;
        if (gh == p->g_in && gw == p->g_in) g.pos = p->wset->pos;        // the file's own grid: the file's table, as in a context of the file's size
        else {
            const size_t bytes = ((size_t)gh * gw + 1) * p->D * 4;
            HIP_TRY(take_table(p, bytes, &g.pos, &g.pos_bytes));
            g.own = true; p->scratch_bytes += bytes;
            const hipError_t e = launch_pos_resample(p->wset->pos, p->g_in, p->g_in, p->D, gh, gw, p->pos_interp, g.pos, st);
            if (e != hipSuccess) { give_back(p, g); set_error("vitx_pack_forward: launch_pos_resample: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
            ++p->launches;
        }
        if (p->rope) {
            const size_t tab = (size_t)gh * gw * half;
            // a fresh piece of the arenas: nothing reads it yet.  The table is computed into the same piece of the pinned mirror and uploaded on the
            // call's stream, in front of the launches that read it; the host does not wait
            float *hc = p->rope_host + p->rope_top, *hs = p->rope_host + p->rope_cap + p->rope_top;
            rc = vitx_model_rope_table(p->model, gh, gw, hc, hs);
            hipError_t e = rc ? hipSuccess : hipMemcpyAsync(p->rope_cos + p->rope_top, hc, tab * 4, hipMemcpyHostToDevice, st);
            if (!rc && e == hipSuccess) e = hipMemcpyAsync(p->rope_sin + p->rope_top, hs, tab * 4, hipMemcpyHostToDevice, st);
            if (rc || e != hipSuccess) {
                give_back(p, g);
                if (!rc) { set_error("vitx_pack_forward: rotary table upload: %s", hipGetErrorString(e)); rc = VITX_ERR_HIP; }
                return rc;
            }
            g.rope_off = p->rope_top; p->rope_top += (long)tab;
        }
        p->grids.push_back(g);
    }
    return VITX_OK;
}

// nothing of this context is in flight while buffers and tables change hands
int pack_quiesce(vitx_pack *p) {
    if (p->uploaded_pending) { HIP_TRY(hipEventSynchronize(p->uploaded)); p->uploaded_pending = false; }
    return wait_done(p);
}

// the segment tables for the parts that will be set (PackLayout): a fresh zeroed buffer in place of the old one
int resize_tables(vitx_pack *p, const char *api, unsigned parts) {
    const size_t ints = PackLayout{(size_t)p->max_images, parts}.ints();
    if (p->host.size() == ints) return VITX_OK;
    int *t = nullptr;
    HIP_TRY(hipMalloc((void **)&t, ints * 4));
    if (const hipError_t e = hipMemset(t, 0, ints * 4); e != hipSuccess) { (void)hipFree(t); set_error("%s: %s", api, hipGetErrorString(e)); return VITX_ERR_HIP; }
    std::replace(p->allocs.begin(), p->allocs.end(), (void *)p->tab, (void *)t);
    (void)hipFree(p->tab);
    p->scratch_bytes += ints * 4; p->scratch_bytes -= p->host.size() * 4;
    p->tab = t; p->host.assign(ints, 0);
    return VITX_OK;
}

// the end of a set call: a failed resize leaves the count, and the state the caller is about to replace, as they were
int pack_commit(vitx_pack *p, const char *api, unsigned parts, size_t old_bytes, size_t new_bytes) {
    if (const int rc = resize_tables(p, api, parts)) return rc;
    p->scratch_bytes -= old_bytes; p->scratch_bytes += new_bytes;
    return VITX_OK;
}

int pack_next_shapes(const vitx_pack *p, const char *api, const int32_t *shapes, int n, std::vector<int32_t> *next) {
    if (!shapes || n == 0) { next->clear(); return VITX_OK; }
    if (n < 1 || n > p->max_images) { set_error("%s: n = %d is outside 1 .. max_images = %d", api, n, p->max_images); return VITX_ERR_ARG; }
    next->assign(shapes, shapes + (size_t)2 * n);
    return VITX_OK;
}

extern "C" {

int vitx_pack_create(const vitx_model *m, int device, int max_tokens, int max_images, int dtype, const vitx_pack_options *opt, vitx_pack **out) {
    if (!m || !out || max_tokens <= 0 || max_images <= 0) { set_error("vitx_pack_create: invalid argument"); return VITX_ERR_ARG; }
    *out = nullptr;
    if (m->kind != VITX_KIND_IMAGE) { set_error("vitx_pack_create: a text-tower model takes a text context (vitx_text_create), not a packed context"); return VITX_ERR_ARG; }
    if (dtype == VITX_MXFP8) { set_error("vitx_pack_create: VITX_MXFP8 is not supported by packed contexts (VITX_F16 or VITX_BF16)"); return VITX_ERR_UNSUPPORTED; }
    if (dtype != VITX_F16 && dtype != VITX_BF16) { set_error("vitx_pack_create: unknown dtype %d", dtype); return VITX_ERR_ARG; }
    const int pos_interp = opt ? opt->pos_interp : VITX_POS_BICUBIC, max_grids = opt && opt->max_grids ? opt->max_grids : 32;
    if (pos_interp != VITX_POS_BICUBIC && pos_interp != VITX_POS_BICUBIC_AA) { set_error("vitx_pack_create: unknown pos_interp %d (0 bicubic, 1 bicubic with antialias)", pos_interp); return VITX_ERR_ARG; }
    if (max_grids < 1) { set_error("vitx_pack_create: max_grids %d is not positive", max_grids); return VITX_ERR_ARG; }
    // every refusal before the first device call: nothing is launched after one
    if (m->in_chans == 1) { set_error("vitx_pack_create: a ViTSTR (one-channel) model takes no packed context"); return VITX_ERR_UNSUPPORTED; }
    if (m->head_pool != VITX_POOL_CLS) { set_error("vitx_pack_create: packed contexts take the class-token head only, not the pooled (cls + mean) or the attention-pooling head"); return VITX_ERR_UNSUPPORTED; }
    const vitx_hparams &hp = m->hp;
    const int D = hp.hidden_size, H = hp.num_attention_heads, F1 = m->mlp_fc1_rows();
    if (!attention_packed_supports(D, H)) { set_error("vitx_pack_create: attention needs a head_dim that is a multiple of 8 up to 128 (this model: %d / %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    if (!layernorm_supports(D)) { set_error("vitx_pack_create: hidden_size %d has no LayerNorm instantiation", D); return VITX_ERR_UNSUPPORTED; }
    if (m->rope_kind && !rope_supports(D, H)) { set_error("vitx_pack_create: rotary position embeddings need an even head dim (D %d, H %d)", D, H); return VITX_ERR_UNSUPPORTED; }
    if (hp.patch_size <= 0 || hp.img_size % hp.patch_size) { set_error("vitx_pack_create: the file's img_size %d is not a multiple of its patch size %d", hp.img_size, hp.patch_size); return VITX_ERR_UNSUPPORTED; }
    if ((long)max_tokens > (long)(0xf0000000u / ((size_t)std::max(F1, 3 * D) * 2)) / 256 * 256) { set_error("vitx_pack_create: max_tokens %d exceeds the kernels' 32-bit buffer window", max_tokens); return VITX_ERR_UNSUPPORTED; }
    const Tuning *tune = nullptr;
    int rc;
    if ((rc = open_device("vitx_pack_create", device, &tune))) return rc;
    std::unique_ptr<vitx_pack> p(new (std::nothrow) vitx_pack());
    if (!p) return VITX_ERR_NOMEM;
    p->model = m; p->device = device; p->dtype = dtype; p->tune = tune;
    p->D = D; p->L = hp.num_hidden_layers; p->H = H; p->C = hp.num_classes; p->C_pad = head_cols_pad(m); p->P = hp.patch_size;
    p->nreg = m->num_registers; p->Tp = 1 + p->nreg; p->g_in = hp.img_size / hp.patch_size; p->Kpe_pad = patch_k_pad(m);
    p->glu = m->glu_kind != VITX_GLU_NONE; p->F = m->mlp_hidden(); p->F1 = F1; p->rope = m->rope_kind != VITX_ROPE_NONE;
    p->fc1_epi = p->glu ? EPI_BIAS : act_epi(m->activation); p->eps = hp.eps;
    p->tm = gemm_tile_m(); p->tn = gemm_tile_n();
    p->max_tokens = max_tokens; p->max_images = max_images; p->max_grids = max_grids; p->pos_interp = pos_interp;
    // quantised block matrices are expanded at upload: block mode 0, as in the text context
    if ((rc = obtain_weights({m, device, dtype, false}, &p->wset, &p->weights_shared))) return rc;
    auto dmalloc = [&](void **q, size_t bytes) -> int {
        HIP_TRY(hipMalloc(q, bytes));
        p->allocs.push_back(*q); p->scratch_bytes += bytes;
        HIP_TRY(hipMemset(*q, 0, bytes));
        return VITX_OK;
    };
    const size_t Mp = (size_t)round_up(max_tokens, p->tm), Bp = (size_t)round_up(max_images, p->tm);
    p->host.assign(p->layout().ints(), 0);
    if ((rc = dmalloc((void **)&p->tab, p->host.size() * 4))) return rc;
    if ((rc = dmalloc((void **)&p->X, Mp * D * 4))) return rc;
    if ((rc = dmalloc(&p->U, Mp * D * 2))) return rc;
    if ((rc = dmalloc(&p->QKV, Mp * 3 * D * 2))) return rc;
    if ((rc = dmalloc(&p->Hbuf, Mp * (size_t)F1 * 2))) return rc;
    if (p->glu && (rc = dmalloc(&p->Hg, Mp * (size_t)p->F * 2))) return rc;
    if ((rc = dmalloc(&p->Z, Bp * D * 2))) return rc;
    if ((rc = dmalloc((void **)&p->logits, Bp * (size_t)p->C_pad * 4))) return rc;
    if ((rc = dmalloc((void **)&p->probs, (size_t)max_images * p->C * 4))) return rc;
    if ((rc = dmalloc((void **)&p->logits_out, (size_t)max_images * p->C * 4))) return rc;
    if (p->rope) {       // a call's grids hold at most max_tokens patches; twice that, so that grids of earlier calls stay cached
        p->rope_cap = 2L * max_tokens * (D / H / 2);
        if ((rc = dmalloc((void **)&p->rope_cos, (size_t)p->rope_cap * 4))) return rc;
        if ((rc = dmalloc((void **)&p->rope_sin, (size_t)p->rope_cap * 4))) return rc;
        HIP_TRY(hipHostMalloc((void **)&p->rope_host, (size_t)p->rope_cap * 2 * 4, hipHostMallocDefault));
    }
    HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&p->uploaded, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p->done, hipEventDisableTiming));
    HIP_TRY(hipDeviceSynchronize());
    *out = p.release();
    return VITX_OK;
}

void vitx_pack_free(vitx_pack *p) { delete p; }
int vitx_pack_shares_weights(const vitx_pack *p) { return p && p->weights_shared ? 1 : 0; }
size_t vitx_pack_scratch_bytes(const vitx_pack *p) { return p ? p->scratch_bytes : 0; }
int vitx_pack_launches(const vitx_pack *p, int *patch_embed) {
    if (!p) return 0;
    if (patch_embed) *patch_embed = p->pe_launches;
    return p->launches;
}

}  // extern "C"
