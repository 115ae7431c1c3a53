// packed_input.cpp -- how pixels get into a packed context besides f32 (packed_context.h; include/vitx.h "packed batches", u8 sources): decoded u8
// originals, each of its own size, stretched on the device to each image's own shape by ONE launch per pack (image_preprocess.hip
// pp_pil_packed_kernel).  Opt-in; the forward (packed_forward.cpp) allocates and launches nothing for it while it is off.  The part's state is
// PackU8 (packed_context.h): vitx_pack_u8_set is a set call like the heads' (alloc_counted, pack_commit), vitx_pack_u8_sources declares the
// sources' shapes of the next call (pack_next_shapes), which check_call consumes; its tables of a call are a PackU8Call.  The context's f32 pixel
// buffer is the set's own only where no vitx_pack_forward had allocated it before.
#include <algorithm>

#include "packed_context.h"
#include "preproc_resample.h"

extern "C" {

// Every argument check comes before the first device call; the state is built in a local and moved in, so a refused or failed set leaves what was set.
int vitx_pack_u8_set(vitx_pack *p, const vitx_preproc *pp, size_t max_src_bytes) {
    if (!p) { set_error("vitx_pack_u8_set: NULL context"); return VITX_ERR_ARG; }
    const bool off = max_src_bytes == 0;
    vitx_preproc d;
    if (!off) {
        if (pp) d = *pp;
        else if (const int rc = vitx_model_preproc(p->model, &d)) return rc;
        if (const char *bad = pp_check(d)) { set_error("vitx_pack_u8_set: %s", bad); return VITX_ERR_ARG; }
        if (!pp_filter_is_pil(d.filter)) { set_error("vitx_pack_u8_set: the reference's filters resize to squares only (use a PIL filter)"); return VITX_ERR_UNSUPPORTED; }
        if (max_src_bytes > (size_t)-1 - 3) { set_error("vitx_pack_u8_set: max_src_bytes = %zu", max_src_bytes); return VITX_ERR_ARG; }
    }
    HIP_TRY(hipSetDevice(p->device));
    if (const int rc = pack_quiesce(p)) return rc;
    const bool owned = p->u8 && p->u8->own_img;                      // the pixel buffer is the last set's: it goes with that set
    const size_t old_bytes = p->u8 ? p->u8->bytes : 0;
    if (off) {       // the tables first: a failed resize leaves the mode as it was
        if (const int rc = pack_commit(p, "vitx_pack_u8_set", p->parts() & ~kU8, old_bytes, 0)) return rc;
        if (owned) p->img = DevMem();
        p->u8.reset();
        return VITX_OK;
    }
    auto u = std::make_unique<PackU8>();
    u->pp = d; u->max_src_bytes = max_src_bytes;
    const size_t src_bytes = (max_src_bytes + 3) / 4 * 4;
    u->own_img = !p->img || owned;                                   // else an earlier vitx_pack_forward's: it stays, now and when u8 goes off
    DevMem img;
    if (!alloc_counted(u->src, src_bytes, &u->bytes) || (u->own_img && !alloc_counted(img, (size_t)p->max_tokens * p->P * p->P * 3 * 4, &u->bytes))) {
        set_error("vitx_pack_u8_set: cannot allocate %zu source bytes and the pixels of %d tokens", src_bytes, p->max_tokens);
        return VITX_ERR_NOMEM;
    }
    HIP_TRY(hipMemset(u->src.p, 0, src_bytes));
    HIP_TRY(hipDeviceSynchronize());
    if (const int rc = pack_commit(p, "vitx_pack_u8_set", p->parts() | kU8, old_bytes, u->bytes)) return rc;
    if (u->own_img) p->img = std::move(img);                         // (the last set's own buffer is freed by the move)
    p->u8 = std::move(u);
    return VITX_OK;
}

int vitx_pack_u8_sources(vitx_pack *p, const int32_t *src_shapes, int n) {
    if (!p || !p->u8) { set_error("vitx_pack_u8_sources: u8 sources are off (vitx_pack_u8_set)"); return VITX_ERR_ARG; }
    return pack_next_shapes(p, "vitx_pack_u8_sources", src_shapes, n, &p->u8->next_src);
}

int vitx_pack_fit_shapes(const vitx_model *m, const int32_t *src_shapes, int n, int short_side, int max_long, int32_t *shapes) {
    if (!m || !src_shapes || !shapes || n < 1) { set_error("vitx_pack_fit_shapes: invalid argument"); return VITX_ERR_ARG; }
    for (int i = 0; i < n; ++i) {
        int w = 0, h = 0;
        if (const char *bad = pp_rect_shape(src_shapes[2 * i + 1], src_shapes[2 * i], m->hp.patch_size, short_side, max_long, w, h)) {
            set_error("vitx_pack_fit_shapes: image %d: %s", i, bad);
            return VITX_ERR_ARG;
        }
        shapes[2 * i] = h; shapes[2 * i + 1] = w;
    }
    return VITX_OK;
}

}  // extern "C"
