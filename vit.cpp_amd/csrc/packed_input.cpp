// packed_input.cpp -- how pixels get into a packed context besides f32 (packed_context.h; include/vitx.h "packed batches", u8 sources): decoded u8
// originals, each of its own size, stretched on the device to each image's own shape by ONE launch per pack (image_preprocess.hip
// pp_pil_packed_kernel).  Opt-in; the forward (packed_forward.cpp) allocates and launches nothing for it while it is off.
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
    const size_t img_bytes = (size_t)p->max_tokens * p->P * p->P * 3 * 4;
    // what the last set added goes: the staging with its owner, the pixel buffer only where that set allocated it
    auto drop = [&]() {
        if (!p->u8) return;
        if (p->u8->own_img) { (void)hipFree(p->img); p->img = nullptr; }
        p->scratch_bytes -= p->u8->bytes;
        p->u8.reset();
    };
    if (off) {       // the tables first: a failed resize leaves the mode as it was
        if (const int rc = resize_tables(p, "vitx_pack_u8_set", (bool)p->dense, (bool)p->depth, false, p->rollout())) return rc;
        drop();
        return VITX_OK;
    }
    auto u = std::make_unique<PackU8>();
    u->pp = d; u->max_src_bytes = max_src_bytes;
    const size_t src_bytes = (max_src_bytes + 3) / 4 * 4;
    const bool have_img = p->img && !(p->u8 && p->u8->own_img);      // an earlier vitx_pack_forward's: it stays
    float *img = nullptr;
    if (!u->src.alloc(src_bytes) || (!have_img && hipMalloc((void **)&img, img_bytes) != hipSuccess)) {
        (void)hipGetLastError();
        set_error("vitx_pack_u8_set: cannot allocate %zu source bytes and the pixels of %d tokens", src_bytes, p->max_tokens);
        return VITX_ERR_NOMEM;
    }
    DevMem img_own(img);
    HIP_TRY(hipMemset(u->src.p, 0, src_bytes));
    HIP_TRY(hipDeviceSynchronize());
    if (const int rc = resize_tables(p, "vitx_pack_u8_set", (bool)p->dense, (bool)p->depth, true, p->rollout())) return rc;
    drop();
    if (!have_img) { p->img = img; img_own.p = nullptr; u->own_img = true; }
    u->bytes = src_bytes + (u->own_img ? img_bytes : 0);
    p->scratch_bytes += u->bytes;
    p->u8 = std::move(u);
    return VITX_OK;
}

int vitx_pack_u8_sources(vitx_pack *p, const int32_t *src_shapes, int n) {
    if (!p || !p->u8) { set_error("vitx_pack_u8_sources: u8 sources are off (vitx_pack_u8_set)"); return VITX_ERR_ARG; }
    if (!src_shapes || n == 0) { p->u8->next_src.clear(); p->u8->declared = false; return VITX_OK; }
    if (n < 1 || n > p->max_images) { set_error("vitx_pack_u8_sources: n = %d is outside 1 .. max_images = %d", n, p->max_images); return VITX_ERR_ARG; }
    p->u8->next_src.assign(src_shapes, src_shapes + (size_t)2 * n);
    p->u8->declared = true;
    return VITX_OK;
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
