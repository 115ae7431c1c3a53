// pos_resample_host.cpp -- host side of the position-embedding resampler: vitx_pos_embed_resample (the loop over pos_resample.h that the device
// kernel restates thread by thread) and vitx_model_resize_file (a model file at another img_size).  Host only, no GPU.
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "model_file.h"
#include "pos_resample.h"

using namespace vitx;

extern "C" int vitx_pos_embed_resample(const float *pos, int gy_in, int gx_in, int D, int gy_out, int gx_out, int interp, float *out) {
    if (!pos_resample_args_ok(pos, gy_in, gx_in, D, gy_out, gx_out, interp, out)) { set_error("vitx_pos_embed_resample: invalid argument"); return VITX_ERR_ARG; }
    const size_t rows_out = (size_t)gy_out * gx_out + 1;
    if (gy_in == gy_out && gx_in == gx_out) { memmove(out, pos, rows_out * D * 4); return VITX_OK; }
    memmove(out, pos, (size_t)D * 4);                                   // the class token's row
    const float sy = pos_scale(gy_in, gy_out), sx = pos_scale(gx_in, gx_out);
    std::vector<PosAxis> axs((size_t)gx_out);
    for (int ox = 0; ox < gx_out; ++ox) axs[ox] = pos_axis(interp, gx_in, gx_out, sx, ox);
    for (int oy = 0; oy < gy_out; ++oy) {
        const PosAxis ay = pos_axis(interp, gy_in, gy_out, sy, oy);
        for (int ox = 0; ox < gx_out; ++ox) {
            float *o = out + ((size_t)oy * gx_out + ox + 1) * D;
            for (int d = 0; d < D; ++d) { float v[1]; pos_cell<1>(pos + D, gy_in, gx_in, D, interp, ay, axs[ox], d, v); o[d] = v[0]; }
        }
    }
    return VITX_OK;
}

namespace {

struct Cursor {
    const std::vector<uint8_t> &b; size_t at = 0; bool ok = true;
    bool i32(int32_t &v) { if (at + 4 > b.size()) return ok = false; memcpy(&v, &b[at], 4); at += 4; return true; }
    bool skip(size_t n) { if (n > b.size() - at) return ok = false; at += n; return true; }
};

}  // namespace

extern "C" int vitx_model_resize_file(const char *path_in, const char *path_out, int img_size, int interp) {
    if (!path_in || !path_out) { set_error("vitx_model_resize_file: NULL path"); return VITX_ERR_ARG; }
    if (img_size <= 0) { set_error("vitx_model_resize_file: img_size %d is not positive", img_size); return VITX_ERR_ARG; }
    if (interp != POS_BICUBIC && interp != POS_BICUBIC_AA) { set_error("vitx_model_resize_file: unknown interpolation %d (0 bicubic, 1 bicubic with antialias)", interp); return VITX_ERR_ARG; }
    if (strcmp(path_in, path_out) == 0) { set_error("vitx_model_resize_file: input and output are the same file '%s'", path_in); return VITX_ERR_ARG; }
    // the loader validates the whole file; the bytes are then walked a second time and copied through, so that nothing but the header's
    // img_size and the pos_embed record changes (label order, the header's ftype word and every other tensor record stay as they are)
    vitx_model *m = nullptr;
    int rc = vitx_model_load(path_in, &m);
    if (rc != VITX_OK) return rc;
    if (m->kind != VITX_KIND_IMAGE) { vitx_model_free(m); set_error("vitx_model_resize_file: '%s' is a text-tower file: it has no image size", path_in); return VITX_ERR_ARG; }
    const vitx_hparams hp = m->hp;
    const int in_chans = m->in_chans;
    const bool map_head = m->head_pool == VITX_POOL_MAP;
    const bool has_preproc = m->has_preproc;
    const vitx_preproc pp_in = m->preproc;
    std::vector<float> pos;
    if (const HostTensor *t = m->find("pos_embed")) { pos.resize((size_t)t->nelements()); t->decode_f32(pos.data()); }
    vitx_model_free(m);
    if (img_size % hp.patch_size) { set_error("vitx_model_resize_file: img_size %d is not a multiple of the patch size %d", img_size, hp.patch_size); return VITX_ERR_ARG; }
    if (map_head) { set_error("vitx_model_resize_file: a file with the attention-pooling head has a position table without a class row: resampling it is not supported yet"); return VITX_ERR_UNSUPPORTED; }
    if (in_chans == 1 && img_size != hp.img_size) { set_error("vitx_model_resize_file: a ViTSTR file stays at its own img_size (%d)", hp.img_size); return VITX_ERR_UNSUPPORTED; }
    float pp_slots[16] = {0};
    if (has_preproc) {                                                // the model's preprocessing follows the size (vitx_preproc_at_size)
        vitx_preproc pp_out;
        if ((rc = vitx_preproc_at_size(&pp_in, img_size, &pp_out))) return rc;
        pp_to_slots(pp_out, pp_slots);
    }
    const int g_in = hp.img_size / hp.patch_size, g_out = img_size / hp.patch_size, D = hp.hidden_size;
    std::vector<float> res(((size_t)g_out * g_out + 1) * D);
    if ((rc = vitx_pos_embed_resample(pos.data(), g_in, g_in, D, g_out, g_out, interp, res.data()))) return rc;

    std::vector<uint8_t> in;
    {
        FILE *f = fopen(path_in, "rb");
        if (!f) { set_error("vitx_model_resize_file: failed to open '%s'", path_in); return VITX_ERR_IO; }
        uint8_t buf[1 << 16]; size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) in.insert(in.end(), buf, buf + n);
        fclose(f);
    }
    const std::string tmp = std::string(path_out) + ".tmp" + std::to_string((long)getpid());
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) { set_error("vitx_model_resize_file: failed to open '%s' for writing", tmp.c_str()); return VITX_ERR_IO; }
    bool ok = true, found = false;
    auto put = [&](const void *p, size_t n) { ok = ok && (n == 0 || fwrite(p, n, 1, f) == 1); };
    Cursor cu{in};
    int32_t v = 0, nl = 0;
    for (int i = 0; i < 8; ++i) cu.i32(v);                             // magic + 7 hparams
    cu.i32(nl);
    for (int i = 0; cu.ok && i < nl; ++i) { int32_t key, len; if (cu.i32(key) && cu.i32(len) && len >= 0) cu.skip((size_t)len); else cu.ok = false; }
    if (cu.ok) {
        put(in.data(), 24);
        const int32_t s = img_size; put(&s, 4);                        // hparams word 5 = img_size
        put(in.data() + 28, cu.at - 28);
    }
    while (cu.ok && cu.at < in.size()) {
        const size_t rec = cu.at;
        int32_t n_dims, name_len, ttype, ne[4] = {1, 1, 1, 1};
        if (!cu.i32(n_dims) || !cu.i32(name_len) || !cu.i32(ttype) || n_dims < 1 || n_dims > 4 || name_len <= 0) { cu.ok = false; break; }
        for (int i = 0; i < n_dims; ++i) cu.i32(ne[i]);
        const size_t name_at = cu.at;
        if (!cu.skip((size_t)name_len)) break;
        const int bb = type_block_bytes(ttype), be = type_block_elems(ttype);
        if (!bb) { cu.ok = false; break; }
        const size_t nbytes = (size_t)((int64_t)ne[0] * ne[1] * ne[2] * ne[3] / be) * bb, data_at = cu.at;
        if (!cu.skip(nbytes)) break;
        if (std::string((const char *)&in[name_at], (size_t)name_len) == "pos_embed") {
            found = true;
            int32_t head[3] = {n_dims, name_len, ttype};
            ne[1] = g_out * g_out + 1;
            put(head, 12); put(ne, 4 * (size_t)n_dims); put(&in[name_at], (size_t)name_len); put(res.data(), res.size() * 4);
        } else if (has_preproc && nbytes == sizeof(pp_slots) && std::string((const char *)&in[name_at], (size_t)name_len) == "preproc") {
            put(&in[rec], data_at - rec); put(pp_slots, sizeof(pp_slots));
        } else put(&in[rec], data_at + nbytes - rec);
    }
    if (fclose(f) != 0) ok = false;
    if (!cu.ok || !found) { (void)remove(tmp.c_str()); set_error("vitx_model_resize_file: '%s' changed while it was read", path_in); return VITX_ERR_FORMAT; }
    if (!ok) { (void)remove(tmp.c_str()); set_error("vitx_model_resize_file: short write to '%s'", tmp.c_str()); return VITX_ERR_IO; }
    if (rename(tmp.c_str(), path_out) != 0) { (void)remove(tmp.c_str()); set_error("vitx_model_resize_file: cannot move the result to '%s'", path_out); return VITX_ERR_IO; }
    return VITX_OK;
}
