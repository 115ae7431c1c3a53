// model_file.cpp -- legacy-ggml ".gguf" reader (host only, no GPU, no ggml).
//
// Same acceptance rules as the reference loader (/root/reference/vit.cpp:308-712):
// magic (320-328), 7 int32 hparams (335-341, ftype %= 1000 at 354), id2label (356-371),
// then named tensors until EOF (590-695): unknown name -> error (618-622), element-count
// and shape must match what the hparams imply (627-641), byte size must match the type
// (680-685), and every expected tensor must appear exactly once (697-701).  One deliberate
// widening: patch_embed.proj.weight is accepted as f32 as well as f16 (the reference only
// takes f16 there, vit.cpp:515, so "--ftype 0" files it cannot load are loadable here).
// Two optional extensions the reference's loader has no slot for (DINOv2-class models; include/vitx.h "Register tokens and the pooled
// head"), recognised by name and shape: `reg_token` f32 [1][R][D], and a `head.weight` of [C][2 D].
// Two more (include/vitx.h "Activation, epsilon and pre-norm"): `arch` f32 [4] = {activation, eps, 0, 0} and the pair `pre_norm.weight`,
// `pre_norm.bias` f32 [D] (CLIP's pre_layrnorm).  Without `arch` a file means tanh-GELU and eps 1e-6, the reference's arithmetic.
// One more (include/vitx.h "no class token and the attention-pooling head"): the thirteen `attn_pool.*` tensors of a SigLIP-class model, which
// come without cls_token / reg_token and with a pos_embed of g^2 rows (VITX_POOL_MAP).
// One more (include/vitx.h "rotary position embeddings"): `rope` f32 [4] = {kind, theta, 0, 0} of a DINOv3-class model; its pos_embed is all zero.
// One more (include/vitx.h "gated MLP"): `glu` f32 [4] = {kind, F, 0, 0} in front of the first blocks.* record; mlp.fc1.* then has 2 F rows and
// mlp.fc2.weight rows of F.
// A text-tower file (include/vitx.h "the text tower") is told by patch_size == 0: token_embed.weight [V][D] (f16 or f32) and pos_embed [T][D]
// in place of the image front, the same blocks, norm.* and head.* [E][D]; `arch` is then required and its last two slots are {causal, eos + 1};
// `zs` f32 [4] = {kind, scale, bias, 0} is optional.  cls_token, reg_token, pre_norm.*, preproc and attn_pool.* do not belong in one.
#include "model_file.h"

#include <math.h>
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <atomic>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>

namespace vitx {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
const char *last_error() { return g_err; }

int type_block_bytes(int t) {
    switch (t) { case T_F32: return 4; case T_F16: return 2; case T_Q4_0: return 18; case T_Q4_1: return 20;
                 case T_Q5_0: return 22; case T_Q5_1: return 24; case T_Q8_0: return 34; default: return 0; }
}
int type_block_elems(int t) { return (t == T_F32 || t == T_F16) ? 1 : 32; }

float f16_bits_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t exp = (h >> 10) & 0x1f, man = h & 0x3ffu, bits;
    if (exp == 0) {
        if (man == 0) bits = sign;
        else { int e = -1; do { ++e; man <<= 1; } while (!(man & 0x400u)); bits = sign | ((uint32_t)(127 - 15 - e) << 23) | ((man & 0x3ffu) << 13); }
    } else if (exp == 31) bits = sign | 0x7f800000u | (man << 13);
    else bits = sign | ((exp + 112) << 23) | (man << 13);
    float f; memcpy(&f, &bits, 4); return f;
}
uint16_t f32_to_f16_bits(float f) {
    uint32_t x; memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u; x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0));   // inf / nan
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                    // rounds to inf
    if (x < 0x33000001u) return (uint16_t)sign;                                                 // rounds to zero
    if (x < 0x38800000u) {                                                                      // subnormal half
        const int shift = 126 - (int)(x >> 23);                  // 14..24
        const uint32_t man = (x & 0x7fffffu) | 0x800000u;
        uint32_t r = man >> shift; const uint32_t rem = man & ((1u << shift) - 1), halfway = 1u << (shift - 1);
        if (rem > halfway || (rem == halfway && (r & 1))) ++r;
        return (uint16_t)(sign | r);
    }
    uint32_t r = ((x - 0x38000000u) >> 13); const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1))) ++r;
    return (uint16_t)(sign | r);
}
uint16_t f32_to_bf16_bits(float f) {
    uint32_t x; memcpy(&x, &f, 4);
    if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x40u);
    x += 0x7fffu + ((x >> 16) & 1u);
    return (uint16_t)(x >> 16);
}

static inline float rd16(const uint8_t *p) { uint16_t h; memcpy(&h, p, 2); return f16_bits_to_f32(h); }

void HostTensor::decode_f32(float *out) const {
    const int64_t n = nelements();
    if (type == T_F32) { memcpy(out, raw.data(), (size_t)n * 4); return; }
    if (type == T_F16) { const uint8_t *p = raw.data(); for (int64_t i = 0; i < n; ++i) out[i] = rd16(p + 2 * i); return; }
    const int bb = type_block_bytes(type);
    const int64_t nb = n / 32;
    for (int64_t b = 0; b < nb; ++b) {
        const uint8_t *p = raw.data() + (size_t)b * bb; float *o = out + b * 32;
        switch (type) {
        case T_Q4_0: { const float d = rd16(p); const uint8_t *qs = p + 2;
            for (int j = 0; j < 16; ++j) { o[j] = ((qs[j] & 0x0F) - 8) * d; o[j + 16] = ((qs[j] >> 4) - 8) * d; } } break;
        case T_Q4_1: { const float d = rd16(p), m = rd16(p + 2); const uint8_t *qs = p + 4;
            for (int j = 0; j < 16; ++j) { o[j] = (qs[j] & 0x0F) * d + m; o[j + 16] = (qs[j] >> 4) * d + m; } } break;
        case T_Q5_0: { const float d = rd16(p); uint32_t qh; memcpy(&qh, p + 2, 4); const uint8_t *qs = p + 6;
            for (int j = 0; j < 16; ++j) { const uint8_t h0 = ((qh >> j) << 4) & 0x10, h1 = (qh >> (j + 12)) & 0x10;
                o[j] = (((qs[j] & 0x0F) | h0) - 16) * d; o[j + 16] = (((qs[j] >> 4) | h1) - 16) * d; } } break;
        case T_Q5_1: { const float d = rd16(p), m = rd16(p + 2); uint32_t qh; memcpy(&qh, p + 4, 4); const uint8_t *qs = p + 8;
            for (int j = 0; j < 16; ++j) { const uint8_t h0 = ((qh >> j) << 4) & 0x10, h1 = (qh >> (j + 12)) & 0x10;
                o[j] = ((qs[j] & 0x0F) | h0) * d + m; o[j + 16] = ((qs[j] >> 4) | h1) * d + m; } } break;
        case T_Q8_0: { const float d = rd16(p); const int8_t *qs = (const int8_t *)(p + 2);
            for (int j = 0; j < 32; ++j) o[j] = qs[j] * d; } break;
        }
    }
}

// expected tensors and their ggml shapes (vit.cpp:506-581); type classes: 0 = must be f32,
// 1 = "wtype" (f32/f16/q*), 2 = patch kernel (f16, f32 also accepted here), 3 = attn_pool.* matrix (f16 or f32: never block-quantised)
struct Expect { int64_t ne[4]; int cls; };
static std::map<std::string, Expect> expected_tensors(const vitx_hparams &hp) {
    std::map<std::string, Expect> e;
    const int64_t D = hp.hidden_size, C = hp.num_classes, P = hp.patch_size;
    if (P == 0) {                                                    // a text tower (include/vitx.h "the text tower"): img_size = T; V is token_embed.weight's row count
        e["pos_embed"] = {{D, hp.img_size, 1, 1}, 0};
        e["token_embed.weight"] = {{D, 0, 1, 1}, 2};
    } else {
        const int64_t g = hp.img_size / P, N = g * g + 1;
        e["pos_embed"] = {{D, N, 1, 1}, 0};
        e["cls_token"] = {{D, 1, 1, 1}, 0};
        e["patch_embed.proj.weight"] = {{P, P, 3, D}, 2};
        e["patch_embed.proj.bias"] = {{1, 1, D, 1}, 0};
    }
    for (int i = 0; i < hp.num_hidden_layers; ++i) {
        const std::string p = "blocks." + std::to_string(i) + ".";
        e[p + "norm1.weight"] = {{D, 1, 1, 1}, 0}; e[p + "norm1.bias"] = {{D, 1, 1, 1}, 0};
        e[p + "attn.qkv.weight"] = {{D, 3 * D, 1, 1}, 1}; e[p + "attn.qkv.bias"] = {{3 * D, 1, 1, 1}, 0};
        e[p + "attn.proj.weight"] = {{D, D, 1, 1}, 1}; e[p + "attn.proj.bias"] = {{D, 1, 1, 1}, 0};
        e[p + "norm2.weight"] = {{D, 1, 1, 1}, 0}; e[p + "norm2.bias"] = {{D, 1, 1, 1}, 0};
        e[p + "mlp.fc1.weight"] = {{D, 4 * D, 1, 1}, 1}; e[p + "mlp.fc1.bias"] = {{4 * D, 1, 1, 1}, 0};
        e[p + "mlp.fc2.weight"] = {{4 * D, D, 1, 1}, 1}; e[p + "mlp.fc2.bias"] = {{D, 1, 1, 1}, 0};
    }
    e["norm.weight"] = {{D, 1, 1, 1}, 0}; e["norm.bias"] = {{D, 1, 1, 1}, 0};
    e["head.weight"] = {{D, C, 1, 1}, 1}; e["head.bias"] = {{C, 1, 1, 1}, 0};
    return e;
}

// the attention-pooling head (VITX_POOL_MAP): all thirteen or none; matrices f32 or f16 (never block-quantised), everything else f32
static std::map<std::string, Expect> pool_tensors(const vitx_hparams &hp) {
    std::map<std::string, Expect> e;
    const int64_t D = hp.hidden_size;
    e["attn_pool.latent"] = {{D, 1, 1, 1}, 0};
    e["attn_pool.q.weight"] = {{D, D, 1, 1}, 3}; e["attn_pool.q.bias"] = {{D, 1, 1, 1}, 0};
    e["attn_pool.kv.weight"] = {{D, 2 * D, 1, 1}, 3}; e["attn_pool.kv.bias"] = {{2 * D, 1, 1, 1}, 0};
    e["attn_pool.proj.weight"] = {{D, D, 1, 1}, 3}; e["attn_pool.proj.bias"] = {{D, 1, 1, 1}, 0};
    e["attn_pool.norm.weight"] = {{D, 1, 1, 1}, 0}; e["attn_pool.norm.bias"] = {{D, 1, 1, 1}, 0};
    e["attn_pool.mlp.fc1.weight"] = {{D, 4 * D, 1, 1}, 3}; e["attn_pool.mlp.fc1.bias"] = {{4 * D, 1, 1, 1}, 0};
    e["attn_pool.mlp.fc2.weight"] = {{4 * D, D, 1, 1}, 3}; e["attn_pool.mlp.fc2.bias"] = {{D, 1, 1, 1}, 0};
    return e;
}

struct FileCloser { void operator()(FILE *f) const { if (f) fclose(f); } };

static int load_impl(const char *path, vitx_model &m) {
    std::unique_ptr<FILE, FileCloser> fh(fopen(path, "rb"));
    FILE *f = fh.get();
    if (!f) { set_error("vitx_model_load: failed to open '%s'", path); return VITX_ERR_IO; }
    auto rd_i32 = [&](int32_t &v) { return fread(&v, 4, 1, f) == 1; };
    int32_t magic = 0;
    if (!rd_i32(magic) || (uint32_t)magic != 0x67676d6cu) { set_error("vitx_model_load: invalid model file '%s' (bad magic)", path); return VITX_ERR_FORMAT; }
    int32_t hv[7];
    for (int i = 0; i < 7; ++i) if (!rd_i32(hv[i])) { set_error("vitx_model_load: truncated header"); return VITX_ERR_IO; }
    vitx_hparams &hp = m.hp;
    hp.hidden_size = hv[0]; hp.num_hidden_layers = hv[1]; hp.num_attention_heads = hv[2]; hp.num_classes = hv[3];
    hp.patch_size = hv[4]; hp.img_size = hv[5]; hp.ftype = hv[6] % 1000 /* GGML_QNT_VERSION_FACTOR */; hp.eps = 1e-6f;
    const bool text = hp.patch_size == 0;                            // THE mark of a text-tower file: no image file has it
    m.kind = text ? VITX_KIND_TEXT : VITX_KIND_IMAGE;
    if (hp.hidden_size <= 0 || hp.num_hidden_layers <= 0 || hp.num_attention_heads <= 0 || hp.num_classes <= 0 || hp.patch_size < 0 ||
        hp.img_size <= 0 || (!text && hp.img_size % hp.patch_size) || hp.hidden_size % hp.num_attention_heads || hp.num_hidden_layers > 4096) {
        set_error("vitx_model_load: implausible hparams in '%s'", path); return VITX_ERR_FORMAT;
    }
    if (!type_block_bytes(hp.ftype)) { set_error("vitx_model_load: invalid model file '%s' (bad ftype value %d)", path, hp.ftype); return VITX_ERR_FORMAT; }
    int32_t nl = 0;
    if (!rd_i32(nl) || nl < 0 || nl > (1 << 24)) { set_error("vitx_model_load: bad label count"); return VITX_ERR_FORMAT; }
    for (int i = 0; i < nl; ++i) {
        int32_t key, len;
        if (!rd_i32(key) || !rd_i32(len) || len < 0 || len > (1 << 20)) { set_error("vitx_model_load: bad id2label entry"); return VITX_ERR_FORMAT; }
        std::string v((size_t)len, '\0');
        if (len && fread(&v[0], 1, (size_t)len, f) != (size_t)len) { set_error("vitx_model_load: truncated id2label"); return VITX_ERR_IO; }
        m.id2label[key] = v;
    }
    auto expect = expected_tensors(hp);                              // (`glu` rewrites the MLP shapes of every block: it stands in front of them)
    const auto pool_expect = text ? std::map<std::string, Expect>() : pool_tensors(hp);
    int n_optional = 0;                                              // `arch`, `preproc`, `pre_norm.*` records seen
    int n_pool = 0;                                                  // `attn_pool.*` records seen
    bool pos_no_cls = false;                                         // pos_embed has g^2 rows (no class row)
    bool seen_block = false;                                         // a blocks.* record has been read
    for (;;) {
        int32_t n_dims, name_len, ttype;
        if (!rd_i32(n_dims)) break;                                  // clean EOF (vit.cpp:600-603)
        if (!rd_i32(name_len) || !rd_i32(ttype)) { set_error("vitx_model_load: truncated tensor header"); return VITX_ERR_IO; }
        if (n_dims < 1 || n_dims > 4 || name_len <= 0 || name_len > 255) { set_error("vitx_model_load: bad tensor header"); return VITX_ERR_FORMAT; }
        vitx::HostTensor t; t.n_dims = n_dims; t.type = ttype;
        for (int i = 0; i < n_dims; ++i) { int32_t v; if (!rd_i32(v) || v <= 0) { set_error("vitx_model_load: bad dims"); return VITX_ERR_FORMAT; } t.ne[i] = v; }
        t.name.resize((size_t)name_len);
        if (fread(&t.name[0], 1, (size_t)name_len, f) != (size_t)name_len) { set_error("vitx_model_load: truncated name"); return VITX_ERR_IO; }
        if (t.name == "reg_token") {                                 // optional: R register tokens, f32 [1][R][D] (ggml order [D, R, 1])
            if (m.index.count(t.name)) { set_error("vitx_model_load: duplicate tensor '%s'", t.name.c_str()); return VITX_ERR_FORMAT; }
            if (ttype != T_F32 || n_dims != 3 || t.ne[0] != hp.hidden_size || t.ne[1] < 1 || t.ne[1] > 4096 || t.ne[2] != 1) {
                set_error("vitx_model_load: tensor 'reg_token' must be f32 [1][R][%d] with 1 <= R <= 4096: got type %d, %d dims [%lld, %lld, %lld]", hp.hidden_size, ttype, n_dims,
                          (long long)t.ne[0], (long long)t.ne[1], (long long)t.ne[2]);
                return VITX_ERR_FORMAT;
            }
            const size_t nbytes = (size_t)t.nelements() * 4;
            t.raw.resize(nbytes);
            if (fread(t.raw.data(), 1, nbytes, f) != nbytes) { set_error("vitx_model_load: tensor '%s' is truncated", t.name.c_str()); return VITX_ERR_IO; }
            m.num_registers = (int)t.ne[1];
            m.index[t.name] = (int)m.tensors.size();
            m.tensors.push_back(std::move(t));
            continue;
        }
        if (t.name == "arch") {                                      // optional: f32 [4] = {activation, eps, 0, 0} (include/vitx.h "Activation, epsilon and pre-norm")
            if (m.index.count(t.name)) { set_error("vitx_model_load: duplicate tensor '%s'", t.name.c_str()); return VITX_ERR_FORMAT; }
            if (ttype != T_F32 || n_dims != 1 || t.ne[0] != 4) {
                set_error("vitx_model_load: tensor 'arch' must be f32 [4] = {activation, eps, 0, 0}: got type %d, %d dims [%lld, ..]", ttype, n_dims, (long long)t.ne[0]);
                return VITX_ERR_FORMAT;
            }
            t.raw.resize(16);
            if (fread(t.raw.data(), 1, 16, f) != 16) { set_error("vitx_model_load: tensor '%s' is truncated", t.name.c_str()); return VITX_ERR_IO; }
            float a[4]; memcpy(a, t.raw.data(), 16);
            if (a[0] != (float)VITX_ACT_GELU_TANH && a[0] != (float)VITX_ACT_GELU_ERF && a[0] != (float)VITX_ACT_QUICK_GELU) {
                set_error("vitx_model_load: tensor 'arch' names activation %g: 0 tanh-GELU, 1 erf-GELU and 2 QuickGELU exist", (double)a[0]); return VITX_ERR_FORMAT;
            }
            if (!(a[1] > 0.0f) || !(a[1] <= 3.402823466e38f)) { set_error("vitx_model_load: tensor 'arch' carries LayerNorm eps %g: it must be finite and positive", (double)a[1]); return VITX_ERR_FORMAT; }
            if (!text && (a[2] != 0.0f || a[3] != 0.0f)) { set_error("vitx_model_load: tensor 'arch' has reserved slots {%g, %g}: they must be 0", (double)a[2], (double)a[3]); return VITX_ERR_FORMAT; }
            if (text) {                                              // {.., causal, eos + 1}
                if (a[2] != 0.0f && a[2] != 1.0f) { set_error("vitx_model_load: tensor 'arch' of a text file names causal %g: 0 (no mask) and 1 (causal) exist", (double)a[2]); return VITX_ERR_FORMAT; }
                if (!(a[3] >= 0.0f) || a[3] > 16777216.0f || a[3] != floorf(a[3])) { set_error("vitx_model_load: tensor 'arch' of a text file carries eos + 1 = %g: it must be a whole number, 0 for none", (double)a[3]); return VITX_ERR_FORMAT; }
                m.causal = (int)a[2]; m.eos = (int)a[3] - 1;
            }
            m.activation = (int)a[0]; hp.eps = a[1];
            m.index[t.name] = (int)m.tensors.size();
            m.tensors.push_back(std::move(t));
            ++n_optional;
            continue;
        }
        if (t.name == "zs" && text) {                                // optional, text files: f32 [4] = {kind, scale, bias, 0}
            if (m.index.count(t.name)) { set_error("vitx_model_load: duplicate tensor '%s'", t.name.c_str()); return VITX_ERR_FORMAT; }
            if (ttype != T_F32 || n_dims != 1 || t.ne[0] != 4) { set_error("vitx_model_load: tensor 'zs' must be f32 [4] = {kind, scale, bias, 0}: got type %d, %d dims [%lld, ..]", ttype, n_dims, (long long)t.ne[0]); return VITX_ERR_FORMAT; }
            t.raw.resize(16);
            if (fread(t.raw.data(), 1, 16, f) != 16) { set_error("vitx_model_load: tensor '%s' is truncated", t.name.c_str()); return VITX_ERR_IO; }
            float a[4]; memcpy(a, t.raw.data(), 16);
            if (a[0] != (float)VITX_ZS_SOFTMAX && a[0] != (float)VITX_ZS_SIGMOID) { set_error("vitx_model_load: tensor 'zs' names kind %g: 0 softmax and 1 sigmoid exist", (double)a[0]); return VITX_ERR_FORMAT; }
            if (!std::isfinite(a[1]) || !std::isfinite(a[2]) || a[3] != 0.0f) { set_error("vitx_model_load: tensor 'zs' needs a finite scale and bias and a zero last slot"); return VITX_ERR_FORMAT; }
            m.has_zs = true; m.zs_kind = (int)a[0]; m.zs_scale = a[1]; m.zs_bias = a[2];
            m.index[t.name] = (int)m.tensors.size();
            m.tensors.push_back(std::move(t));
            ++n_optional;
            continue;
        }
        if (t.name == "rope") {                                      // optional: f32 [4] = {kind, theta, 0, 0} (include/vitx.h "rotary position embeddings")
            if (m.index.count(t.name)) { set_error("vitx_model_load: duplicate tensor '%s'", t.name.c_str()); return VITX_ERR_FORMAT; }
            if (text) { set_error("vitx_model_load: text-tower file: tensor 'rope' belongs to image files"); return VITX_ERR_FORMAT; }
            if (ttype != T_F32 || n_dims != 1 || t.ne[0] != 4) {
                set_error("vitx_model_load: tensor 'rope' must be f32 [4] = {kind, theta, 0, 0}: got type %d, %d dims [%lld, ..]", ttype, n_dims, (long long)t.ne[0]);
                return VITX_ERR_FORMAT;
            }
            t.raw.resize(16);
            if (fread(t.raw.data(), 1, 16, f) != 16) { set_error("vitx_model_load: tensor '%s' is truncated", t.name.c_str()); return VITX_ERR_IO; }
            float a[4]; memcpy(a, t.raw.data(), 16);
            if (a[0] != (float)VITX_ROPE_DINOV3_AXIAL) { set_error("vitx_model_load: tensor 'rope' names kind %g: only 1 (DINOv3 axial) exists", (double)a[0]); return VITX_ERR_FORMAT; }
            if (!(a[1] > 0.0f) || !(a[1] <= 3.402823466e38f)) { set_error("vitx_model_load: tensor 'rope' carries theta %g: it must be finite and positive", (double)a[1]); return VITX_ERR_FORMAT; }
            if (a[2] != 0.0f || a[3] != 0.0f) { set_error("vitx_model_load: tensor 'rope' has reserved slots {%g, %g}: they must be 0", (double)a[2], (double)a[3]); return VITX_ERR_FORMAT; }
            if ((hp.hidden_size / hp.num_attention_heads) % 4) { set_error("vitx_model_load: tensor 'rope' needs a head dim that is a multiple of 4 (this file: %d)", hp.hidden_size / hp.num_attention_heads); return VITX_ERR_FORMAT; }
            m.rope_kind = (int)a[0]; m.rope_theta = a[1];
            m.index[t.name] = (int)m.tensors.size();
            m.tensors.push_back(std::move(t));
            ++n_optional;
            continue;
        }
        if (t.name == "glu") {                                       // optional: f32 [4] = {kind, F, 0, 0} (include/vitx.h "gated MLP")
            if (m.index.count(t.name)) { set_error("vitx_model_load: duplicate tensor '%s'", t.name.c_str()); return VITX_ERR_FORMAT; }
            if (text) { set_error("vitx_model_load: text-tower file: tensor 'glu' belongs to image files"); return VITX_ERR_FORMAT; }
            if (ttype != T_F32 || n_dims != 1 || t.ne[0] != 4) {
                set_error("vitx_model_load: tensor 'glu' must be f32 [4] = {kind, F, 0, 0}: got type %d, %d dims [%lld, ..]", ttype, n_dims, (long long)t.ne[0]);
                return VITX_ERR_FORMAT;
            }
            if (seen_block) { set_error("vitx_model_load: tensor 'glu' stands behind a blocks.* record: it sets their shapes and must come in front of the first one"); return VITX_ERR_FORMAT; }
            t.raw.resize(16);
            if (fread(t.raw.data(), 1, 16, f) != 16) { set_error("vitx_model_load: tensor '%s' is truncated", t.name.c_str()); return VITX_ERR_IO; }
            float a[4]; memcpy(a, t.raw.data(), 16);
            if (a[0] != (float)VITX_GLU_SWIGLU) { set_error("vitx_model_load: tensor 'glu' names kind %g: only 1 (SwiGLU) exists", (double)a[0]); return VITX_ERR_FORMAT; }
            if (!(a[1] >= 64.0f) || a[1] > 16777216.0f || a[1] != floorf(a[1]) || (int64_t)a[1] % 64) {
                set_error("vitx_model_load: tensor 'glu' carries the hidden width %g: it must be a whole number, at least 64 and a multiple of 64 (the GEMMs' K step)", (double)a[1]);
                return VITX_ERR_FORMAT;
            }
            if (a[2] != 0.0f || a[3] != 0.0f) { set_error("vitx_model_load: tensor 'glu' has reserved slots {%g, %g}: they must be 0", (double)a[2], (double)a[3]); return VITX_ERR_FORMAT; }
            m.glu_kind = (int)a[0]; m.glu_width = (int)a[1];
            const int64_t D = hp.hidden_size, F = m.glu_width;
            for (int i = 0; i < hp.num_hidden_layers; ++i) {
                const std::string p = "blocks." + std::to_string(i) + ".mlp.";
                expect[p + "fc1.weight"] = {{D, 2 * F, 1, 1}, 1}; expect[p + "fc1.bias"] = {{2 * F, 1, 1, 1}, 0};
                expect[p + "fc2.weight"] = {{F, D, 1, 1}, 1};
            }
            m.index[t.name] = (int)m.tensors.size();
            m.tensors.push_back(std::move(t));
            ++n_optional;
            continue;
        }
        if (t.name == "preproc") {                                   // optional: f32 [16], the model's own preprocessing (include/vitx.h "each model's own preprocessing")
            if (m.index.count(t.name)) { set_error("vitx_model_load: duplicate tensor '%s'", t.name.c_str()); return VITX_ERR_FORMAT; }
            if (ttype != T_F32 || n_dims != 1 || t.ne[0] != 16) {
                set_error("vitx_model_load: tensor 'preproc' must be f32 [16]: got type %d, %d dims [%lld, ..]", ttype, n_dims, (long long)t.ne[0]);
                return VITX_ERR_FORMAT;
            }
            t.raw.resize(64);
            if (fread(t.raw.data(), 1, 64, f) != 64) { set_error("vitx_model_load: tensor '%s' is truncated", t.name.c_str()); return VITX_ERR_IO; }
            float a[16]; memcpy(a, t.raw.data(), 64);
            if (const char *bad = pp_from_slots(a, m.preproc)) { set_error("vitx_model_load: tensor 'preproc': %s", bad); return VITX_ERR_FORMAT; }
            const int side = m.preproc.crop ? m.preproc.crop : m.preproc.resize_a;
            if (side != hp.img_size) { set_error("vitx_model_load: tensor 'preproc' describes a %d x %d output, the model takes %d x %d", side, side, hp.img_size, hp.img_size); return VITX_ERR_FORMAT; }
            m.has_preproc = true;
            m.index[t.name] = (int)m.tensors.size();
            m.tensors.push_back(std::move(t));
            ++n_optional;
            continue;
        }
        if (t.name == "pre_norm.weight" || t.name == "pre_norm.bias") {   // optional pair: LayerNorm of the token rows in front of layer 0, f32 [D]
            if (m.index.count(t.name)) { set_error("vitx_model_load: duplicate tensor '%s'", t.name.c_str()); return VITX_ERR_FORMAT; }
            if (ttype != T_F32 || n_dims != 1 || t.ne[0] != hp.hidden_size) {
                set_error("vitx_model_load: tensor '%s' must be f32 [%d]: got type %d, %d dims [%lld, ..]", t.name.c_str(), hp.hidden_size, ttype, n_dims, (long long)t.ne[0]);
                return VITX_ERR_FORMAT;
            }
            const size_t nbytes = (size_t)t.nelements() * 4;
            t.raw.resize(nbytes);
            if (fread(t.raw.data(), 1, nbytes, f) != nbytes) { set_error("vitx_model_load: tensor '%s' is truncated", t.name.c_str()); return VITX_ERR_IO; }
            m.index[t.name] = (int)m.tensors.size();
            m.tensors.push_back(std::move(t));
            ++n_optional;
            continue;
        }
        const Expect *known = nullptr;
        bool is_pool = false;
        if (auto it = expect.find(t.name); it != expect.end()) known = &it->second;
        else if (auto ip = pool_expect.find(t.name); ip != pool_expect.end()) { known = &ip->second; is_pool = true; }
        if (!known) { set_error("vitx_model_load: unknown tensor '%s' in model file", t.name.c_str()); return VITX_ERR_FORMAT; }
        if (m.index.count(t.name)) { set_error("vitx_model_load: duplicate tensor '%s'", t.name.c_str()); return VITX_ERR_FORMAT; }
        Expect ex = *known;
        if (is_pool) ++n_pool;
        if (t.name.compare(0, 7, "blocks.") == 0) seen_block = true;
        // attn_pool.latent is [1][1][D] (ggml dims [D, 1, 1]); a model without a class token has a pos_embed of g^2 rows (checked against attn_pool.* below)
        if (t.name == "token_embed.weight" && n_dims == 2) { ex.ne[1] = t.ne[1]; m.vocab = (int)t.ne[1]; }      // V: any row count
        if (!text && t.name == "pos_embed" && t.ne[1] == ex.ne[1] - 1 && t.ne[1] >= 1) { ex.ne[1] -= 1; pos_no_cls = true; }
        // ViTSTR files (extensions/vitstr.cpp/vitstr.cpp:482) carry a ONE-channel patch kernel [P, P, 1, D]: same format otherwise
        if (t.name == "patch_embed.proj.weight" && t.ne[2] == 1 && t.ne[0] == ex.ne[0] && t.ne[1] == ex.ne[1] && t.ne[3] == ex.ne[3]) { ex.ne[2] = 1; m.in_chans = 1; }
        // a head over concat(cls, mean of the patch tokens) has rows of 2 D (VITX_POOL_CLS_MEAN); any other row length fails the shape check below
        if (!text && t.name == "head.weight" && t.ne[0] == 2 * ex.ne[0] && t.ne[1] == ex.ne[1] && t.ne[2] == 1 && t.ne[3] == 1) { ex.ne[0] *= 2; m.head_pool = VITX_POOL_CLS_MEAN; }
        const int64_t want = ex.ne[0] * ex.ne[1] * ex.ne[2] * ex.ne[3];
        if (t.nelements() != want) { set_error("vitx_model_load: tensor '%s' has wrong size in model file: got %lld, expected %lld", t.name.c_str(), (long long)t.nelements(), (long long)want); return VITX_ERR_FORMAT; }
        if (t.ne[0] != ex.ne[0] || t.ne[1] != ex.ne[1] || t.ne[2] != ex.ne[2] || t.ne[3] != ex.ne[3]) {
            set_error("vitx_model_load: tensor '%s' has wrong shape in model file: got [%lld, %lld, %lld, %lld], expected [%lld, %lld, %lld, %lld]", t.name.c_str(),
                      (long long)t.ne[0], (long long)t.ne[1], (long long)t.ne[2], (long long)t.ne[3], (long long)ex.ne[0], (long long)ex.ne[1], (long long)ex.ne[2], (long long)ex.ne[3]);
            return VITX_ERR_FORMAT;
        }
        const int bb = type_block_bytes(ttype), be = type_block_elems(ttype);
        if (!bb) { set_error("vitx_model_load: unknown ftype %d in model file", ttype); return VITX_ERR_FORMAT; }
        if (be > 1 && t.ne[0] % 64) { set_error("vitx_model_load: quantised tensor '%s' needs ne[0] %% 64 == 0", t.name.c_str()); return VITX_ERR_FORMAT; }
        // the declared type of each slot decides the expected byte size (vit.cpp:680-685)
        const bool type_ok = (ex.cls == 0) ? (ttype == T_F32) : (ex.cls == 2 || ex.cls == 3) ? (ttype == T_F16 || ttype == T_F32) : (ttype == hp.ftype);
        if (!type_ok) { set_error("vitx_model_load: tensor '%s' has wrong size in model file (type %d not allowed for this slot, file ftype %d)", t.name.c_str(), ttype, hp.ftype); return VITX_ERR_FORMAT; }
        const size_t nbytes = (size_t)(t.nelements() / be) * bb;
        t.raw.resize(nbytes);
        if (fread(t.raw.data(), 1, nbytes, f) != nbytes) { set_error("vitx_model_load: tensor '%s' is truncated", t.name.c_str()); return VITX_ERR_IO; }
        m.index[t.name] = (int)m.tensors.size();
        m.tensors.push_back(std::move(t));
    }
    if ((m.find("pre_norm.weight") != nullptr) != (m.find("pre_norm.bias") != nullptr)) {
        set_error("vitx_model_load: tensor '%s' has no partner: pre_norm.weight and pre_norm.bias come together", m.find("pre_norm.weight") ? "pre_norm.weight" : "pre_norm.bias");
        return VITX_ERR_FORMAT;
    }
    m.has_pre_norm = m.find("pre_norm.weight") != nullptr;
    if (text) {
        // a text tower: every expected tensor and `arch`; nothing an image front or head brings
        for (const auto &kv : expect)
            if (!m.find(kv.first)) { set_error("vitx_model_load: text-tower file: tensor '%s' is missing", kv.first.c_str()); return VITX_ERR_FORMAT; }
        if (!m.find("arch")) { set_error("vitx_model_load: text-tower file: tensor 'arch' = {activation, eps, causal, eos + 1} is missing"); return VITX_ERR_FORMAT; }
        for (const char *n : {"pre_norm.weight", "preproc", "reg_token"})
            if (m.find(n)) { set_error("vitx_model_load: text-tower file: tensor '%s' belongs to image files", n); return VITX_ERR_FORMAT; }
        if (m.eos >= m.vocab) { set_error("vitx_model_load: text-tower file: eos token %d is not below the vocabulary size %d", m.eos, m.vocab); return VITX_ERR_FORMAT; }
        if (m.tensors.size() != expect.size() + (size_t)n_optional) { set_error("vitx_model_load: model file has %d tensors, but %d tensors were expected", (int)m.tensors.size(), (int)(expect.size() + (size_t)n_optional)); return VITX_ERR_FORMAT; }
        return VITX_OK;
    }
    if (m.has_preproc && m.in_chans == 1) { set_error("vitx_model_load: tensor 'preproc' in a one-channel (ViTSTR) file: its preprocessing is fixed"); return VITX_ERR_FORMAT; }
    if (!m.has_preproc) m.preproc = pp_default(hp.img_size);
    // the attention-pooling head: all thirteen tensors, no class or register token, a position table without a class row -- or none of it
    const bool has_cls = m.find("cls_token") != nullptr;
    if (n_pool) {
        if (m.rope_kind) { set_error("vitx_model_load: tensor 'rope' together with attn_pool.*: the attention-pooling head has no rotary form"); return VITX_ERR_FORMAT; }
        if (m.glu_kind) { set_error("vitx_model_load: tensor 'glu' together with attn_pool.*: the attention-pooling head's MLP has no gated form"); return VITX_ERR_FORMAT; }
        for (const auto &kv : pool_expect)
            if (!m.find(kv.first)) { set_error("vitx_model_load: the attention-pooling head is incomplete: tensor '%s' is missing (%d of %d attn_pool.* tensors)", kv.first.c_str(), n_pool, (int)pool_expect.size()); return VITX_ERR_FORMAT; }
        if (has_cls || m.num_registers) { set_error("vitx_model_load: attn_pool.* together with '%s': a model with the attention-pooling head has no class or register token", has_cls ? "cls_token" : "reg_token"); return VITX_ERR_FORMAT; }
        if (!pos_no_cls && m.find("pos_embed")) { set_error("vitx_model_load: tensor 'pos_embed' has a class row, but the file has attn_pool.* and no class token"); return VITX_ERR_FORMAT; }
        if (m.head_pool != VITX_POOL_CLS) { set_error("vitx_model_load: attn_pool.* together with a [C][2 D] head: the head of such a model reads the pooled embedding [D]"); return VITX_ERR_FORMAT; }
        m.head_pool = VITX_POOL_MAP;
    } else {
        if (!has_cls) { set_error("vitx_model_load: tensor 'cls_token' is missing (only a file with the attn_pool.* tensors has no class token)"); return VITX_ERR_FORMAT; }
        if (pos_no_cls) { set_error("vitx_model_load: tensor 'pos_embed' has no class row, but the file has a class token"); return VITX_ERR_FORMAT; }
    }
    const size_t n_expect = expect.size() - (n_pool ? 1 : 0) + (size_t)n_pool + (m.num_registers ? 1 : 0) + (size_t)n_optional;
    if (m.tensors.size() != n_expect) {
        set_error("vitx_model_load: model file has %d tensors, but %d tensors were expected", (int)m.tensors.size(), (int)n_expect);
        return VITX_ERR_FORMAT;
    }
    return VITX_OK;
}

}  // namespace vitx

extern "C" {

const char *vitx_status_str(int s) {
    switch (s) {
    case VITX_OK: return "ok"; case VITX_ERR_IO: return "io error"; case VITX_ERR_FORMAT: return "bad model file";
    case VITX_ERR_ARG: return "invalid argument"; case VITX_ERR_HIP: return "HIP error"; case VITX_ERR_UNSUPPORTED: return "unsupported model shape";
    case VITX_ERR_NOMEM: return "out of memory"; default: return "unknown status";
    }
}
const char *vitx_last_error(void) { return vitx::last_error(); }

int vitx_model_load(const char *path, vitx_model **out) {
    if (!path || !out) { vitx::set_error("vitx_model_load: NULL argument"); return VITX_ERR_ARG; }
    *out = nullptr;
    std::unique_ptr<vitx_model> m(new (std::nothrow) vitx_model());
    if (!m) return VITX_ERR_NOMEM;
    const int rc = vitx::load_impl(path, *m);
    if (rc != VITX_OK) return rc;
    static std::atomic<uint64_t> next_uid{1};
    m->uid = next_uid.fetch_add(1);
    *out = m.release();
    return VITX_OK;
}
void vitx_model_free(vitx_model *m) { delete m; }
uint64_t vitx_model_uid(const vitx_model *m) { return m ? m->uid : 0; }
int vitx_model_hparams(const vitx_model *m, vitx_hparams *out) {
    if (!m || !out) return VITX_ERR_ARG;
    *out = m->hp; return VITX_OK;
}
int vitx_model_kind(const vitx_model *m) { return m ? m->kind : 0; }
int vitx_model_text_info(const vitx_model *m, int *V, int *T, int *causal, int *eos) {
    if (!m || m->kind != VITX_KIND_TEXT) { vitx::set_error("vitx_model_text_info: not a text-tower model"); return VITX_ERR_ARG; }
    if (V) *V = m->vocab;
    if (T) *T = m->hp.img_size;
    if (causal) *causal = m->causal;
    if (eos) *eos = m->eos;
    return VITX_OK;
}
int vitx_model_text_zs(const vitx_model *m, int *kind, float *scale, float *bias) {
    if (!m || !m->has_zs) return 0;
    if (kind) *kind = m->zs_kind;
    if (scale) *scale = m->zs_scale;
    if (bias) *bias = m->zs_bias;
    return 1;
}
int vitx_model_num_labels(const vitx_model *m) { return m ? (int)m->id2label.size() : 0; }
int vitx_model_in_channels(const vitx_model *m) { return m ? m->in_chans : 0; }
int vitx_model_num_registers(const vitx_model *m) { return m ? m->num_registers : 0; }
int vitx_model_head_pool(const vitx_model *m) { return m ? m->head_pool : 0; }
int vitx_model_num_prefix(const vitx_model *m) { return m ? (m->head_pool == VITX_POOL_MAP ? 0 : 1 + m->num_registers) : 0; }
// u_h = Wk_h^T q_h / sqrt(d), q = Wq latent + bq, in double from the file's f32 decode; rounded once to f32 (include/vitx.h)
int vitx_model_pool_query(const vitx_model *m, float *out) {
    if (!m || !out) { vitx::set_error("vitx_model_pool_query: NULL argument"); return VITX_ERR_ARG; }
    if (m->head_pool != VITX_POOL_MAP) { vitx::set_error("vitx_model_pool_query: the model has no attention-pooling head"); return VITX_ERR_ARG; }
    const int D = m->hp.hidden_size, H = m->hp.num_attention_heads, d = D / H;
    auto dec = [&](const char *n) { const vitx::HostTensor *t = m->find(n); std::vector<float> v((size_t)t->nelements()); t->decode_f32(v.data()); return v; };
    const std::vector<float> lat = dec("attn_pool.latent"), wq = dec("attn_pool.q.weight"), bq = dec("attn_pool.q.bias"), wkv = dec("attn_pool.kv.weight");
    std::vector<double> q((size_t)D);
    for (int i = 0; i < D; ++i) { double s = 0.0; for (int k = 0; k < D; ++k) s += (double)wq[(size_t)i * D + k] * (double)lat[k]; q[i] = s + (double)bq[i]; }
    const double scale = 1.0 / sqrt((double)d);
    for (int h = 0; h < H; ++h)
        for (int k = 0; k < D; ++k) {
            double s = 0.0;
            for (int j = 0; j < d; ++j) s += (double)wkv[(size_t)(h * d + j) * D + k] * q[h * d + j];      // the K half: rows 0 .. D-1 of kv.weight
            out[(size_t)h * D + k] = (float)(s * scale);
        }
    return VITX_OK;
}
int vitx_model_rope(const vitx_model *m, int *kind, float *theta) {
    if (!m || !m->rope_kind) return 0;
    if (kind) *kind = m->rope_kind;
    if (theta) *theta = m->rope_theta;
    return 1;
}
int vitx_model_glu(const vitx_model *m, int *kind, int *width) {
    if (!m || !m->glu_kind) return 0;
    if (kind) *kind = m->glu_kind;
    if (width) *width = m->glu_width;
    return 1;
}
// DINOv3's axial table (include/vitx.h "rotary position embeddings"): double throughout, cos / sin rounded once to f32
int vitx_model_rope_table(const vitx_model *m, int gh, int gw, float *cos_out, float *sin_out) {
    if (!m || !cos_out || !sin_out) { vitx::set_error("vitx_model_rope_table: NULL argument"); return VITX_ERR_ARG; }
    if (!m->rope_kind) { vitx::set_error("vitx_model_rope_table: the model has no `rope` tensor"); return VITX_ERR_ARG; }
    if (gh <= 0 || gw <= 0 || (int64_t)gh * gw > (1 << 24)) { vitx::set_error("vitx_model_rope_table: grid %d x %d is not a positive size", gh, gw); return VITX_ERR_ARG; }
    const int hd = m->hp.hidden_size / m->hp.num_attention_heads, q = hd / 4, half = hd / 2;
    const double two_pi = 6.283185307179586476925286766559;
    std::vector<double> inv((size_t)q);
    for (int j = 0; j < q; ++j) inv[j] = pow((double)m->rope_theta, -4.0 * j / hd);
    for (int y = 0; y < gh; ++y)
        for (int x = 0; x < gw; ++x) {
            const double cy = 2.0 * (y + 0.5) / gh - 1.0, cx = 2.0 * (x + 0.5) / gw - 1.0;
            float *co = cos_out + ((size_t)y * gw + x) * half, *so = sin_out + ((size_t)y * gw + x) * half;
            for (int j = 0; j < q; ++j) {
                const double ay = two_pi * cy * inv[j], ax = two_pi * cx * inv[j];
                co[j] = (float)cos(ay); so[j] = (float)sin(ay);
                co[q + j] = (float)cos(ax); so[q + j] = (float)sin(ax);
            }
        }
    return VITX_OK;
}
int vitx_model_activation(const vitx_model *m) { return m ? m->activation : 0; }
int vitx_model_has_pre_norm(const vitx_model *m) { return m && m->has_pre_norm ? 1 : 0; }
int vitx_model_has_preproc(const vitx_model *m) { return m && m->has_preproc ? 1 : 0; }
int vitx_model_preproc(const vitx_model *m, vitx_preproc *out) {
    if (!m || !out) return VITX_ERR_ARG;
    *out = m->preproc; return VITX_OK;
}
int vitx_model_seq_len(const vitx_model *m) { return (m && m->in_chans == 1) ? VITX_VITSTR_SEQ_LEN : 0; }
const char *vitx_model_label(const vitx_model *m, int id) {
    if (!m) return nullptr;
    auto it = m->id2label.find(id);
    return it == m->id2label.end() ? nullptr : it->second.c_str();
}
int vitx_model_num_tensors(const vitx_model *m) { return m ? (int)m->tensors.size() : 0; }
int vitx_model_tensor_info(const vitx_model *m, int i, const char **name, int32_t *type, int64_t ne[4], size_t *nbytes) {
    if (!m || i < 0 || i >= (int)m->tensors.size()) return VITX_ERR_ARG;
    const vitx::HostTensor &t = m->tensors[i];
    if (name) *name = t.name.c_str();
    if (type) *type = t.type;
    if (ne) for (int k = 0; k < 4; ++k) ne[k] = t.ne[k];
    if (nbytes) *nbytes = t.raw.size();
    return VITX_OK;
}
int vitx_model_tensor_f32(const vitx_model *m, int i, float *out, size_t n) {
    if (!m || !out || i < 0 || i >= (int)m->tensors.size() || n != (size_t)m->tensors[i].nelements()) return VITX_ERR_ARG;
    m->tensors[i].decode_f32(out); return VITX_OK;
}

int vitx_topk(const float *probs, int C, int k, int32_t *idx, float *p) {
    if (!probs || !idx || C <= 0 || k <= 0) return VITX_ERR_ARG;
    if (k > C) k = C;
    // descending by probability (vit.cpp:1053-1057); ties broken by lower class id for determinism.  NaN entries come last, by class id:
    // with them left to `>` and `==` the comparison is no strict weak order and std::partial_sort is undefined.  topk_kernel
    // (softmax_topk.hip) follows the same order.
    std::vector<int32_t> order((size_t)C);
    for (int i = 0; i < C; ++i) order[i] = i;
    std::partial_sort(order.begin(), order.begin() + k, order.end(), [&](int32_t a, int32_t b) {
        const float pa = probs[a], pb = probs[b];
        const bool na = pa != pa, nb = pb != pb;
        if (na || nb) return na == nb ? a < b : nb;
        return pa > pb || (pa == pb && a < b);
    });
    for (int i = 0; i < k; ++i) { idx[i] = order[i]; if (p) p[i] = probs[order[i]]; }
    return VITX_OK;
}

}  // extern "C"
