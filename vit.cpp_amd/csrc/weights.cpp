// weights.cpp -- upload of a loaded model's weights into HBM in the MFMA operand type, and the registry that shares one device copy between the contexts
// that ask for the same WeightSpec.  Every quantity an upload reads is derived here from the model and the spec: no context type is seen.
#include <string.h>

#include <iterator>
#include <map>
#include <mutex>
#include <string>
#include <tuple>

#include "weights.h"

namespace vitx {

std::vector<uint16_t> operand_matrix_host(int dtype, const float *f, const uint16_t *bits, int Nrows, int K, int n_pad, int k_pad, int patch_P, int patch_Cin) {
    std::vector<uint16_t> h((size_t)n_pad * k_pad, 0);
    for (int n = 0; n < Nrows; ++n) {
        if (bits) { memcpy(&h[(size_t)n * k_pad], bits + (size_t)n * K, (size_t)K * 2); continue; }
        for (int k = 0; k < K; ++k) h[(size_t)n * k_pad + k] = dtype == VITX_F16 ? f32_to_f16_bits(f[(size_t)n * K + k]) : f32_to_bf16_bits(f[(size_t)n * K + k]);
    }
    if (patch_P > 0) { std::vector<uint16_t> hp(h.size(), 0); patch_embed_permute_k(h.data(), hp.data(), Nrows, patch_Cin, patch_P, k_pad); h.swap(hp); }
    return h;
}

int open_device(const char *api, int device, const Tuning **tune) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("%s: no HIP device available (this engine has no CPU fallback)", api); return VITX_ERR_HIP; }
    if (device < 0 || device >= ndev) { set_error("%s: device %d out of range (%d devices)", api, device, ndev); return VITX_ERR_ARG; }
    HIP_TRY(hipSetDevice(device));
    if (!(*tune = tuning_for_device(device))) { set_error("%s: kernel bring-up on device %d failed: %s", api, device, hipGetErrorString(hipGetLastError())); return VITX_ERR_HIP; }
    return VITX_OK;
}

namespace {

struct Upload {                  // one upload in progress: the set being filled and what its layouts follow from
    const vitx_model *m;
    WeightSet &ws;
    int dtype;                   // the operand type: VITX_BF16 in an MXFP8 set
    bool mx, quant_on_device;
    int D, L, tn;
    const HostTensor *T(const std::string &n) const { return m->find(n); }
};

// host bytes -> a device allocation of the set; `counts`: they are weight-matrix bytes (WeightSet::weight_bytes)
int upload_bytes(const Upload &u, void **out, const void *h, size_t bytes, bool counts) {
    int rc = u.ws.alloc(out, bytes);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(*out, h, bytes, hipMemcpyHostToDevice));
    if (counts) u.ws.weight_bytes += bytes;
    return VITX_OK;
}

// f32 vector -> device f32 (padded with zeros to n_pad)
int upload_f32(const Upload &u, const HostTensor *t, float **out, size_t n_pad = 0) {
    std::vector<float> h((size_t)t->nelements());
    t->decode_f32(h.data());
    if (n_pad > h.size()) h.resize(n_pad, 0.0f);
    return upload_bytes(u, (void **)out, h.data(), h.size() * 4, false);
}

// [N][K] matrix -> operand type, rows padded to n_pad, cols to k_pad (zeros).  f16 file data is
// forwarded bit-exact in F16 mode; everything else is decoded to f32 and rounded once (RNE).
// patch_P > 0: the patch-embedding kernel [D][Cin * P * P]: its K axis is permuted to the image's memory order (patch_embed.hip)
int upload_matrix(const Upload &u, const HostTensor *t, int Nrows, int K, int n_pad, int k_pad, void **out, int patch_P = 0, int patch_Cin = 0) {
    const bool exact = t->type == T_F16 && u.dtype == VITX_F16;
    std::vector<float> f(exact ? 0 : (size_t)Nrows * K);
    if (!exact) t->decode_f32(f.data());
    const std::vector<uint16_t> h = operand_matrix_host(u.dtype, f.data(), exact ? (const uint16_t *)t->raw.data() : nullptr, Nrows, K, n_pad, k_pad, patch_P, patch_Cin);
    return upload_bytes(u, out, h.data(), h.size() * 2, true);
}

// Quantised [N][K] matrix -> device, still in block form.  Returns VITX_OK with q->blocks == nullptr when the tensor is not a
// block type (the caller then uploads the expanded matrix).
int upload_quant(const Upload &u, const HostTensor *t, int Nrows, int K, int n_pad, QuantW *q) {
    const int bb = type_block_bytes(t->type);
    if (t->type == T_F32 || t->type == T_F16 || !bb || K % 32) return VITX_OK;
    const size_t nbk = (size_t)K / 32;
    q->type = t->type; q->N = Nrows; q->K = K; q->n_pad = n_pad;
    if (t->type != T_Q4_0) return upload_bytes(u, &q->blocks, t->raw.data(), (size_t)Nrows * nbk * bb, true);
    // q4_0: split planes, rows padded (zero scales -> the pad rows expand to zeros)
    std::vector<uint8_t> qs((size_t)n_pad * nbk * 16, 0);
    std::vector<uint16_t> ds((size_t)n_pad * nbk, 0);
    const uint8_t *src = t->raw.data();
    for (size_t b = 0; b < (size_t)Nrows * nbk; ++b) { memcpy(&ds[b], src + b * 18, 2); memcpy(&qs[b * 16], src + b * 18 + 2, 16); }
    int rc = upload_bytes(u, &q->blocks, qs.data(), qs.size(), true);
    return rc ? rc : upload_bytes(u, (void **)&q->scales, ds.data(), ds.size() * 2, true);
}

// A 2-D "*weight" tensor: block types stay quantised on the device (q), everything else is uploaded expanded (dense).
int upload_weight(const Upload &u, const HostTensor *t, int Nrows, int K, int n_pad, void **dense, QuantW *q) {
    *dense = nullptr;
    if (u.quant_on_device) { int rc = upload_quant(u, t, Nrows, K, n_pad, q); if (rc) return rc; }
    if (q->blocks) return VITX_OK;
    return upload_matrix(u, t, Nrows, K, n_pad, K, dense);
}

// [N][K] matrix -> MX operand (VITX_MXFP8): the f32 decode of any file type, encoded once on the host; rows N..n_pad are zero blocks
int upload_mx(const Upload &u, const HostTensor *t, int Nrows, int K, int n_pad, MxW *w) {
    w->N = Nrows; w->K = K; w->n_pad = n_pad; w->k_pad = mx_k_pad(K);
    std::vector<float> f((size_t)n_pad * K, 0.0f);
    t->decode_f32(f.data());
    std::vector<uint8_t> q((size_t)n_pad * w->k_pad), sc((size_t)n_pad * (w->k_pad / kMxBlock));
    mxfp8_encode_rows(f.data(), n_pad, K, w->k_pad, q.data(), sc.data());
    int rc = upload_bytes(u, (void **)&w->q, q.data(), q.size(), true);
    return rc ? rc : upload_bytes(u, (void **)&w->s, sc.data(), sc.size(), true);
}

// The attention-pooling head (VITX_POOL_MAP; include/vitx.h): the folded probe u, the V half of kv.*, proj, norm, fc1, fc2.  The matrices are f32
// or f16 in the file, never blocks.
int upload_map_head(const Upload &u) {
    WeightSet &ws = u.ws;
    const int D = u.D, tn = u.tn;
    int rc;
    std::vector<float> pu((size_t)u.m->hp.num_attention_heads * D);
    if ((rc = vitx_model_pool_query(u.m, pu.data()))) return rc;
    if ((rc = upload_bytes(u, (void **)&ws.map_u, pu.data(), pu.size() * 4, false))) return rc;
    // V: rows D .. 2 D of kv.weight, elements D .. 2 D of kv.bias; 128 zero rows behind them: the value projection of the last head reads a whole column tile
    std::vector<float> f((size_t)2 * D * D), fb((size_t)2 * D);
    u.T("attn_pool.kv.weight")->decode_f32(f.data()); u.T("attn_pool.kv.bias")->decode_f32(fb.data());
    const int v_pad = round_up(D, tn) + 128;
    const std::vector<uint16_t> hv = operand_matrix_host(u.dtype, f.data() + (size_t)D * D, nullptr, D, D, v_pad, D, 0, 0);
    if ((rc = upload_bytes(u, &ws.map_v_w, hv.data(), hv.size() * 2, true))) return rc;
    std::vector<float> vb(fb.begin() + D, fb.end());
    vb.resize((size_t)v_pad, 0.0f);
    if ((rc = upload_bytes(u, (void **)&ws.map_v_b, vb.data(), vb.size() * 4, false))) return rc;
    if ((rc = upload_f32(u, u.T("attn_pool.proj.bias"), &ws.map_proj_b, round_up(D, tn)))) return rc;
    if ((rc = upload_f32(u, u.T("attn_pool.norm.weight"), &ws.map_ln_w))) return rc;
    if ((rc = upload_f32(u, u.T("attn_pool.norm.bias"), &ws.map_ln_b))) return rc;
    if ((rc = upload_f32(u, u.T("attn_pool.mlp.fc1.bias"), &ws.map_fc1_b, round_up(4 * D, tn)))) return rc;
    if ((rc = upload_f32(u, u.T("attn_pool.mlp.fc2.bias"), &ws.map_fc2_b, round_up(D, tn)))) return rc;
    if ((rc = upload_matrix(u, u.T("attn_pool.proj.weight"), D, D, round_up(D, tn), D, &ws.map_proj_w))) return rc;
    if ((rc = upload_matrix(u, u.T("attn_pool.mlp.fc1.weight"), 4 * D, D, round_up(4 * D, tn), D, &ws.map_fc1_w))) return rc;
    if ((rc = upload_matrix(u, u.T("attn_pool.mlp.fc2.weight"), D, 4 * D, round_up(D, tn), 4 * D, &ws.map_fc2_w))) return rc;
    return VITX_OK;
}

// The transformer blocks blocks.{i}.* of a model file: the same twelve tensors per layer in an image file and a text file
int upload_blocks(const Upload &u) {
    const int D = u.D, tn = u.tn, F = u.m->mlp_hidden(), F1 = u.m->mlp_fc1_rows();
    int rc;
    u.ws.layers.resize(u.L);
    for (int i = 0; i < u.L; ++i) {
        const std::string p = "blocks." + std::to_string(i) + ".";
        LayerW &w = u.ws.layers[i];
        if ((rc = upload_f32(u, u.T(p + "norm1.weight"), &w.ln1_w))) return rc;
        if ((rc = upload_f32(u, u.T(p + "norm1.bias"), &w.ln1_b))) return rc;
        if ((rc = upload_f32(u, u.T(p + "norm2.weight"), &w.ln2_w))) return rc;
        if ((rc = upload_f32(u, u.T(p + "norm2.bias"), &w.ln2_b))) return rc;
        if ((rc = upload_f32(u, u.T(p + "attn.qkv.bias"), &w.qkv_b, round_up(3 * D, tn)))) return rc;
        if ((rc = upload_f32(u, u.T(p + "attn.proj.bias"), &w.proj_b, round_up(D, tn)))) return rc;
        if ((rc = upload_f32(u, u.T(p + "mlp.fc1.bias"), &w.fc1_b, round_up(F1, tn)))) return rc;
        if ((rc = upload_f32(u, u.T(p + "mlp.fc2.bias"), &w.fc2_b, round_up(D, tn)))) return rc;
        // a block's matrix: an MX operand in an MXFP8 set (but proj, which stays bf16), else blocks or the expanded operand type
        auto matrix = [&](const char *name, int k, int N, int K, void **dense) {
            return u.mx && k != W_PROJ ? upload_mx(u, u.T(p + name), N, K, round_up(N, 128), &w.mx[k]) : upload_weight(u, u.T(p + name), N, K, round_up(N, tn), dense, &w.q[k]);
        };
        if ((rc = matrix("attn.qkv.weight", W_QKV, 3 * D, D, &w.qkv_w))) return rc;
        if ((rc = matrix("mlp.fc1.weight", W_FC1, F1, D, &w.fc1_w))) return rc;
        if ((rc = matrix("mlp.fc2.weight", W_FC2, D, F, &w.fc2_w))) return rc;
        if ((rc = matrix("attn.proj.weight", W_PROJ, D, D, &w.proj_w))) return rc;
    }
    return VITX_OK;
}

// What follows the front of both kinds of file: blocks, final norm, the attention-pooling head of a `map` model, the head (K = head_k)
int upload_rest(const Upload &u, bool map, int head_k) {
    WeightSet &ws = u.ws;
    const int C_pad = head_cols_pad(u.m);
    int rc;
    if ((rc = upload_blocks(u))) return rc;
    if ((rc = upload_f32(u, u.T("norm.weight"), &ws.norm_w))) return rc;
    if ((rc = upload_f32(u, u.T("norm.bias"), &ws.norm_b))) return rc;
    if (map && (rc = upload_map_head(u))) return rc;
    if ((rc = upload_f32(u, u.T("head.bias"), &ws.head_b, C_pad))) return rc;
    return upload_weight(u, u.T("head.weight"), u.m->hp.num_classes, head_k, C_pad, &ws.head_w, &ws.head_q);
}

// a text tower (text_forward.cpp): the token table as filed (a gather reads it), the position table, the same blocks, final norm, projection
int upload_text(const Upload &u) {
    WeightSet &ws = u.ws;
    int rc;
    const HostTensor *tok = u.T("token_embed.weight");
    ws.tok_f16 = tok->type == T_F16;
    if ((rc = upload_bytes(u, &ws.tok, tok->raw.data(), tok->raw.size(), true))) return rc;
    if ((rc = upload_f32(u, u.T("pos_embed"), &ws.pos))) return rc;
    return upload_rest(u, false, u.D);
}

int upload_image(const Upload &u) {
    const vitx_model *m = u.m;
    WeightSet &ws = u.ws;
    const int D = u.D, tn = u.tn;
    const bool pool = m->head_pool == VITX_POOL_CLS_MEAN, map = m->head_pool == VITX_POOL_MAP;
    int rc;
    if (!map && (rc = upload_f32(u, u.T("cls_token"), &ws.cls))) return rc;
    if (m->num_registers && (rc = upload_f32(u, u.T("reg_token"), &ws.reg))) return rc;
    if ((rc = upload_f32(u, u.T("pos_embed"), &ws.pos))) return rc;
    if (m->has_pre_norm && ((rc = upload_f32(u, u.T("pre_norm.weight"), &ws.pre_w)) || (rc = upload_f32(u, u.T("pre_norm.bias"), &ws.pre_b)))) return rc;
    if ((rc = upload_f32(u, u.T("patch_embed.proj.bias"), &ws.pe_b, round_up(D, tn)))) return rc;
    if ((rc = upload_matrix(u, u.T("patch_embed.proj.weight"), D, patch_k(m), round_up(D, tn), patch_k_pad(m), &ws.pe_w, m->hp.patch_size, m->in_chans))) return rc;
    return upload_rest(u, map, pool ? 2 * D : D);
}

}  // namespace

int obtain_weights(const WeightSpec &spec, std::shared_ptr<WeightSet> *out, bool *shared) {
    const vitx_model *m = spec.model;
    static std::mutex wreg_mu;
    static std::map<std::tuple<uint64_t, int, int, int>, std::weak_ptr<WeightSet>> wreg;
    const auto wkey = std::make_tuple(m->uid, spec.device, spec.dtype, spec.quant_on_device ? 1 : 0);
    std::unique_lock<std::mutex> wlock(wreg_mu);           // held through the upload: a second context of the same model waits for the first
    for (auto it = wreg.begin(); it != wreg.end();) it = it->second.expired() ? wreg.erase(it) : std::next(it);      // sets whose last context is gone
    if ((*out = wreg[wkey].lock())) { *shared = true; return VITX_OK; }
    *out = std::make_shared<WeightSet>(spec.device);
    const bool mx = spec.dtype == VITX_MXFP8;              // everything but the MX GEMMs' operands is laid out as in a VITX_BF16 set
    const Upload u{m, **out, mx ? VITX_BF16 : spec.dtype, mx, spec.quant_on_device, m->hp.hidden_size, m->hp.num_hidden_layers, gemm_tile_n()};
    const int rc = m->kind == VITX_KIND_TEXT ? upload_text(u) : upload_image(u);
    if (!rc) wreg[wkey] = *out;   // only a complete upload is registered; the caller frees a partial one by dropping *out
    return rc;                    // (the lock is released here: held through the upload)
}

}  // namespace vitx
