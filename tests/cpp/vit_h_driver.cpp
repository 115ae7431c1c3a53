// vit_h_driver.cpp -- a test driver on the C++ header (vit.cpp_amd/vit.h): runs a script of calls on ONE vit_model / vit_state pair (and one
// vit_text_state) and writes what every call returned as raw little-endian arrays, for tests/test_gpu_vit_h.py and tests/test_cpu_vit_h.py to
// compare with the C ABI.  Not part of libvitx.so.
//
//     vit_h_driver MODEL DATA_DIR SCRIPT OUT_DIR
//
// DATA_DIR holds raw arrays NAME.bin (tests/vit_h_data.py writes them): pixels.bin (f32, the images end to end, HWC) and hw.bin (i32 [images][2] = (h, w))
// are read at start; every other array is named by the step that takes it.  SCRIPT holds one step per line, `op key=value ...` ('#' starts a comment);
// numbers are decimal integers or C hex floats, `-` names an empty array:
//     predict  n= at=                      vit_predict_batch on images at .. at + n - 1
//     pack     n= at=                      vit_pack_batch
//     embed    n= at= flags=               vit_embed_batch
//     zeroshot n= at= topk= bank= K= E= kind= scale= bias=
//     nn       n= at= gallery= G= E= k= source= labels= n_labels= temperature=
//     dense    n= at= weight= bias= K= Dc= layers=a,b out_h= out_w= score=
//     depth    n= at= wp= wc= bias= bins= K= Dc= layers=a,b upsample= min_depth= max_depth= norm= out_h= out_w=
//     text     n= flags= ids=              vit_text_embed_batch on the first n prompts of ids
//     set      dtype= device= img_size= shape=HxW pos_interp= text_dtype= text_device=     (any of them)
//     reload   [path=]                     vit_model_load into the same vit_model again (path: another file)
// After step s it writes OUT_DIR/out_<s>_<name>.bin -- rc (i32) and prediction (f32) always; pairs / counts (per-image sizes), feat, nn_pairs, vote,
// hw, labels, score, depth, text by kind -- and prints one line `STEP s op rc=... key=value ...` with the state of state.ctx, state.pack and the text
// state.  A step whose call returns 1 is a result, not a failure: the exit status is 0 unless the script or the data cannot be read.
#include "vit.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

namespace {

[[noreturn]] void die(const std::string &what) { fprintf(stderr, "vit_h_driver: %s\n", what.c_str()); exit(2); }

std::string g_data, g_out;

template <class T> std::vector<T> load(const std::string &name) {
    std::vector<T> v;
    if (name.empty() || name == "-") return v;
    std::ifstream f(g_data + "/" + name + ".bin", std::ios::binary);
    if (!f) die("cannot read '" + g_data + "/" + name + ".bin'");
    std::string bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (bytes.size() % sizeof(T)) die("'" + name + ".bin' is not a whole number of elements");
    v.resize(bytes.size() / sizeof(T));
    if (!v.empty()) memcpy(v.data(), bytes.data(), bytes.size());
    return v;
}

void dump(int step, const char *name, const void *p, size_t bytes) {
    const std::string path = g_out + "/out_" + std::to_string(step) + "_" + name + ".bin";
    std::ofstream f(path, std::ios::binary);
    if (bytes) f.write((const char *)p, (std::streamsize)bytes);
    if (!f) die("cannot write '" + path + "'");
}
template <class T> void dump(int step, const char *name, const std::vector<T> &v) { dump(step, name, v.data(), v.size() * sizeof(T)); }

struct Args {
    std::map<std::string, std::string> kv;
    bool has(const std::string &k) const { return kv.count(k) != 0; }
    std::string s(const std::string &k, const std::string &d = "-") const { auto it = kv.find(k); return it == kv.end() ? d : it->second; }
    long i(const std::string &k, long d = 0) const { return has(k) ? strtol(kv.at(k).c_str(), nullptr, 0) : d; }
    float f(const std::string &k, float d = 0.0f) const { return has(k) ? strtof(kv.at(k).c_str(), nullptr) : d; }
    std::vector<int> list(const std::string &k) const {
        std::vector<int> v;
        std::string t = s(k);
        if (t == "-" || t.empty()) return v;
        std::stringstream ss(t);
        for (std::string e; std::getline(ss, e, ',');) v.push_back(atoi(e.c_str()));
        return v;
    }
};

struct Pair { float v; int32_t i; };
static_assert(sizeof(Pair) == 8, "a pair is written as 8 bytes");

// the pairs of every image end to end, and how many each image has
void dump_pairs(int step, const char *name, const char *counts_name, const std::vector<std::vector<std::pair<float, int>>> &all) {
    std::vector<Pair> flat; std::vector<int32_t> counts;
    for (const auto &p : all) { counts.push_back((int32_t)p.size()); for (const auto &e : p) flat.push_back({e.first, (int32_t)e.second}); }
    dump(step, name, flat); dump(step, counts_name, counts);
}
void dump_rows(int step, const char *name, const char *counts_name, const std::vector<std::vector<float>> &all) {
    std::vector<float> flat; std::vector<int32_t> counts;
    for (const auto &r : all) { counts.push_back((int32_t)r.size()); flat.insert(flat.end(), r.begin(), r.end()); }
    dump(step, name, flat); dump(step, counts_name, counts);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 5) die("usage: vit_h_driver MODEL DATA_DIR SCRIPT OUT_DIR");
    const std::string model_path = argv[1];
    g_data = argv[2]; g_out = argv[4];
    std::ifstream script(argv[3]);
    if (!script) die(std::string("cannot read the script '") + argv[3] + "'");

    // the images: pixels end to end, one (h, w) row each
    const std::vector<float> pixels = load<float>("pixels");
    const std::vector<int32_t> hw = load<int32_t>("hw");
    std::vector<image_f32> images(hw.size() / 2);
    size_t off = 0;
    for (size_t k = 0; k < images.size(); ++k) {
        const int h = hw[2 * k], w = hw[2 * k + 1];
        const size_t fl = (size_t)3 * h * w;
        if (h <= 0 || w <= 0 || off + fl > pixels.size()) die("pixels.bin does not hold the images of hw.bin");
        images[k].nx = w; images[k].ny = h;
        images[k].data.assign(pixels.begin() + off, pixels.begin() + off + fl);
        off += fl;
    }

    vit_model model;
    vit_state state;
    vit_text_state tstate;
    vit_params params;
    if (!vit_model_load(model_path, model)) die("vit_model_load failed for '" + model_path + "'");

    int step = 0;
    for (std::string line; std::getline(script, line);) {
        if (const size_t c = line.find('#'); c != std::string::npos) line.resize(c);
        std::stringstream ss(line);
        std::string op;
        if (!(ss >> op)) continue;
        Args a;
        for (std::string tok; ss >> tok;) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) die("step " + std::to_string(step) + ": '" + tok + "' is not key=value");
            a.kv[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
        const int n = (int)a.i("n", 1);
        const long at = a.i("at", 0);
        if (at < 0 || (n > 0 && (size_t)(at + n) > images.size() && op != "text" && op != "set" && op != "reload")) die("step " + std::to_string(step) + ": images " + std::to_string(at) + " .. are not in hw.bin");
        const image_f32 *imgs = images.empty() ? nullptr : images.data() + at;
        int rc = 0;

        if (op == "set") {
            if (a.has("dtype")) state.dtype = (int)a.i("dtype");
            if (a.has("device")) state.device = (int)a.i("device");
            if (a.has("img_size")) state.img_size = (int)a.i("img_size");
            if (a.has("pos_interp")) state.pos_interp = (int)a.i("pos_interp");
            if (a.has("shape")) { if (sscanf(a.s("shape").c_str(), "%dx%d", &state.img_h, &state.img_w) != 2) die("set shape=HxW"); }
            if (a.has("text_dtype")) tstate.dtype = (int)a.i("text_dtype");
            if (a.has("text_device")) tstate.device = (int)a.i("text_device");
        } else if (op == "reload") {
            rc = vit_model_load(a.s("path", model_path), model) ? 0 : 1;
        } else if (op == "predict" || op == "pack") {
            std::vector<std::vector<std::pair<float, int>>> preds;
            rc = op == "predict" ? vit_predict_batch(model, state, imgs, n, params, preds) : vit_pack_batch(model, state, imgs, n, preds);
            dump_pairs(step, "pairs", "counts", preds);
        } else if (op == "embed") {
            std::vector<std::vector<float>> out;
            rc = vit_embed_batch(model, state, imgs, n, (int)a.i("flags"), out);
            dump_rows(step, "feat", "counts", out);
        } else if (op == "zeroshot") {
            vit_zeroshot_bank bank;
            bank.embeds = load<float>(a.s("bank")); bank.K = (int)a.i("K"); bank.E = (int)a.i("E"); bank.kind = (int)a.i("kind");
            bank.scale = a.f("scale", 1.0f); bank.bias = a.f("bias", 0.0f);
            std::vector<std::vector<std::pair<float, int>>> out;
            rc = vit_zeroshot_batch(model, state, imgs, n, bank, out, (int)a.i("topk", 5));
            dump_pairs(step, "pairs", "counts", out);
        } else if (op == "nn") {
            vit_nn_gallery g;
            g.embeds = load<float>(a.s("gallery")); g.G = a.i("G"); g.E = (int)a.i("E"); g.k = (int)a.i("k", 5); g.source = (int)a.i("source");
            g.labels = load<int32_t>(a.s("labels")); g.n_labels = (int)a.i("n_labels"); g.temperature = a.f("temperature", 0.07f);
            std::vector<vit_nn_result> out;
            rc = vit_nn_batch(model, state, imgs, n, g, out);
            std::vector<std::vector<std::pair<float, int>>> nb; std::vector<std::vector<float>> votes;
            for (const auto &r : out) { nb.push_back(r.neighbours); votes.push_back(r.vote); }
            dump_pairs(step, "nn_pairs", "counts", nb);
            dump_rows(step, "vote", "vote_counts", votes);
        } else if (op == "dense") {
            vit_dense_head h;
            h.weight = load<float>(a.s("weight")); h.bias = load<float>(a.s("bias")); h.K = (int)a.i("K"); h.Dc = (int)a.i("Dc"); h.layers = a.list("layers");
            h.out_h = (int)a.i("out_h"); h.out_w = (int)a.i("out_w"); h.want_score = a.i("score") != 0;
            std::vector<vit_dense_result> out;
            rc = vit_dense_batch(model, state, imgs, n, h, out);
            std::vector<int32_t> shp, counts; std::vector<uint8_t> labels; std::vector<float> score;
            for (const auto &r : out) {
                shp.push_back(r.h); shp.push_back(r.w); counts.push_back((int32_t)r.labels.size()); counts.push_back((int32_t)r.score.size());
                labels.insert(labels.end(), r.labels.begin(), r.labels.end()); score.insert(score.end(), r.score.begin(), r.score.end());
            }
            dump(step, "hw", shp); dump(step, "counts", counts); dump(step, "labels", labels); dump(step, "score", score);
        } else if (op == "depth") {
            vit_depth_head h;
            h.wp = load<float>(a.s("wp")); h.wc = load<float>(a.s("wc")); h.bias = load<float>(a.s("bias")); h.bins = load<float>(a.s("bins"));
            h.K = (int)a.i("K"); h.Dc = (int)a.i("Dc"); h.layers = a.list("layers"); h.upsample = (int)a.i("upsample", 4);
            h.min_depth = a.f("min_depth", 0.001f); h.max_depth = a.f("max_depth", 10.0f); h.norm = a.i("norm") != 0;
            h.out_h = (int)a.i("out_h"); h.out_w = (int)a.i("out_w");
            std::vector<vit_depth_result> out;
            rc = vit_depth_batch(model, state, imgs, n, h, out);
            std::vector<int32_t> shp, counts; std::vector<float> depth;
            for (const auto &r : out) { shp.push_back(r.h); shp.push_back(r.w); counts.push_back((int32_t)r.depth.size()); depth.insert(depth.end(), r.depth.begin(), r.depth.end()); }
            dump(step, "hw", shp); dump(step, "counts", counts); dump(step, "depth", depth);
        } else if (op == "text") {
            const std::vector<int32_t> ids = load<int32_t>(a.s("ids"));
            std::vector<std::vector<float>> out;
            rc = vit_text_embed_batch(model, tstate, ids.empty() ? nullptr : ids.data(), n, (int)a.i("flags"), out);
            dump_rows(step, "text", "counts", out);
        } else {
            die("step " + std::to_string(step) + ": unknown op '" + op + "'");
        }

        const int32_t rc32 = rc;
        dump(step, "rc", &rc32, sizeof(rc32));
        dump(step, "prediction", state.prediction);
        int ch = 0, cw = 0;
        if (state.ctx) (void)vitx_ctx_img_shape(state.ctx, &ch, &cw);
        const vitx_ctx *c = state.ctx;
        printf("STEP %d %s rc=%d ctx=%d max_batch=%d img_h=%d img_w=%d dense_classes=%d depth_bins=%d zeroshot_classes=%d nn_k=%d feat_floats=%d "
               "pack=%d pack_tokens=%d pack_images=%d text=%d text_max_prompts=%d\n",
               step, op.c_str(), rc, c ? 1 : 0, c ? vitx_ctx_max_batch(c) : 0, ch, cw, c ? vitx_dense_classes(c) : 0, c ? vitx_depth_bins(c) : 0,
               c ? vitx_zeroshot_classes(c) : 0, c ? vitx_nn_k(c) : 0, c ? vitx_feat_floats(c) : 0, state.pack ? 1 : 0, state.pack_tokens, state.pack_images,
               tstate.ctx ? 1 : 0, tstate.max_prompts);
        fflush(stdout);
        ++step;
    }
    return 0;
}
