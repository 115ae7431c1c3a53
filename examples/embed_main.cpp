// embed_main.cpp -- image embeddings through the C++ header vit.cpp_amd/vit.h: loads a model and two images, takes the class-token
// embedding of both in ONE forward (vit_embed_batch, which the reference has no counterpart of) and prints their cosine similarity.
//   usage: embed_main MODEL.gguf IMAGE_A IMAGE_B [--img-size N | --img-shape HxW] [--out FILE]
// The images are preprocessed as the model file describes (vit_image_preprocess_model: CLIP's and DINOv2's resize + centre crop, their mean / std;
// the reference's preprocess for a file without a description).  --img-size N runs the state at N x N instead of the file's size
// (vit_state::img_size: the position table is resampled, the preprocessing follows); --img-shape HxW runs it
// on H x W images in a rectangular context (vit_state::img_h, img_w; both images stretched to that shape by vit_image_preprocess_rect); --out writes image A's embedding as raw f32.
// Build:  g++ -std=c++17 -O2 examples/embed_main.cpp -Ivit.cpp_amd -Lvit.cpp_amd -lvitx -Wl,-rpath,$PWD/vit.cpp_amd -o embed_main
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "vit.h"

int main(int argc, char **argv) {
    int img_size = 0, img_h = 0, img_w = 0;
    const char *out_path = nullptr;
    bool bad = argc < 4;
    for (int i = 4; i < argc && !bad; ++i) {
        const std::string a = argv[i];
        if (a == "--img-size" && i + 1 < argc) img_size = atoi(argv[++i]);
        else if (a == "--img-shape" && i + 1 < argc) bad = sscanf(argv[++i], "%dx%d", &img_h, &img_w) != 2 || img_h <= 0 || img_w <= 0;
        else if (a == "--out" && i + 1 < argc) out_path = argv[++i];
        else bad = true;
    }
    if (img_size && img_h) bad = true;
    if (bad) { fprintf(stderr, "usage: %s MODEL.gguf IMAGE_A IMAGE_B [--img-size N | --img-shape HxW] [--out FILE]\n", argv[0]); return 1; }
    vit_model model;
    vit_state state;
    if (!vit_model_load(argv[1], model)) { fprintf(stderr, "%s: failed to load model from '%s'\n", __func__, argv[1]); return 1; }
    state.img_size = img_size;                      // 0 = the file's
    state.img_h = img_h; state.img_w = img_w;       // both 0 = a square state
    image_f32 imgs[2];
    for (int i = 0; i < 2; ++i) {
        image_u8 raw;
        if (!load_image_from_file(argv[2 + i], raw)) { fprintf(stderr, "%s: failed to load image from '%s'\n", __func__, argv[2 + i]); return 1; }
        if (!(img_h ? vit_image_preprocess_rect(raw, imgs[i], model, img_w, img_h) : vit_image_preprocess_model(raw, imgs[i], model, img_size))) { fprintf(stderr, "%s: failed to preprocess '%s'\n", __func__, argv[2 + i]); return 1; }
    }
    std::vector<std::vector<float>> emb;
    if (vit_embed_batch(model, state, imgs, 2, VITX_FEAT_CLS | VITX_FEAT_L2, emb) != 0) return 1;
    double dot = 0.0, na = 0.0, nb = 0.0;          // the vectors are unit length already (VITX_FEAT_L2); the norms are kept for clarity
    for (size_t k = 0; k < emb[0].size(); ++k) { dot += (double)emb[0][k] * emb[1][k]; na += (double)emb[0][k] * emb[0][k]; nb += (double)emb[1][k] * emb[1][k]; }
    if (out_path) {
        FILE *f = fopen(out_path, "wb");
        if (!f || fwrite(emb[0].data(), sizeof(float), emb[0].size(), f) != emb[0].size()) { fprintf(stderr, "%s: cannot write '%s'\n", __func__, out_path); return 1; }
        fclose(f);
    }
    printf("embedding: %zu floats per image (class token, final norm, L2-normalised)\n", emb[0].size());
    printf("cosine similarity : %.6f\n", dot / std::sqrt(na * nb));
    return 0;
}
