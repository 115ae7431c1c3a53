// text_embed_main.cpp -- text embeddings through the C++ header vit.cpp_amd/vit.h: loads a text-tower file (convert.py --text-out) and a file of
// tokenised prompts, runs vit_text_embed_batch and prints one embedding per line.  There is no tokenizer in the engine: the ids come from the caller.
//   usage: text_embed_main TEXT.gguf IDS.i32 [--l2] [--bf16]
// IDS.i32: raw little-endian int32, n * T of them (T = the file's context length), prompt after prompt.
// Build:  g++ -std=c++17 -O2 examples/text_embed_main.cpp -Ivit.cpp_amd -Lvit.cpp_amd -lvitx -Wl,-rpath,$PWD/vit.cpp_amd -o text_embed_main
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "vit.h"

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s TEXT.gguf IDS.i32 [--l2] [--bf16]\n", argv[0]); return 2; }
    int flags = 0, dtype = VITX_F16;
    for (int i = 3; i < argc; ++i) {
        if (!strcmp(argv[i], "--l2")) flags |= VITX_TEXT_L2;
        else if (!strcmp(argv[i], "--bf16")) dtype = VITX_BF16;
        else { fprintf(stderr, "%s: unknown option '%s'\n", argv[0], argv[i]); return 2; }
    }
    vit_model model;
    if (!vit_model_load(argv[1], model)) { fprintf(stderr, "%s: failed to load '%s'\n", argv[0], argv[1]); return 1; }
    if (vitx_model_kind(model.handle) != VITX_KIND_TEXT) { fprintf(stderr, "%s: '%s' is an image model: it has no text tower\n", argv[0], argv[1]); return 1; }
    const int T = model.hparams.img_size;
    FILE *f = fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "%s: failed to open '%s'\n", argv[0], argv[2]); return 1; }
    std::vector<int32_t> ids;
    int32_t buf[1024];
    for (size_t got; (got = fread(buf, 4, 1024, f)) > 0;) ids.insert(ids.end(), buf, buf + got);
    fclose(f);
    if (ids.empty() || ids.size() % (size_t)T) { fprintf(stderr, "%s: '%s' holds %zu ids, not a positive multiple of the context length %d\n", argv[0], argv[2], ids.size(), T); return 1; }
    const int n = (int)(ids.size() / (size_t)T);
    vit_text_state state;
    state.dtype = dtype;
    std::vector<std::vector<float>> out;
    if (vit_text_embed_batch(model, state, ids.data(), n, flags, out) != 0) return 1;
    printf("%d prompts of %d tokens, width %zu\n", n, T, out[0].size());
    for (const std::vector<float> &e : out) {
        printf("embedding");
        for (float v : e) printf(" %.9g", v);
        printf("\n");
    }
    return 0;
}
