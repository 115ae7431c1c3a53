// preproc_sanitize_main.cpp -- the host preprocessing (csrc/preprocess.cpp: vitx_preprocess_ex, the PIL resize, the crop window, the border taps)
// under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain CPU program: no GPU, no Python.  It walks the geometries of
// tests/preproc_data.py with both PIL filters and both crop roundings, shortest-edge crops with non-zero offsets, an up-scale, 1-pixel sources
// and the strongest down-scales, on buffers allocated to the exact size so that any overrun is a report.  Not part of the library build:
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/preproc_sanitize_main.cpp vit.cpp_amd/csrc/preprocess.cpp vit.cpp_amd/csrc/model_file.cpp -lpthread -o preproc_sanitize && ./preproc_sanitize
#include <stdint.h>
#include <stdio.h>

#include <memory>

#include "vitx.h"

static int fails = 0;

static uint32_t run(const vitx_preproc &pp, int nx, int ny, int want_rc, unsigned seed) {
    std::unique_ptr<uint8_t[]> src(new uint8_t[(size_t)nx * ny * 3]);
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < (size_t)nx * ny * 3; ++i) { s = s * 1664525u + 1013904223u; src[i] = (uint8_t)(s >> 24); }
    const int S = pp.crop ? pp.crop : pp.resize_a;
    std::unique_ptr<float[]> out(new float[want_rc == VITX_OK ? (size_t)S * S * 3 : 1]);
    const int rc = vitx_preprocess_ex(&pp, src.get(), nx, ny, out.get());
    if (rc != want_rc) { printf("FAIL %d x %d -> mode %d a %d b %d crop %d filter %d: status %d, expected %d (%s)\n", nx, ny, pp.resize_mode, pp.resize_a, pp.resize_b, pp.crop, pp.filter, rc, want_rc, vitx_last_error()); ++fails; return 0; }
    uint32_t h = 2166136261u;
    if (rc == VITX_OK) for (size_t i = 0; i < (size_t)S * S * 3; ++i) { const float v = out[i]; if (!(v >= 0.0f && v <= 255.0f)) { ++fails; printf("FAIL value %g\n", (double)v); break; } h = (h ^ (uint32_t)v) * 16777619u; }
    return h;
}

int main() {
    const int geo[][4] = {{37, 23, 16, 16}, {500, 375, 298, 224}, {640, 480, 341, 256}, {100, 60, 224, 134}, {17, 400, 14, 329}, {224, 224, 224, 224},
                          {1000, 31, 224, 7}, {33, 33, 32, 32}, {64, 64, 16, 16}, {3, 2, 8, 8}};
    uint32_t h = 0; int n = 0;
    for (int filter = VITX_PP_PIL_BILINEAR; filter <= VITX_PP_PIL_BICUBIC; ++filter) {
        for (int round = 0; round < 2; ++round) {
            for (const auto &g : geo) {
                vitx_preproc pp = {VITX_PP_STRETCH, g[2], g[3], filter, g[2] < g[3] ? g[2] : g[3], round, {0, 0, 0}, {1, 1, 1}};
                h ^= run(pp, g[0], g[1], VITX_OK, ++n);
            }
            const int se[][4] = {{500, 375, 224, 224}, {375, 500, 224, 224}, {50, 37, 18, 16}, {50, 37, 18, 13}, {50, 37, 18, 15}, {90, 70, 48, 33}, {70, 130, 40, 35},
                                 {13, 9, 20, 16}, {1, 1, 8, 8}, {1, 300, 4, 4}, {300, 1, 4, 4}, {4032, 3024, 256, 224}, {2, 4000, 2, 2}};
            for (const auto &c : se) {
                vitx_preproc pp = {VITX_PP_SHORTEST_EDGE, c[2], 0, filter, c[3], round, {0, 0, 0}, {1, 1, 1}};
                h ^= run(pp, c[0], c[1], VITX_OK, ++n);
            }
            vitx_preproc down = {VITX_PP_STRETCH, 8, 8, filter, 0, round, {0, 0, 0}, {1, 1, 1}};
            h ^= run(down, 8, 2048, VITX_OK, ++n); h ^= run(down, 2048, 8, VITX_OK, ++n); h ^= run(down, 8, 8, VITX_OK, ++n);
            vitx_preproc big = {VITX_PP_SHORTEST_EDGE, 18, 0, filter, 19, round, {0, 0, 0}, {1, 1, 1}};
            h ^= run(big, 50, 37, VITX_ERR_ARG, ++n);
        }
    }
    for (int filter = VITX_PP_REF_BICUBIC; filter <= VITX_PP_REF_BILINEAR; ++filter) {
        vitx_preproc ref = {VITX_PP_STRETCH, 64, 64, filter, 0, 0, {0, 0, 0}, {1, 1, 1}};
        h ^= run(ref, 90, 70, VITX_OK, ++n); h ^= run(ref, 1, 1, VITX_OK, ++n); h ^= run(ref, 640, 3, VITX_OK, ++n);
    }
    printf("%d cases, %d failures, checksum %08x\n", n, fails, h);
    return fails ? 1 : 0;
}
