// preprocess.cpp -- host resize + normalise, replaces vit_image_preprocess
// (/root/reference/vit.cpp:289-305; bicubic 204-287, bilinear 130-196, clip 198-201).
//
// Behaviour kept from the reference: direct (aspect-ignoring) resize to img_size^2 with
// source scale nx/img_size, no half-pixel offset and no antialiasing for bicubic;
// 4x4 neighbourhood with edge clamp; cubic coefficients evaluated in double then narrowed
// to float, polynomial in float; result rounded, clamped to [0,255], narrowed to u8 and
// normalised with the ImageNet mean/std (vit.cpp:233-234).  Rows are independent, so the
// work is split over host threads (the reference runs it on one thread).
#include <math.h>
#include <stdint.h>

#include <thread>
#include <vector>

#include "model_file.h"
#include "preproc_resample.h"

namespace {

const float kMean[3] = {123.675f, 116.280f, 103.530f};
const float kStd[3] = {58.395f, 57.120f, 57.375f};

inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
inline float to_u8_norm(float v, float mean, float sd) {
    const uint8_t q = (uint8_t)fminf(fmaxf(roundf(v), 0.0f), 255.0f);
    return ((float)q - mean) / sd;
}
// the reference's cubic through 4 samples p0..p3 at fractional offset t (vit.cpp:260-268)
inline float cubic(float p0, float p1, float p2, float p3, float t) {
    const float d0 = p0 - p1, d2 = p2 - p1, d3 = p3 - p1;
    const float a1 = (float)(-1.0 / 3 * d0 + d2 - 1.0 / 6 * d3);
    const float a2 = (float)(1.0 / 2 * d0 + 1.0 / 2 * d2);
    const float a3 = (float)(-1.0 / 6 * d0 - 1.0 / 2 * d2 + 1.0 / 6 * d3);
    return p1 + a1 * t + a2 * t * t + a3 * t * t * t;
}

void bicubic_rows(const uint8_t *src, int nx, int ny, int S, const float *mean, const float *sd, float *dst, int row0, int row1) {
    const float tx = (float)nx / (float)S, ty = (float)ny / (float)S;
    for (int i = row0; i < row1; ++i) {
        const int y = (int)(ty * i);
        const float dy = ty * i - y;
        int ys[4];
        for (int jj = 0; jj < 4; ++jj) ys[jj] = clampi(y - 1 + jj, 0, ny - 1);
        for (int j = 0; j < S; ++j) {
            const int x = (int)(tx * j);
            const float dx = tx * j - x;
            const int x0 = clampi(x - 1, 0, nx - 1), x1 = clampi(x, 0, nx - 1), x2 = clampi(x + 1, 0, nx - 1), x3 = clampi(x + 2, 0, nx - 1);
            for (int k = 0; k < 3; ++k) {
                float C[4];
                for (int jj = 0; jj < 4; ++jj) {
                    const uint8_t *r = src + (size_t)ys[jj] * nx * 3 + k;
                    C[jj] = cubic(r[x0 * 3], r[x1 * 3], r[x2 * 3], r[x3 * 3], dx);
                }
                dst[((size_t)i * S + j) * 3 + k] = to_u8_norm(cubic(C[0], C[1], C[2], C[3], dy), mean[k], sd[k]);
            }
        }
    }
}

void bilinear_rows(const uint8_t *src, int nx, int ny, int S, const float *mean, const float *sd, float *dst, int row0, int row1) {
    const float xs = nx / (float)S, ys = ny / (float)S;
    for (int y = row0; y < row1; ++y) {
        const float sy = (y + 0.5f) * ys - 0.5f;
        const int y0 = sy < 0.0f ? 0 : (int)floorf(sy), y1 = y0 + 1 < ny - 1 ? y0 + 1 : ny - 1;
        const float dy = sy - y0;
        for (int x = 0; x < S; ++x) {
            const float sx = (x + 0.5f) * xs - 0.5f;
            const int x0 = sx < 0.0f ? 0 : (int)floorf(sx), x1 = x0 + 1 < nx - 1 ? x0 + 1 : nx - 1;
            const float dx = sx - x0;
            for (int c = 0; c < 3; ++c) {
                const float v00 = src[3 * ((size_t)y0 * nx + x0) + c], v01 = src[3 * ((size_t)y0 * nx + x1) + c];
                const float v10 = src[3 * ((size_t)y1 * nx + x0) + c], v11 = src[3 * ((size_t)y1 * nx + x1) + c];
                const float v0 = v00 * (1.0f - dx) + v01 * dx, v1 = v10 * (1.0f - dx) + v11 * dx;
                dst[3 * ((size_t)y * S + x) + c] = to_u8_norm(v0 * (1.0f - dy) + v1 * dy, mean[c], sd[c]);
            }
        }
    }
}

// [0, rows) cut into contiguous pieces, one per host thread (at most 16, at least 8 rows each); run(r0, r1) handles rows r0 .. r1 - 1
template <class F> void parallel_rows(int rows, F run) {
    unsigned nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 1;
    if (nt > 16) nt = 16;
    if ((unsigned)rows < nt * 8) nt = 1;
    if (nt == 1) { run(0, rows); return; }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(run, (int)((long)rows * t / nt), (int)((long)rows * (t + 1) / nt));
    for (auto &t : th) t.join();
}

void reference_resize(const uint8_t *hwc, int nx, int ny, int S, bool bicubic, const float *mean, const float *sd, float *out) {
    parallel_rows(S, [&](int r0, int r1) { if (bicubic) bicubic_rows(hwc, nx, ny, S, mean, sd, out, r0, r1); else bilinear_rows(hwc, nx, ny, S, mean, sd, out, r0, r1); });
}

// One axis of the output window: first tap, tap count and the fixed-point coefficients of its S target indices (preproc_resample.h)
struct PilTable {
    std::vector<int> first, n;
    std::vector<int32_t> k;
    int ksize = 1, lo = 0, hi = 0;          // the source range [lo, hi) the window's taps cover
    PilTable(const vitx::PilAxis &a, int o0, int S) : first((size_t)S), n((size_t)S), k((size_t)S * a.ksize), ksize(a.ksize) {
        for (int i = 0; i < S; ++i) {
            vitx::pil_bounds(a, o0 + i, first[i], n[i]);
            const double ww = vitx::pil_total(a, o0 + i, first[i], n[i]);
            for (int j = 0; j < n[i]; ++j) k[(size_t)i * ksize + j] = vitx::pil_coeff(a, o0 + i, first[i], j, ww);
            if (i == 0 || first[i] < lo) lo = first[i];
            if (i == 0 || first[i] + n[i] > hi) hi = first[i] + n[i];
        }
    }
};

// Pillow's Image.resize on u8, the crop window only: horizontal pass over the source rows the window's vertical taps need into a u8
// intermediate [rows][SW][3], then the vertical pass, clamp and normalise.  The window is SW x SH (square for a description's geometry)
void pil_resize(const vitx_preproc &p, const vitx::PpGeom &g, const uint8_t *src, int nx, int ny, float *out) {
    const int bicubic = p.filter == VITX_PP_PIL_BICUBIC, SW = g.SW, SH = g.SH;
    const PilTable tx(vitx::pil_axis(bicubic, nx, g.W), g.left, SW), ty(vitx::pil_axis(bicubic, ny, g.H), g.top, SH);
    const int y0 = ty.lo, rows = ty.hi - ty.lo;
    const size_t line = (size_t)SW * 3;
    std::vector<uint8_t> mid((size_t)rows * line);
    parallel_rows(rows, [&](int r0, int r1) {
        for (int r = r0; r < r1; ++r) {
            const uint8_t *row = src + (size_t)(y0 + r) * nx * 3;
            uint8_t *m = mid.data() + (size_t)r * line;
            for (int c = 0; c < SW; ++c) {
                const int32_t *k = tx.k.data() + (size_t)c * tx.ksize;
                const uint8_t *px = row + (size_t)tx.first[c] * 3;
                for (int ch = 0; ch < 3; ++ch) {
                    int32_t acc = 1 << (vitx::PIL_PRECISION_BITS - 1);
                    for (int j = 0; j < tx.n[c]; ++j) acc += (int32_t)px[(size_t)j * 3 + ch] * k[j];
                    m[(size_t)c * 3 + ch] = (uint8_t)vitx::pil_clip8(acc);
                }
            }
        }
    });
    parallel_rows(SH, [&](int r0, int r1) {
        for (int oy = r0; oy < r1; ++oy) {
            const int32_t *k = ty.k.data() + (size_t)oy * ty.ksize;
            const uint8_t *m = mid.data() + (size_t)(ty.first[oy] - y0) * line;
            float *o = out + (size_t)oy * line;
            for (size_t e = 0; e < line; ++e) {
                int32_t acc = 1 << (vitx::PIL_PRECISION_BITS - 1);
                for (int i = 0; i < ty.n[oy]; ++i) acc += (int32_t)m[(size_t)i * line + e] * k[i];
                const int c = (int)(e % 3);
                o[e] = ((float)vitx::pil_clip8(acc) - p.mean255[c]) / p.std255[c];
            }
        }
    });
}

}  // namespace

namespace vitx {

vitx_preproc pp_default(int img_size) {
    vitx_preproc p;
    p.resize_mode = VITX_PP_STRETCH; p.resize_a = img_size; p.resize_b = img_size; p.filter = VITX_PP_REF_BICUBIC; p.crop = 0; p.crop_round = 0;
    for (int c = 0; c < 3; ++c) { p.mean255[c] = kMean[c]; p.std255[c] = kStd[c]; }
    return p;
}

void pp_to_slots(const vitx_preproc &p, float s[16]) {
    const float v[16] = {(float)p.resize_mode, (float)p.resize_a, (float)p.resize_b, (float)p.filter, (float)p.crop, (float)p.crop_round,
                         p.mean255[0], p.mean255[1], p.mean255[2], p.std255[0], p.std255[1], p.std255[2], 0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 16; ++i) s[i] = v[i];
}

const char *pp_from_slots(const float s[16], vitx_preproc &p) {
    int32_t iv[6];
    for (int i = 0; i < 6; ++i) {
        if (!(s[i] >= 0.0f && s[i] <= (float)PP_MAX_SIDE) || s[i] != (float)(int32_t)s[i]) return "an integer slot is not an integer in 0 .. 16384";
        iv[i] = (int32_t)s[i];
    }
    for (int i = 12; i < 16; ++i) if (s[i] != 0.0f) return "a reserved slot is not 0";
    p.resize_mode = iv[0]; p.resize_a = iv[1]; p.resize_b = iv[2]; p.filter = iv[3]; p.crop = iv[4]; p.crop_round = iv[5];
    for (int c = 0; c < 3; ++c) { p.mean255[c] = s[6 + c]; p.std255[c] = s[9 + c]; }
    return pp_check(p);
}

}  // namespace vitx

extern "C" int vitx_preprocess_u8(const uint8_t *hwc, int nx, int ny, int img_size, int interp, float *out) {
    if (!hwc || !out || nx <= 0 || ny <= 0 || img_size <= 0) { vitx::set_error("vitx_preprocess_u8: invalid argument"); return VITX_ERR_ARG; }
    if (interp != VITX_BICUBIC && interp != VITX_BILINEAR) {   // vit.cpp:300-304 returns false for any other mode
        vitx::set_error("vitx_preprocess_u8: interpolation mode %d is not supported", interp); return VITX_ERR_ARG;
    }
    reference_resize(hwc, nx, ny, img_size, interp == VITX_BICUBIC, kMean, kStd, out);
    return VITX_OK;
}

extern "C" int vitx_preprocess_ex(const vitx_preproc *pp, const uint8_t *hwc, int nx, int ny, float *out) {
    if (!pp || !hwc || !out) { vitx::set_error("vitx_preprocess_ex: NULL argument"); return VITX_ERR_ARG; }
    vitx::PpGeom g;
    const char *bad = vitx::pp_check(*pp);
    if (!bad) bad = vitx::pp_geometry(*pp, nx, ny, g);
    if (bad) { vitx::set_error("vitx_preprocess_ex: %s", bad); return VITX_ERR_ARG; }
    if (!vitx::pp_filter_is_pil(pp->filter)) reference_resize(hwc, nx, ny, g.SW, pp->filter == VITX_PP_REF_BICUBIC, pp->mean255, pp->std255, out);
    else pil_resize(*pp, g, hwc, nx, ny, out);
    return VITX_OK;
}

// ---- rectangular outputs (include/vitx.h "rectangular contexts") ---------------------------------------------------------
extern "C" int vitx_rect_shape(int nx, int ny, int patch, int short_side, int max_long, int *out_w, int *out_h) {
    if (!out_w || !out_h) { vitx::set_error("vitx_rect_shape: NULL argument"); return VITX_ERR_ARG; }
    int w = 0, h = 0;
    if (const char *bad = vitx::pp_rect_shape(nx, ny, patch, short_side, max_long, w, h)) { vitx::set_error("vitx_rect_shape: %s", bad); return VITX_ERR_ARG; }
    *out_w = w; *out_h = h;
    return VITX_OK;
}

extern "C" int vitx_preprocess_rect(const vitx_preproc *pp, const uint8_t *hwc, int nx, int ny, int out_w, int out_h, float *out) {
    if (!pp || !hwc || !out) { vitx::set_error("vitx_preprocess_rect: NULL argument"); return VITX_ERR_ARG; }
    vitx::PpGeom g;
    const char *bad = vitx::pp_check(*pp);
    if (!bad) bad = vitx::pp_geometry_rect(nx, ny, out_w, out_h, g);
    if (bad) { vitx::set_error("vitx_preprocess_rect: %s", bad); return VITX_ERR_ARG; }
    if (!vitx::pp_filter_is_pil(pp->filter)) { vitx::set_error("vitx_preprocess_rect: the reference's filters resize to squares only (use a PIL filter)"); return VITX_ERR_UNSUPPORTED; }
    pil_resize(*pp, g, hwc, nx, ny, out);
    return VITX_OK;
}

extern "C" int vitx_preproc_at_size(const vitx_preproc *in, int img_size, vitx_preproc *out) {
    if (!in || !out) { vitx::set_error("vitx_preproc_at_size: NULL argument"); return VITX_ERR_ARG; }
    if (const char *bad = vitx::pp_check(*in)) { vitx::set_error("vitx_preproc_at_size: %s", bad); return VITX_ERR_ARG; }
    if (img_size <= 0 || img_size > vitx::PP_MAX_SIDE) { vitx::set_error("vitx_preproc_at_size: img_size %d is not in 1 .. 16384", img_size); return VITX_ERR_ARG; }
    vitx_preproc p = *in;
    const int64_t old = in->crop ? in->crop : in->resize_a;
    auto side = [&](int32_t v) { return (int32_t)((2 * (int64_t)v * img_size + old) / (2 * old)); };
    p.resize_a = side(in->resize_a);
    if (in->resize_b) p.resize_b = side(in->resize_b);
    if (in->crop) p.crop = img_size;
    if (const char *bad = vitx::pp_check(p)) { vitx::set_error("vitx_preproc_at_size: at img_size %d: %s", img_size, bad); return VITX_ERR_ARG; }
    *out = p;
    return VITX_OK;
}

// ---- ViTSTR (extensions/vitstr.cpp) ------------------------------------------------------------------------------------
// vit_image_preprocess of the scene-text extension (vitstr.cpp:135-201): RGB -> grey with PIL's weights evaluated in double and
// TRUNCATED to u8 (:128-132), direct resize by (nx / S, ny / S) with a 2x2 linear blend anchored at the truncated source
// coordinate (clamped so that the +1 neighbour exists), then (v / 255 - 0.5) * 2.  The "padding" loops of the reference run from
// res.nx == S and are no-ops.  Output: ONE channel, [S][S] f32.
extern "C" int vitx_preprocess_vitstr_u8(const uint8_t *hwc, int nx, int ny, int img_size, float *out) {
    if (!hwc || !out || nx <= 0 || ny <= 0 || img_size <= 0) { vitx::set_error("vitx_preprocess_vitstr_u8: invalid argument"); return VITX_ERR_ARG; }
    // the reference reads pixel (x + 1, y + 1) unconditionally: a 1-pixel-wide or 1-pixel-high image is outside its domain
    if (nx < 2 || ny < 2) { vitx::set_error("vitx_preprocess_vitstr_u8: image must be at least 2 x 2 (got %d x %d)", nx, ny); return VITX_ERR_ARG; }
    const int S = img_size;
    std::vector<uint8_t> grey((size_t)nx * ny);
    for (size_t i = 0; i < (size_t)nx * ny; ++i) grey[i] = (uint8_t)(0.299 * hwc[3 * i] + 0.587 * hwc[3 * i + 1] + 0.114 * hwc[3 * i + 2]);
    const float xs = (float)nx / S, ys = (float)ny / S;
    for (int y = 0; y < S; ++y) {
        for (int x = 0; x < S; ++x) {
            const float gx = x * xs, gy = y * ys;
            const int gxi = (int)gx, gyi = (int)gy;
            const float u = gx - gxi, v = gy - gyi;
            const int px0 = clampi(gxi, 0, nx - 2), py0 = clampi(gyi, 0, ny - 2), px1 = px0 + 1, py1 = py0 + 1;
            float val = (1 - u) * (1 - v) * grey[(size_t)py0 * nx + px0] + u * (1 - v) * grey[(size_t)py0 * nx + px1] +
                        (1 - u) * v * grey[(size_t)py1 * nx + px0] + u * v * grey[(size_t)py1 * nx + px1];
            val = (val / 255.0f - 0.5f) * 2.0f;
            out[(size_t)y * S + x] = val;
        }
    }
    return VITX_OK;
}

// The greedy decode of the extension's vit_predict (vitstr.cpp:1025-1051): positions 1 .. seq_len - 1 (position 0 is the [GO] slot),
// arg-max class per position (first maximum wins, strict '>'), stop at class 1 = "[s]"; the score is the product of the maxima of
// the characters emitted.  ids receives the class of every emitted character.
extern "C" int vitx_vitstr_decode(const float *probs, int seq_len, int num_classes, int32_t *ids, int *n_ids, double *score) {
    if (!probs || !ids || !n_ids || seq_len <= 0 || num_classes <= 0) { vitx::set_error("vitx_vitstr_decode: invalid argument"); return VITX_ERR_ARG; }
    double conf = 1.0; int n = 0;
    for (int col = 1; col < seq_len; ++col) {
        const float *p = probs + (size_t)col * num_classes;
        int best = 0; float best_v = p[0];
        for (int row = 1; row < num_classes; ++row) if (p[row] > best_v) { best_v = p[row]; best = row; }
        if (best == 1) break;
        conf *= best_v;
        ids[n++] = best;
    }
    *n_ids = n;
    if (score) *score = conf;
    return VITX_OK;
}
