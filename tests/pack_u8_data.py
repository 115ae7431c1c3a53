"""Fixtures of the u8-source tests of packed batches (include/vitx.h "packed batches", u8 sources), shared by tests/test_cpu_pack_u8.py and
tests/test_gpu_pack_u8.py: a numpy-free restatement of the preprocessing launch's tables (preproc_resample.h pil_bounds and pp_tiling,
image_preprocess.hip pp_pack_tables) and the packs the kernel is tried on.  Shapes are (rows, columns) everywhere: a source is (ny, nx), an
output (h, w)."""
import math

import numpy as np

import preproc_data as PPD

TW, TH, WAVES, LDS_LIMIT = 32, 8, 4, 64 * 1024           # preproc_resample.h PP_TW, PP_TH, PP_WAVES, PP_LDS_LIMIT
SEG_INTS = 14                                            # kernels.h kPpSegInts


def axis(bicubic, n_in, n_out):
    """preproc_resample.h pil_axis: (in, scale, support, ksize)."""
    scale = n_in / n_out
    support = (2.0 if bicubic else 1.0) * max(scale, 1.0)
    return n_in, n_out, scale, support, 1 if n_in == n_out else int(math.ceil(support)) * 2 + 1


def bounds(ax, o):
    """pil_bounds: (first, n) of target index o.  Python floats are IEEE doubles and int() truncates, as the C casts do."""
    n_in, n_out, scale, support, ksize = ax
    if n_in == n_out:
        return o, 1
    center = (o + 0.5) * scale
    lo, hi = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), n_in)
    lo = min(lo, n_in)
    return lo, min(max(hi - lo, 0), ksize)


def _widest(ax, out, tile):
    most = 1
    for o0 in range(0, out, tile):
        o1 = min(o0 + tile, out) - 1
        (f0, n0), (f1, n1) = bounds(ax, o0), bounds(ax, o1)
        most = max(most, max(f1 + n1, f0 + n0) - f0)
    return most


def tiling(bicubic, src, out):
    """pp_tiling of a source (ny, nx) stretched to (h, w): dict(kx, ky, rows, span, stage, lds)."""
    (ny, nx), (h, w) = src, out
    ax, ay = axis(bicubic, nx, w), axis(bicubic, ny, h)
    span, rows = _widest(ax, w, TW), _widest(ay, h, TH)
    stage = (3 * span + 3) // 4 * 4 + 4
    lds = (TW + TH) * 16 + 4 * (TW * ax[4] + TH * ay[4]) + rows * TW * 3 + WAVES * stage
    return dict(kx=ax[4], ky=ay[4], rows=rows, span=span, stage=stage, lds=lds)


def tables(bicubic, srcs, outs):
    """pp_pack_tables: (src0 [n + 1] bytes, dst0 [n + 1] floats, tile0 [n + 1], the launch's LDS)."""
    src0, dst0, tile0, lds = [0], [0], [0], 0
    for (ny, nx), (h, w) in zip(srcs, outs):
        src0.append(src0[-1] + 3 * nx * ny)
        dst0.append(dst0[-1] + 3 * w * h)
        tile0.append(tile0[-1] + -(-w // TW) * -(-h // TH))
        lds = max(lds, tiling(bicubic, (ny, nx), (h, w))["lds"])
    return np.asarray(src0, np.int64), np.asarray(dst0, np.int64), np.asarray(tile0, np.int32), lds


# ---- the pack of the kernel test: (source (ny, nx), output (h, w), what it is there for)
# The strong down-scale is 4 x NEAR_NX -> 16 x 8, the geometry of test_preprocess_rect_device_beyond_the_lds_bound (4 x 40000 -> 16 x 8) with the
# widest source row whose tiling still fits: one tile whose 8 columns span the whole row (kx about NEAR_NX / 2 coefficients per column, the staged
# row 3 NEAR_NX bytes per wave), beside a 3 x 2 source.  tests/test_cpu_pack_u8.py checks every property claimed here.
NEAR_NX = {True: 832, False: 1456}                     # bicubic, bilinear: the largest multiple of 16 columns inside the bound


def kernel_pack(bicubic):
    return [((9, 1), (16, 8), "a 1-pixel-wide source"),
            ((1, 7), (8, 40), "a 1-pixel-high source, two tiles, the second partial"),
            ((23, 37), (23, 37), "the identity"),
            ((23, 37), (32, 48), "an upscale, sides that are multiples of the tile"),
            ((4, NEAR_NX[bicubic]), (16, 8), "a strong down-scale just inside the LDS bound"),
            ((3, 2), (5, 3), "a tiny image: one partial tile"),
            ((61, 83), (45, 70), "3 x 6 tiles, neither side a multiple of the tile"),
            ((120, 91), (28, 42), "a down-scale by about 4 and 2")]


def sources(pack, seed=0):
    """One u8 image per entry, the patterns of preproc_data.PATTERNS in turn."""
    return [PPD.image(PPD.PATTERNS[i % len(PPD.PATTERNS)], nx, ny, seed=seed + i) for i, ((ny, nx), _, _) in enumerate(pack)]


# ---- the originals of the forward test: their aspect-preserving shapes at short side 2 P give five distinct grids, a repeated one, a 1-pixel-high original
ORIGINALS = [(30, 41), (17, 100), (90, 33), (64, 64), (20, 53), (1, 9), (50, 50)]


def originals(seed=20):
    return [PPD.image(PPD.PATTERNS[i % 2], nx, ny, seed=seed + i) for i, (ny, nx) in enumerate(ORIGINALS)]
