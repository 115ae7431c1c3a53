"""Fixtures of the dense head on packed batches (include/vitx.h "packed batches", the dense head), shared by tests/test_cpu_pack_dense.py and
tests/test_gpu_pack_dense.py.

The pack of the kernel tests: six images, each with its own grid and output shape --
    grids    (1, 1)  (16, 37)  (2, 3)   (14, 14)  (1, 5)    (1, 1)
    outputs  (2, 5)  (16, 37)  (5, 17)  (37, 37)  (16, 80)  (1, 1)
10, 592, 85, 1369, 1280 and 1 pixels: odd counts, so later images start off the 4-byte (labels) and 16-byte (scores) boundaries; widths 5, 17, 37
and 80 around the 4-pixel pack of a lane and the 64-pixel tile, heights around the 16-row tile; the scale-1 image (16, 37) has a window of 16 x 37
cells, which forces class chunks at K = 150 and 256 for the WHOLE launch (the LDS and the chunk of a packed launch come from its widest window).

Logit rows: dense_data.hostile per image (its own seed), each image's rows behind `Tp` prefix rows filled with NaN and +inf -- the rows of the class
and register tokens in a packed context, which the label kernel must never read.

tables(...) restates dense_pack_tables (csrc/dense_label.hip) in numpy; reference(...) is the host function vitx_dense_labels_host image by image,
restated(...) dense_data.labels image by image (with its mutants)."""
import numpy as np

import dense_data as DD

GRIDS = ((1, 1), (16, 37), (2, 3), (14, 14), (1, 5), (1, 1))
OUTS = ((2, 5), (16, 37), (5, 17), (37, 37), (16, 80), (1, 1))
TILE_W, TILE_H = 64, 16                              # csrc/dense_resample.h kDenseTileW, kDenseTileH
MAX_OUT = 8192                                       # csrc/kernels.h kDenseMaxOut
PREFIXES = (0, 1, 5)                                 # no prefix rows; a class token; a class token and four registers


def tables(outs):
    """(pix0 int64 [n + 1], tile0 int32 [n + 1]): the running pixel count and the running count of 64 x 16 output tiles."""
    px = [int(h) * int(w) for h, w in outs]
    tl = [-(-int(w) // TILE_W) * -(-int(h) // TILE_H) for h, w in outs]
    return np.concatenate([[0], np.cumsum(px)]).astype(np.int64), np.concatenate([[0], np.cumsum(tl)]).astype(np.int32)


def pack_logits(grids, K, Tp, ld=None, seed=0):
    """(logits [rows][ld] f32, lrow [n]): image i's gh gw hostile rows behind Tp poisoned prefix rows; ld defaults to the engine's padding of K + 1, so
    that K = 128 and 256 have pad columns too (the pad_leak mutant needs one)."""
    ld = DD.pad_to(K + 1) if ld is None else ld
    blocks, lrow, at = [], [], 0
    for i, (gh, gw) in enumerate(grids):
        pre = np.where((np.arange(Tp * ld) % 2 == 0), np.float32(np.nan), np.float32(np.inf)).astype(np.float32).reshape(Tp, ld)
        blocks += [pre, DD.hostile(1, gh, gw, K, ld, seed=seed + 11 * i + gh * gw)]
        lrow.append(at + Tp); at += Tp + gh * gw
    return np.ascontiguousarray(np.concatenate(blocks)), np.asarray(lrow, np.int32)


def image_rows(logits, lrow, grids, i):
    gh, gw = grids[i]
    return np.ascontiguousarray(logits[lrow[i]:lrow[i] + gh * gw])


def reference(binding, logits, lrow, grids, outs, K):
    """(labels u8 [sum oh ow], score bits u32 [sum oh ow]): binding.dense_labels_host on every image alone, the maps end to end."""
    lab, sc = [], []
    for i, ((gh, gw), (oh, ow)) in enumerate(zip(grids, outs)):
        l, s = binding.dense_labels_host(image_rows(logits, lrow, grids, i), 1, gh, gw, K, oh, ow)
        lab.append(l.ravel()); sc.append(np.ascontiguousarray(s, np.float32).view(np.uint32).ravel())
    return np.concatenate(lab), np.concatenate(sc)


def restated(logits, lrow, grids, outs, K, mutant=None):
    """The same from dense_data.labels (numpy, with its mutants)."""
    lab, sc = [], []
    for i, ((gh, gw), (oh, ow)) in enumerate(zip(grids, outs)):
        l, s = DD.labels(image_rows(logits, lrow, grids, i), 1, gh, gw, K, oh, ow, mutant=mutant)
        lab.append(l.ravel()); sc.append(s.ravel())
    return np.concatenate(lab), np.concatenate(sc)


def original_like(shapes, P):
    """Output shapes like the sizes of originals before an aspect-preserving resize: a few pixels more than the image on each side, never a
    multiple of the patch (28 x 70 -> 31 x 75)."""
    return [(h + 3, w + 5) for h, w in shapes]
