"""Fixtures of the depth head on packed batches (include/vitx.h "packed batches", the depth head), shared by tests/test_cpu_pack_depth.py and
tests/test_gpu_pack_depth.py.

The pack of the kernel tests: six images, each with its own grid; per upsampling factor u its own output shapes (never below the fine plane u gh x u gw) --
    grids          (1, 1)  (16, 37)   (2, 3)    (14, 14)  (1, 5)    (1, 1)
    outputs u = 1  (2, 5)  (17, 65)   (2, 3)    (37, 37)  (16, 80)  (1, 1)
    outputs u = 2  (2, 5)  (32, 74)   (17, 65)  (37, 37)  (16, 80)  (3, 3)
    outputs u = 4  (5, 7)  (65, 149)  (17, 65)  (56, 56)  (16, 81)  (4, 4)
Every row has an output equal to its fine plane (a resize of scale 1), widths that are no multiple of the 4 pixels of a lane (5, 65, 37, 149, 81), odd
pixel counts in front of later images, so their maps and the rows of odd widths start off the 16-byte boundary of the packed store, and sides one past
a tile edge (17 rows, 65 columns; 65 rows at u = 4).  The (16, 37) grid at u = 1 has a fine-tile window of 16 x 19 cells, which forces bin chunks at
K = 64 and more for the WHOLE launch (the LDS and the chunk of a packed launch come from its widest window); beside it the (2, 3) grid has a window of
6 cells.

Logit rows: depth_data.hostile per image (its own seed), each image's rows behind `Tp` prefix rows filled with NaN and +inf -- the rows of the class
and register tokens in a packed context, which the fine kernel must never read.  Offsets: one row per image (depth_data.hostile's), behind a row 0 of
NaN that belongs to nobody: orow[i] = i + 1.

tables(...) restates depth_pack_tables (csrc/depth_map.hip) in numpy; reference(...) is the host function vitx_depth_host image by image; restated(...)
is depth_data.depth image by image on its slice of the pack's rows, with the mistakes of a PACK the tests must be able to see (MUTANTS):
    offset_image0     every image takes image 0's offsets
    tile_neighbour    the first 64 x 16 output tile of every image comes from the rows of the image behind it (a work item given to the wrong image)
    lrow_no_prefix    an image's first logit row is its first prefix row
    fine_base_off     the resize reads an image's fine plane where the next image's begins
    grid_swapped      gh and gw change places (the rows are read as a gw x gh grid, the plane that comes out as u gh x u gw)

The model of the end-to-end tests (l4_file): rect_data's "p14r4" micro fixture (patch 14, file grid 4 x 4, four registers, D 128) drawn with FOUR layers,
so that a head over four layers exists, and read with 4 heads of 32 as pack_data's variants are, so that an image context runs the generic attention
arithmetic too and a pack of one shape can be compared with a rectangular context bit for bit.  ref64.forward64(..., heads=4) restates it."""
import dataclasses

import numpy as np

import dense_data as DD
import depth_data as XD
import rect_data as RD

GRIDS = ((1, 1), (16, 37), (2, 3), (14, 14), (1, 5), (1, 1))
OUTS = {1: ((2, 5), (17, 65), (2, 3), (37, 37), (16, 80), (1, 1)),
        2: ((2, 5), (32, 74), (17, 65), (37, 37), (16, 80), (3, 3)),
        4: ((5, 7), (65, 149), (17, 65), (56, 56), (16, 81), (4, 4))}
US = (1, 2, 4)
KS = (1, 5, 64, 255, 256)
PREFIXES = (1, 5)                                    # a class token; a class token and four registers
FINE_TILE, OUT_W, OUT_H = 16, 64, 16                 # csrc/depth_bins.h kDepthTile, kDepthOutW, kDepthOutH
MAX_OUT = 8192                                       # csrc/depth_bins.h kDepthMaxOut
MUTANTS = ("offset_image0", "tile_neighbour", "lrow_no_prefix", "fine_base_off", "grid_swapped")
F = np.float32


def fines(grids, u):
    return [(u * gh, u * gw) for gh, gw in grids]


def tables(grids, outs, u):
    """(pix0 int64, fine0 int64, ftile0 int32, otile0 int32), each [n + 1]: the running pixel counts of the maps and of the fine planes, the running
    counts of 16 x 16 fine tiles and of 64 x 16 output tiles."""
    run = lambda v, t: np.concatenate([[0], np.cumsum(v)]).astype(t)
    fs = fines(grids, u)
    return (run([int(h) * int(w) for h, w in outs], np.int64), run([h * w for h, w in fs], np.int64),
            run([-(-w // FINE_TILE) * -(-h // FINE_TILE) for h, w in fs], np.int32), run([-(-int(w) // OUT_W) * -(-int(h) // OUT_H) for h, w in outs], np.int32))


def pack_logits(grids, K, Tp, ld=None, seed=0, make=None):
    """(logits [rows][ld] f32, offsets [n + 1][ld] f32, bins [K], lrow [n], orow [n]): image i's gh gw rows of `make` (depth_data.hostile) behind Tp
    poisoned prefix rows; its offsets are row orow[i] = i + 1, row 0 is NaN; ld defaults to the engine's padding of K + 1, so that K = 256 has pad
    columns too."""
    make = XD.hostile if make is None else make
    ld = XD.pad_to(K + 1) if ld is None else ld
    blocks, offs, lrow, at, bins = [], [np.full((1, ld), np.nan, F)], [], 0, None
    for i, (gh, gw) in enumerate(grids):
        pre = np.where((np.arange(Tp * ld) % 2 == 0), F(np.nan), F(np.inf)).astype(F).reshape(Tp, ld)
        lg, off, bins = make(1, gh, gw, K, ld, seed=seed + 11 * i + gh * gw)
        blocks += [pre, lg]; offs.append(off)
        lrow.append(at + Tp); at += Tp + gh * gw
    return (np.ascontiguousarray(np.concatenate(blocks)), np.ascontiguousarray(np.concatenate(offs)), bins, np.asarray(lrow, np.int32),
            np.arange(1, len(grids) + 1, dtype=np.int32))


def image_rows(logits, lrow, grids, i):
    gh, gw = grids[i]
    return np.ascontiguousarray(logits[lrow[i]:lrow[i] + gh * gw])


def reference(binding, logits, offsets, bins, lrow, orow, grids, outs, K, u, lo=XD.LO, hi=XD.HI):
    """(depth bits u32 [sum oh ow], fine bits u32 [sum u^2 gh gw]): binding.depth_host on every image alone, planes and maps end to end.  offsets None:
    nothing is added."""
    dm, fn = [], []
    for i, ((gh, gw), (oh, ow)) in enumerate(zip(grids, outs)):
        off = None if offsets is None else np.ascontiguousarray(offsets[orow[i]:orow[i] + 1])
        d, f = binding.depth_host(image_rows(logits, lrow, grids, i), off, bins, 1, gh, gw, K, u, oh, ow, float(lo), float(hi))
        dm.append(np.ascontiguousarray(d, F).view(np.uint32).ravel()); fn.append(np.ascontiguousarray(f, F).view(np.uint32).ravel())
    return np.concatenate(dm), np.concatenate(fn)


def _resize(fine_bits, fh, fw, oh, ow, lo, hi):
    """depth_data.depth's second half on one plane: the bilinear resize of "dense prediction", the clamp, the quiet NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = DD.values(np.ascontiguousarray(fine_bits).view(F).reshape(fh * fw, 1), 1, fh, fw, 1, oh, ow)[..., 0]
        d = np.where(d < F(lo), F(lo), np.where(d > F(hi), F(hi), d)).astype(F)
    return XD._quiet(d).ravel()


def restated(logits, offsets, bins, lrow, orow, grids, outs, K, u, Tp=0, lo=XD.LO, hi=XD.HI, mutant=None):
    """The same from depth_data.depth (numpy) on each image's slice of the pack's rows, with the pack's mutants."""
    assert mutant is None or mutant in MUTANTS
    n, total = len(grids), logits.shape[0]
    rows_at = lambda first, cnt: np.ascontiguousarray(logits[(first + np.arange(cnt)) % total])
    dm, fn = [], []
    for i, ((gh, gw), (oh, ow)) in enumerate(zip(grids, outs)):
        first = lrow[i] - (Tp if mutant == "lrow_no_prefix" else 0)
        off = None if offsets is None else offsets[orow[0 if mutant == "offset_image0" else i]][None]
        if mutant == "grid_swapped":
            f = XD.depth(rows_at(first, gh * gw), off, bins, 1, gw, gh, K, u, u * gw, u * gh, lo, hi)[1].ravel()
            d = _resize(f, u * gh, u * gw, oh, ow, lo, hi)
        else:
            d, f = XD.depth(rows_at(first, gh * gw), off, bins, 1, gh, gw, K, u, oh, ow, lo, hi)
            d, f = d.ravel(), f.ravel()
        if mutant == "tile_neighbour":
            j = (i + 1) % n
            other = XD.depth(rows_at(lrow[j], gh * gw), off, bins, 1, gh, gw, K, u, oh, ow, lo, hi)[0].reshape(oh, ow)
            d = d.reshape(oh, ow).copy(); d[:OUT_H, :OUT_W] = other[:OUT_H, :OUT_W]; d = d.ravel()
        dm.append(d); fn.append(f)
    fine = np.concatenate(fn)
    if mutant == "fine_base_off":
        fine0 = tables(grids, outs, u)[1]
        for i, ((gh, gw), (oh, ow)) in enumerate(zip(grids, outs)):
            at = int(fine0[i + 1]) % fine.size
            plane = fine[(at + np.arange(u * gh * u * gw)) % fine.size]
            dm[i] = _resize(plane, u * gh, u * gw, oh, ow, lo, hi)
    return np.concatenate(dm), fine


def original_like(shapes, u=1):
    """Output shapes like the sizes of originals before an aspect-preserving resize: a few pixels more than the image on each side, never a multiple of
    the patch (28 x 70 -> 31 x 75); with u they are never below the fine plane of the micro fixtures (u / P < 1)."""
    return [(h + 3, w + 5) for h, w in shapes]


L4_LAYERS, L4_HEADS, L4_REGISTERS = 4, 4, 4


def l4_tensors(pkg):
    """(hparams, tensors) of the four-layer fixture: rect_data.fixture_tensors' recipe ("p14r4") on four layers."""
    name, registers = RD.FIXTURES["p14r4"]
    assert registers == L4_REGISTERS
    hp = dataclasses.replace(pkg.synth.hparams_for(name), num_hidden_layers=L4_LAYERS)
    t = dict(pkg.synth.make_weights(hp, head_scale=4.0, registers=registers))
    D = hp.hidden_size
    t["pos_embed"] = (t["pos_embed"] * np.float32(RD.POS_SCALE)).astype(np.float32)
    for i in range(hp.num_hidden_layers):
        for nm in (f"blocks.{i}.attn.qkv.weight", f"blocks.{i}.attn.qkv.bias"):
            a = t[nm].copy(); a[:2 * D] *= np.float32(RD.QK_SCALE); t[nm] = a
    return dataclasses.replace(hp, num_attention_heads=L4_HEADS), t


def l4_file(pkg, ftype=1):
    """Path of the (cached) model file of the four-layer fixture."""
    from ref64 import cached_file
    return cached_file(f"packdepth-l4-p{RD.POS_SCALE:g}-q{RD.QK_SCALE:g}-ft{ftype}", lambda tmp: pkg.ggml_file.write_model(tmp, *l4_tensors(pkg), ftype=ftype))
