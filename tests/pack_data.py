"""Fixtures of the packed-batch tests (include/vitx.h "packed batches"), shared by tests/test_cpu_pack.py and tests/test_gpu_pack.py.

The restatement is tests/rect_data.py::forward64 on every image of a pack alone, at its own shape: a packed context promises that an image's result
is a function of its own pixels and shape.  The micro fixtures are rect_data's (p16, p14r4, p14rope: D 128, L 2, 2 heads of 64).

VARIANTS are the same tensors read with 4 heads of 32 -- the head count is a header field, the qkv rows are laid out head by head either way -- so
that an image context runs the generic attention arithmetic too and a pack of one shape can be compared with a rectangular context bit for bit:
    p16h4, p14r4h4, p14ropeh4      rect_data's three fixtures
    gluh4                          swiglu_data's "hplus" (4 registers, `rope`, a gated MLP, class-token head)
    preerfh4                       arch_data's "tanh_pre" (a pre-norm, eps 1e-5) with the erf activation
rect_data.forward64(..., heads=4) restates the first three."""
import dataclasses
import os

import numpy as np

import arch_data as AD
import rect_data as XD
import swiglu_data as SD

HEADS4 = 4
VARIANTS = ("p16h4", "p14r4h4", "p14ropeh4", "gluh4", "preerfh4")
UNIFORM_SHAPE = {16: (48, 80), 14: (28, 70)}        # the one-shape pack of each patch size (rect_data.CASES' shapes)


def mixed_shapes(P):
    """The mixed pack: grids 1 x 1, 1 x 7, 5 x 2, 4 x 4 (the micro files' own grid), 2 x 5, 4 x 4 again and 1 x 1 again -- five distinct grids, token
    counts 2 .. 17 (6 .. 21 with registers), a repeated shape that is not adjacent to its twin."""
    return [(P, P), (P, 7 * P), (5 * P, 2 * P), (4 * P, 4 * P), (2 * P, 5 * P), (4 * P, 4 * P), (P, P)]


def pack_of(shapes, seed=3):
    """One exact image (rect_data.images) per shape, each from its own seed: the twins of a repeated shape differ."""
    return [XD.images(1, h, w, seed=seed + 7 * i)[0] for i, (h, w) in enumerate(shapes)]


def variant_tensors(pkg, kind):
    assert kind in VARIANTS
    if kind == "gluh4":
        hp, t = SD.fixture_tensors(pkg, "hplus")
    elif kind == "preerfh4":
        hp, t = AD.fixture_tensors(pkg, "tanh_pre")
        t = dict(t); t["arch"] = np.array([AD.ACT_ERF, 1e-5, 0, 0], np.float32)
    else:
        hp, t = XD.fixture_tensors(pkg, kind[:-2])
    return dataclasses.replace(hp, num_attention_heads=HEADS4), t


def variant_file(pkg, kind, ftype=1):
    """Path of the (cached) model file of a 4-head variant."""
    cache_dir = os.environ.get("VITX_CACHE", "/tmp/vitx_cache")
    os.makedirs(cache_dir, exist_ok=True)
    path = os.path.join(cache_dir, f"pack-{kind}-p{XD.POS_SCALE:g}-q{XD.QK_SCALE:g}-ft{ftype}.gguf")
    if not os.path.exists(path):
        hp, t = variant_tensors(pkg, kind)
        tmp = path + f".tmp{os.getpid()}"
        pkg.ggml_file.write_model(tmp, hp, t, ftype=ftype)
        os.replace(tmp, path)
    return path


def row0_of(shapes, P, registers):
    """row0 [n + 1] of a pack: image i holds 1 + registers + (h / P)(w / P) token rows."""
    n = [1 + registers + (h // P) * (w // P) for h, w in shapes]
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
