"""Pins the oracle AND the product's host code to code compiled from the REAL reference sources (oracle/_ref, built by
oracle/build_ref.sh from the reference's vit.cpp / vit.h / quantize.cpp line ranges -- the parts that need no ggml), through what that
code returned on the inputs below, recorded in tests/golden/ref_vit.json (tests/golden/make_ref_golden.py):

  * vit_image_preprocess (bicubic + bilinear, vit.cpp:130-305) on the reference's 10 bundled images and on edge shapes:
    reference-compiled (-ffp-contract=off build) == oracle/vit_oracle.c == libvitx.so (vitx_preprocess_u8), BIT FOR BIT.
    The reference is not bit-reproducible against ITSELF across compiler flags: built the way its own CMakeLists does on an
    FMA-capable x86 (-O3 -march=native, GCC contracts a*b+c) it moves a handful of values per image by one u8 step
    (measured: bicubic 0-4 of 150 528 values, bilinear up to 177 of 442 368).  The product and the oracle equal the
    no-contraction build exactly and are asserted to stay within that one-step band of the contracting build;
  * the prediction fill + descending sort of vit_predict (vit.cpp:1043-1058) vs vitx_topk;
  * which tensors `quantize` re-encodes (quantize.cpp:207-223) vs the native quantize tool's selection;
  * vit_hparams defaults and accessors (vit.h:20-37, vit.cpp:30-48).

Everything else on the path (the ggml graph) stays "parity unpinned": ggml is an empty submodule in the reference.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
ASSET_DIR = os.path.join(HERE, "golden", "assets")
ASSETS = sorted(os.listdir(ASSET_DIR))
BUILDS = ["libvit_ref_fma.so", "libvit_ref_strict.so"]
# What the reference-compiled code returned on every input below (tests/golden/make_ref_golden.py): the pins hold without the
# reference sources; where build() could compile oracle/_ref, every test also checks that the live libraries still return exactly this.
GOLDEN = os.path.join(HERE, "golden", "ref_vit.json")
EDGE_SHAPES = [(1, 1), (2, 3), (37, 53), (224, 224), (500, 31), (31, 500), (640, 480), (1117, 2212)]


def _ref(build):
    """The reference-compiled library in oracle/_ref, or None where it was not built (no reference sources on this machine)."""
    path = os.path.join(REF_DIR, build)
    if not os.path.exists(path):
        return None
    L = C.CDLL(path)
    L.ref_preprocess.argtypes = [C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_float)]
    L.ref_sorted_predictions.argtypes = [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.ref_quantizes_tensor.argtypes = [C.c_char_p, C.c_int]
    L.ref_hparams_defaults.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_float)]
    return L


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


def _ref_preprocess(L, img, S, mode):
    img = np.ascontiguousarray(img, np.uint8); ny, nx = img.shape[:2]
    out = np.empty((S, S, 3), np.float32)
    rc = L.ref_preprocess(img.ctypes.data_as(C.POINTER(C.c_uint8)), nx, ny, S, mode.encode(), out.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, out


def _sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def preprocess_record(Ls, Lf, img, S, mode):
    """The strict build's output as a sha1 (the product must equal it bit for bit) and, with Lf, the few values the FMA-contracting
    build returns differently: [flat indices, its values]."""
    rc, strict = _ref_preprocess(Ls, img, S, mode)
    rec = {"rc": rc, "sha1": _sha1(strict)}
    if Lf is not None:
        fma = _ref_preprocess(Lf, img, S, mode)[1]
        idx = np.flatnonzero(fma != strict)
        rec["fma"] = [idx.tolist(), fma.reshape(-1)[idx].tolist()]
    return rec


def _fma_build_output(strict, rec):
    out = strict.copy()
    idx, val = rec["fma"]
    out.reshape(-1)[idx] = np.asarray(val, np.float32)
    return out


def sort_inputs():
    rng = np.random.default_rng(5)
    out = []
    for n in (10, 1000):
        logits = rng.standard_normal(n).astype(np.float32) * 3
        p = np.exp(logits - logits.max()); out.append((p / p.sum()).astype(np.float32))
    return out


def sort_record(L, p):
    n = len(p)
    idx = (C.c_int * n)(); val = (C.c_float * n)()
    L.ref_sorted_predictions(p.ctypes.data_as(C.POINTER(C.c_float)), n, idx, val)
    return {"idx": list(idx), "val": list(val)}


QUANT_PROBES = [("blocks.0.attn.qkv.weight", 2), ("blocks.0.attn.qkv.bias", 1), ("patch_embed.proj.weight", 4), ("pos_embed", 3), ("xweight", 2), ("weightx", 2)]


def n_dims_in_file(name):      # as the converter writes them (convert-pth-to-ggml.py:141-158)
    if name in ("patch_embed.proj.weight", "patch_embed.proj.bias"): return 4
    if name in ("cls_token", "pos_embed"): return 3
    return 2 if name.endswith(".weight") and ("attn." in name or "mlp." in name or name == "head.weight") else 1


def quantize_record(L, names_dims):
    return [[name, nd, L.ref_quantizes_tensor(name.encode(), nd)] for name, nd in names_dims]


def hparams_record(L):
    out = (C.c_int * 9)(); eps = C.c_float()
    L.ref_hparams_defaults(out, C.byref(eps))
    return {"ints": list(out), "eps": eps.value}


def _decode(name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(ASSET_DIR, name)).convert("RGB"), dtype=np.uint8)


def edge_image(shape):
    return np.random.default_rng(shape[0] * 4099 + shape[1]).integers(0, 256, size=(shape[0], shape[1], 3), dtype=np.uint8)


MEAN = np.array([123.675, 116.28, 103.53], np.float32)
STD = np.array([58.395, 57.12, 57.375], np.float32)


def _same_or_one_step(got, want):
    """Equal, or (vs the FMA-contracting reference build) at most 0.1 % of the values one u8 step away."""
    if np.array_equal(got, want):
        return True
    step = np.abs(np.rint(got * STD + MEAN) - np.rint(want * STD + MEAN))
    return step.max() <= 1 and (got != want).mean() <= 1e-3


def test_preprocess_of_the_bundled_images_equals_reference_compiled_code(binding, oracle, gold):
    Ls, Lf = _ref("libvit_ref_strict.so"), _ref("libvit_ref_fma.so")
    n_fma_diff = 0
    for a in ASSETS:
        img = _decode(a)
        for mode, code in (("bicubic", binding.BICUBIC), ("bilinear", binding.BILINEAR)):
            for S in (224, 384):
                rec = gold["preprocess"][f"{a}|{mode}|{S}"]
                if Ls is not None:
                    assert preprocess_record(Ls, None, img, S, mode) == {"rc": rec["rc"], "sha1": rec["sha1"]}, (a, mode, S, "live strict build vs the recording")
                assert rec["rc"] == 0
                ours = binding.preprocess(img, S, code)
                assert _sha1(oracle.preprocess(img, S, mode)) == rec["sha1"], (a, mode, S, "oracle")
                assert _sha1(ours) == rec["sha1"], (a, mode, S, "libvitx")
                fmas = [_fma_build_output(ours, rec)] + ([_ref_preprocess(Lf, img, S, mode)[1]] if Lf is not None else [])
                for fma in fmas:       # the recorded contracting build and, where it is built here, the live one (its compiler may differ)
                    assert _same_or_one_step(ours, fma), (a, mode, S, "vs the FMA-contracting reference build")
                n_fma_diff += int((ours != fmas[0]).sum())
    print("values that differ from the FMA-contracting reference build over all assets/modes/sizes:", n_fma_diff)


@pytest.mark.parametrize("build", ["libvit_ref_strict.so"])
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_preprocess_edge_shapes_equal_reference_compiled_code(binding, oracle, gold, build, shape):
    """1x1, extreme aspect ratios, identity size, up- and down-scaling, and the largest bundled geometry (2212 x 1117: the float
    pixel-index arithmetic of vit.cpp:260-263 is still exact there)."""
    L = _ref(build)
    img = edge_image(shape)
    for mode, code in (("bicubic", binding.BICUBIC), ("bilinear", binding.BILINEAR)):
        for S in (32, 224):
            rec = gold["edge"][f"{shape[0]}x{shape[1]}|{mode}|{S}"]
            if L is not None:
                assert preprocess_record(L, None, img, S, mode) == rec, (mode, S, "the live reference build differs from the recording")
            assert rec["rc"] == 0
            assert _sha1(oracle.preprocess(img, S, mode)) == rec["sha1"], (mode, S, "oracle")
            assert _sha1(binding.preprocess(img, S, code)) == rec["sha1"], (mode, S, "libvitx")


def test_reference_builds_differ_by_at_most_one_u8_step_and_unknown_mode_is_rejected(binding, gold):
    """Records the fact the product's "bit-exact" claim rests on: the reference's two builds are NOT identical (so "bit-exact
    against the reference binary" only has a meaning per build); they stay within one u8 step on < 0.1 % of the values."""
    Lf = _ref(BUILDS[0])
    differing = 0
    for a in ASSETS:
        img = _decode(a)
        for mode, code in (("bicubic", binding.BICUBIC), ("bilinear", binding.BILINEAR)):
            rec = gold["preprocess"][f"{a}|{mode}|224"]
            s = binding.preprocess(img, 224, code)
            assert _sha1(s) == rec["sha1"], (a, mode)         # the strict build's output, as recorded
            for f in [_fma_build_output(s, rec)] + ([_ref_preprocess(Lf, img, 224, mode)[1]] if Lf is not None else []):
                assert _same_or_one_step(f, s), (a, mode)
                differing += int((f != s).sum())
    assert differing > 0, "the two reference builds now agree bit for bit: update DESIGN.md section 3 and the module docstring"
    if Lf is not None:
        assert _ref_preprocess(Lf, _decode(ASSETS[0]), 224, "nearest")[0] == gold["nearest_rc"]
    assert gold["nearest_rc"] == 1                                            # vit.cpp:300-304 returns false


def test_prediction_sort_equals_reference_compiled_code(binding, gold):
    L = _ref(BUILDS[1])
    for p, rec in zip(sort_inputs(), gold["sort"]):
        n = len(p)
        assert len(np.unique(p)) == n                      # no ties: std::sort's order is then fully determined
        if L is not None:
            assert sort_record(L, p) == rec
        got_idx, got_val = binding.topk(p, n)
        assert rec["idx"] == got_idx and rec["val"] == got_val
        got5_idx, got5_val = binding.topk(p, 5)
        assert rec["idx"][:5] == got5_idx and rec["val"][:5] == got5_val


def test_quantize_tensor_selection_equals_reference_compiled_code(pkg, binding, gold, tmp_path):
    """Every tensor name of a real model file x n_dims: the native quantize tool re-encodes exactly the tensors the reference's
    regex + n_dims rule selects (quantize.cpp:207-223)."""
    L = _ref(BUILDS[1])
    src = pkg.synth.cached_synthetic("vit_micro_patch16_64", head_scale=4.0)
    dst = str(tmp_path / "q8.gguf")
    binding.quantize_file(src, dst, 8)
    before = {t[0]: t for t in binding.Model(src).tensors()}
    after = {t[0]: t for t in binding.Model(dst).tensors()}
    assert before.keys() == after.keys()
    names_dims = [(name, n_dims_in_file(name)) for name in sorted(after)]
    if L is not None:
        assert quantize_record(L, names_dims) == gold["quantize_file"]
        assert quantize_record(L, QUANT_PROBES) == gold["quantize_probes"]
    assert [r[:2] for r in gold["quantize_file"]] == [list(nd) for nd in names_dims]
    n_q = 0
    for name, _, want in gold["quantize_file"]:
        _, ttype, ne, _ = after[name]
        assert (ttype == 8) == bool(want), (name, ttype, ne)
        n_q += want
    assert n_q == 4 * 2 + 1                                # qkv, proj, fc1, fc2 per layer + head.weight
    assert [r[2] for r in gold["quantize_probes"]] == [1, 0, 0, 0, 1, 0]


def test_hparams_defaults_equal_reference_compiled_code(binding, gold):
    """vit.h:22-30 defaults are the patch-8 base model; accessors as vit.cpp:30-48."""
    L = _ref(BUILDS[1])
    if L is not None:
        assert hparams_record(L) == gold["hparams"]
    assert gold["hparams"]["ints"] == [768, 12, 12, 1000, 8, 224, 1, 28, 64]
    assert abs(gold["hparams"]["eps"] - 1e-6) < 1e-12
