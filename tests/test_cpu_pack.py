"""Packed batches, the host side (include/vitx.h "packed batches"): every refusal vitx_pack_check makes, row0 of a mixed list with and without
register tokens, the distinct-grid count a forward compares with max_grids, pack_images against rect_shape, and the 4-head fixture variants."""
import numpy as np
import pytest

import pack_data as KD
import preproc_data as PPD
import rect_data as XD
import text_data as TD


def _model(pkg, binding, kind):
    return binding.Model(XD.fixture_file(pkg, kind))


def _refused(binding, model, shapes, max_tokens, max_images):
    with pytest.raises(binding.VitxError) as ei:
        binding.pack_check(model, shapes, max_tokens, max_images)
    return ei.value.code


@pytest.mark.parametrize("kind,registers", [("p16", 0), ("p14r4", 4)])
def test_row0_of_a_mixed_list(pkg, binding, kind, registers):
    model = _model(pkg, binding, kind)
    P = model.hparams.patch_size
    shapes = KD.mixed_shapes(P)
    want = KD.row0_of(shapes, P, registers)
    assert want[-1] == sum(g + 1 + registers for g in (1, 7, 10, 16, 10, 16, 1))
    got = binding.pack_check(model, shapes, int(want[-1]), len(shapes))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(binding.pack_check(model, shapes[::-1], 10 ** 6, 64), KD.row0_of(shapes[::-1], P, registers))
    assert np.array_equal(binding.pack_check(model, shapes[:1], 10 ** 6, 1), [0, 2 + registers])
    model.close()


def test_every_refusal_of_a_forward_call(pkg, binding):
    model = _model(pkg, binding, "p14r4")
    P = 14
    shapes = KD.mixed_shapes(P)
    rows = int(KD.row0_of(shapes, P, 4)[-1])
    ARG = binding.ERR_ARG
    for bad in ((P + 1, P), (P, P - 1), (0, P), (P, 0), (-P, P), (P, -P), (16, 16)):      # not a positive multiple of the patch size (16: the other fixture's)
        assert _refused(binding, model, shapes[:3] + [bad] + shapes[3:], 10 ** 6, 64) == ARG, bad
        assert "patch size" in str(binding.lib().vitx_last_error())
    assert _refused(binding, model, shapes, 10 ** 6, len(shapes) - 1) == ARG              # n above max_images
    assert _refused(binding, model, shapes, rows - 1, 64) == ARG                          # one token above max_tokens
    assert "max_tokens" in str(binding.lib().vitx_last_error())
    assert binding.pack_check(model, shapes, rows, len(shapes))[-1] == rows               # both bounds are inclusive
    L = binding.lib()
    import ctypes as C
    s = np.ascontiguousarray(shapes, np.int32)
    i32p = C.POINTER(C.c_int32)
    assert L.vitx_pack_check(model._h, s.ctypes.data_as(i32p), 0, 10 ** 6, 64, None) == ARG       # n = 0
    assert L.vitx_pack_check(model._h, s.ctypes.data_as(i32p), -1, 10 ** 6, 64, None) == ARG
    assert L.vitx_pack_check(model._h, None, 1, 10 ** 6, 64, None) == ARG
    assert L.vitx_pack_check(None, s.ctypes.data_as(i32p), 1, 10 ** 6, 64, None) == ARG
    assert L.vitx_pack_check(model._h, s.ctypes.data_as(i32p), len(shapes), 10 ** 6, 64, None) == 0      # row0 may be NULL
    model.close()
    text = binding.Model(TD.text_file(pkg, "clip"))
    assert _refused(binding, text, [(16, 16)], 10 ** 6, 4) == ARG                         # a text model
    assert "text" in str(binding.lib().vitx_last_error())
    text.close()


def test_distinct_grids_against_max_grids(pkg, binding):
    """What a forward compares with its context's max_grids: the mixed pack names five grids, twins and transposes counted as they are."""
    model = _model(pkg, binding, "p16")
    P = 16
    assert binding.pack_distinct_grids(model, KD.mixed_shapes(P)) == 5
    assert binding.pack_distinct_grids(model, [(P, 2 * P), (2 * P, P)]) == 2              # a grid and its transpose are two
    assert binding.pack_distinct_grids(model, [(3 * P, 2 * P)] * 9) == 1
    assert binding.pack_distinct_grids(model, [(P, k * P) for k in range(1, 41)]) == 40   # above the default cache of 32: such a call is refused
    model.close()


def test_pack_images_shapes_are_rect_shape(pkg, binding):
    pp = binding.Preproc.make(resize_a=16, resize_b=16, filter=binding.PP_PIL_BICUBIC, mean255=(127.5,) * 3, std255=(127.5,) * 3)
    srcs = [PPD.image("random", nx, ny, seed=nx) for nx, ny in ((50, 37), (37, 50), (40, 40), (90, 31))]
    for P, short in ((16, 32), (14, 28)):
        pixels, shapes = binding.pack_images(srcs, pp, short, patch=P)
        assert shapes.dtype == np.int32 and shapes.shape == (4, 2)
        at = 0
        for img, (h, w) in zip(srcs, shapes):
            assert (w, h) == binding.rect_shape(img.shape[1], img.shape[0], P, short) and min(h, w) == short and h % P == 0 and w % P == 0
            one = binding.preprocess_rect(img, pp, w, h)
            assert np.array_equal(pixels[at:at + one.size].view(np.uint32), one.ravel().view(np.uint32))
            at += one.size
        assert at == pixels.size
    capped = binding.pack_images(srcs[3:], pp, 32, 48, patch=16)[1]
    assert tuple(capped[0]) == binding.rect_shape(90, 31, 16, 32, 48)[::-1] and max(capped[0]) == 48


@pytest.mark.parametrize("kind", KD.VARIANTS)
def test_the_four_head_variants_load(pkg, binding, kind):
    """The variants are the two-head fixtures' tensors under a header with 4 heads: head dim 32, everything else as filed."""
    model = binding.Model(KD.variant_file(pkg, kind))
    hp = model.hparams
    assert (hp.hidden_size, hp.num_hidden_layers, hp.num_attention_heads) == (128, 2, KD.HEADS4)
    assert model.head_pool == binding.POOL_CLS and model.in_channels == 3
    assert (model.glu is not None) == (kind == "gluh4") and bool(model.has_pre_norm) == (kind == "preerfh4")
    assert (model.rope is not None) == (kind in ("p14ropeh4", "gluh4"))
    model.close()
