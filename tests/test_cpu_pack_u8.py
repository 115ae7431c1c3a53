"""Packed batches fed from u8 originals, the host side (include/vitx.h "packed batches", u8 sources): vitx_pack_fit_shapes against rect_shape,
vitx_pack_u8_check -- its tables against the restatement of tests/pack_u8_data.py and every refusal with its code --, the refusals of
vitx_op_preprocess_pack that come before its first device call, and the properties tests/test_gpu_pack_u8.py claims for its packs.  No kernel is
launched here."""
import numpy as np
import pytest

import pack_data as KD
import pack_u8_data as UD
import preproc_data as PPD
import rect_data as RD


def _model(pkg, binding, kind="p16"):
    return binding.Model(RD.fixture_file(pkg, kind))


def _pp(binding, filt=PPD.PP_PIL_BICUBIC):
    mean, std = PPD.mean_std255(PPD.IMAGENET)
    return binding.Preproc.make(resize_a=16, resize_b=16, filter=filt, mean255=mean, std255=std)


def _code(binding, fn, *a, **k):
    with pytest.raises(binding.VitxError) as ei:
        fn(*a, **k)
    return ei.value.code, str(ei.value)


def test_fit_shapes_is_rect_shape_per_image(pkg, binding):
    for kind in ("p16", "p14rope"):
        model = _model(pkg, binding, kind)
        P = model.hparams.patch_size
        srcs = UD.ORIGINALS + [(375, 500), (500, 375), (1, 1), (7, 400)]
        for short, max_long in ((2 * P, 0), (3 * P, 5 * P), (P, P)):
            got = binding.pack_fit_shapes(model, srcs, short, max_long)
            want = [binding.rect_shape(nx, ny, P, short, max_long)[::-1] for ny, nx in srcs]
            assert got.dtype == np.int32 and got.tolist() == [list(w) for w in want], (kind, short, max_long)
        # vitx_rect_shape's refusals, naming the image
        code, text = _code(binding, binding.pack_fit_shapes, model, [(30, 41), (0, 5)], 2 * P)
        assert code == binding.ERR_ARG and "image 1" in text
        assert _code(binding, binding.pack_fit_shapes, model, [(30, 41)], 2 * P + 1)[0] == binding.ERR_ARG
        model.close()
    # the originals of the forward test: five distinct grids, one of them twice
    shapes = [binding.rect_shape(nx, ny, 16, 32)[::-1] for ny, nx in UD.ORIGINALS]
    assert len(set(shapes)) == 5 and len(shapes) == 7 and shapes[3] == shapes[6], shapes


def test_check_returns_the_tables(pkg, binding):
    """src0, tile0 and lds of the mixed pack and of the kernel test's packs equal the restatement, for both filters; any table may be NULL."""
    model = _model(pkg, binding)
    P = model.hparams.patch_size
    shapes = KD.mixed_shapes(P)
    srcs = [(37, 23), (9, 200), (301, 77), (64, 64), (1, 5), (500, 375), (2, 3)]
    for fname, filt in PPD.FILTERS.items():
        bic = filt == PPD.PP_PIL_BICUBIC
        src0, tile0, lds = binding.pack_u8_check(model, _pp(binding, filt), srcs, shapes)
        want = UD.tables(bic, srcs, shapes)
        assert src0.dtype == np.int64 and tile0.dtype == np.int32
        assert np.array_equal(src0, want[0]) and np.array_equal(tile0, want[2]) and lds == want[3], fname
        assert lds == max(UD.tiling(bic, s, o)["lds"] for s, o in zip(srcs, shapes)) and tile0[-1] > len(shapes)
        # max_src_bytes is inclusive
        binding.pack_u8_check(model, _pp(binding, filt), srcs, shapes, int(want[0][-1]))
    import ctypes as C
    i32p = C.POINTER(C.c_int32)
    s, o = np.asarray(srcs, np.int32), np.asarray(shapes, np.int32)
    pp = _pp(binding)
    assert binding.lib().vitx_pack_u8_check(model._h, C.byref(pp), s.ctypes.data_as(i32p), o.ctypes.data_as(i32p), len(srcs), 0, None, None, None) == 0
    model.close()


def test_the_kernel_packs_are_what_they_claim(binding):
    """A check of the FIXTURE (tests/pack_u8_data.py) against its own restatement, as tests/test_cpu_rollout_data.py is for its module: every start
    alignment, a total that is no multiple of 4, the down-scale just inside the bound beside a tiny image, tilings that differ widely.  The library is
    asked about the bound itself: the fixed-shape kernel's _supports agrees on both sides of it, and the packed op refuses the pack with the source 16
    columns wider, naming the image, before any device call."""
    for bic in (True, False):
        pack = UD.kernel_pack(bic)
        srcs, outs = [p[0] for p in pack], [p[1] for p in pack]
        src0, dst0, tile0, lds = UD.tables(bic, srcs, outs)
        assert {3 * ny * nx % 4 for ny, nx in srcs} == {0, 1, 2, 3}
        assert {int(v) % 4 for v in src0[:-1]} == {0, 1, 2, 3} and src0[-1] % 4 != 0
        near, tiny = UD.tiling(bic, *pack[4][:2]), UD.tiling(bic, *pack[5][:2])
        wider = UD.tiling(bic, (4, UD.NEAR_NX[bic] + 16), (16, 8))
        assert 0.98 * UD.LDS_LIMIT < near["lds"] <= UD.LDS_LIMIT < wider["lds"] and lds == near["lds"]
        assert near["kx"] > 50 * tiny["kx"] and near["span"] > 100 * tiny["span"] and near["lds"] > 30 * tiny["lds"]
        assert tile0[6] - tile0[5] == 1 and outs[5][0] < UD.TH and outs[5][1] < UD.TW                # one partial tile
        assert tile0[7] - tile0[6] == 18 and outs[6][0] % UD.TH and outs[6][1] % UD.TW
        assert srcs[2] == outs[2] and srcs[0][1] == 1 and srcs[1][0] == 1
        pp = _pp(binding, PPD.PP_PIL_BICUBIC if bic else PPD.PP_PIL_BILINEAR)
        nx = UD.NEAR_NX[bic]
        assert binding.preprocess_rect_device_supports(pp, nx, 4, 8, 16) and not binding.preprocess_rect_device_supports(pp, nx + 16, 4, 8, 16)
        code, text = _code(binding, binding.preprocess_pack, pp, 4096, [srcs[5], (4, nx + 16)], [outs[5], (16, 8)], 8192)
        assert code == binding.ERR_UNSUPPORTED and "image 1" in text


def test_check_refusals(pkg, binding):
    """Every refusal a forward call adds while u8 sources are declared for it, by code and word."""
    model = _model(pkg, binding)
    P = model.hparams.patch_size
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    pp = _pp(binding)
    srcs, shapes = [(30, 41), (17, 100), (64, 64)], [(P, 2 * P), (P, 4 * P), (2 * P, 2 * P)]
    check = lambda *a, **k: _code(binding, binding.pack_u8_check, model, *a, **k)
    binding.pack_u8_check(model, pp, srcs, shapes)
    # the description: a REF filter is vitx_preprocess_rect's refusal; the file's own description here is the reference default, a REF filter
    for f in (PPD.PP_REF_BICUBIC, PPD.PP_REF_BILINEAR):
        code, text = check(_pp(binding, f), srcs, shapes)
        assert code == U and "PIL filter" in text
    assert not model.has_preproc and check(None, srcs, shapes)[0] == U
    assert check(binding.Preproc.make(resize_a=16, resize_b=16, filter=PPD.PP_PIL_BICUBIC, std255=(1.0, 0.0, 1.0)), srcs, shapes)[0] == A
    assert check(binding.Preproc.make(resize_a=16, resize_b=16, filter=9), srcs, shapes)[0] == A
    # the geometry of an image
    for bad in ((0, 41), (30, 0), (30, 2 ** 20 + 1), (-1, 5)):
        code, text = check(pp, [srcs[0], bad, srcs[2]], shapes)
        assert code == A and "image 1" in text, bad
    # one image beyond the LDS bound among fine ones: test_preprocess_rect_device_beyond_the_lds_bound's geometry, 4 x 40000 -> 16 x 8 (P = 16: 16 x 16 here)
    assert binding.preprocess_rect_device_supports(pp, 41, 30, 2 * P, P) and not binding.preprocess_rect_device_supports(pp, 40000, 4, P, P)
    code, text = check(pp, [srcs[0], srcs[1], (4, 40000)], [shapes[0], shapes[1], (P, P)])
    assert code == U and "image 2" in text and "LDS" in text
    # bytes above max_src_bytes; an n that differs from the call's
    total = sum(3 * ny * nx for ny, nx in srcs)
    code, text = check(pp, srcs, shapes, total - 1)
    assert code == A and "max_src_bytes" in text
    # (the C call takes one n for both lists, so binding.pack_u8_check words this refusal itself; check_u8's own n_src != n branch is reached only by a
    # declaration, vitx_pack_u8_sources + a forward call: tests/test_gpu_pack_u8.py::test_declarations_are_consumed_and_refused_calls_launch_nothing)
    assert check(pp, srcs[:2], shapes)[0] == A
    # the shapes themselves: vitx_pack_check's refusals come first
    assert check(pp, srcs, [(P, 2 * P), (P + 1, 4 * P), (2 * P, 2 * P)])[0] == A
    # more than 2^31 - 1 tiles: 2^20 + 1 images of 16384 x P outputs, 2048 tiles each (and 1025 tokens each: the token count stays below 2^31)
    n = 2 ** 20 + 1
    code, text = check(pp, np.tile(np.asarray([[8, 8]], np.int32), (n, 1)), np.tile(np.asarray([[16384, P]], np.int32), (n, 1)))
    assert code == A and "tiles" in text
    model.close()


def test_op_refusals_come_before_any_device_call(binding):
    """vitx_op_preprocess_pack with pointers that are never followed: the table refusals and the alignment of d_srcs."""
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    pp = _pp(binding)
    op = lambda *a: _code(binding, binding.preprocess_pack, *a)[0]
    assert op(pp, 4096, [(30, 41)], [(16, 32)], 0) == A and op(pp, 0, [(30, 41)], [(16, 32)], 4096) == A
    assert op(pp, 4097, [(30, 41)], [(16, 32)], 8192) == A and op(pp, 4096, [(30, 41)], [(16, 32)], 8194) == A
    assert op(_pp(binding, PPD.PP_REF_BICUBIC), 4096, [(30, 41)], [(16, 32)], 8192) == U
    assert op(pp, 4096, [(30, 41), (4, 40000)], [(16, 32), (16, 8)], 8192) == U
    assert op(pp, 4096, [(30, 41)], [(16, 16385)], 8192) == A and op(pp, 4096, [(30, 41)], [(0, 16)], 8192) == A
