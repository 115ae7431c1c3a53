"""The dense head on packed batches, the host side (include/vitx.h "packed batches", the dense head): vitx_pack_dense_check -- its tables against the
numpy restatement of tests/pack_dense_data.py and every refusal -- and the fixtures of tests/test_gpu_pack_dense.py: the reference (the host function
image by image) pinned to dense_data.labels, and every mutant of dense_data visible on the pack.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest

import dense_data as DD
import pack_data as KD
import pack_dense_data as QD
import rect_data as XD


def _model(pkg, binding, kind="p16"):
    return binding.Model(XD.fixture_file(pkg, kind))


def test_check_returns_the_tables(pkg, binding):
    """pix0 and tile0 of mixed shapes, at the images' own shapes and at given output shapes, equal the restatement; either table may be NULL."""
    for kind in ("p16", "p14r4"):
        model = _model(pkg, binding, kind)
        P = model.hparams.patch_size
        shapes = KD.mixed_shapes(P) + [(9 * P, 20 * P), (P, 70 * P)]                     # more than one tile across and down
        for outs in (None, QD.original_like(shapes, P), [(h * 3 + 1, w * 2) for h, w in shapes]):
            want_p, want_t = QD.tables(shapes if outs is None else outs)
            pix0, tile0 = binding.pack_dense_check(model, shapes, outs, 21, int(want_p[-1]))           # max_pixels is inclusive
            assert pix0.dtype == np.int64 and tile0.dtype == np.int32
            assert np.array_equal(pix0, want_p) and np.array_equal(tile0, want_t), (kind, outs)
        assert want_t[-1] > len(shapes)
        s = np.asarray(shapes, np.int32)
        i32p = C.POINTER(C.c_int32)
        assert binding.lib().vitx_pack_dense_check(model._h, s.ctypes.data_as(i32p), None, len(shapes), 21, 10 ** 9, None, None) == 0
        model.close()
    # the kernel tests' pack: the restatement's own numbers
    pix0, tile0 = QD.tables(QD.OUTS)
    assert pix0.tolist() == [0, 10, 602, 687, 2056, 3336, 3337] and tile0.tolist() == [0, 1, 2, 3, 6, 8, 9]


def test_device_table_rows(binding):
    """vitx_dense_pack_tables: the running tile count, then per image lrow, grid, output, pix0 in two words, the bits of f32(g) / f32(out) per axis, 0."""
    lrow = np.cumsum([5 + gh * gw for gh, gw in QD.GRIDS]) - [gh * gw for gh, gw in QD.GRIDS]
    tab, tiles, cells = binding.dense_pack_tables(QD.GRIDS, QD.OUTS, lrow)
    n = len(QD.GRIDS)
    pix0, tile0 = QD.tables(QD.OUTS)
    assert np.array_equal(tab[:n + 1], tile0) and tiles == tile0[-1]
    for i, ((gh, gw), (oh, ow)) in enumerate(zip(QD.GRIDS, QD.OUTS)):
        sy, sx = np.float32(gh) / np.float32(oh), np.float32(gw) / np.float32(ow)
        want = [lrow[i], gh, gw, oh, ow, int(pix0[i]), 0, int(np.float32(sy).view(np.int32)), int(np.float32(sx).view(np.int32)), 0]
        assert tab[n + 1 + 10 * i:n + 11 + 10 * i].tolist() == want, i
    # the widest window: the scale-1 image's whole 16 x 37 grid (a 64 x 16 tile of it touches min(g, (T - 1) scale + 4) cells per axis)
    assert cells == 16 * 37
    with pytest.raises(binding.VitxError):
        binding.dense_pack_tables([(2, 3)], [(1, 3)], [0])


def test_check_refusals(pkg, binding):
    model = _model(pkg, binding)
    P = model.hparams.patch_size
    shapes = KD.mixed_shapes(P)
    px = sum(h * w for h, w in shapes)
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED

    def refused(code, word, *a):
        with pytest.raises(binding.VitxError) as ei:
            binding.pack_dense_check(model, *a)
        assert ei.value.code == code and word in str(ei.value), (str(ei.value), a)

    own = [tuple(s) for s in shapes]
    for i, (h, w) in enumerate(shapes):
        gh, gw = h // P, w // P
        if gh > 1:
            refused(A, "upsampling only", shapes, own[:i] + [(gh - 1, w)] + own[i + 1:], 21, 10 ** 9)        # a side below the grid
        if gw > 1:
            refused(A, "upsampling only", shapes, own[:i] + [(h, gw - 1)] + own[i + 1:], 21, 10 ** 9)
    binding.pack_dense_check(model, shapes, [(h // P, w // P) for h, w in shapes], 21, 10 ** 9)              # the grid itself is the lower bound
    binding.pack_dense_check(model, shapes[:1], [(QD.MAX_OUT, QD.MAX_OUT)], 21, QD.MAX_OUT ** 2)             # 8192 the upper
    refused(A, "upsampling only", shapes[:1], [(QD.MAX_OUT + 1, P)], 21, 10 ** 12)
    refused(A, "upsampling only", shapes[:1], [(P, QD.MAX_OUT + 1)], 21, 10 ** 12)
    refused(A, "images", shapes, own[:-1], 21, 10 ** 9)                                                      # n mismatch
    refused(A, "images", shapes, own + own[:1], 21, 10 ** 9)
    binding.pack_dense_check(model, shapes, None, 21, px)
    refused(A, "max_pixels", shapes, None, 21, px - 1)                                                       # one pixel too many
    refused(A, "max_pixels", shapes, own[:-1] + [(own[-1][0], own[-1][1] + 1)], 21, px + own[-1][0] - 1)
    refused(A, "classes", shapes, None, 0, 10 ** 9)
    refused(U, "classes", shapes, None, 257, 10 ** 9)
    binding.pack_dense_check(model, shapes, None, 256, 10 ** 9)
    refused(A, "patch size", [(P + 1, P)], None, 21, 10 ** 9)                                                # vitx_pack_check's refusals come first
    model.close()


@pytest.mark.parametrize("K", DD.KS)
def test_reference_is_the_restatement(binding, K):
    """pack_dense_data.reference (vitx_dense_labels_host image by image, the maps end to end) equals dense_data.labels on the kernel tests' pack, in both
    orders and behind every count of prefix rows; the prefix rows and the pad columns do hold NaN and +inf."""
    for Tp in QD.PREFIXES:
        for grids, outs in ((QD.GRIDS, QD.OUTS), (QD.GRIDS[::-1], QD.OUTS[::-1])):
            lg, lrow = QD.pack_logits(grids, K, Tp, seed=K)
            assert lg.shape[0] == sum(Tp + gh * gw for gh, gw in grids)
            for i in range(len(grids)):
                assert Tp == 0 or not np.isfinite(lg[lrow[i] - Tp:lrow[i]]).any()
            assert not np.isfinite(lg[:, K:]).any()
            lab, bits = QD.reference(binding, lg, lrow, grids, outs, K)
            want_lab, want_bits = QD.restated(lg, lrow, grids, outs, K)
            assert lab.size == QD.tables(outs)[0][-1]
            assert np.array_equal(lab, want_lab) and np.array_equal(bits, want_bits), (K, Tp)


@pytest.mark.parametrize("K", [K for K in DD.KS if K >= 3])
def test_the_pack_tells_the_mutants_apart(K):
    """Each mistake of dense_data.MUTANTS changes at least one label or score of the pack."""
    lg, lrow = QD.pack_logits(QD.GRIDS, K, 1, seed=K)
    lab, bits = QD.restated(lg, lrow, QD.GRIDS, QD.OUTS, K)
    for m in DD.MUTANTS:
        mlab, mbits = QD.restated(lg, lrow, QD.GRIDS, QD.OUTS, K, mutant=m)
        assert (mlab != lab).any() or (mbits != bits).any(), (K, m)
