"""The depth head on packed batches, the host side (include/vitx.h "packed batches", the depth head): vitx_pack_depth_check -- its tables against the
numpy restatement of tests/pack_depth_data.py and every refusal --, the device table of vitx_depth_pack_tables, and the fixtures of
tests/test_gpu_pack_depth.py: the reference (the host function image by image) pinned to depth_data.depth, and every mutant of pack_depth_data visible
on the pack.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest

import depth_data as XD
import pack_data as KD
import pack_depth_data as QD
import rect_data as RD


def _model(pkg, binding, kind="p16"):
    return binding.Model(RD.fixture_file(pkg, kind))


def test_check_returns_the_tables(pkg, binding):
    """pix0, fine0, ftile0 and otile0 of mixed shapes, at the images' own shapes and at given output shapes, for every u, equal the restatement; any
    table may be NULL."""
    for kind in ("p16", "p14r4"):
        model = _model(pkg, binding, kind)
        P = model.hparams.patch_size
        shapes = KD.mixed_shapes(P) + [(9 * P, 20 * P), (P, 70 * P)]                     # more than one tile across and down
        grids = [(h // P, w // P) for h, w in shapes]
        for u in QD.US:
            for outs in (None, QD.original_like(shapes), [(h * 3 + 1, w * 2) for h, w in shapes]):
                want = QD.tables(grids, shapes if outs is None else outs, u)
                got = binding.pack_depth_check(model, shapes, outs, 21, u, int(want[0][-1]))               # max_pixels is inclusive
                assert [a.dtype for a in got] == [np.int64, np.int64, np.int32, np.int32]
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), (kind, u, outs)
            assert want[3][-1] > len(shapes) and (u == 1 or want[2][-1] > len(shapes))
        s = np.asarray(shapes, np.int32)
        i32p = C.POINTER(C.c_int32)
        assert binding.lib().vitx_pack_depth_check(model._h, s.ctypes.data_as(i32p), None, len(shapes), 21, 4, 10 ** 9, None, None, None, None) == 0
        model.close()
    # the kernel tests' pack: the restatement's own numbers
    pix0, fine0, ftile0, otile0 = QD.tables(QD.GRIDS, QD.OUTS[4], 4)
    assert pix0.tolist() == [0, 35, 9720, 10825, 13961, 15257, 15273] and fine0.tolist() == [0, 16, 9488, 9584, 12720, 12800, 12816]
    assert ftile0.tolist() == [0, 1, 41, 42, 58, 60, 61] and otile0.tolist() == [0, 1, 16, 20, 24, 26, 27]


def test_device_table_rows(binding):
    """vitx_depth_pack_tables: the two running tile counts, then per image lrow, orow, grid, fine plane, output, fine0 and pix0 in two words each, the bits
    of f32(g) / f32(fine) and of f32(fine) / f32(out) per axis."""
    n = len(QD.GRIDS)
    lrow = np.cumsum([5 + gh * gw for gh, gw in QD.GRIDS]) - [gh * gw for gh, gw in QD.GRIDS]
    orow = np.arange(1, n + 1)
    for u in QD.US:
        outs = QD.OUTS[u]
        tab, ft, ot, cells = binding.depth_pack_tables(QD.GRIDS, outs, lrow, orow, u)
        pix0, fine0, ftile0, otile0 = QD.tables(QD.GRIDS, outs, u)
        assert np.array_equal(tab[:n + 1], ftile0) and np.array_equal(tab[n + 1:2 * n + 2], otile0) and (ft, ot) == (ftile0[-1], otile0[-1])
        bits = lambda a, b: int((np.float32(a) / np.float32(b)).view(np.int32))
        for i, ((gh, gw), (oh, ow)) in enumerate(zip(QD.GRIDS, outs)):
            fh, fw = u * gh, u * gw
            want = [lrow[i], orow[i], gh, gw, fh, fw, oh, ow, int(fine0[i]), 0, int(pix0[i]), 0, bits(gh, fh), bits(gw, fw), bits(fh, oh), bits(fw, ow)]
            assert tab[2 * n + 2 + 16 * i:2 * n + 18 + 16 * i].tolist() == want, (u, i)
        # the widest window: a 16 x 16 fine tile of the (16, 37) grid touches min(g, (T - 1) / u + 4) cells per axis
        assert cells == min(16, 15 // u + 4) * min(37, 15 // u + 4), u
    A = binding.VitxError
    for bad in (dict(outs=[(1, 3)]), dict(outs=[(8, 11)], u=4), dict(u=3), dict(outs=[(8193, 3)]), dict(grids=[(0, 3)])):
        a = dict(grids=[(2, 3)], outs=[(8, 12)], u=1); a.update(bad)
        with pytest.raises(A):
            binding.depth_pack_tables(a["grids"], a["outs"], [0], [0], a["u"])
    binding.depth_pack_tables([(2, 3)], [(8, 12)], [0], [0], 4)


def test_check_refusals(pkg, binding):
    """Every refusal a forward call adds while a depth head is set, by code and word."""
    model = _model(pkg, binding)
    P = model.hparams.patch_size
    shapes = KD.mixed_shapes(P)
    px = sum(h * w for h, w in shapes)
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED

    def refused(code, word, *a):
        with pytest.raises(binding.VitxError) as ei:
            binding.pack_depth_check(model, *a)
        assert ei.value.code == code and word in str(ei.value), (str(ei.value), a)

    own = [tuple(s) for s in shapes]
    for u in QD.US:
        for i, (h, w) in enumerate(shapes):
            fh, fw = u * (h // P), u * (w // P)
            if fh > 1:
                refused(A, "upsampling only", shapes, own[:i] + [(fh - 1, w)] + own[i + 1:], 21, u, 10 ** 9)     # a side below the fine plane
            if fw > 1:
                refused(A, "upsampling only", shapes, own[:i] + [(h, fw - 1)] + own[i + 1:], 21, u, 10 ** 9)
        binding.pack_depth_check(model, shapes, [(u * (h // P), u * (w // P)) for h, w in shapes], 21, u, 10 ** 9)   # the fine plane itself is the lower bound
    binding.pack_depth_check(model, shapes[:1], [(QD.MAX_OUT, QD.MAX_OUT)], 21, 4, QD.MAX_OUT ** 2)          # 8192 the upper
    refused(A, "upsampling only", shapes[:1], [(QD.MAX_OUT + 1, P)], 21, 4, 10 ** 12)
    refused(A, "upsampling only", shapes[:1], [(P, QD.MAX_OUT + 1)], 21, 4, 10 ** 12)
    wide = [(P, 2049 * P)]                                                                                   # a fine side above 8192 at u = 4, inside at u = 2
    refused(U, "fine plane", wide, [(QD.MAX_OUT, QD.MAX_OUT)], 21, 4, 10 ** 12)
    refused(U, "fine plane", [(2049 * P, P)], None, 21, 4, 10 ** 12)
    binding.pack_depth_check(model, wide, [(4, QD.MAX_OUT)], 21, 2, 10 ** 12)
    refused(A, "images", shapes, own[:-1], 21, 4, 10 ** 9)                                                   # n mismatch
    refused(A, "images", shapes, own + own[:1], 21, 4, 10 ** 9)
    binding.pack_depth_check(model, shapes, None, 21, 4, px)
    refused(A, "max_pixels", shapes, None, 21, 4, px - 1)                                                    # one pixel too many
    refused(A, "max_pixels", shapes, own[:-1] + [(own[-1][0], own[-1][1] + 1)], 21, 4, px + own[-1][0] - 1)
    refused(A, "max_pixels", shapes, None, 21, 4, 0)
    refused(A, "bins", shapes, None, 0, 4, 10 ** 9)
    refused(U, "bins", shapes, None, 257, 4, 10 ** 9)
    binding.pack_depth_check(model, shapes, None, 256, 4, 10 ** 9)
    for u in (0, 3, 8):
        refused(U, "upsample", shapes, None, 21, u, 10 ** 9)
    refused(A, "patch size", [(P + 1, P)], None, 21, 4, 10 ** 9)                                             # vitx_pack_check's refusals come first
    model.close()


@pytest.mark.parametrize("u", QD.US)
@pytest.mark.parametrize("K", QD.KS)
def test_reference_is_the_restatement(binding, K, u):
    """pack_depth_data.reference (vitx_depth_host image by image, planes and maps end to end) equals depth_data.depth on the kernel tests' pack, on hostile
    and on ordinary data, behind both counts of prefix rows, in both orders, with offsets and without; the prefix rows, the offsets' row 0 and the pad
    columns do hold NaN and +inf."""
    for make, Tp, rev, with_off in ((XD.hostile, 1, False, True), (XD.hostile, 5, True, True), (XD.normal, 5, False, True), (XD.hostile, 1, False, False)):
        grids, outs = (QD.GRIDS[::-1], QD.OUTS[u][::-1]) if rev else (QD.GRIDS, QD.OUTS[u])
        lg, off, bins, lrow, orow = QD.pack_logits(grids, K, Tp, seed=K, make=make)
        assert lg.shape[0] == sum(Tp + gh * gw for gh, gw in grids) and off.shape[0] == len(grids) + 1
        for i in range(len(grids)):
            assert not np.isfinite(lg[lrow[i] - Tp:lrow[i]]).any()
        assert not np.isfinite(lg[:, K:]).any() and not np.isfinite(off[0]).any() and not np.isfinite(off[:, K:]).any()
        o = off if with_off else None
        d, f = QD.reference(binding, lg, o, bins, lrow, orow, grids, outs, K, u)
        want_d, want_f = QD.restated(lg, o, bins, lrow, orow, grids, outs, K, u, Tp)
        pix0, fine0 = QD.tables(grids, outs, u)[:2]
        assert d.size == pix0[-1] and f.size == fine0[-1]
        assert np.array_equal(f, want_f) and np.array_equal(d, want_d), (K, u, make.__name__, Tp, rev, with_off)


@pytest.mark.parametrize("u", QD.US)
@pytest.mark.parametrize("K", [5, 64])
def test_the_pack_tells_the_mutants_apart(K, u):
    """Each mistake of pack_depth_data.MUTANTS changes at least one depth or fine cell of the pack, so the GPU tests cannot pass with it."""
    for Tp in QD.PREFIXES:
        lg, off, bins, lrow, orow = QD.pack_logits(QD.GRIDS, K, Tp, seed=K)
        d, f = QD.restated(lg, off, bins, lrow, orow, QD.GRIDS, QD.OUTS[u], K, u, Tp)
        for m in QD.MUTANTS:
            md, mf = QD.restated(lg, off, bins, lrow, orow, QD.GRIDS, QD.OUTS[u], K, u, Tp, mutant=m)
            assert (md != d).any() or (mf != f).any(), (K, u, Tp, m)


def test_the_four_layer_fixture(pkg, binding):
    """pack_depth_data.l4_file: four layers, 4 heads of 32, four registers, patch 14 -- and a packed context would take it (vitx_pack_check)."""
    model = binding.Model(QD.l4_file(pkg))
    hp = model.hparams
    assert (hp.num_hidden_layers, hp.num_attention_heads, hp.hidden_size, hp.patch_size) == (QD.L4_LAYERS, QD.L4_HEADS, 128, 14)
    row0 = binding.pack_check(model, KD.mixed_shapes(14), 256, 8)
    assert row0[1] - row0[0] == 1 + QD.L4_REGISTERS + 1
    model.close()


def test_binding_argument_errors(pkg, binding):
    """What the binding refuses before it calls the library."""
    pack = binding.PackContext.__new__(binding.PackContext)                  # no device: these calls never reach the library
    for kw in (dict(wp=np.zeros(8, np.float32), bins=np.ones(8, np.float32)), dict(wp=np.zeros((3, 8), np.float32)),
               dict(wp=np.zeros((3, 8), np.float32), bins=np.ones(4, np.float32)), dict(wp=np.zeros((3, 8), np.float32), bins=np.ones(3, np.float32), wc=np.zeros((3, 4), np.float32)),
               dict(wp=np.zeros((3, 8), np.float32), bins=np.ones(3, np.float32), bias=np.zeros(2, np.float32))):
        with pytest.raises(ValueError):
            pack.depth_set(**kw)
    with pytest.raises(binding.VitxError) as ei:
        pack.depth_read()
    assert ei.value.code == binding.ERR_ARG
    with pytest.raises(ValueError):
        binding.op_depth_fine_packed(0, 128, 0, 0, [(1, 1), (2, 3)], [0], None, 5, 4, 0)
    with pytest.raises(ValueError):
        binding.op_depth_fine_packed(0, 128, 0, 0, [(1, 1)], [0], [0, 1], 5, 4, 0)
    with pytest.raises(ValueError):
        binding.op_depth_resize_packed(0, [(1, 1), (2, 3)], [(2, 2)], 0.0, 1.0, 0)
    with pytest.raises(ValueError):
        binding.depth_pack_tables([(1, 1)], [(1, 1), (2, 2)], [0], [0], 1)
    model = _model(pkg, binding)
    P = model.hparams.patch_size
    with pytest.raises(binding.VitxError) as ei:
        binding.pack_depth_check(model, [(P, P), (P, P)], [(P, P)], 5, 4, 10 ** 6)
    assert ei.value.code == binding.ERR_ARG
    model.close()
