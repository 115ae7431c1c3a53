"""The depth head on packed batches on the MI355X (include/vitx.h "packed batches", the depth head).
1. The two packed kernels alone (vitx_op_depth_fine_packed, vitx_op_depth_resize_packed) against the host function vitx_depth_host image by image, bit
   for bit on the fine planes and the maps, on the hostile pack of tests/pack_depth_data.py: every K and u, poisoned prefix rows, the reverse order,
   with offsets and without, canaries around both outputs on and off the 16-byte boundary, the inputs unchanged.
2. Neighbour independence: an image alone, first, last and beside NaN neighbours, and against the fixed-shape ops on it alone; the (2, 3) grid
   beside (16, 37) at K = 256, u = 1 (the launch stages its windows in chunks of bins then, alone it does not).
3. Every shape of depth_data.cases() as a uniform pack against the fixed-shape ops (the one shared tile body each).
4. Op refusals: nothing is written.
5. The head on a packed context end to end, on the four-layer fixture of pack_depth_data (4 heads of 32: both context types run the generic attention).
6. Invariants: the forward's own outputs, both heads at once, launches, scratch, a refused set, vitx_pack_depth_out and refused calls, the device
   entry point.
7. vit_cli.py --pack --depth-head.

Where this departs from the words of the issue, and why:
 * "the measure and bound test_gpu_depth.py::test_forward_end_to_end applies, imported": that test has them inline, not under a name, and it applies them
   to the float64 product of RNE(the SAME forward's features) x RNE(W) -- an f32 inner-product bound, (Dc + 1) 2^-24 sum |a_i w_i| (+ |bias|), which no
   result can meet against features from another arithmetic.  A packed context returns the last layer's final-norm rows only, so here that bound is
   applied, restated, where those are the operand (VITX_DEPTH_NORM, the last layer).  Against the float64 forward of tests/ref64.py every case is held to
   rms(d) / rms <= pack_data.TOKEN_GATE, the gate tests/test_gpu_pack.py holds the final norm's patch rows to (the bf16 stage gate of ref64.py): the
   logits are a fixed linear map of such rows, or of the raw stream that gate was made for, and the reference rounds operand and weights as the engine does.
   Raw and four-layer operands are pinned exactly by the uniform pack, whose kept logits, offsets, planes and maps equal a rectangular context's bit
   for bit -- the context test_gpu_depth.py checks against the exact bound.
 * the micro fixtures have two layers; "four layers" runs on pack_depth_data.l4_file, the same recipe drawn with four.
 * vitx_pack_depth_check takes one n, so its n-mismatch refusal is the binding's (tests/test_cpu_pack_depth.py); the forward's own is tested here.
 * the CLI writes a map at the ORIGINAL's size and the per-image --img-fit run one at the preprocessed size: they can be equal only for originals that
   already have their fitted shape, so the test draws such originals (and checks the sizes on two golden assets, whose originals do not)."""
import ctypes as C

import numpy as np
import pytest

import arch_data as AD
import depth_data as XD
import pack_data as KD
import pack_depth_data as QD
import poison_data as PZ
import prefix_data as PD
import rect_data as RD
import ref64 as R64
from test_gpu_arch import ROUND
from test_gpu_depth import CAN, HI, K_E2E, LO, _bits, _head

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. the two kernels on given logits
def _run_packed(binding, torch, d_lg, ld, d_off, d_bins, grids, outs, lrow, orow, K, u, shift=0):
    """(depth bits [px], fine bits [fpx]) between poisoned canaries; shift: floats by which both outputs start off their buffers' 16-byte boundary."""
    pix0, fine0 = QD.tables(grids, outs, u)[:2]
    px, fpx, o = int(pix0[-1]), int(fine0[-1]), 16 + shift
    d_fine = torch.full((o + fpx + 16,), CAN, dtype=torch.float32, device="cuda")
    d_out = torch.full((o + px + 16,), CAN, dtype=torch.float32, device="cuda")
    binding.op_depth_fine_packed(d_lg.data_ptr(), ld, d_off.data_ptr() if d_off is not None else 0, d_bins.data_ptr(), grids, lrow, orow if d_off is not None else None,
                                 K, u, d_fine.data_ptr() + 4 * o)
    binding.op_depth_resize_packed(d_fine.data_ptr() + 4 * o, QD.fines(grids, u), outs, LO, HI, d_out.data_ptr() + 4 * o)
    torch.cuda.synchronize()
    f, d = d_fine.cpu().numpy(), d_out.cpu().numpy()
    assert (f[:o] == CAN).all() and (f[o + fpx:] == CAN).all(), "a canary of the fine planes was written"
    assert (d[:o] == CAN).all() and (d[o + px:] == CAN).all(), "a canary of the depth maps was written"
    return d[o:o + px].view(np.uint32), f[o:o + fpx].view(np.uint32)


@pytest.mark.parametrize("u", QD.US)
@pytest.mark.parametrize("K", QD.KS)
def test_packed_kernels_equal_the_host_function_bit_for_bit(binding, torch_gpu, K, u):
    """The hostile pack behind 1 and 5 poisoned prefix rows per image; in reverse order; with offsets (image i's row is i + 1, row 0 NaN) and without;
    outputs on and off the 16-byte boundary; logits, offsets and bins are what they were afterwards."""
    torch = torch_gpu
    for Tp in QD.PREFIXES:
        for grids, outs in ((QD.GRIDS, QD.OUTS[u]), (QD.GRIDS[::-1], QD.OUTS[u][::-1])):
            lg, off, bins, lrow, orow = QD.pack_logits(grids, K, Tp, seed=K)
            d_lg, d_off, d_bins = torch.from_numpy(lg).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(bins).cuda()
            for with_off in (True, False):
                want_d, want_f = QD.reference(binding, lg, off if with_off else None, bins, lrow, orow, grids, outs, K, u)
                for shift in (0, 1) if with_off else (1,):
                    d, f = _run_packed(binding, torch, d_lg, lg.shape[1], d_off if with_off else None, d_bins, grids, outs, lrow, orow, K, u, shift)
                    tag = (K, u, Tp, grids[0], with_off, shift)
                    assert np.array_equal(f, want_f), (tag, np.argwhere(f != want_f)[:5].tolist())
                    assert np.array_equal(d, want_d), (tag, np.argwhere(d != want_d)[:5].tolist())
            assert np.array_equal(_bits(d_lg.cpu().numpy()), _bits(lg)) and np.array_equal(_bits(d_off.cpu().numpy()), _bits(off)) and np.array_equal(d_bins.cpu().numpy(), bins)


# ------------------------------------------------------------------------------------------------ 2. neighbour independence
@pytest.mark.parametrize("K,u", [(256, 1), (64, 2), (5, 4)])
def test_an_image_does_not_depend_on_its_neighbours(binding, torch_gpu, K, u):
    """Every image's plane and map in the pack equal those of the fixed-shape ops on the image alone, of a pack of that image alone, of packs with the
    image first and last, and of a pack where it stands between two images whose logits are all NaN.  At K = 256, u = 1 the (16, 37) grid's window
    of 16 x 19 cells makes the whole launch stage its logits in chunks of 52 bins; the (2, 3) grid alone takes all 256 at once: the same bits say
    that no bit depends on the chunk."""
    torch = torch_gpu
    grids, outs, n = QD.GRIDS, QD.OUTS[u], len(QD.GRIDS)
    lg, off, bins, lrow, orow = QD.pack_logits(grids, K, 1, seed=K)
    ld = lg.shape[1]
    nan_at = lg.shape[0]                                                    # a block of NaN rows behind the pack: the NaN neighbours' logits
    lg = np.concatenate([lg, np.full((16 * 37, ld), np.nan, np.float32)])
    d_lg, d_off, d_bins = torch.from_numpy(lg).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(bins).cuda()
    d, f = _run_packed(binding, torch, d_lg, ld, d_off, d_bins, grids, outs, lrow, orow, K, u)
    pix0, fine0 = QD.tables(grids, outs, u)[:2]

    def sub(ids, nan_ids=()):
        """The pack of images `ids` of the same buffers (negative: a NaN image with the grid and output of image -id - 1): {id: (depth, fine)}."""
        g = [grids[i if i >= 0 else -i - 1] for i in ids]; o = [outs[i if i >= 0 else -i - 1] for i in ids]
        lr = np.asarray([lrow[i] if i >= 0 else nan_at for i in ids], np.int32); orr = np.asarray([orow[i if i >= 0 else -i - 1] for i in ids], np.int32)
        dd, ff = _run_packed(binding, torch, d_lg, ld, d_off, d_bins, g, o, lr, orr, K, u)
        p0, f0 = QD.tables(g, o, u)[:2]
        return {i: (dd[p0[j]:p0[j + 1]], ff[f0[j]:f0[j + 1]]) for j, i in enumerate(ids)}

    for i, ((gh, gw), (oh, ow)) in enumerate(zip(grids, outs)):
        mine = (d[pix0[i]:pix0[i + 1]], f[fine0[i]:fine0[i + 1]])
        same = lambda got, what: (np.array_equal(got[0], mine[0]) and np.array_equal(got[1], mine[1]), (K, u, i, what))
        # the fixed-shape ops on the image alone
        d_one = torch.from_numpy(QD.image_rows(lg, lrow, grids, i)).cuda()
        d_o1 = torch.from_numpy(np.ascontiguousarray(off[orow[i]:orow[i] + 1])).cuda()
        d_f = torch.full((u * gh * u * gw,), CAN, dtype=torch.float32, device="cuda")
        d_d = torch.full((oh * ow,), CAN, dtype=torch.float32, device="cuda")
        binding.op_depth_fine(d_one.data_ptr(), ld, d_o1.data_ptr(), d_bins.data_ptr(), 1, gh, gw, K, u, d_f.data_ptr())
        binding.op_depth_resize(d_f.data_ptr(), 1, u * gh, u * gw, oh, ow, LO, HI, d_d.data_ptr())
        torch.cuda.synchronize()
        ok, tag = same((_bits(d_d.cpu().numpy()), _bits(d_f.cpu().numpy())), "fixed-shape ops"); assert ok, tag
        others = [j for j in range(n) if j != i]
        ok, tag = same(sub([i])[i], "alone"); assert ok, tag
        ok, tag = same(sub([i] + others)[i], "first"); assert ok, tag
        ok, tag = same(sub(others + [i])[i], "last"); assert ok, tag
        big = -2                                                             # a NaN image of the (16, 37) grid on either side
        got = sub([big, i, big])
        assert np.isnan(got[big][1].view(np.float32)).all(), "the NaN neighbour is not NaN"
        ok, tag = same(got[i], "between NaN neighbours"); assert ok, tag
    if (K, u) == (256, 1):
        small = QD.GRIDS.index((2, 3))
        alone = sub([small])[small]
        assert np.array_equal(alone[0], d[pix0[small]:pix0[small + 1]]) and np.array_equal(alone[1], f[fine0[small]:fine0[small + 1]])
        assert len(np.unique(alone[1])) > 2


# ------------------------------------------------------------------------------------------------ 3. uniform packs
def test_a_uniform_pack_equals_the_fixed_shape_kernels(binding, torch_gpu):
    """Every shape of depth_data.cases() through the packed launchers as a pack of n images of that shape, lrow[i] = i gh gw, orow[i] = i: bit for bit
    vitx_op_depth_fine and vitx_op_depth_resize on the same rows -- one tile body behind each pair of kernels."""
    torch = torch_gpu
    for c, (gh, gw, u, K, oh, ow, n) in enumerate(XD.cases()):
        ld = XD.pad_to(K)
        lg, off, bins = XD.hostile(n, gh, gw, K, ld, seed=c)
        d_lg, d_off, d_bins = torch.from_numpy(lg).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(bins).cuda()
        d_f = torch.full((n * u * gh * u * gw,), CAN, dtype=torch.float32, device="cuda")
        d_d = torch.full((n * oh * ow,), CAN, dtype=torch.float32, device="cuda")
        binding.op_depth_fine(d_lg.data_ptr(), ld, d_off.data_ptr(), d_bins.data_ptr(), n, gh, gw, K, u, d_f.data_ptr())
        binding.op_depth_resize(d_f.data_ptr(), n, u * gh, u * gw, oh, ow, LO, HI, d_d.data_ptr())
        d, f = _run_packed(binding, torch, d_lg, ld, d_off, d_bins, [(gh, gw)] * n, [(oh, ow)] * n, np.arange(n) * gh * gw, np.arange(n), K, u, shift=c & 1)
        assert np.array_equal(f, _bits(d_f.cpu().numpy())) and np.array_equal(d, _bits(d_d.cpu().numpy())), (gh, gw, u, K, oh, ow, n)


# ------------------------------------------------------------------------------------------------ 4. op refusals
def test_op_refusals(binding, torch_gpu):
    """vitx_op_depth_fine's and vitx_op_depth_resize's checks, image by image, before anything is launched: nothing is written."""
    torch = torch_gpu
    d_lg = torch.zeros((64, 128), dtype=torch.float32, device="cuda")
    d_bins = torch.ones((256,), dtype=torch.float32, device="cuda")
    d_f = torch.full((4096,), CAN, dtype=torch.float32, device="cuda")
    d_o = torch.full((4096,), CAN, dtype=torch.float32, device="cuda")
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    for code, args in ((A, dict(K=0)), (U, dict(K=257, ld=384)), (A, dict(ld=20)), (A, dict(lrow=[0, -1])), (A, dict(grids=[(1, 1), (0, 3)])), (U, dict(u=3)),
                       (U, dict(grids=[(1, 1), (1, 2049)], u=4))):
        a = dict(ld=128, grids=[(1, 1), (2, 3)], lrow=[1, 3], K=21, u=4)
        a.update(args)
        with pytest.raises(binding.VitxError) as ei:
            binding.op_depth_fine_packed(d_lg.data_ptr(), a["ld"], 0, d_bins.data_ptr(), a["grids"], a["lrow"], None, a["K"], a["u"], d_f.data_ptr())
        assert ei.value.code == code, (args, str(ei.value))
    with pytest.raises(binding.VitxError):
        binding.op_depth_fine_packed(d_lg.data_ptr() + 4, 128, 0, d_bins.data_ptr(), [(1, 1)], [0], None, 21, 4, d_f.data_ptr())      # logits off the 16-byte boundary
    with pytest.raises(binding.VitxError):
        binding.op_depth_fine_packed(d_lg.data_ptr(), 128, d_lg.data_ptr(), d_bins.data_ptr(), [(1, 1)], [0], [-1], 21, 4, d_f.data_ptr())
    for code, args in ((U, dict(outs=[(4, 4), (7, 12)])), (U, dict(outs=[(4, 4), (8, 8193)])), (A, dict(lo=3.0, hi=2.0)), (A, dict(lo=float("nan"))), (A, dict(fines=[(4, 4), (0, 12)]))):
        a = dict(fines=[(4, 4), (8, 12)], outs=[(5, 7), (17, 65)], lo=LO, hi=HI)
        a.update(args)
        with pytest.raises(binding.VitxError) as ei:
            binding.op_depth_resize_packed(d_f.data_ptr(), a["fines"], a["outs"], a["lo"], a["hi"], d_o.data_ptr())
        assert ei.value.code == code, (args, str(ei.value))
    torch.cuda.synchronize()
    assert (d_f.cpu().numpy() == CAN).all() and (d_o.cpu().numpy() == CAN).all()


# ------------------------------------------------------------------------------------------------ 5. the head on a packed context
U_E2E, LO_E2E, HI_E2E = 4, 3.0, 7.0
ALL4 = [0, 1, 2, 3]
_T, _REF = {}, {}


def _tensors(pkg):
    if "t" not in _T:
        _T["t"] = PD.file_tensors(pkg, QD.l4_file(pkg))
    return _T["t"]


def _ref_rows(pkg, binding, dtype, norm, sel):
    """Per image of the mixed pack, from ref64.forward64 at its own shape with the operand rounding of `dtype`: (patch operand rows [gh gw][Dc], class
    operand row [Dc]) float64 -- the stream that leaves each selected layer (raw) or its final norm, rounded as the engine rounds the head's operand."""
    t = _tensors(pkg)
    if dtype not in _REF:
        _REF[dtype] = [R64.forward64(t, im[None], QD.L4_HEADS, wround=ROUND[dtype], uround=ROUND[dtype], binding=binding)["trace"][1:, 0]
                       for im in KD.pack_of(KD.mixed_shapes(14))]
    eps = float(np.float32(AD.arch_of(t)[1]))
    T = 1 + QD.L4_REGISTERS
    f8 = lambda a: np.asarray(a, np.float64)
    out = []
    for tr in _REF[dtype]:
        rows = [f8(ROUND[dtype](R64.layernorm64(tr[l], f8(t["norm.weight"]), f8(t["norm.bias"]), eps) if norm else tr[l])) for l in sel]
        a = np.concatenate(rows, axis=1)
        out.append((a[T:], a[0]))
    return out


def _host_maps(binding, kept, koff, bins, shapes, outs, P, u, lo, hi):
    """The host function on each image's kept logits and offsets (padded to ld = 128 with NaN columns): lists of depth bits and fine bits."""
    dm, fn = [], []
    for i, (lg, (h, w), (oh, ow)) in enumerate(zip(kept, shapes, outs)):
        gh, gw = h // P, w // P
        K = lg.shape[1]
        lgp = np.full((gh * gw, XD.pad_to(K)), np.nan, np.float32); lgp[:, :K] = lg
        ofp = np.full((1, XD.pad_to(K)), np.nan, np.float32); ofp[0, :K] = koff[i]
        d, f = binding.depth_host(lgp, ofp, bins, 1, gh, gw, K, u, oh, ow, lo, hi)
        dm.append(_bits(d[0])); fn.append(_bits(f[0]))
    return dm, fn


def _run(pack, imgs):
    """([(depth, fine, kept logits, offsets) per image], probs, logits) of one forward."""
    p, lg = pack.forward(imgs)
    dm, fn, kept, koff = pack.depth_read()
    return [(dm[i], fn[i], kept[i], koff[i]) for i in range(len(imgs))], p, lg


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _rel_rms(got, ref):
    return float(np.sqrt(((got - ref) ** 2).mean()) / np.sqrt((ref ** 2).mean()))


@pytest.mark.parametrize("dtype", [1, 0], ids=["bf16", "f16"])
@pytest.mark.parametrize("layers", [None, ALL4], ids=["last", "0+1+2+3"])
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "norm"])
def test_pack_forward_end_to_end(pkg, binding, torch_gpu, norm, layers, dtype):
    """The mixed pack of pack_data.mixed_shapes on the four-layer fixture, K = 21, u = 4, with a class half and without.  The maps and fine planes
    equal vitx_depth_host on the kept logits and offsets bit for bit; the kept logits and offsets lie within pack_data.TOKEN_GATE (rms(d) / rms) of
    the float64 forward of tests/ref64.py and, where the pack's own features are the operand (VITX_DEPTH_NORM, the last layer), under the f32
    inner-product bound of the float64 product of RNE(features) x RNE(W) (the module docstring says why these two); without a class half the
    offsets are the bias; the forward's probabilities and logits are those of the context without a head; launches grow by m + 5 / m + 3."""
    model = binding.Model(QD.l4_file(pkg))
    P, D, L_ = model.hparams.patch_size, model.hparams.hidden_size, model.hparams.num_hidden_layers
    shapes = KD.mixed_shapes(P)
    imgs = KD.pack_of(shapes)
    n = len(imgs)
    sel = [L_ - 1] if layers is None else layers
    Dc = D * len(sel)
    wp, wc, bias, bins = _head(K_E2E, Dc, seed=len(sel), scale=0.25 if norm else 0.05)
    pack = binding.PackContext(model, device=0, max_tokens=256, max_images=2 * n, dtype=dtype)
    own_feats = norm and layers is None
    if own_feats:
        pack.feat_enable(cls=True, tokens=True)
    plain = pack.forward(imgs)                                     # also builds every grid's tables: the launch counts below compare like with like
    plain = pack.forward(imgs)
    base_launches, base_scratch = pack.launches[0], pack.scratch_bytes
    assert pack.depth_device() == 0 and pack.depth_scratch_bytes() == 0
    ref = _ref_rows(pkg, binding, dtype, norm, sel)
    f64 = lambda x: np.asarray(x, np.float64)
    wpr, wcr = f64(binding.round_operand(wp, dtype)), f64(binding.round_operand(wc, dtype))
    for cls_half in (True, False):
        pack.depth_set(wp, wc if cls_half else None, bias, bins, layers, U_E2E, LO_E2E, HI_E2E, norm=norm, logits=True, fine=True)
        assert pack.depth_device() != 0 and pack.scratch_bytes > base_scratch + pack.depth_scratch_bytes() > base_scratch
        res, p, lg = _run(pack, imgs)
        assert np.array_equal(_bits(p), _bits(plain[0])) and np.array_equal(_bits(lg), _bits(plain[1])), "the head moved the forward's own outputs"
        assert pack.launches[0] == base_launches + len(sel) + (5 if cls_half else 3)
        want_d, want_f = _host_maps(binding, [r[2] for r in res], [r[3] for r in res], bins, shapes, shapes, P, U_E2E, LO_E2E, HI_E2E)
        worst_l = worst_o = 0.0
        for i, (h, w) in enumerate(shapes):
            gh, gw = h // P, w // P
            depth, fine, kept, koff = res[i]
            assert depth.shape == (h, w) and fine.shape == (U_E2E * gh, U_E2E * gw) and kept.shape == (gh * gw, K_E2E) and koff.shape == (K_E2E,)
            assert np.array_equal(_bits(fine), want_f[i]) and np.array_equal(_bits(depth), want_d[i]), (cls_half, i)
            assert np.isfinite(depth).all() and depth.min() >= LO_E2E and depth.max() <= HI_E2E
            worst_l = max(worst_l, _rel_rms(kept, ref[i][0] @ wpr.T))
            if cls_half:
                worst_o = max(worst_o, _rel_rms(koff, ref[i][1] @ wcr.T + f64(bias)))
            else:
                assert np.array_equal(_bits(koff), _bits(bias)), "without a class half the offsets are the bias"
        print(f"{'norm' if norm else 'raw'} {len(sel)} layers dtype {dtype} class half {cls_half}: kept logits rms(d) / rms {worst_l:.3e}, offsets {worst_o:.3e} (gate {KD.TOKEN_GATE})")
        assert worst_l <= KD.TOKEN_GATE and worst_o <= KD.TOKEN_GATE
        assert len(np.unique(np.concatenate([r[0].ravel() for r in res]))) > 2, "constant depth maps check nothing"
        if own_feats:
            cls, tok = pack.feat_read()
            for i in range(n):
                a = f64(binding.round_operand(tok[i].reshape(-1, D), dtype))
                bound = (Dc + 1) * 2.0 ** -24 * (np.abs(a) @ np.abs(wpr).T)
                assert (np.abs(res[i][2] - a @ wpr.T) <= bound).all(), "the patch logits are not the products of RNE(features) x RNE(Wp)"
                if cls_half:
                    ac = f64(binding.round_operand(cls[i], dtype))
                    bound = (Dc + 1) * 2.0 ** -24 * (np.abs(ac) @ np.abs(wcr).T + np.abs(bias))
                    assert (np.abs(res[i][3] - (ac @ wcr.T + f64(bias))) <= bound).all(), "the offsets are not bias + RNE(class features) x RNE(Wc)"
    # off: the buffers go, the forward is the one it was
    pack.depth_set(None)
    assert pack.scratch_bytes == base_scratch and pack.depth_device() == 0 and pack.depth_scratch_bytes() == 0
    off = pack.forward(imgs)
    assert pack.launches[0] == base_launches and np.array_equal(_bits(off[0]), _bits(plain[0]))
    pack.close(); model.close()


@pytest.mark.parametrize("dtype", [1, 0], ids=["bf16", "f16"])
def test_uniform_pack_equals_the_rect_context(pkg, binding, torch_gpu, dtype):
    """Five images of pack_data.UNIFORM_SHAPE: raw and VITX_DEPTH_NORM, four layers and the last alone, with a class half and without -- maps, fine planes,
    kept logits and offsets of the pack equal those of a rectangular Context(img_shape=...) with the same head (head dim 32: both run the generic
    attention arithmetic)."""
    model = binding.Model(QD.l4_file(pkg))
    P, D = model.hparams.patch_size, model.hparams.hidden_size
    shape = KD.UNIFORM_SHAPE[P]
    n = 5
    imgs = RD.images(n, *shape)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, img_shape=shape, last_layer_all_rows=1)
    pack = binding.PackContext(model, device=0, max_tokens=n * ctx.tokens, max_images=n, dtype=dtype)
    for norm in (False, True):
        for layers in (ALL4, None):
            for cls_half in (True, False):
                wp, wc, bias, bins = _head(K_E2E, D * (4 if layers else 1), seed=5, scale=0.25 if norm else 0.05)
                wc = wc if cls_half else None
                ctx.depth_set(wp, wc, bias, bins, layers, U_E2E, LO_E2E, HI_E2E, norm=norm, logits=True, fine=True)
                ctx.forward(imgs)
                depth, fine, kept, koff = ctx.depth_read(n)
                pack.depth_set(wp, wc, bias, bins, layers, U_E2E, LO_E2E, HI_E2E, norm=norm, logits=True, fine=True)
                res = _run(pack, list(imgs))[0]
                for i in range(n):
                    assert _same(res[i], (depth[i], fine[i], kept[i], koff[i])), (norm, layers, cls_half, i)
                assert len(np.unique(depth)) > 2
    ctx.close(); pack.close(); model.close()


# ------------------------------------------------------------------------------------------------ 6. invariants
def _device_floats(ptr, count):
    out = np.empty(count, np.float32)
    assert C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), 4 * count, 2) == 0
    return out


def test_neighbours_positions_and_both_heads(pkg, binding, torch_gpu):
    """On a packed context: an image's kept logits, offsets, plane and map have the same bits alone, at another position (the pack reversed) and beside
    NaN-pixel neighbours.  A dense head set beside the depth head changes neither's bits, the launches add up (m + 2 and m + 5), and turning
    either off leaves the other and gives its launches and scratch back."""
    model = binding.Model(QD.l4_file(pkg))
    P, D = model.hparams.patch_size, model.hparams.hidden_size
    shapes = KD.mixed_shapes(P)
    imgs = KD.pack_of(shapes)
    n = len(imgs)
    wp, wc, bias, bins = _head(K_E2E, 2 * D, seed=9)
    pack = binding.PackContext(model, device=0, max_tokens=256, max_images=2 * n, dtype=1)
    pack.forward(imgs)
    plain = pack.forward(imgs)
    base_launches, base_scratch = pack.launches[0], pack.scratch_bytes
    pack.depth_set(wp, wc, bias, bins, [1, 3], U_E2E, LO_E2E, HI_E2E, logits=True, fine=True)
    res = _run(pack, imgs)[0]
    depth_scratch = pack.scratch_bytes
    for i in range(n):
        assert _same(_run(pack, [imgs[i]])[0][0], res[i]), ("alone", i)
    rev = _run(pack, imgs[::-1])[0]
    for i in range(n):
        assert _same(rev[n - 1 - i], res[i]), ("reversed", i)
    sand = []
    for im in imgs:
        sand += [im, PZ.poison_images(im[None], (0,), "nan")[0]]
    sres = _run(pack, sand[:-1])[0]
    for i in range(n):
        assert _same(sres[2 * i], res[i]), ("beside NaN images", i)
    assert np.isnan(sres[1][0]).all(), "the poison did not go through"
    # the dense head beside it
    rng = np.random.default_rng(4)
    W, b = (rng.standard_normal((5, D)) * 0.25).astype(np.float32), rng.standard_normal(5).astype(np.float32)
    pack.depth_set(None)
    assert pack.scratch_bytes == base_scratch
    pack.dense_set(W, b, None, score=True, logits=True)
    pack.forward(imgs)
    dense_alone = pack.dense_read()
    dense_scratch = pack.scratch_bytes
    assert pack.launches[0] == base_launches + 1 + 2
    pack.depth_set(wp, wc, bias, bins, [1, 3], U_E2E, LO_E2E, HI_E2E, logits=True, fine=True)
    both, p, lg = _run(pack, imgs)
    dense_both = pack.dense_read()
    assert pack.launches[0] == base_launches + (1 + 2) + (2 + 5)
    assert np.array_equal(_bits(p), _bits(plain[0])) and np.array_equal(_bits(lg), _bits(plain[1]))
    assert all(_same(both[i], res[i]) for i in range(n)), "the dense head moved the depth head's bits"
    for i in range(n):
        assert np.array_equal(dense_both[0][i], dense_alone[0][i]) and _same((dense_both[1][i], dense_both[2][i]), (dense_alone[1][i], dense_alone[2][i])), ("the depth head moved the dense head's bits", i)
    pack.dense_set(None)                                                         # the depth head stays, with its tables
    assert pack.scratch_bytes == depth_scratch
    assert all(_same(a, b) for a, b in zip(_run(pack, imgs)[0], res)) and pack.launches[0] == base_launches + 2 + 5
    pack.dense_set(W, b, None, score=True, logits=True)
    pack.depth_set(None)                                                         # the dense head stays
    assert pack.scratch_bytes == dense_scratch
    pack.forward(imgs)
    assert pack.launches[0] == base_launches + 1 + 2 and np.array_equal(pack.dense_read()[0][3], dense_alone[0][3])
    pack.dense_set(None)
    assert pack.scratch_bytes == base_scratch and pack.forward(imgs) is not None and pack.launches[0] == base_launches
    pack.close(); model.close()


def test_output_shapes_and_refused_calls(pkg, binding, torch_gpu):
    """vitx_pack_depth_out to original-like sizes (28 x 70 -> 31 x 75) is consumed by one forward, the next is back at h x w; every refused call
    leaves the depth buffer as it was (canaries through vitx_pack_depth_device), consumes the shapes it was given and leaves the context usable;
    a refused set leaves the head that was set."""
    L = binding.lib()
    model = binding.Model(QD.l4_file(pkg))
    P, D = model.hparams.patch_size, model.hparams.hidden_size
    shapes = KD.mixed_shapes(P)
    imgs = KD.pack_of(shapes)
    n = len(imgs)
    outs = QD.original_like(shapes)
    px_out = sum(h * w for h, w in outs)
    wp, wc, bias, bins = _head(K_E2E, D, seed=3)
    pack = binding.PackContext(model, device=0, max_tokens=256, max_images=n, dtype=1)
    with pytest.raises(binding.VitxError):
        pack.depth_out(outs)                                                     # no head is set
    pack.depth_set(wp, wc, bias, bins, None, U_E2E, LO_E2E, HI_E2E, max_pixels=px_out, logits=True, fine=True)
    with pytest.raises(binding.VitxError) as ei:
        pack.depth_read()                                                        # before any forward with the head set
    assert ei.value.code == binding.ERR_ARG
    own = _run(pack, imgs)[0]
    pack.depth_out(outs)
    big = _run(pack, imgs)[0]
    want_d, want_f = _host_maps(binding, [r[2] for r in big], [r[3] for r in big], bins, shapes, outs, P, U_E2E, LO_E2E, HI_E2E)
    for i in range(n):
        assert big[i][0].shape == tuple(outs[i]) and _same(big[i][1:], own[i][1:]), i
        assert np.array_equal(_bits(big[i][0]), want_d[i]) and np.array_equal(_bits(big[i][1]), want_f[i]), i
    dev = _device_floats(pack.depth_device(), px_out)
    assert np.array_equal(_bits(dev), _bits(np.concatenate([r[0].ravel() for r in big]))), "the device buffer is what read returns"
    back = _run(pack, imgs)[0]                                                   # consumed: h x w again
    assert all(_same(back[i], own[i]) for i in range(n))
    # refused calls: fill the depth buffer with canaries, be refused, find the canaries
    hip = C.cdll.LoadLibrary("libamdhip64.so")
    ptr = pack.depth_device()
    CANB = np.full(px_out, 0xA5A5A5A5, np.uint32)

    def refused(code, word, call_imgs, out_shapes):
        assert hip.hipMemset(C.c_void_p(ptr), 0xA5, 4 * px_out) == 0 and hip.hipDeviceSynchronize() == 0
        if out_shapes is not None:
            pack.depth_out(out_shapes)
        with pytest.raises(binding.VitxError) as ei:
            pack.forward(call_imgs)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)
        assert hip.hipDeviceSynchronize() == 0 and np.array_equal(_bits(_device_floats(ptr, px_out)), CANB), "a refused call wrote depths"
        again = _run(pack, imgs)[0]                                              # usable, and the refused call consumed its shapes
        assert all(_same(again[i], own[i]) for i in range(n)), word

    A = binding.ERR_ARG
    refused(A, "images", imgs, outs[:-1])                                        # n differs from the forward's
    refused(A, "upsampling only", imgs, outs[:2] + [(U_E2E * (shapes[2][0] // P) - 1, shapes[2][1])] + outs[3:])
    refused(A, "upsampling only", imgs, outs[:-1] + [(QD.MAX_OUT + 1, P)])
    refused(A, "max_pixels", imgs, outs[:-1] + [(outs[-1][0], outs[-1][1] + 1)])  # one column of one image too many
    refused(A, "patch size", [np.zeros((P + 1, P, 3), np.float32)], None)        # vitx_pack_check's refusals still come first
    # a refused set leaves the head in place
    bad = wp.copy(); bad[3, 5] = np.nan
    badbins = bins.copy(); badbins[2] = 0.0
    fp = C.POINTER(C.c_float)
    q = lambda a: a.ctypes.data_as(fp) if a is not None else None
    lo, hi = C.c_float(LO_E2E), C.c_float(HI_E2E)
    U = binding.ERR_UNSUPPORTED
    big_w = np.zeros((257, D), np.float32)
    for args, code in (((q(bad), None, q(bias), q(bins), K_E2E, D, 0, 4, lo, hi, px_out, 0), A), ((q(wp), q(bad), q(bias), q(bins), K_E2E, D, 0, 4, lo, hi, px_out, 0), A),
                       ((q(wp), None, q(bias), q(badbins), K_E2E, D, 0, 4, lo, hi, px_out, 0), A), ((q(wp), None, q(bias), None, K_E2E, D, 0, 4, lo, hi, px_out, 0), A),
                       ((q(wp), None, q(bias), q(bins), K_E2E, 2 * D, 0, 4, lo, hi, px_out, 0), A), ((q(wp), None, q(bias), q(bins), K_E2E, D, 0, 4, lo, hi, px_out, 8), A),
                       ((q(wp), None, q(bias), q(bins), K_E2E, D, 0, 4, lo, hi, 0, 0), A), ((q(wp), None, q(bias), q(bins), K_E2E, D, 1 << 4, 4, lo, hi, px_out, 0), A),
                       ((q(wp), None, q(bias), q(bins), K_E2E, D, 0, 4, hi, lo, px_out, 0), A), ((None, None, None, q(bins), 3, D, 0, 4, lo, hi, px_out, 0), A),
                       ((q(wp), None, q(bias), q(bins), K_E2E, D, 0, 3, lo, hi, px_out, 0), U),
                       ((q(big_w), None, None, q(np.ones(257, np.float32)), 257, D, 0, 4, lo, hi, px_out, 0), U)):
        assert L.vitx_pack_depth_set(pack._h, *args) == code, args[4:]
    still = _run(pack, imgs)[0]
    assert all(_same(still[i], own[i]) for i in range(n))
    pack.close(); model.close()


def test_the_device_entry_point_with_a_head_set(pkg, binding, torch_gpu):
    """vitx_pack_forward_device goes through the same check of a call as vitx_pack_forward.  With a head set and depth_out(original_like):
    forward_device + depth_read give the bits of forward + depth_read, probabilities and logits included.  A forward_device refused for its output
    shapes (given for n - 1 images) is ERR_ARG, leaves the canaries in the depth buffer and the probabilities' sentinel, consumes its depth_out shapes --
    the following forward_device, at the images' own shapes, equals the host path's."""
    torch = torch_gpu
    model = binding.Model(QD.l4_file(pkg))
    P, D = model.hparams.patch_size, model.hparams.hidden_size
    shapes = KD.mixed_shapes(P)
    imgs = KD.pack_of(shapes)
    n = len(imgs)
    outs = QD.original_like(shapes)
    px_out = sum(h * w for h, w in outs)
    wp, wc, bias, bins = _head(K_E2E, D, seed=3)
    pack = binding.PackContext(model, device=0, max_tokens=256, max_images=n, dtype=1)
    pack.depth_set(wp, wc, bias, bins, None, U_E2E, LO_E2E, HI_E2E, max_pixels=px_out, logits=True, fine=True)
    own, own_p, own_lg = _run(pack, imgs)
    pack.depth_out(outs)
    big, big_p, big_lg = _run(pack, imgs)
    assert all(big[i][0].shape == tuple(outs[i]) for i in range(n)) and any(big[i][0].shape != own[i][0].shape for i in range(n))
    d_pix = torch.from_numpy(np.concatenate([a.ravel() for a in imgs])).cuda()
    SENT = -7.25

    def device_run(out_shapes):
        d_p = torch.full((n, model.num_classes), SENT, dtype=torch.float32, device="cuda")
        d_lg = torch.full((n, model.num_classes), SENT, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        if out_shapes is not None:
            pack.depth_out(out_shapes)
        pack.forward_device(d_pix.data_ptr(), shapes, d_p.data_ptr(), d_lg.data_ptr())
        dm, fn, kept, koff = pack.depth_read()
        torch.cuda.synchronize()
        return [(dm[i], fn[i], kept[i], koff[i]) for i in range(n)], d_p.cpu().numpy(), d_lg.cpu().numpy()

    got, p, lg = device_run(outs)
    assert all(_same(got[i], big[i]) for i in range(n)), "forward_device with depth_out"
    assert np.array_equal(_bits(p), _bits(big_p)) and np.array_equal(_bits(lg), _bits(big_lg))
    hip = C.cdll.LoadLibrary("libamdhip64.so")
    ptr = pack.depth_device()
    assert hip.hipMemset(C.c_void_p(ptr), 0xA5, 4 * px_out) == 0 and hip.hipDeviceSynchronize() == 0
    d_p = torch.full((n, model.num_classes), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pack.depth_out(outs[:-1])
    with pytest.raises(binding.VitxError) as ei:
        pack.forward_device(d_pix.data_ptr(), shapes, d_p.data_ptr())
    assert ei.value.code == binding.ERR_ARG and "images" in str(ei.value), str(ei.value)
    assert hip.hipDeviceSynchronize() == 0 and (_bits(_device_floats(ptr, px_out)) == 0xA5A5A5A5).all(), "a refused call wrote depths"
    assert bool((d_p == SENT).all()), "a refused call wrote probabilities"
    again, p, lg = device_run(None)
    assert all(_same(again[i], own[i]) for i in range(n)), "the refused call did not consume its shapes"
    assert np.array_equal(_bits(p), _bits(own_p)) and np.array_equal(_bits(lg), _bits(own_lg))
    pack.close(); model.close()


# ------------------------------------------------------------------------------------------------ 7. the command line
def test_cli_writes_a_depth_map_per_image_at_the_original_size(pkg, binding, torch_gpu, tmp_path):
    """vit_cli.py --pack --img-fit 32 --depth-head head.npz --depth-out PREFIX.  On two golden assets: PREFIX.<i>.npy is a float32 map at the ORIGINAL
    image's size inside the head's depth range.  On three drawn originals that already have their fitted shape (32 x 48, 32 x 80, 64 x 32 at patch 16):
    each map equals, bit for bit, the one the per-image run --img-fit 32 --depth-head --depth-out writes (the 4-head variant: both paths run the
    generic attention arithmetic)."""
    import os
    import subprocess
    import sys
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = KD.variant_file(pkg, "p16h4")
    D = binding.Model(src).hparams.hidden_size
    wp, wc, bias, bins = _head(K_E2E, 2 * D, seed=8)
    head = str(tmp_path / "head.npz")
    pkg.convert.write_depth_head(head, {"wp": wp, "wc": wc, "bias": bias, "bins": bins, "layers": [0, 1], "upsample": 4, "min_depth": LO_E2E, "max_depth": HI_E2E, "norm": False})
    cli = [sys.executable, os.path.join(root, "vit_cli.py"), "-m", src, "--dtype", "bf16", "--img-fit", "32", "--depth-head", head]
    files = [os.path.join(root, "tests", "golden", "assets", f) for f in ("tench.jpg", "kiwi.jpg")]
    prefix = str(tmp_path / "depth")
    r = subprocess.run(cli + ["--pack", "-i", ",".join(files), "--depth-out", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for i, f in enumerate(files):
        ny, nx = binding.load_image(f).shape[:2]
        dm = np.load(f"{prefix}.{i}.npy")
        assert dm.dtype == np.float32 and dm.shape == (ny, nx) and np.isfinite(dm).all() and dm.min() >= LO_E2E and dm.max() <= HI_E2E and len(np.unique(dm)) > 2, i
    assert len([ln for ln in r.stdout.split("\n") if ln.startswith(" > depth : min ")]) == len(files)
    rng = np.random.default_rng(12)
    drawn = []
    for i, (h, w) in enumerate(((32, 48), (32, 80), (64, 32))):
        path = str(tmp_path / f"drawn{i}.png")
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)
        drawn.append(path)
    prefix = str(tmp_path / "fit")
    r = subprocess.run(cli + ["--pack", "-i", ",".join(drawn), "--depth-out", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for i, (f, (h, w)) in enumerate(zip(drawn, ((32, 48), (32, 80), (64, 32)))):
        one = str(tmp_path / f"one{i}.npy")
        r1 = subprocess.run(cli + ["-i", f, "--depth-out", one], capture_output=True, text=True, timeout=300)
        assert r1.returncode == 0, r1.stderr
        a, b = np.load(f"{prefix}.{i}.npy"), np.load(one)
        assert a.shape == b.shape == (h, w) and np.array_equal(_bits(a), _bits(b)), i
