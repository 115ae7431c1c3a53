"""The dense head on packed batches on the MI355X (include/vitx.h "packed batches", the dense head).
1. The packed label kernel alone (vitx_op_dense_labels_packed) against the host function image by image, bit for bit on labels and score bits, on the
   hostile pack of tests/pack_dense_data.py: every K, poisoned prefix rows, one image, the reverse order, canaries on and off alignment, no score
   buffer; every image against vitx_op_dense_labels on it alone and beside a neighbour that forces class chunks; every shape of
   dense_data.cases() as a uniform pack against the fixed-shape kernel (the one shared tile body).
2. The head on a packed context end to end: kept logits under the f32 inner-product bound, labels and scores equal to the host function on the kept
   logits, determinism (alone, another position, a NaN neighbour), a uniform pack against the rectangular context, the forward's own outputs unchanged,
   launches, scratch, vitx_pack_dense_out, refusals that write nothing; the device entry point with a head set against the host entry point, run and
   refused."""
import ctypes as C

import numpy as np
import pytest

import dense_data as DD
import pack_data as KD
import pack_dense_data as QD
import poison_data as PZ
import rect_data as XD

pytestmark = pytest.mark.gpu

CAN_U8, CAN_F = 0xA5, -12345.5
K_E2E = 21


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the label kernel on given logits
def _run_packed(binding, torch, d_lg, ld, grids, outs, lrow, K, off_u8=64, off_f=16, score=True):
    """(labels u8 [px], score bits u32 [px] or None) between poisoned canaries; off_u8 / off_f: where the outputs start inside their buffers."""
    px = int(QD.tables(outs)[0][-1])
    d_lab = torch.full((off_u8 + px + 64,), CAN_U8, dtype=torch.uint8, device="cuda")
    d_sc = torch.full((off_f + px + 16,), CAN_F, dtype=torch.float32, device="cuda")
    binding.op_dense_labels_packed(d_lg.data_ptr(), ld, grids, outs, lrow, K, d_lab.data_ptr() + off_u8, d_sc.data_ptr() + 4 * off_f if score else 0)
    torch.cuda.synchronize()
    lab, sc = d_lab.cpu().numpy(), d_sc.cpu().numpy()
    assert (lab[:off_u8] == CAN_U8).all() and (lab[off_u8 + px:] == CAN_U8).all(), "a label canary was written"
    if not score:
        assert (sc == CAN_F).all(), "the score buffer was written without being given"
        return lab[off_u8:off_u8 + px], None
    assert (sc[:off_f] == CAN_F).all() and (sc[off_f + px:] == CAN_F).all(), "a score canary was written"
    return lab[off_u8:off_u8 + px], sc[off_f:off_f + px].view(np.uint32)


@pytest.mark.parametrize("K", DD.KS)
def test_packed_label_kernel_equals_the_host_function_bit_for_bit(binding, torch_gpu, K):
    """The hostile pack behind 0, 1 and 5 poisoned prefix rows per image; in reverse order; its first image alone; output buffers on (64 / 16) and off
    (61 / 17) the 4- and 16-byte boundaries; without a score buffer."""
    torch = torch_gpu
    for Tp in QD.PREFIXES:
        for grids, outs in ((QD.GRIDS, QD.OUTS), (QD.GRIDS[::-1], QD.OUTS[::-1]), (QD.GRIDS[3:4], QD.OUTS[3:4])):
            lg, lrow = QD.pack_logits(grids, K, Tp, seed=K)
            want_lab, want_bits = QD.reference(binding, lg, lrow, grids, outs, K)
            d_lg = torch.from_numpy(lg).cuda()
            for off_u8, off_f in ((64, 16), (61, 17)):
                lab, bits = _run_packed(binding, torch, d_lg, lg.shape[1], grids, outs, lrow, K, off_u8, off_f)
                tag = (K, Tp, len(grids), grids[0], off_u8)
                assert np.array_equal(lab, want_lab), (tag, np.argwhere(lab != want_lab)[:5].tolist())
                assert np.array_equal(bits, want_bits), (tag, np.argwhere(bits != want_bits)[:5].tolist())
            lab, none = _run_packed(binding, torch, d_lg, lg.shape[1], grids, outs, lrow, K, score=False)
            assert none is None and np.array_equal(lab, want_lab), (K, Tp, "no score buffer")


@pytest.mark.parametrize("K", [21, 150, 256])
def test_an_image_does_not_depend_on_its_neighbours(binding, torch_gpu, K):
    """Every image's bytes in the pack equal those of the image launched alone through vitx_op_dense_labels (the fixed-shape kernel) -- and, for the
    images with small windows, those of a pack WITHOUT the scale-1 image: at K = 150 and 256 that image's 16 x 37 window forces class chunks on the
    whole launch, without it the launch has one chunk."""
    torch = torch_gpu
    lg, lrow = QD.pack_logits(QD.GRIDS, K, 1, seed=K)
    ld = lg.shape[1]
    d_lg = torch.from_numpy(lg).cuda()
    lab, bits = _run_packed(binding, torch, d_lg, ld, QD.GRIDS, QD.OUTS, lrow, K)
    pix0 = QD.tables(QD.OUTS)[0]
    for i, ((gh, gw), (oh, ow)) in enumerate(zip(QD.GRIDS, QD.OUTS)):
        d_one = torch.from_numpy(QD.image_rows(lg, lrow, QD.GRIDS, i)).cuda()
        d_l = torch.full((oh * ow,), CAN_U8, dtype=torch.uint8, device="cuda")
        d_s = torch.full((oh * ow,), CAN_F, dtype=torch.float32, device="cuda")
        binding.op_dense_labels(d_one.data_ptr(), ld, 1, gh, gw, K, oh, ow, d_l.data_ptr(), d_s.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(lab[pix0[i]:pix0[i + 1]], d_l.cpu().numpy()), (K, i)
        assert np.array_equal(bits[pix0[i]:pix0[i + 1]], d_s.cpu().numpy().view(np.uint32)), (K, i)
    keep = [i for i in range(len(QD.GRIDS)) if QD.GRIDS[i] != (16, 37)]
    grids, outs = [QD.GRIDS[i] for i in keep], [QD.OUTS[i] for i in keep]
    lab2, bits2 = _run_packed(binding, torch, d_lg, ld, grids, outs, lrow[keep], K)            # the same rows of the same buffer, the big image skipped
    pix2 = QD.tables(outs)[0]
    for j, i in enumerate(keep):
        assert np.array_equal(lab2[pix2[j]:pix2[j + 1]], lab[pix0[i]:pix0[i + 1]]) and np.array_equal(bits2[pix2[j]:pix2[j + 1]], bits[pix0[i]:pix0[i + 1]]), (K, i)


def test_a_uniform_pack_equals_the_fixed_shape_kernel(binding, torch_gpu):
    """Every shape of dense_data.cases() through the packed launcher as a pack of n images of that shape, lrow[i] = i gh gw: bit for bit
    vitx_op_dense_labels on the same rows -- one tile body behind both kernels."""
    torch = torch_gpu
    for c, (gh, gw, oh, ow, K, n) in enumerate(DD.cases()):
        ld = DD.pad_to(K)
        lg = DD.hostile(n, gh, gw, K, ld, seed=c)
        d_lg = torch.from_numpy(lg).cuda()
        px = n * oh * ow
        d_l = torch.full((px,), CAN_U8, dtype=torch.uint8, device="cuda")
        d_s = torch.full((px,), CAN_F, dtype=torch.float32, device="cuda")
        binding.op_dense_labels(d_lg.data_ptr(), ld, n, gh, gw, K, oh, ow, d_l.data_ptr(), d_s.data_ptr())
        lab, bits = _run_packed(binding, torch, d_lg, ld, [(gh, gw)] * n, [(oh, ow)] * n, np.arange(n) * gh * gw, K)
        assert np.array_equal(lab, d_l.cpu().numpy()) and np.array_equal(bits, d_s.cpu().numpy().view(np.uint32)), (gh, gw, oh, ow, K, n)


def test_op_refusals(binding, torch_gpu):
    """vitx_op_dense_labels's checks, image by image, before anything is launched."""
    torch = torch_gpu
    d_lg = torch.zeros((64, 128), dtype=torch.float32, device="cuda")
    d_l = torch.full((4096,), CAN_U8, dtype=torch.uint8, device="cuda")
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    for code, args in ((U, dict(outs=[(2, 5), (1, 3)])), (U, dict(outs=[(2, 5), (8193, 3)])), (A, dict(K=0)), (U, dict(K=257, ld=384)), (A, dict(ld=20)), (A, dict(lrow=[0, -1])),
                       (A, dict(grids=[(1, 1), (0, 3)]))):
        a = dict(ld=128, grids=[(1, 1), (2, 3)], outs=[(2, 5), (5, 17)], lrow=[1, 3], K=21)
        a.update(args)
        with pytest.raises(binding.VitxError) as ei:
            binding.op_dense_labels_packed(d_lg.data_ptr(), a["ld"], a["grids"], a["outs"], a["lrow"], a["K"], d_l.data_ptr())
        assert ei.value.code == code, (args, str(ei.value))
    with pytest.raises(binding.VitxError):
        binding.op_dense_labels_packed(d_lg.data_ptr() + 4, 128, [(1, 1)], [(2, 5)], [0], 21, d_l.data_ptr())
    torch.cuda.synchronize()
    assert (d_l.cpu().numpy() == CAN_U8).all()


# ------------------------------------------------------------------------------------------------ 2. the head on a packed context
E2E_KINDS = ("p16h4", "p14r4h4", "p14ropeh4")


def _head(K, Dc, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((K, Dc)) * 0.25).astype(np.float32), rng.standard_normal(K).astype(np.float32)


def _host_maps(binding, kept, shapes, outs, P):
    """The host function on each image's kept logits (padded to ld = 128 with NaN columns): lists of labels and score bits."""
    lab, bits = [], []
    for lg, (h, w), (oh, ow) in zip(kept, shapes, outs):
        gh, gw = h // P, w // P
        padded = np.full((gh * gw, DD.pad_to(K_E2E)), np.nan, np.float32); padded[:, :K_E2E] = lg
        l, s = binding.dense_labels_host(padded, 1, gh, gw, K_E2E, oh, ow)
        lab.append(l[0]); bits.append(_bits(s[0]))
    return lab, bits


def _same(a, b):
    """Two images' (labels, score, logits) triples: equal bits."""
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2]))


def _run(pack, imgs):
    p, lg = pack.forward(imgs)
    lab, sc, kept = pack.dense_read()
    return [(lab[i], sc[i], kept[i]) for i in range(len(imgs))], p, lg


@pytest.mark.parametrize("dtype", [1, 0], ids=["bf16", "f16"])
@pytest.mark.parametrize("layers", [None, [0, 1]], ids=["last", "0+1"])
@pytest.mark.parametrize("kind", E2E_KINDS)
def test_pack_forward_end_to_end(pkg, binding, torch_gpu, kind, layers, dtype):
    """The mixed pack of pack_data.mixed_shapes, K = 21.  Last layer alone, with VITX_FEAT_TOKENS on: the kept logits lie under
    (Dc + 1) 2^-24 (|a| @ |w|.T + |bias|) of the float64 product of RNE(tokens) and RNE(W) (test_gpu_dense.py's bound: f32 accumulation of Dc products
    and the bias, whatever the order).  Both: labels and scores equal the host function on the kept logits bit for bit; every map of a grid of more
    than one cell holds more than one class (a 1 x 1 grid has one logit row, so its map is one class by construction); an image's logits, labels and
    scores have the same bits alone, at another position (the pack reversed) and beside NaN-pixel neighbours; the forward's probabilities and
    logits are those of the context without a head; launches grow by m + 2."""
    model = binding.Model(KD.variant_file(pkg, kind))
    P, D, L_ = model.hparams.patch_size, model.hparams.hidden_size, model.hparams.num_hidden_layers
    shapes = KD.mixed_shapes(P)
    imgs = KD.pack_of(shapes)
    n = len(imgs)
    sel = [L_ - 1] if layers is None else layers
    Dc = D * len(sel)
    W, b = _head(K_E2E, Dc, seed=len(sel))
    pack = binding.PackContext(model, device=0, max_tokens=256, max_images=2 * n, dtype=dtype)
    if layers is None:
        pack.feat_enable(cls=False, tokens=True)
    plain = pack.forward(imgs)                                     # also builds every grid's tables: the launch counts below compare like with like
    plain = pack.forward(imgs)
    base_launches, base_scratch = pack.launches[0], pack.scratch_bytes
    assert pack.dense_device() == 0 and pack.dense_scratch_bytes() == 0
    pack.dense_set(W, b, layers, score=True, logits=True)
    assert pack.dense_device() != 0 and pack.scratch_bytes > base_scratch + pack.dense_scratch_bytes() > base_scratch
    res, p, lg = _run(pack, imgs)
    assert np.array_equal(_bits(p), _bits(plain[0])) and np.array_equal(_bits(lg), _bits(plain[1])), "the head moved the forward's own outputs"
    assert pack.launches[0] == base_launches + len(sel) + 2
    if layers is None:
        tok = pack.feat_read()[1]
        wr = binding.round_operand(W, dtype)
        for i in range(n):
            a = binding.round_operand(tok[i].reshape(-1, D), dtype)
            want = DD.patch_logits64(a, wr, b)
            bound = (Dc + 1) * 2.0 ** -24 * (np.abs(a).astype(np.float64) @ np.abs(wr).astype(np.float64).T + np.abs(b)[None, :])
            worst = float((np.abs(res[i][2] - want) / bound).max())
            print(f"{kind} dtype {dtype} image {i}: max |logit - float64| / bound = {worst:.3e}")
            assert worst <= 1.0, i
    want_lab, want_bits = _host_maps(binding, [r[2] for r in res], shapes, shapes, P)
    for i, (h, w) in enumerate(shapes):
        assert res[i][0].shape == (h, w) and res[i][2].shape == ((h // P) * (w // P), K_E2E)
        assert np.array_equal(res[i][0], want_lab[i]) and np.array_equal(_bits(res[i][1]), want_bits[i]), i
        assert len(np.unique(res[i][0])) > (1 if h * w > P * P else 0), (i, "a label map of one class checks nothing")
    # determinism: alone; at another position; beside NaN neighbours
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
    # off: the buffers go, the forward is the one it was
    pack.dense_set(None)
    assert pack.scratch_bytes == base_scratch and pack.dense_device() == 0 and pack.dense_scratch_bytes() == 0
    off = pack.forward(imgs)
    assert pack.launches[0] == base_launches and np.array_equal(_bits(off[0]), _bits(plain[0]))
    pack.close(); model.close()


@pytest.mark.parametrize("dtype", [1, 0], ids=["bf16", "f16"])
@pytest.mark.parametrize("kind", E2E_KINDS)
def test_uniform_pack_equals_the_rect_context(pkg, binding, torch_gpu, kind, dtype):
    """Five images of pack_data.UNIFORM_SHAPE, layers [0, 1] and the last layer alone: labels, scores and kept logits of the pack equal those of a
    rectangular Context(img_shape=...) with the same head (head dim 32: both run the generic attention arithmetic)."""
    model = binding.Model(KD.variant_file(pkg, kind))
    P, D = model.hparams.patch_size, model.hparams.hidden_size
    shape = KD.UNIFORM_SHAPE[P]
    n = 5
    imgs = XD.images(n, *shape)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, img_shape=shape, last_layer_all_rows=1)
    pack = binding.PackContext(model, device=0, max_tokens=n * ctx.tokens, max_images=n, dtype=dtype)
    for layers in ([0, 1], None):
        W, b = _head(K_E2E, D * (2 if layers else 1), seed=5)
        ctx.dense_set(W, b, layers, score=True, logits=True)
        ctx.forward(imgs)
        lab, sc, kept = ctx.dense_read(n)
        pack.dense_set(W, b, layers, score=True, logits=True)
        res = _run(pack, list(imgs))[0]
        for i in range(n):
            assert _same(res[i], (lab[i], sc[i], kept[i])), (layers, i)
    ctx.close(); pack.close(); model.close()


def test_cli_writes_a_label_map_per_image_at_the_original_size(pkg, binding, torch_gpu, tmp_path):
    """vit_cli.py --pack --img-fit 32 --dense-head head.npz --dense-out PREFIX on two golden assets: PREFIX.<i>.pgm holds class bytes at the ORIGINAL
    image's size, and the printed shares are those of the map."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = KD.variant_file(pkg, "p16h4")
    D = binding.Model(src).hparams.hidden_size
    W, b = _head(5, D, seed=8)
    names = ["sky", "road", "tree", "grass", "water"]
    head = str(tmp_path / "head.npz")
    pkg.convert.write_dense_head(head, {"weight": W, "bias": b, "layers": [1], "names": names})
    files = [os.path.join(root, "tests", "golden", "assets", f) for f in ("tench.jpg", "kiwi.jpg")]
    prefix = str(tmp_path / "labels")
    r = subprocess.run([sys.executable, os.path.join(root, "vit_cli.py"), "-m", src, "--dtype", "bf16", "--img-fit", "32", "--pack", "-i", ",".join(files),
                        "--dense-head", head, "--dense-out", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    printed = r.stdout.split("\n")
    at = 0
    for i, f in enumerate(files):
        ny, nx = binding.load_image(f).shape[:2]
        blob = open(f"{prefix}.{i}.pgm", "rb").read()
        hdr = f"P5\n{nx} {ny}\n255\n".encode()
        assert blob.startswith(hdr) and len(blob) == len(hdr) + nx * ny, (i, blob[:20])
        lab = np.frombuffer(blob[len(hdr):], np.uint8)
        assert lab.max() < 5 and len(np.unique(lab)) > 1
        share = np.bincount(lab, minlength=5) / lab.size
        for k in np.argsort(-share, kind="stable"):
            if share[k] > 0:
                assert printed[at] == f" > {names[k]} : {share[k]:.2f}", (i, printed[at]); at += 1
    assert printed[at:] == [""]


def _device_bytes(ptr, count):
    out = np.empty(count, np.uint8)
    assert C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), count, 2) == 0
    return out


def test_output_shapes_and_refused_calls(pkg, binding, torch_gpu):
    """vitx_pack_dense_out to original-like sizes (28 x 70 -> 31 x 75) is consumed by one forward, the next is back at h x w; every refused call
    leaves the label buffer as it was (canaries through vitx_pack_dense_device), consumes the shapes it was given and leaves the context usable;
    a refused set leaves the head that was set."""
    L = binding.lib()
    model = binding.Model(KD.variant_file(pkg, "p14r4h4"))
    P, D = model.hparams.patch_size, model.hparams.hidden_size
    shapes = KD.mixed_shapes(P)
    imgs = KD.pack_of(shapes)
    n = len(imgs)
    outs = QD.original_like(shapes, P)
    px_out = sum(h * w for h, w in outs)
    W, b = _head(K_E2E, D, seed=3)
    pack = binding.PackContext(model, device=0, max_tokens=256, max_images=n, dtype=1)
    with pytest.raises(binding.VitxError):
        pack.dense_out(outs)                                                     # no head is set
    pack.dense_set(W, b, None, max_pixels=px_out, score=True, logits=True)
    with pytest.raises(binding.VitxError) as ei:
        pack.dense_read()                                                        # before any forward with the head set
    assert ei.value.code == binding.ERR_ARG
    own = _run(pack, imgs)[0]
    pack.dense_out(outs)
    big = _run(pack, imgs)[0]
    want_lab, want_bits = _host_maps(binding, [r[2] for r in big], shapes, outs, P)
    for i in range(n):
        assert big[i][0].shape == tuple(outs[i]) and np.array_equal(_bits(big[i][2]), _bits(own[i][2])), i
        assert np.array_equal(big[i][0], want_lab[i]) and np.array_equal(_bits(big[i][1]), want_bits[i]), i
    dev = _device_bytes(pack.dense_device(), px_out)
    assert np.array_equal(dev, np.concatenate([r[0].ravel() for r in big])), "the device buffer is what read returns"
    back = _run(pack, imgs)[0]                                                   # consumed: h x w again
    assert all(_same(back[i], own[i]) for i in range(n))
    # refused calls: fill the label buffer with canaries, be refused, find the canaries
    hip = C.cdll.LoadLibrary("libamdhip64.so")
    ptr = pack.dense_device()

    def refused(word, call_imgs, out_shapes):
        assert hip.hipMemset(C.c_void_p(ptr), CAN_U8, px_out) == 0 and hip.hipDeviceSynchronize() == 0
        if out_shapes is not None:
            pack.dense_out(out_shapes)
        with pytest.raises(binding.VitxError) as ei:
            pack.forward(call_imgs)
        assert ei.value.code == binding.ERR_ARG and word in str(ei.value), str(ei.value)
        assert hip.hipDeviceSynchronize() == 0 and (_device_bytes(ptr, px_out) == CAN_U8).all(), "a refused call wrote labels"
        again = _run(pack, imgs)[0]                                              # usable, and the refused call consumed its shapes
        assert all(_same(again[i], own[i]) for i in range(n)), word

    refused("images", imgs, outs[:-1])                                           # n differs from the forward's
    refused("upsampling only", imgs, outs[:2] + [(shapes[2][0] // P - 1, shapes[2][1])] + outs[3:])
    refused("upsampling only", imgs, outs[:-1] + [(QD.MAX_OUT + 1, P)])
    refused("max_pixels", imgs, outs[:-1] + [(outs[-1][0], outs[-1][1] + 1)])    # one column of one image too many
    refused("patch size", [np.zeros((P + 1, P, 3), np.float32)], None)           # vitx_pack_check's refusals still come first
    # a refused set leaves the head in place
    bad = W.copy(); bad[3, 5] = np.nan
    fp = C.POINTER(C.c_float)
    for args, code in (((bad.ctypes.data_as(fp), None, K_E2E, D, 0, px_out, 0), binding.ERR_ARG), ((W.ctypes.data_as(fp), None, K_E2E, 2 * D, 0, px_out, 0), binding.ERR_ARG),
                       ((W.ctypes.data_as(fp), None, K_E2E, D, 0, px_out, 4), binding.ERR_ARG), ((W.ctypes.data_as(fp), None, K_E2E, D, 0, 0, 0), binding.ERR_ARG),
                       ((W.ctypes.data_as(fp), None, K_E2E, D, 1 << 2, px_out, 0), binding.ERR_ARG), ((None, None, 3, D, 0, px_out, 0), binding.ERR_ARG),
                       ((np.zeros((257, D), np.float32).ctypes.data_as(fp), None, 257, D, 0, px_out, 0), binding.ERR_UNSUPPORTED)):
        assert L.vitx_pack_dense_set(pack._h, *args) == code, args[2:]
    still = _run(pack, imgs)[0]
    assert all(_same(still[i], own[i]) for i in range(n))
    pack.close(); model.close()


def test_the_device_entry_point_with_a_head_set(pkg, binding, torch_gpu):
    """vitx_pack_forward_device goes through the same check of a call as vitx_pack_forward.  With a head set (score and logits on) and
    dense_out(original_like): forward_device + dense_read give the bits of forward + dense_read, probabilities and logits included.  A forward_device
    refused for its output shapes (given for n - 1 images) is ERR_ARG, leaves the canaries in the label buffer and the probabilities' sentinel,
    consumes its dense_out shapes -- the following forward_device, at the images' own shapes, equals the host path's."""
    torch = torch_gpu
    model = binding.Model(KD.variant_file(pkg, "p14r4h4"))
    P, D = model.hparams.patch_size, model.hparams.hidden_size
    shapes = KD.mixed_shapes(P)
    imgs = KD.pack_of(shapes)
    n = len(imgs)
    outs = QD.original_like(shapes, P)
    px_out = sum(h * w for h, w in outs)
    W, b = _head(K_E2E, D, seed=3)
    pack = binding.PackContext(model, device=0, max_tokens=256, max_images=n, dtype=1)
    pack.dense_set(W, b, None, max_pixels=px_out, score=True, logits=True)
    own, own_p, own_lg = _run(pack, imgs)
    pack.dense_out(outs)
    big, big_p, big_lg = _run(pack, imgs)
    assert all(big[i][0].shape == tuple(outs[i]) for i in range(n)) and any(big[i][0].shape != own[i][0].shape for i in range(n))
    d_pix = torch.from_numpy(np.concatenate([a.ravel() for a in imgs])).cuda()
    SENT = -7.25

    def device_run(out_shapes):
        d_p = torch.full((n, model.num_classes), SENT, dtype=torch.float32, device="cuda")
        d_lg = torch.full((n, model.num_classes), SENT, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        if out_shapes is not None:
            pack.dense_out(out_shapes)
        pack.forward_device(d_pix.data_ptr(), shapes, d_p.data_ptr(), d_lg.data_ptr())
        lab, sc, kept = pack.dense_read()
        torch.cuda.synchronize()
        return [(lab[i], sc[i], kept[i]) for i in range(n)], d_p.cpu().numpy(), d_lg.cpu().numpy()

    got, p, lg = device_run(outs)
    assert all(_same(got[i], big[i]) for i in range(n)), "forward_device with dense_out"
    assert np.array_equal(_bits(p), _bits(big_p)) and np.array_equal(_bits(lg), _bits(big_lg))
    # refused for its output shapes: nothing is written, the shapes are consumed
    hip = C.cdll.LoadLibrary("libamdhip64.so")
    ptr = pack.dense_device()
    assert hip.hipMemset(C.c_void_p(ptr), CAN_U8, px_out) == 0 and hip.hipDeviceSynchronize() == 0
    d_p = torch.full((n, model.num_classes), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pack.dense_out(outs[:-1])
    with pytest.raises(binding.VitxError) as ei:
        pack.forward_device(d_pix.data_ptr(), shapes, d_p.data_ptr())
    assert ei.value.code == binding.ERR_ARG and "images" in str(ei.value), str(ei.value)
    assert hip.hipDeviceSynchronize() == 0 and (_device_bytes(ptr, px_out) == CAN_U8).all(), "a refused call wrote labels"
    assert bool((d_p == SENT).all()), "a refused call wrote probabilities"
    again, p, lg = device_run(None)
    assert all(_same(again[i], own[i]) for i in range(n)), "the refused call did not consume its shapes"
    assert np.array_equal(_bits(p), _bits(own_p)) and np.array_equal(_bits(lg), _bits(own_lg))
    pack.close(); model.close()
