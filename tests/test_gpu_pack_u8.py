"""Packed batches fed from u8 originals on the GPU (include/vitx.h "packed batches", u8 sources):
1. The packed preprocessing kernel alone (vitx_op_preprocess_pack) against the host function (vitx_preprocess_rect) image by image, bit for bit, both
   filters, on the pack of tests/pack_u8_data.py: every start alignment, 1-pixel sources, the identity, an upscale, a down-scale just inside the LDS
   bound beside a tiny image, partial tiles; guard floats in front of and behind the outputs.
2. Position and neighbours: an image's bits first, last, alone and beside neighbours of other tilings (the launch's LDS differs, the bits do not).
3. The forward: vitx_pack_forward_u8 and vitx_pack_u8_sources + vitx_pack_forward_device against forward_flat(*pack_images(...)), bit for bit on
   probabilities, logits, features and (once) the dense head's labels; the launch count.
4. Once-only semantics, refused calls, scratch.
5. Stream order: the u8 mode behind a stalled caller stream (the harness of tests/stream_data.py).
6. vit_cli.py --pack --pack-u8."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pack_data as KD
import pack_u8_data as UD
import preproc_data as PPD
import rect_data as XD
import stream_data as S

pytestmark = pytest.mark.gpu

L = 2                      # layers of rect_data's micro fixtures
SENT = -12345.5
GUARD = 64                 # floats in front of and behind the outputs (256 bytes: the output keeps its alignment)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pp(binding, filt=PPD.PP_PIL_BICUBIC):
    mean, std = PPD.mean_std255(PPD.IMAGENET)
    return binding.Preproc.make(resize_a=16, resize_b=16, filter=filt, mean255=mean, std255=std)


def _device_sources(torch, imgs):
    """The sources strictly end to end in a buffer of their byte count rounded up to 4 (the pad bytes are 171), and that byte count."""
    flat = np.concatenate([np.ascontiguousarray(im, np.uint8).ravel() for im in imgs])
    buf = np.full((flat.size + 3) // 4 * 4, 171, np.uint8)
    buf[:flat.size] = flat
    return torch.from_numpy(buf).cuda(), flat.size


def _preprocess_pack(binding, torch, pp, imgs, outs):
    """vitx_op_preprocess_pack on `imgs`, each to its own outs[i] = (h, w): the per-image outputs; the guards hold their sentinel."""
    d_src, _ = _device_sources(torch, imgs)
    floats = [3 * h * w for h, w in outs]
    d_out = torch.full((GUARD + sum(floats) + GUARD,), SENT, dtype=torch.float32, device="cuda")
    binding.preprocess_pack(pp, d_src.data_ptr(), [im.shape[:2] for im in imgs], outs, d_out.data_ptr() + 4 * GUARD)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:GUARD] == SENT).all() and (out[GUARD + sum(floats):] == SENT).all(), "a float outside the outputs was written"
    at = np.concatenate([[0], np.cumsum(floats)]) + GUARD
    return [out[at[i]:at[i + 1]].reshape(h, w, 3) for i, (h, w) in enumerate(outs)]


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("fname", list(PPD.FILTERS))
def test_preprocess_pack_equals_the_host_per_image(binding, torch_gpu, fname):
    filt = PPD.FILTERS[fname]
    pp = _pp(binding, filt)
    pack = UD.kernel_pack(filt == PPD.PP_PIL_BICUBIC)
    imgs, outs = UD.sources(pack), [p[1] for p in pack]
    got = _preprocess_pack(binding, torch_gpu, pp, imgs, outs)
    for i, (im, (h, w), g) in enumerate(zip(imgs, outs, got)):
        want = binding.preprocess_rect(im, pp, w, h)
        bad = np.argwhere(_bits(g) != _bits(want))
        assert bad.size == 0, (fname, i, pack[i][2], len(bad), bad[:5].tolist())


# ------------------------------------------------------------------------------------------------ 2. position and neighbours
@pytest.mark.parametrize("fname", list(PPD.FILTERS))
def test_an_images_bits_do_not_depend_on_position_neighbours_or_the_launchs_lds(binding, torch_gpu, fname):
    filt = PPD.FILTERS[fname]
    bic = filt == PPD.PP_PIL_BICUBIC
    pp = _pp(binding, filt)
    pack = UD.kernel_pack(bic)
    imgs = UD.sources(pack)
    X, NEAR, TINY, DOWN = 6, 4, 5, 7                     # 3 x 6 tiles; the down-scale at the bound; one partial tile; a down-scale by 4 and 2
    orders = ([X], [X, TINY], [TINY, X], [NEAR, X], [X, NEAR], [NEAR, TINY, X], [TINY], [NEAR], [TINY, NEAR], [DOWN, TINY, X, NEAR])
    seen, lds = {}, {}
    for order in orders:
        got = _preprocess_pack(binding, torch_gpu, pp, [imgs[i] for i in order], [pack[i][1] for i in order])
        lds[tuple(order)] = UD.tables(bic, [pack[i][0] for i in order], [pack[i][1] for i in order])[3]
        for i, g in zip(order, got):
            if i in seen:
                assert np.array_equal(_bits(g), seen[i][1]), (fname, "image", i, "in", order, "differs from", seen[i][0])
            else:
                seen[i] = (order, _bits(g).copy())
    # the launches above really had different LDS sizes for the same image
    assert lds[(X,)] < lds[(DOWN, TINY, X, NEAR)] == lds[(NEAR, X)] and lds[(TINY,)] < lds[(X, TINY)] < lds[(TINY, NEAR)]


# ------------------------------------------------------------------------------------------------ 3. the forward
def _setup(pkg, binding, kind, dtype, feat=True):
    model = binding.Model(XD.fixture_file(pkg, kind))
    P = model.hparams.patch_size
    imgs, pp = UD.originals(), _pp(binding)
    pixels, shapes = binding.pack_images(imgs, pp, 2 * P, patch=P)
    assert np.array_equal(shapes, binding.pack_fit_shapes(model, UD.ORIGINALS, 2 * P))
    tokens = int(binding.pack_check(model, shapes, 2 ** 31 - 1, len(imgs))[-1])
    packs = [binding.PackContext(model, device=0, max_tokens=tokens, max_images=len(imgs), dtype=dtype) for _ in range(2)]
    if feat:
        for p in packs:
            p.feat_enable(cls=True, tokens=True)
    return model, imgs, pp, pixels, shapes, packs


def _same_features(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and len(a[1]) == len(b[1]) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", ["p16", "p14rope"])
def test_forward_u8_equals_the_host_preprocessing_bit_for_bit(pkg, binding, torch_gpu, kind, dtype):
    torch = torch_gpu
    model, imgs, pp, pixels, shapes, (plain, ctx) = _setup(pkg, binding, kind, dtype)
    n, Cn = len(imgs), model.num_classes
    plain.forward_flat(pixels, shapes)                             # builds every grid's tables: the launch counts below compare like with like
    want = plain.forward_flat(pixels, shapes)
    want_feat = plain.feat_read()
    count = KD.pack_launches(shapes.tolist(), L, 0, rope=kind == "p14rope", feat=True)
    assert plain.launches == count
    total = sum(im.size for im in imgs)
    ctx.u8_set(pp, max_src_bytes=total)
    ctx.forward_u8(imgs, shapes)
    got = ctx.forward_u8(imgs, shapes)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1])), "probabilities or logits differ"
    assert _same_features(ctx.feat_read(), want_feat), "feature tokens differ"
    assert ctx.launches == (count[0] + 1, count[1])
    # the device path: the declaration, then the existing entry point on the u8 buffer
    d_src, nbytes = _device_sources(torch, imgs)
    assert nbytes == total and nbytes % 4 != 0
    d_probs, d_logits = (torch.full((n * Cn,), SENT, dtype=torch.float32, device="cuda") for _ in range(2))
    ctx.u8_sources([im.shape[:2] for im in imgs])
    ctx.forward_device(d_src.data_ptr(), shapes, d_probs.data_ptr(), d_logits.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_probs.cpu().numpy()), _bits(want[0]).ravel()) and np.array_equal(_bits(d_logits.cpu().numpy()), _bits(want[1]).ravel())
    assert _same_features(ctx.feat_read(), want_feat) and ctx.launches == (count[0] + 1, count[1])
    # once, with a dense head set: the labels too
    if kind == "p16" and dtype == 1:
        rng = np.random.default_rng(4)
        D = model.hparams.hidden_size
        W, b = (rng.standard_normal((5, D)) * 0.25).astype(np.float32), rng.standard_normal(5).astype(np.float32)
        outs = [im.shape[:2] if min(im.shape[:2]) >= 8 else tuple(s) for im, s in zip(imgs, shapes.tolist())]
        for p in (plain, ctx):
            p.dense_set(W, b, None, max_pixels=sum(h * w for h, w in outs), score=True)
            p.dense_out(outs)
        want = plain.forward_flat(pixels, shapes)
        got = ctx.forward_u8(imgs, shapes)
        assert np.array_equal(_bits(got[0]), _bits(want[0]))
        (la, sa, _), (lb, sb, _) = plain.dense_read(), ctx.dense_read()
        assert all(np.array_equal(x, y) for x, y in zip(la, lb)) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(sa, sb))
        assert ctx.launches[0] == plain.launches[0] + 1
    plain.close(); ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 4. once-only semantics, refusals, scratch
def test_declarations_are_consumed_and_refused_calls_launch_nothing(pkg, binding, torch_gpu):
    torch = torch_gpu
    model, imgs, pp, pixels, shapes, (plain, ctx) = _setup(pkg, binding, "p16", 1, feat=False)
    P, n, Cn = model.hparams.patch_size, len(imgs), model.num_classes
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    srcs = [im.shape[:2] for im in imgs]

    def code(fn, *a, **k):
        with pytest.raises(binding.VitxError) as ei:
            fn(*a, **k)
        return ei.value.code
    plain.forward_flat(pixels, shapes)
    want = plain.forward_flat(pixels, shapes)
    base_launches = plain.launches
    # off: nothing to declare; a refused set leaves it off; scratch
    base = ctx.scratch_bytes
    assert code(ctx.u8_sources, srcs) == A and code(ctx.forward_u8, imgs, shapes) == A
    assert code(ctx.u8_set, _pp(binding, PPD.PP_REF_BICUBIC), 1000) == U and not model.has_preproc and code(ctx.u8_set, None, 1000) == U
    assert ctx.scratch_bytes == base and code(ctx.u8_sources, srcs) == A
    big = 3 * 4 * 40000 + 50000                                    # holds the source beyond the LDS bound below
    ctx.u8_set(pp, max_src_bytes=big)
    tokens = int(binding.pack_check(model, shapes, 2 ** 31 - 1, n)[-1])
    assert ctx.scratch_bytes >= base + big + tokens * P * P * 3 * 4
    assert code(ctx.u8_set, _pp(binding, PPD.PP_REF_BICUBIC), 1000) == U        # what was set stays
    ctx.forward_u8(imgs, shapes)                                   # builds every grid's tables
    got = ctx.forward_u8(imgs, shapes)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and ctx.launches[0] == base_launches[0] + 1
    # after a u8 call a plain call takes f32 pixels again and is the plain context's
    got = ctx.forward_flat(pixels, shapes)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1])) and ctx.launches == base_launches
    # refused calls: nothing launched, nothing written, the declaration consumed
    d_src, _ = _device_sources(torch, imgs)
    d_pix = torch.from_numpy(np.ascontiguousarray(pixels, np.float32)).cuda()
    d_probs, d_logits = (torch.full((n * Cn,), SENT, dtype=torch.float32, device="cuda") for _ in range(2))
    dev = lambda p, s=shapes: ctx.forward_device(p, s, d_probs.data_ptr(), d_logits.data_ptr())
    wide = [(4, 40000)] + srcs[1:]
    assert not binding.preprocess_rect_device_supports(pp, 40000, 4, int(shapes[0][1]), int(shapes[0][0]))
    refusals = ((srcs[:-1], d_src.data_ptr(), shapes, A, "an n that differs from the call's"),
                (srcs, d_src.data_ptr() + 1, shapes, A, "a misaligned buffer"),
                ([(400, 400)] * n, d_src.data_ptr(), shapes, A, "more than max_src_bytes"),
                (wide, d_src.data_ptr(), shapes, U, "an image beyond the LDS bound"),
                (srcs, d_src.data_ptr(), [(P + 1, P)] * n, A, "a shape vitx_pack_check refuses"))
    for decl, ptr, shp, want_code, what in refusals:
        ctx.u8_sources(decl)
        assert code(dev, ptr, shp) == want_code, what
        torch.cuda.synchronize()
        assert ctx.launches == base_launches and bool((d_probs == SENT).all()) and bool((d_logits == SENT).all()), what
        dev(d_pix.data_ptr())                                      # the declaration is gone: f32 pixels, the plain context's bits and launches
        torch.cuda.synchronize()
        assert np.array_equal(_bits(d_probs.cpu().numpy()), _bits(want[0]).ravel()) and ctx.launches == base_launches, what
        d_probs.fill_(SENT); d_logits.fill_(SENT)
    # the host f32 entry point refuses a call for which sources are declared, and consumes the declaration
    ctx.u8_sources(srcs)
    assert code(ctx.forward_flat, pixels, shapes) == A
    assert np.array_equal(_bits(ctx.forward_flat(pixels, shapes)[0]), _bits(want[0]))
    # a withdrawn declaration
    ctx.u8_sources(srcs); ctx.u8_sources(None)
    dev(d_pix.data_ptr()); torch.cuda.synchronize()
    assert np.array_equal(_bits(d_probs.cpu().numpy()), _bits(want[0]).ravel())
    # off again: scratch returns to its base (the pixel buffer was the set's own), and to the base with the host entry point's buffer when that came first
    # (the position tables of the grids the forwards built stay cached: the plain context holds the same ones, and the host entry point's pixel buffer)
    ctx.u8_set(None, 0)
    assert ctx.scratch_bytes == plain.scratch_bytes - tokens * P * P * 3 * 4 and ctx.scratch_bytes >= base and code(ctx.u8_sources, srcs) == A
    off = ctx.scratch_bytes
    ctx.u8_set(pp, max_src_bytes=big)
    assert ctx.scratch_bytes >= off + big + tokens * P * P * 3 * 4
    ctx.u8_set(None, 0)
    assert ctx.scratch_bytes == off
    held = plain.scratch_bytes
    plain.u8_set(pp, max_src_bytes=1000)
    assert plain.scratch_bytes > held
    plain.u8_set(pp, max_src_bytes=2000)
    plain.u8_set(None, 0)
    assert plain.scratch_bytes == held
    assert np.array_equal(_bits(plain.forward_flat(pixels, shapes)[0]), _bits(want[0])) and plain.launches == base_launches
    plain.close(); ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 5. stream order
class PackU8Step(S.Step):
    """vitx_pack_u8_sources + vitx_pack_forward_device on packs = (stalled, fenced): the u8 sources arrive by a producer copy over a u8 decoy."""

    def __init__(self, torch, packs, model, imgs, shapes, seed):
        self.packs, self.shapes, self.srcs = packs, shapes, [im.shape[:2] for im in imgs]
        flat = np.concatenate([im.ravel() for im in imgs])
        real = np.full((flat.size + 3) // 4 * 4, 171, np.uint8)
        real[:flat.size] = flat
        self.x = S.Input(torch.from_numpy(real).cuda(), torch.from_numpy(S.decoy_u8(real, seed)).cuda())
        self.inputs = [self.x]
        floats = len(imgs) * model.num_classes
        self.probs, self.logits = (torch.empty(floats, dtype=torch.float32, device="cuda") for _ in range(2))
        self.snaps = [S.Snap(torch, "probabilities", self.probs.data_ptr(), floats, torch.float32), S.Snap(torch, "logits", self.logits.data_ptr(), floats, torch.float32)]

    def call(self, fenced, stream):
        pack = self.packs[1 if fenced else 0]
        pack.u8_sources(self.srcs)
        pack.forward_device(self.x.p, self.shapes, self.probs.data_ptr(), self.logits.data_ptr(), stream)


def test_u8_mode_behind_a_stalled_caller_stream(pkg, binding, torch_gpu):
    """The table upload, the preprocessing launch and the forward all sit behind the producer on the caller's stream, and the call returns under the
    stall.  A fresh pair of contexts per run, as the other packed scenarios have: the stalled call is then the one that builds its grids' tables."""
    torch = torch_gpu
    model = binding.Model(XD.fixture_file(pkg, KD.CACHE_KIND))
    P = model.hparams.patch_size
    imgs, pp = UD.originals()[:4], _pp(binding)
    shapes = binding.pack_fit_shapes(model, UD.ORIGINALS[:4], 2 * P)
    tokens = int(binding.pack_check(model, shapes, 2 ** 31 - 1, len(imgs))[-1])

    def make():
        packs = tuple(binding.PackContext(model, device=0, max_tokens=tokens, max_images=len(imgs), dtype=binding.BF16) for _ in range(2))
        for p in packs:
            p.u8_set(pp, max_src_bytes=sum(im.size for im in imgs))
        step = PackU8Step(torch, packs, model, imgs, shapes, 60)
        step.close = lambda: [p.close() for p in packs]
        return [step]
    S.harness(torch).check("packed u8 sources -> preprocess -> forward bf16, 4 originals", make, fresh=True)
    model.close()


# ------------------------------------------------------------------------------------------------ 6. the command line
def test_cli_pack_u8_prints_the_lines_of_the_host_path(pkg, binding, torch_gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = KD.variant_file(pkg, "p16h4")
    # two golden assets inside the device kernel's LDS bound at short side 32 (612 x 408 and 500 x 470; kiwi.jpg, 1200 x 902 -> 32 x 32, is beyond it: below)
    files = [os.path.join(root, "tests", "golden", "assets", f) for f in ("tench.jpg", "magpie.jpeg")]
    cli = [sys.executable, os.path.join(root, "vit_cli.py"), "-m", src, "--dtype", "bf16", "--img-fit", "32", "--pack", "-i", ",".join(files)]
    host = subprocess.run(cli, capture_output=True, text=True, timeout=300)
    u8 = subprocess.run(cli + ["--pack-u8"], capture_output=True, text=True, timeout=300)
    assert host.returncode == 0 and u8.returncode == 0, (host.stderr, u8.stderr)
    assert u8.stdout.count(" > ") == 10 and u8.stdout == host.stdout
    bad = subprocess.run(cli[:-3] + ["-i", files[0], "--pack-u8"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "--pack-u8 goes with --pack" in bad.stderr
    # an original beyond the bound is refused by name, not resized some other way
    far = subprocess.run(cli[:-1] + [",".join([files[0], os.path.join(root, "tests", "golden", "assets", "kiwi.jpg")]), "--pack-u8"], capture_output=True, text=True, timeout=300)
    assert far.returncode == 1 and "image 1" in far.stderr and "LDS" in far.stderr and " > " not in far.stdout
