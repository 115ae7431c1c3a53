"""Rectangular contexts without a GPU (include/vitx.h "rectangular contexts"): the float64 restatement (tests/ref64.py) and the converter against
transformers' ViTModel (interpolate_pos_encoding=True), Dinov2Model and DINOv3ViTModel on non-square inputs, the separation of the fixtures'
mutants from operand rounding, vitx_rect_shape, vitx_preprocess_rect against Pillow bit for bit, and the argument errors of vitx_ctx_create_rect
that are decided before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import preproc_data as PPD
import prefix_data as PD
import rect_data as XD
import ref64 as R64
from ref64 import PROB_TOL, stage_errors, stage_ok
from test_gpu_arch import ROUND, _apart

ERR_ARG, ERR_HIP, ERR_UNSUPPORTED = 3, 4, 5
MICRO16 = "vit_micro_patch16_64"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("kind,shape", XD.CASES, ids=[f"{k}-{h}x{w}" for k, (h, w) in XD.CASES])
def test_fixture_separates_the_mutants_from_operand_rounding(pkg, binding, kind, shape):
    """Computed, not assumed (rect_data.POS_SCALE, QK_SCALE): on every fixture, shape and image of the GPU forward tests the operand-rounded
    restatement lies inside HALF of tests/ref64.py's stage and probability gates of the unrounded one, and every mutant lies more than TWICE
    a gate from the real thing -- so a GPU result inside the gates of the restatement is outside those of every mutant."""
    h, w = shape
    t = PD.file_tensors(pkg, XD.fixture_file(pkg, kind))
    imgs = XD.images(17, h, w)
    exact = R64.forward64(t, imgs, XD.HEADS, binding=binding)
    assert exact["trace"].shape[2] == (h // t["patch_embed.proj.weight"].shape[-1]) * (w // t["patch_embed.proj.weight"].shape[-1]) + 1 + XD.FIXTURES[kind][1]
    for dtype in (0, 1):
        ref = R64.forward64(t, imgs, XD.HEADS, wround=ROUND[dtype], uround=ROUND[dtype], binding=binding)
        se = stage_errors(ref["trace"], exact["trace"])
        dp = float(np.abs(ref["probs"] - exact["probs"]).max())
        print(f"{kind} {h}x{w} dtype {dtype}: rounded against unrounded: stages (e_max, e_rms) {[(round(a, 5), round(b, 5)) for a, b in se]}, max|dprob| {dp:.2e}")
        assert all(stage_ok(a, b, dtype, 0.5) for a, b in se) and dp <= 0.5 * PROB_TOL[dtype]
        for mut in XD.mutants_of(t):
            m = R64.forward64(t, imgs, XD.HEADS, mutant=mut, wround=ROUND[dtype], uround=ROUND[dtype], binding=binding)
            sm = stage_errors(m["trace"], ref["trace"])
            dm = float(np.abs(ref["probs"] - m["probs"]).max())
            print(f"{kind} {h}x{w} dtype {dtype}: mutant {mut}: stages {[(round(a, 4), round(b, 4)) for a, b in sm]}, max|dprob| {dm:.3f}")
            assert _apart(ref, m, dtype), (kind, shape, dtype, mut)


def test_square_input_is_the_square_restatement(pkg, binding):
    """On a square image at the file's size the table ref64.forward64 makes (rect_data.pos_table: no resampling) is the file's own handed in as it
    is, to the last bit."""
    t = PD.file_tensors(pkg, XD.fixture_file(pkg, "p14r4"))
    imgs = PD.exact_images(2, 56, seed=5)
    a, b = R64.forward64(t, imgs, XD.HEADS, binding=binding), R64.forward64(t, imgs, 2, pos=t["pos_embed"][0])
    assert np.array_equal(a["trace"], b["trace"]) and np.array_equal(a["probs"], b["probs"])


# ------------------------------------------------------------------------------------------------ pinned to transformers
@pytest.mark.parametrize("shape", [(28, 70), (70, 28), (56, 56)])
@pytest.mark.parametrize("kind", ["vit", "dinov2"])
def test_converter_and_restatement_against_transformers(pkg, binding, tmp_path, kind, shape):
    """convert_hf_model at ftype 0, then ref64.forward64 on the file's tensors against the model's f32 last_hidden_state on a non-square input:
    HuggingFace ViT with interpolate_pos_encoding=True and DINOv2 (which always interpolates), both F.interpolate(size=(gh, gw), mode="bicubic",
    align_corners=False) -- the host resampler at (gh, gw).  The bound is tests/test_cpu_rope.py::test_converter_and_restatement_against_transformers':
    1e-4 for the restatement, every mutant further than 0.1."""
    from test_cpu_arch import _hf_model
    torch, m = _hf_model(kind)
    path = str(tmp_path / f"{kind}.gguf")
    pkg.convert.convert_hf_model(m, path, ftype=0)
    t = PD.file_tensors(pkg, path)
    h, w = shape
    imgs = pkg.synth.normalize_u8(np.random.default_rng(3).integers(0, 256, (2, h, w, 3), dtype=np.uint8))
    px = torch.from_numpy(imgs).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        want = (m.vit(pixel_values=px, interpolate_pos_encoding=True) if kind == "vit" else m.dinov2(pixel_values=px)).last_hidden_state.numpy()
    r = R64.forward64(t, imgs, heads=2, binding=binding)
    assert r["final"].shape == want.shape == (2, 1 + (h // 14) * (w // 14), 128)
    d = float(np.abs(r["final"] - want).max())
    print(f"{kind} {h}x{w}: max|restatement - transformers| = {d:.3e} on features of magnitude {np.abs(want).max():.2f}")
    assert d <= 1e-4, d
    if h != w:
        for mut in XD.MUTANTS:
            dm = float(np.abs(R64.forward64(t, imgs, heads=2, mutant=mut, binding=binding)["final"] - want).max())
            print(f"{kind} {h}x{w}: mutant {mut}: max|d| = {dm:.3f}")
            assert dm > 0.1, (mut, dm)


@pytest.mark.parametrize("shape", [(28, 70), (70, 28)])
def test_converter_and_restatement_against_transformers_dinov3(pkg, binding, tmp_path, shape):
    """The same for DINOv3ViTModel (tests/test_cpu_rope.py's random model): the rotation table of the (gh, gw) grid, nothing resampled."""
    from test_cpu_rope import _hf_dinov3
    torch, m = _hf_dinov3()
    path = str(tmp_path / "dinov3.gguf")
    pkg.convert.convert_hf_model(m, path, ftype=0)
    t = PD.file_tensors(pkg, path)
    h, w = shape
    imgs = pkg.synth.normalize_u8(np.random.default_rng(3).integers(0, 256, (2, h, w, 3), dtype=np.uint8))
    with torch.no_grad():
        want = m(pixel_values=torch.from_numpy(imgs).permute(0, 3, 1, 2).contiguous()).last_hidden_state.numpy()
    r = R64.forward64(t, imgs, heads=2, binding=binding)
    assert r["final"].shape == want.shape == (2, 5 + (h // 14) * (w // 14), 128)
    d = float(np.abs(r["final"] - want).max())
    print(f"dinov3 {h}x{w}: max|restatement - transformers| = {d:.3e} on features of magnitude {np.abs(want).max():.2f}")
    assert d <= 1e-4, d
    for mut in XD.ROPE_MUTANTS:
        dm = float(np.abs(R64.forward64(t, imgs, heads=2, mutant=mut, binding=binding)["final"] - want).max())
        print(f"dinov3 {h}x{w}: mutant {mut}: max|d| = {dm:.3f}")
        assert dm > 0.1, (mut, dm)


# ------------------------------------------------------------------------------------------------ vitx_rect_shape
def test_rect_shape(binding):
    rs = binding.rect_shape
    assert rs(500, 375, 16, 224) == (288, 224)                      # the worked example: 224 * 500 / 375 = 298 -> 18 patches; an 18 x 14 grid
    assert rs(375, 500, 16, 224) == (224, 288)                      # portrait: the width is the short side
    assert rs(300, 300, 14, 224) == (224, 224) and rs(1, 1, 16, 16) == (16, 16)
    assert rs(640, 480, 14, 518) == (686, 518)                      # 518 * 640 / 480 = 690 -> 49 patches
    assert rs(4000, 375, 16, 224) == (2384, 224)                    # 224 * 4000 / 375 = 2389
    assert rs(4000, 375, 16, 224, 448) == (448, 224) and rs(375, 4000, 16, 224, 448) == (224, 448)      # the cap
    assert rs(500, 375, 16, 224, 288) == (288, 224) and rs(500, 375, 16, 224, 272) == (272, 224) and rs(500, 375, 16, 224, 224) == (224, 224)
    assert rs(1 << 20, 1 << 20, 16, 16384) == (16384, 16384)
    L = binding.lib()
    w, h = C.c_int(-7), C.c_int(-7)
    call = lambda nx=500, ny=375, patch=16, short=224, cap=0, pw=C.byref(w), ph=C.byref(h): L.vitx_rect_shape(nx, ny, patch, short, cap, pw, ph)
    bad = [call(nx=0), call(ny=0), call(nx=-3), call(nx=(1 << 20) + 1), call(patch=0), call(patch=-16), call(short=0), call(short=-224), call(short=230),
           call(short=16400), call(cap=200), call(cap=300), call(cap=208), call(cap=-16), call(cap=16400), call(pw=None), call(ph=None),
           call(nx=100000, ny=10)]                                  # a long side above 16384 without a cap
    assert bad == [ERR_ARG] * len(bad), bad
    assert "vitx_rect_shape" in L.vitx_last_error().decode()
    assert (w.value, h.value) == (-7, -7), "a refused call wrote its outputs"
    assert call(nx=100000, ny=10, cap=4096) == 0 and (w.value, h.value) == (4096, 224)


# ------------------------------------------------------------------------------------------------ vitx_preprocess_rect
# (nx, ny, out_w, out_h): down-scale, up-scale, mixed, one axis the identity (either one), sides of 1 x k and k x 1, the issue's shapes
RECT_GEOMETRIES = [(500, 375, 288, 224), (375, 500, 224, 288), (13, 9, 48, 32), (100, 60, 64, 112), (50, 37, 48, 32), (37, 50, 32, 48), (48, 200, 48, 56),
                   (200, 48, 56, 48), (1, 9, 1, 5), (9, 1, 5, 1), (1, 9, 4, 3), (7, 1, 3, 6), (64, 64, 16, 48)]


@pytest.mark.parametrize("fname", list(PPD.FILTERS))
@pytest.mark.parametrize("g", RECT_GEOMETRIES, ids=PPD.geo_id)
def test_host_rect_resize_is_pillow_bit_for_bit(binding, g, fname):
    """vitx_preprocess_rect with mean 0, std 1 is Image.resize((out_w, out_h)) on u8, element for element; with a mean / std it is the f32 arithmetic
    of the square path on those u8 values.  The description's resize_* and crop fields are ignored."""
    from PIL import Image
    nx, ny, ow, oh = g
    for pattern in ("random", "checker"):
        a = PPD.image(pattern, nx, ny)
        want = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BICUBIC if fname == "bicubic" else Image.BILINEAR))
        pp = binding.Preproc.make(resize_mode=PPD.PP_SHORTEST_EDGE, resize_a=7, resize_b=0, filter=PPD.FILTERS[fname], crop=5)
        got = binding.preprocess_rect(a, pp, ow, oh)
        assert got.shape == (oh, ow, 3) and got.dtype == np.float32
        assert np.array_equal(got, want.astype(np.float32)), (g, pattern, fname, int((got != want).sum()))
        mean, std = PPD.mean_std255(PPD.CLIP)
        pp = PPD.make_pp(binding, dict(resize_mode=PPD.PP_STRETCH, resize_a=9, resize_b=9, filter=PPD.FILTERS[fname], crop=0, crop_round=0), mean, std)
        got = binding.preprocess_rect(a, pp, ow, oh)
        assert np.array_equal(_bits(got), _bits((want.astype(np.float32) - mean) / std)), (g, pattern, fname)


@pytest.mark.parametrize("fname", list(PPD.FILTERS))
def test_square_rect_equals_preprocess_ex(binding, fname):
    """out_w == out_h == S: the bits of vitx_preprocess_ex with {STRETCH, S, S, filter, 0, 0}."""
    mean, std = PPD.mean_std255(PPD.IMAGENET)
    for nx, ny, S in ((500, 375, 224), (37, 23, 16), (13, 9, 28), (33, 33, 33), (224, 100, 224)):
        a = PPD.image("random", nx, ny)
        pp = PPD.make_pp(binding, dict(resize_mode=PPD.PP_STRETCH, resize_a=S, resize_b=S, filter=PPD.FILTERS[fname], crop=0, crop_round=0), mean, std)
        assert np.array_equal(_bits(binding.preprocess_rect(a, pp, S, S)), _bits(binding.preprocess_ex(a, pp))), (nx, ny, S)


def test_preprocess_rect_refusals(binding):
    L = binding.lib()
    a = PPD.image("random", 20, 10)
    src = a.ctypes.data_as(C.POINTER(C.c_uint8))
    out = np.full((8, 12, 3), 7.0, np.float32)
    dst = out.ctypes.data_as(C.POINTER(C.c_float))
    ok = binding.Preproc.make(resize_a=16, resize_b=16, filter=PPD.PP_PIL_BICUBIC)
    call = lambda pp=ok, s=src, nx=20, ny=10, ow=12, oh=8, d=dst: L.vitx_preprocess_rect(C.byref(pp) if pp is not None else None, s, nx, ny, ow, oh, d)
    invalid = binding.Preproc.make(resize_a=16, resize_b=12, filter=PPD.PP_PIL_BICUBIC)          # a description pp_check refuses (a non-square output)
    bad = [call(pp=None), call(s=None), call(d=None), call(nx=0), call(ny=-1), call(ow=0), call(oh=0), call(ow=-4), call(ow=16385), call(oh=16385),
           call(nx=(1 << 20) + 1), call(pp=invalid), call(pp=binding.Preproc.make(resize_a=16, resize_b=16, filter=9))]
    assert bad == [ERR_ARG] * len(bad), bad
    for f in (PPD.PP_REF_BICUBIC, PPD.PP_REF_BILINEAR):
        assert call(pp=binding.Preproc.make(resize_a=16, resize_b=16, filter=f)) == ERR_UNSUPPORTED
        assert "vitx_preprocess_rect" in L.vitx_last_error().decode()
        assert not binding.preprocess_rect_device_supports(binding.Preproc.make(resize_a=16, resize_b=16, filter=f), 20, 10, 12, 8)
    assert (out == 7.0).all(), "a refused call wrote its output"
    assert call() == 0 and (out != 7.0).any()
    # the LDS bound of the device form, without a device: include/vitx.h's limit case and one beyond it
    assert binding.preprocess_rect_device_supports(ok, 500, 375, 288, 224)
    assert binding.preprocess_rect_device_supports(ok, 576, 8, 8, 8) == binding.preprocess_ex_device_supports(binding.Preproc.make(resize_a=8, resize_b=8, filter=PPD.PP_PIL_BICUBIC), 576, 8)
    assert not binding.preprocess_rect_device_supports(ok, 100000, 8, 8, 16)
    assert not binding.preprocess_rect_device_supports(ok, 0, 8, 8, 16) and not binding.preprocess_rect_device_supports(invalid, 20, 10, 12, 8)


# ------------------------------------------------------------------------------------------------ context creation
def test_new_names_are_exported_and_the_options_struct_keeps_its_size(binding):
    L = binding.lib()
    for name in ("vitx_ctx_create_rect", "vitx_ctx_img_shape", "vitx_ctx_grid", "vitx_op_patch_embed_rect", "vitx_rect_shape", "vitx_preprocess_rect",
                 "vitx_preprocess_rect_device", "vitx_preprocess_rect_device_supports"):
        assert name in binding.EXPORTS and hasattr(L, name), name
    assert C.sizeof(binding.CtxOptions) == 48
    a, b = C.c_int(5), C.c_int(5)
    assert L.vitx_ctx_img_shape(None, C.byref(a), C.byref(b)) == ERR_ARG and L.vitx_ctx_grid(None, C.byref(a), C.byref(b)) == ERR_ARG


def test_create_rect_argument_errors_come_before_any_device(pkg, binding):
    """Host-side checks only: they run before any device is touched, so without a GPU a well-formed call ends in VITX_ERR_HIP."""
    L = binding.lib()
    model = binding.Model(pkg.synth.cached_synthetic(MICRO16, head_scale=4.0))

    def create(h, w, m=model, dtype=binding.F16, opt=True, max_batch=1, **kw):
        size = kw.pop("struct_size", 48)
        o = binding.CtxOptions(**kw); o.struct_size = size
        ctx = C.c_void_p()
        rc = L.vitx_ctx_create_rect(m._h if m is not None else None, 0, max_batch, dtype, C.byref(o) if opt else None, h, w, C.byref(ctx))
        geo = None
        if rc == 0:
            a, b, gh, gw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            assert L.vitx_ctx_img_shape(ctx, C.byref(a), C.byref(b)) == 0 and L.vitx_ctx_grid(ctx, C.byref(gh), C.byref(gw)) == 0
            geo = (a.value, b.value, gh.value, gw.value, L.vitx_ctx_img_size(ctx), L.vitx_ctx_tokens(ctx))
            L.vitx_ctx_free(ctx)
        return rc, geo

    rc, geo = create(48, 80)
    assert rc in (0, ERR_HIP) and geo in (None, (48, 80, 3, 5, 0, 16))
    rc, geo = create(48, 80, opt=False)
    assert rc in (0, ERR_HIP) and geo in (None, (48, 80, 3, 5, 0, 16))
    rc, geo = create(96, 96, pos_interp=1)
    assert rc in (0, ERR_HIP) and geo in (None, (96, 96, 6, 6, 96, 37))
    for h, w in ((0, 64), (64, 0), (-16, 64), (64, -16), (40, 64), (64, 40), (8, 64), (0, 0)):
        assert create(h, w)[0] == ERR_ARG, (h, w)
        assert "vitx_ctx_create_rect" in L.vitx_last_error().decode()
    assert create(48, 80, img_size=64)[0] == ERR_ARG and create(48, 80, img_size=96)[0] == ERR_ARG and create(64, 64, img_size=64)[0] == ERR_ARG
    assert "img_size must be 0" in L.vitx_last_error().decode()
    assert create(48, 80, pos_interp=2)[0] == ERR_ARG and create(48, 80, struct_size=52)[0] == ERR_ARG and create(48, 80, streams=9)[0] == ERR_ARG
    assert create(48, 80, m=None)[0] == ERR_ARG and create(48, 80, dtype=7)[0] == ERR_ARG and create(48, 80, max_batch=0)[0] == ERR_ARG
    # an old caller's short struct: img_size lies behind it and is not read
    rc, _ = create(48, 80, struct_size=40, img_size=64)
    assert rc in (0, ERR_HIP)
    vitstr = binding.Model(pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0))
    assert create(224, 448, m=vitstr)[0] == ERR_UNSUPPORTED and create(448, 224, m=vitstr)[0] == ERR_UNSUPPORTED
    assert create(224, 224, m=vitstr)[0] in (0, ERR_HIP)
    with pytest.raises(ValueError, match="img_shape and img_size"):
        binding.Context(model, img_shape=(48, 80), img_size=64)
    vitstr.close(); model.close()
