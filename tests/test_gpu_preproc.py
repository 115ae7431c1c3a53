"""The device side of each model's own preprocessing (vitx_preprocess_ex_device; include/vitx.h "each model's own preprocessing").

tests/test_cpu_preproc.py pins the host path (vitx_preprocess_ex) to Pillow bit for bit; here the gfx950 kernel is pinned to the host path,
bit for bit in f32, inside NaN canaries:
  1. every geometry of tests/preproc_data.py, both PIL filters, both crop roundings, with CLIP's mean / std;
  2. the cases a tiled kernel can get wrong: several images in one launch, windows that are no multiple of the 32 x 8 tile, crop windows
     whose first taps are not at source index 0, an up-scale, a skipped horizontal pass;
  3. the strongest down-scale the kernel covers, and the first one beyond it: VITX_ERR_UNSUPPORTED, decided before any launch;
  4. the default description gives the bits of vitx_preprocess_u8_device; a REF filter with another mean / std gives the host's bits;
  5. end to end on the device-fed path: u8 -> device preprocess -> forward_device is host preprocess_ex + forward, and differs from the
     reference's preprocess."""
import os

import numpy as np
import pytest

import preproc_data as PD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024
CLIP255 = PD.mean_std255(PD.CLIP)


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _device(binding, torch, pp, imgs):
    """imgs u8 [n][ny][nx][3] -> f32 [n][S][S][3] by the device kernel, written between NaN guards that must stay NaN."""
    n, ny, nx = imgs.shape[:3]
    S = pp.out_size
    d_in = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    buf = torch.full((2 * GUARD + n * S * S * 3,), float("nan"), dtype=torch.float32, device="cuda")
    binding.preprocess_ex_device(pp, d_in.data_ptr(), n, nx, ny, buf.data_ptr() + 4 * GUARD)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.isnan(host[:GUARD]).all() and np.isnan(host[-GUARD:]).all(), "the kernel wrote outside its output"
    return host[GUARD:-GUARD].reshape(n, S, S, 3)


def _check(binding, torch, pp, imgs):
    want = np.stack([binding.preprocess_ex(im, pp) for im in imgs])
    assert binding.preprocess_ex_device_supports(pp, imgs.shape[2], imgs.shape[1])
    got = _device(binding, torch, pp, imgs)
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} outputs were never written"
    assert _bits_equal(got, want), f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {want.size} floats differ from vitx_preprocess_ex"


# ------------------------------------------------------------------------------------------------ 1. the geometries
@pytest.mark.parametrize("crop_round", [0, 1], ids=["floor", "torchvision"])
@pytest.mark.parametrize("fname", list(PD.FILTERS))
@pytest.mark.parametrize("g", PD.GEOMETRIES, ids=PD.geo_id)
def test_device_gives_the_host_bits(binding, torch_gpu, g, fname, crop_round):
    pp = PD.make_pp(binding, PD.geometry_spec(g, PD.FILTERS[fname], crop_round), *CLIP255)
    _check(binding, torch_gpu, pp, PD.image("random", g[0], g[1])[None])


@pytest.mark.parametrize("fname", list(PD.FILTERS))
def test_device_clamps_like_the_host_on_a_checkerboard(binding, torch_gpu, fname):
    g = (37, 23, 16, 16)
    pp = PD.make_pp(binding, PD.geometry_spec(g, PD.FILTERS[fname]))
    imgs = np.stack([PD.image(p, g[0], g[1]) for p in ("checker", "zeros", "ones")])
    _check(binding, torch_gpu, pp, imgs)
    got = _device(binding, torch_gpu, pp, imgs)
    assert got.min() >= 0.0 and got.max() <= 255.0 and (got[1] == 0.0).all() and (got[2] == 255.0).all()


# ------------------------------------------------------------------------------------------------ 2. what a tiled kernel can get wrong
@pytest.mark.parametrize("case", PD.DEVICE_EXTRA, ids=[c[0] for c in PD.DEVICE_EXTRA])
def test_device_tiling_cases(binding, torch_gpu, case):
    _, nx, ny, n, spec = case
    pp = PD.make_pp(binding, spec, *CLIP255)
    imgs = np.stack([PD.image("random", nx, ny, seed=i) for i in range(n)])
    _check(binding, torch_gpu, pp, imgs)
    if n > 1:
        assert not np.array_equal(imgs[0], imgs[1])           # different images: a wrong image stride cannot go unnoticed


# ------------------------------------------------------------------------------------------------ 3. the bound
def _stretch8(filt):
    return dict(resize_mode=PD.PP_STRETCH, resize_a=8, resize_b=8, filter=filt, crop=0, crop_round=0)


@pytest.mark.parametrize("fname", list(PD.FILTERS))
def test_strongest_downscale_and_the_first_beyond(binding, torch_gpu, fname):
    """8 x H stretched to 8 x 8: one tile whose vertical taps span all H source rows, so the LDS need grows with H alone."""
    pp = PD.make_pp(binding, _stretch8(PD.FILTERS[fname]), *CLIP255)
    H = 64
    while binding.preprocess_ex_device_supports(pp, 8, H + 1):
        H += 1
        assert H < 1 << 14
    assert H >= 256                                             # scale 32 and more is covered
    _check(binding, torch_gpu, pp, PD.image("random", 8, H)[None])
    # one row more: refused by the status alone -- decided on the host, nothing is launched (the pointers are never dereferenced)
    assert not binding.preprocess_ex_device_supports(pp, 8, H + 1)
    with pytest.raises(binding.VitxError) as e:
        binding.preprocess_ex_device(pp, 4096, 1, 8, H + 1, 4096)
    assert e.value.code == binding.ERR_UNSUPPORTED
    out = binding.preprocess_ex(PD.image("random", 8, H + 1), pp)          # the host path has no bound
    assert out.shape == (8, 8, 3) and np.isfinite(out).all()


def test_a_phone_photo_at_shortest_edge_256_is_covered(binding):
    for f in PD.FILTERS.values():
        spec = dict(resize_mode=PD.PP_SHORTEST_EDGE, resize_a=256, resize_b=0, filter=f, crop=224, crop_round=0)
        assert binding.preprocess_ex_device_supports(PD.make_pp(binding, spec), 4032, 3024)
        assert binding.preprocess_ex_device_supports(PD.make_pp(binding, spec), 3024, 4032)


def test_device_argument_errors(binding, torch_gpu):
    pp = PD.make_pp(binding, dict(resize_mode=PD.PP_SHORTEST_EDGE, resize_a=48, resize_b=0, filter=PD.PP_PIL_BICUBIC, crop=64, crop_round=0))
    with pytest.raises(binding.VitxError) as e:                 # the crop is larger than the resized image
        binding.preprocess_ex_device(pp, 4096, 1, 90, 70, 4096)
    assert e.value.code == binding.ERR_ARG
    assert not binding.preprocess_ex_device_supports(pp, 90, 70)


# ------------------------------------------------------------------------------------------------ 4. the REF filters
@pytest.mark.parametrize("interp", [0, 1], ids=["bicubic", "bilinear"])
def test_default_description_gives_the_bits_of_preprocess_u8_device(binding, pkg, torch_gpu, interp):
    torch = torch_gpu
    model = binding.Model(pkg.synth.cached_synthetic("vit_micro_patch16_64", head_scale=4.0))
    pp = model.preproc()
    assert not model.has_preproc and pp.filter == PD.PP_REF_BICUBIC
    pp.filter = PD.PP_REF_BICUBIC if interp == 0 else PD.PP_REF_BILINEAR
    imgs = np.stack([PD.image("random", 90, 70, seed=i) for i in range(2)])
    got = _device(binding, torch, pp, imgs)
    d_in = torch.from_numpy(imgs).cuda()
    d_out = torch.empty((2, 64, 64, 3), dtype=torch.float32, device="cuda")
    binding.preprocess_device(d_in.data_ptr(), 2, 90, 70, 64, d_out.data_ptr(), interp)
    torch.cuda.synchronize()
    assert _bits_equal(got, d_out.cpu().numpy())
    # and with a mean / std of its own: the host's bits
    pp2 = PD.make_pp(binding, dict(resize_mode=PD.PP_STRETCH, resize_a=64, resize_b=64, filter=pp.filter, crop=0, crop_round=0), *CLIP255)
    _check(binding, torch, pp2, imgs)
    model.close()


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_device_fed_path_end_to_end(binding, pkg, torch_gpu):
    torch = torch_gpu
    slots = pkg.ggml_file.preproc_slots(PD.PP_SHORTEST_EDGE, 32, 0, PD.PP_PIL_BICUBIC, crop=32, mean=PD.CLIP[0], std=PD.CLIP[1])
    path = pkg.synth.cached_synthetic("vit_nano_patch16_32", head_scale=4.0, preproc=slots)
    model = binding.Model(path)
    assert model.has_preproc
    pp = model.preproc()
    assert (pp.resize_mode, pp.resize_a, pp.filter, pp.crop) == (PD.PP_SHORTEST_EDGE, 32, PD.PP_PIL_BICUBIC, 32)
    img = binding.load_image(os.path.join(ROOT, "tests", "golden", "assets", "tench.jpg"))
    ny, nx = img.shape[:2]
    ctx = binding.Context(model, device=0, max_batch=1, dtype=binding.F16)
    host_pre = binding.preprocess_ex(img, pp)
    want = ctx.forward(host_pre[None])
    d_u8 = torch.from_numpy(img).cuda()
    d_pre = torch.empty((1, 32, 32, 3), dtype=torch.float32, device="cuda")
    d_probs = torch.empty((1, model.num_classes), dtype=torch.float32, device="cuda")
    # ONE explicit stream orders the two launches: handle 0 would mean the legacy default stream to the preprocess and the context's own
    # (non-blocking) stream to the forward, which nothing orders against each other
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())             # the upload of d_u8
    s = stream.cuda_stream
    assert s != 0
    binding.preprocess_ex_device(pp, d_u8.data_ptr(), 1, nx, ny, d_pre.data_ptr(), stream=s)
    ctx.forward_device(d_pre.data_ptr(), 1, d_probs.data_ptr(), stream=s)
    stream.synchronize(); ctx.synchronize(); torch.cuda.synchronize()
    assert _bits_equal(d_pre.cpu().numpy()[0], host_pre)
    assert _bits_equal(d_probs.cpu().numpy(), want)
    # the difference the description exists for: the reference's preprocess of the same image is another tensor
    assert not np.array_equal(host_pre, binding.preprocess(img, 32, binding.BICUBIC))
    ctx.close(); model.close()


def test_cli_preprocesses_by_the_files_description(binding, pkg, torch_gpu, tmp_path):
    """vit_cli.py --embed on a file with a `preproc` tensor: the embedding is the one of preprocess_ex + forward (the CLI decodes with PIL);
    --preprocess reference gives the reference preprocess's, and --img-size follows vitx_preproc_at_size."""
    import subprocess
    import sys
    from PIL import Image
    slots = pkg.ggml_file.preproc_slots(PD.PP_SHORTEST_EDGE, 36, 0, PD.PP_PIL_BICUBIC, crop=32, mean=PD.CLIP[0], std=PD.CLIP[1])
    path = pkg.synth.cached_synthetic("vit_nano_patch16_32", head_scale=4.0, preproc=slots)
    img = os.path.join(ROOT, "tests", "golden", "assets", "tench.jpg")
    u8 = np.asarray(Image.open(img).convert("RGB"), dtype=np.uint8)
    model = binding.Model(path)
    pp = model.preproc()

    def cli(*extra):
        out = str(tmp_path / "e.npy")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "vit_cli.py"), "-m", path, "-i", img, "--embed", out, *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return np.load(out)

    def embed(x, **geometry):
        ctx = binding.Context(model, device=0, max_batch=1, dtype=binding.F16, **geometry)
        ctx.feat_enable(cls=True)
        ctx.forward(x[None])
        e = ctx.feat_read()[model.hparams.num_hidden_layers - 1]["cls"].copy()
        ctx.close()
        return e

    own, ref = embed(binding.preprocess_ex(u8, pp)), embed(binding.preprocess(u8, 32, binding.BICUBIC))
    assert not np.array_equal(own, ref)
    assert np.array_equal(cli(), own) and np.array_equal(cli("--preprocess", "model"), own)
    assert np.array_equal(cli("--preprocess", "reference"), ref)
    p48 = binding.preproc_at_size(pp, 48)
    assert (p48.resize_a, p48.crop) == (54, 48)
    assert np.array_equal(cli("--img-size", "48"), embed(binding.preprocess_ex(u8, p48), img_size=48))
    model.close()
