"""Each model's own preprocessing on the host (no GPU): vitx_preprocess_ex against Pillow, bit for bit; shortest-edge sizing and crop offsets;
the normalisation; the default description = vitx_preprocess_u8; the `preproc` tensor through the loader and the file tools; the converters;
vit_image_preprocess_model through a g++-built caller.  include/vitx.h "each model's own preprocessing"; the case tables: tests/preproc_data.py."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import preproc_data as PD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "assets")
ERR_FORMAT, ERR_ARG = 2, 3


def _u8(binding, a, spec):
    """The library's u8 window: with mean 0 and std 1 the f32 output IS q."""
    out = binding.preprocess_ex(a, PD.make_pp(binding, spec))
    q = out.astype(np.uint8)
    assert np.array_equal(q.astype(np.float32), out), "outputs with mean 0 / std 1 must be whole numbers in 0 .. 255"
    return q


# ------------------------------------------------------------------------------------------------ the resize, against Pillow
@pytest.mark.parametrize("fname", list(PD.FILTERS))
@pytest.mark.parametrize("pattern", PD.PATTERNS)
@pytest.mark.parametrize("g", PD.GEOMETRIES, ids=PD.geo_id)
def test_host_resize_is_pillow_bit_for_bit(binding, g, pattern, fname):
    a = PD.image(pattern, g[0], g[1])
    spec = PD.geometry_spec(g, PD.FILTERS[fname])
    got = _u8(binding, a, spec)
    want, (W, H, _, _) = PD.pillow_window(a, spec)
    assert (W, H) == (g[2], g[3])
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ from Pillow, max |d| {int(np.abs(got.astype(int) - want.astype(int)).max())}"
    assert PD.sha1(got) == PD.golden()["sha1"][PD.golden_key(g, pattern, fname)]       # the record of Pillow 12.2.0
    if pattern == "zeros":
        assert (got == 0).all()
    if pattern == "ones":
        assert (got == 255).all()


def test_bicubic_overshoot_clamps(binding):
    """On a 0 / 255 checkerboard up-scaled 2.7 times bicubic's negative lobes drive the sum below 0 and above 255: both must clamp, not wrap."""
    a = PD.image("checker", 3, 2)
    spec = dict(resize_mode=PD.PP_STRETCH, resize_a=8, resize_b=8, filter=PD.PP_PIL_BICUBIC, crop=0, crop_round=0)
    got = _u8(binding, a, spec)
    want, _ = PD.pillow_window(a, spec)
    assert np.array_equal(got, want) and (got == 0).any() and (got == 255).any()


# ------------------------------------------------------------------------------------------------ sizing and crop offsets
def _se(short, crop, crop_round=0, f=PD.PP_PIL_BICUBIC):
    return dict(resize_mode=PD.PP_SHORTEST_EDGE, resize_a=short, resize_b=0, filter=f, crop=crop, crop_round=crop_round)


@pytest.mark.parametrize("nx,ny,short,crop,crop_round,W,H,left,top", [
    (500, 375, 224, 224, 0, 298, 224, 37, 0),        # the long edge truncates: 224 * 500 / 375 = 298.67
    (375, 500, 224, 224, 0, 224, 298, 0, 37),        # portrait
    (50, 37, 18, 16, 0, 24, 18, 4, 1),               # even differences 8 and 2
    (50, 37, 18, 13, 0, 24, 18, 5, 2),               # odd differences 11 and 5: floor 5 and 2 ...
    (50, 37, 18, 13, 1, 24, 18, 6, 2),               # ... torchvision: 5.5 -> 6 (half to even), 2.5 -> 2
    (50, 37, 18, 15, 0, 24, 18, 4, 1),               # differences 9 and 3: floor 4 and 1 ...
    (50, 37, 18, 15, 1, 24, 18, 4, 2),               # ... torchvision: 4.5 -> 4, 1.5 -> 2
])
def test_shortest_edge_sizing_and_crop_offsets(binding, nx, ny, short, crop, crop_round, W, H, left, top):
    from PIL import Image
    a = PD.image("random", nx, ny)
    spec = _se(short, crop, crop_round)
    assert PD.resized_size(nx, ny, PD.PP_SHORTEST_EDGE, short, 0) == (W, H)
    got = _u8(binding, a, spec)
    r = np.asarray(Image.fromarray(a).resize((W, H), Image.BICUBIC))
    assert np.array_equal(got, r[top:top + crop, left:left + crop])          # the offsets stated above, not computed
    want, (W2, H2, l2, t2) = PD.pillow_window(a, spec)                       # ... and the table's restatement agrees with them
    assert (W2, H2, l2, t2) == (W, H, left, top) and np.array_equal(got, want)
    for dl, dt in ((1, 0), (0, 1)):                                            # a neighbouring offset is another window
        l, t = left + dl, top + dt
        if l + crop <= W and t + crop <= H:
            assert not np.array_equal(got, r[t:t + crop, l:l + crop])


def test_description_errors(binding):
    a = PD.image("random", 50, 37)

    def err(spec, img=a, **kw):
        with pytest.raises(binding.VitxError) as e:
            binding.preprocess_ex(img, PD.make_pp(binding, spec, **kw))
        return e.value.code

    assert err(_se(18, 19)) == ERR_ARG                                          # 24 x 18 resized: the crop exceeds the height
    assert err(_se(18, 25)) == ERR_ARG                                          # ... and the width
    assert err(_se(0, 16)) == ERR_ARG and err(_se(-4, 16)) == ERR_ARG           # non-positive sizes
    assert err(dict(_se(18, 16), crop=-1)) == ERR_ARG
    assert err(dict(resize_mode=PD.PP_STRETCH, resize_a=16, resize_b=0, filter=PD.PP_PIL_BICUBIC, crop=0, crop_round=0)) == ERR_ARG
    assert err(dict(_se(18, 16), filter=PD.PP_REF_BICUBIC)) == ERR_ARG          # a REF filter stretches and does not crop
    assert err(dict(resize_mode=PD.PP_STRETCH, resize_a=16, resize_b=16, filter=PD.PP_REF_BILINEAR, crop=8, crop_round=0)) == ERR_ARG
    assert err(dict(_se(18, 16), filter=4)) == ERR_ARG and err(dict(_se(18, 16), filter=-1)) == ERR_ARG       # unknown enum values
    assert err(dict(_se(18, 16), resize_mode=2)) == ERR_ARG and err(dict(_se(18, 16), crop_round=2)) == ERR_ARG
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert err(_se(18, 16), std255=(1.0, bad, 1.0)) == ERR_ARG
    assert err(_se(18, 16), mean255=(float("nan"), 0.0, 0.0)) == ERR_ARG
    assert err(_se(18, 0)) == ERR_ARG                                           # shortest edge without a crop: not square
    assert err(dict(resize_mode=PD.PP_STRETCH, resize_a=16, resize_b=12, filter=PD.PP_PIL_BICUBIC, crop=0, crop_round=0)) == ERR_ARG
    assert binding.preprocess_ex(a, PD.make_pp(binding, _se(18, 18))).shape == (18, 18, 3)      # the largest crop that fits


# ------------------------------------------------------------------------------------------------ normalisation
@pytest.mark.parametrize("name,ms", [("imagenet", PD.IMAGENET), ("clip", PD.CLIP), ("half", PD.HALF)])
def test_normalisation_against_float64(binding, name, ms):
    """All 256 values in all 3 channels through an equal-size (skipped) resize: |out - (q / 255 - mean) / std| <= 1e-6.  The bound covers the
    roundings of mean255 and std255 (2^-24 relative each), the subtraction and the division at |out| <= 2.7: 4 * 2.7 * 6e-8 = 6.5e-7."""
    a = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    a[:, :, 1] = a[::-1, :, 1]; a[:, :, 2] = a[:, ::-1, 2]                      # the channels differ
    m255, s255 = PD.mean_std255(ms)
    for f in PD.FILTERS.values():
        pp = PD.make_pp(binding, dict(resize_mode=PD.PP_STRETCH, resize_a=16, resize_b=16, filter=f, crop=0, crop_round=0), m255, s255)
        out = binding.preprocess_ex(a, pp)
        want = (a.astype(np.float64) / 255.0 - np.asarray(ms[0], np.float64)) / np.asarray(ms[1], np.float64)
        d = float(np.abs(out.astype(np.float64) - want).max())
        print(f"{name}: max |out - float64| = {d:.2e}, max |out| = {np.abs(want).max():.3f}")
        assert np.abs(want).max() <= 2.7 and d <= 1e-6
        # and the f32 form itself: ((float)q - mean255) / std255 with IEEE division
        assert np.array_equal(out, (a.astype(np.float32) - m255) / s255)


def test_imagenet_mean255_is_the_references_literals(binding, pkg):
    m255, s255 = PD.mean_std255(PD.IMAGENET)
    assert np.array_equal(m255, pkg.synth.IMAGENET_MEAN) and np.array_equal(s255, pkg.synth.IMAGENET_STD)
    d = binding.Model(pkg.synth.cached_synthetic("vit_micro_patch16_64", head_scale=4.0)).preproc().fields()
    assert np.array_equal(d["mean255"], m255) and np.array_equal(d["std255"], s255)


# ------------------------------------------------------------------------------------------------ the default description
@pytest.mark.parametrize("asset", ["tench.jpg", "image.png"])
def test_default_description_gives_the_bits_of_preprocess_u8(binding, pkg, asset):
    from PIL import Image
    a = np.asarray(Image.open(os.path.join(ASSETS, asset)).convert("RGB"), dtype=np.uint8)
    model = binding.Model(pkg.synth.cached_synthetic("vit_micro_patch16_64", head_scale=4.0))
    assert not model.has_preproc
    pp = model.preproc()
    assert pp.fields() == dict(resize_mode=PD.PP_STRETCH, resize_a=64, resize_b=64, filter=PD.PP_REF_BICUBIC, crop=0, crop_round=0,
                               mean255=tuple(pkg.synth.IMAGENET_MEAN), std255=tuple(pkg.synth.IMAGENET_STD))
    for f, interp in ((PD.PP_REF_BICUBIC, binding.BICUBIC), (PD.PP_REF_BILINEAR, binding.BILINEAR)):
        pp.filter = f
        got, want = binding.preprocess_ex(a, pp), binding.preprocess(a, 64, interp)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # at another size the default stays the reference's stretch
    p2 = binding.preproc_at_size(model.preproc(), 96)
    assert (p2.resize_a, p2.resize_b, p2.crop, p2.filter) == (96, 96, 0, PD.PP_REF_BICUBIC)
    assert np.array_equal(binding.preprocess_ex(a, p2), binding.preprocess(a, 96, binding.BICUBIC))


def test_preproc_at_size(binding):
    clip = PD.make_pp(binding, _se(224, 224), *PD.mean_std255(PD.CLIP))
    dino = PD.make_pp(binding, _se(256, 224), *PD.mean_std255(PD.IMAGENET))
    vit = PD.make_pp(binding, dict(resize_mode=PD.PP_STRETCH, resize_a=224, resize_b=224, filter=PD.PP_PIL_BILINEAR, crop=0, crop_round=0))
    f = lambda p, S: (lambda q: (q.resize_a, q.resize_b, q.crop))(binding.preproc_at_size(p, S))
    assert f(clip, 336) == (336, 0, 336) and f(clip, 224) == (224, 0, 224)
    assert f(dino, 448) == (512, 0, 448)
    assert f(dino, 518) == (592, 0, 518)              # (2 * 256 * 518 + 224) / 448 = 592.5 -> 592: 256 * 518 / 224 = 592.0 exactly
    assert f(dino, 98) == (112, 0, 98) and f(dino, 100) == (114, 0, 100)       # 114.29 -> 114
    assert f(vit, 384) == (384, 384, 0)
    q = binding.preproc_at_size(dino, 448)
    assert q.fields()["mean255"] == dino.fields()["mean255"] and q.filter == dino.filter and q.crop_round == dino.crop_round
    for bad in (0, -8):
        with pytest.raises(binding.VitxError) as e:
            binding.preproc_at_size(dino, bad)
        assert e.value.code == ERR_ARG


# ------------------------------------------------------------------------------------------------ the file
MICRO = "vit_micro_patch16_64"


def _clip_slots(pkg, S=64, **kw):
    return pkg.ggml_file.preproc_slots(PD.PP_SHORTEST_EDGE, kw.pop("resize", S), 0, PD.PP_PIL_BICUBIC, crop=S, mean=PD.CLIP[0], std=PD.CLIP[1], **kw)


def _record(slots):
    data = np.asarray(slots, "<f4").tobytes()
    return struct.pack("<iii", 1, 7, 0) + struct.pack("<i", len(data) // 4) + b"preproc" + data


def test_file_round_trip(binding, pkg, tmp_path):
    slots = _clip_slots(pkg, resize=73)
    path = pkg.synth.cached_synthetic(MICRO, head_scale=4.0, preproc=slots)
    plain = pkg.synth.cached_synthetic(MICRO, head_scale=4.0)
    # the tensor is the first record and nothing else changed
    a, b = open(path, "rb").read(), open(plain, "rb").read()
    first = b.index(struct.pack("<iii", 3, len("cls_token"), 0))
    assert a == b[:first] + _record(slots) + b[first:]
    model = binding.Model(path)
    assert model.has_preproc
    d = model.preproc().fields()
    assert d == pkg.ggml_file.preproc_fields(slots) == pkg.ggml_file.read_model(path).preproc
    assert (d["resize_mode"], d["resize_a"], d["resize_b"], d["filter"], d["crop"], d["crop_round"]) == (1, 73, 0, 3, 64, 0)
    assert np.array_equal(d["mean255"], PD.mean_std255(PD.CLIP)[0]) and np.array_equal(d["std255"], PD.mean_std255(PD.CLIP)[1])
    assert pkg.ggml_file.read_model(plain).preproc is None
    # the loader takes the record anywhere: here at the end of the file
    moved = str(tmp_path / "moved.gguf")
    open(moved, "wb").write(b + _record(slots))
    assert binding.Model(moved).preproc().fields() == d
    # vitx_quantize_file keeps the bytes
    q = str(tmp_path / "q8.gguf")
    binding.quantize_file(path, q, 8)
    recs = [t for t in pkg.ggml_file.read_model(q).tensors if t.name == "preproc"]
    assert len(recs) == 1 and recs[0].ttype == 0 and recs[0].ne == (16,) and recs[0].raw == np.asarray(slots, "<f4").tobytes()
    assert binding.Model(q).preproc().fields() == d
    # vitx_model_resize_file writes the vitx_preproc_at_size values; every other record but pos_embed is copied through
    r = str(tmp_path / "r96.gguf")
    binding.resize_file(path, r, 96)
    want = binding.preproc_at_size(model.preproc(), 96).fields()
    assert (want["resize_a"], want["crop"]) == (110, 96)                      # (2 * 73 * 96 + 64) / 128 = 110.0: 109.5 rounds up
    assert binding.Model(r).preproc().fields() == want
    ta, tr = pkg.ggml_file.read_model(path).tensors, pkg.ggml_file.read_model(r).tensors
    assert [t.name for t in ta] == [t.name for t in tr]
    assert all(x.raw == y.raw for x, y in zip(ta, tr) if x.name not in ("preproc", "pos_embed"))
    # a file without the tensor is resized without gaining one
    r2 = str(tmp_path / "plain96.gguf")
    binding.resize_file(plain, r2, 96)
    assert not binding.Model(r2).has_preproc and pkg.ggml_file.read_model(r2).preproc is None


def test_malformed_preproc_tensors_are_format_errors(binding, pkg, tmp_path):
    plain = open(pkg.synth.cached_synthetic(MICRO, head_scale=4.0), "rb").read()
    good = _clip_slots(pkg)

    def status(blob, name):
        p = str(tmp_path / f"{name}.gguf")
        open(p, "wb").write(blob)
        try:
            binding.Model(p)
        except binding.VitxError as e:
            return e.code
        return 0

    def variant(**ch):
        s = good.copy()
        for i, v in ch.items():
            s[int(i[1:])] = v
        return s

    assert status(plain + _record(good), "good") == 0
    assert status(plain + _record(good[:15]), "short") == ERR_FORMAT                        # wrong length
    assert status(plain + _record(np.concatenate([good, [0.0]])), "long") == ERR_FORMAT
    f16 = struct.pack("<iii", 1, 7, 1) + struct.pack("<i", 16) + b"preproc" + np.asarray(good, "<f2").tobytes()
    assert status(plain + f16, "f16") == ERR_FORMAT                                          # another type
    two_d = struct.pack("<iii", 2, 7, 0) + struct.pack("<ii", 4, 4) + b"preproc" + np.asarray(good, "<f4").tobytes()
    assert status(plain + two_d, "2d") == ERR_FORMAT                                         # another shape
    assert status(plain + _record(variant(s13=1.0)), "reserved") == ERR_FORMAT             # a non-zero reserved slot
    assert status(plain + _record(variant(s3=4.0)), "filter") == ERR_FORMAT                # bad enums
    assert status(plain + _record(variant(s0=2.0)), "mode") == ERR_FORMAT
    assert status(plain + _record(variant(s5=2.0)), "round") == ERR_FORMAT
    assert status(plain + _record(variant(s1=64.5)), "fraction") == ERR_FORMAT             # integers are stored exactly
    assert status(plain + _record(variant(s4=48.0)), "side") == ERR_FORMAT                 # output side != img_size
    assert status(plain + _record(variant(s1=48.0)), "crop-too-large") == ERR_FORMAT       # a crop above the short edge fits no image
    assert status(plain + _record(variant(s10=0.0)), "std") == ERR_FORMAT                  # an invalid description
    assert status(plain + _record(variant(s3=0.0)), "ref-crop") == ERR_FORMAT
    assert status(plain + _record(good) + _record(good), "twice") == ERR_FORMAT            # a duplicate
    vitstr = str(tmp_path / "vitstr.gguf")                                                   # a one-channel file
    pkg.synth.write_synthetic(vitstr, "vitstr_micro_patch16_64", preproc=good)
    with pytest.raises(binding.VitxError) as e:
        binding.Model(vitstr)
    assert e.value.code == ERR_FORMAT


# ------------------------------------------------------------------------------------------------ the converters
KW = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, patch_size=14, image_size=56)
# the published defaults of the three families (openai/clip-vit-base-patch32, facebook/dinov2-base, google/vit-base-patch16-224), at the toy size 56
PROCESSORS = {
    "clip": dict(image_processor_type="CLIPImageProcessor", do_resize=True, size={"shortest_edge": 56}, resample=3, do_center_crop=True,
                 crop_size={"height": 56, "width": 56}, do_rescale=True, rescale_factor=0.00392156862745098, do_normalize=True,
                 image_mean=list(PD.CLIP[0]), image_std=list(PD.CLIP[1]), do_convert_rgb=True),
    "dinov2": dict(image_processor_type="BitImageProcessor", do_resize=True, size={"shortest_edge": 64}, resample=3, do_center_crop=True,
                   crop_size={"height": 56, "width": 56}, do_rescale=True, rescale_factor=0.00392156862745098, do_normalize=True,
                   image_mean=list(PD.IMAGENET[0]), image_std=list(PD.IMAGENET[1]), do_convert_rgb=True),
    "vit": dict(image_processor_type="ViTImageProcessor", do_resize=True, size={"height": 56, "width": 56}, resample=2, do_rescale=True,
                rescale_factor=0.00392156862745098, do_normalize=True, image_mean=list(PD.HALF[0]), image_std=list(PD.HALF[1])),
}
WANT = {
    "clip": (dict(resize_mode=1, resize_a=56, resize_b=0, filter=PD.PP_PIL_BICUBIC, crop=56, crop_round=0), PD.CLIP),
    "dinov2": (dict(resize_mode=1, resize_a=64, resize_b=0, filter=PD.PP_PIL_BICUBIC, crop=56, crop_round=0), PD.IMAGENET),
    "vit": (dict(resize_mode=0, resize_a=56, resize_b=56, filter=PD.PP_PIL_BILINEAR, crop=0, crop_round=0), PD.HALF),
}


def _hf_model(kind):
    pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    if kind == "vit":
        return tr.ViTForImageClassification(tr.ViTConfig(intermediate_size=512, num_labels=10, **KW)).eval()
    if kind == "dinov2":
        return tr.Dinov2ForImageClassification(tr.Dinov2Config(num_labels=10, **KW)).eval()
    return tr.CLIPVisionModelWithProjection(tr.CLIPVisionConfig(intermediate_size=512, projection_dim=24, hidden_act="quick_gelu", **KW)).eval()


@pytest.mark.parametrize("kind", ["clip", "dinov2", "vit"])
def test_converter_reads_the_preprocessor_config(binding, pkg, tmp_path, kind):
    """A tiny random model saved beside a hand-written preprocessor_config.json of the family's published defaults, converted by the command
    line: the file carries the description, field by field; --no-preproc writes the bytes the converter wrote before it knew about it."""
    m = _hf_model(kind)
    src = tmp_path / "ckpt"
    m.save_pretrained(str(src))
    (src / "preprocessor_config.json").write_text(json.dumps(PROCESSORS[kind]))
    out = str(tmp_path / "with.gguf")
    assert pkg.convert.main([str(src), out]) == 0
    model = binding.Model(out)
    assert model.has_preproc
    d = model.preproc().fields()
    ints, ms = WANT[kind]
    for k, v in ints.items():
        assert d[k] == v, (k, d[k], v)
    m255, s255 = PD.mean_std255(ms)
    assert np.array_equal(d["mean255"], m255) and np.array_equal(d["std255"], s255)
    names = [t.name for t in pkg.ggml_file.read_model(out).tensors]
    assert names.index("preproc") == (names.index("arch") + 1 if "arch" in names else 0)      # directly after `arch`
    # the in-memory route, --no-preproc and a conversion without a config all write the file without the tensor
    bare, nopp = str(tmp_path / "bare.gguf"), str(tmp_path / "nopp.gguf")
    pkg.convert.convert_hf_model(m, bare)
    assert pkg.convert.main([str(src), nopp, "--no-preproc"]) == 0
    assert open(bare, "rb").read() == open(nopp, "rb").read() and "preproc" not in [t.name for t in pkg.ggml_file.read_model(bare).tensors]
    # ... which is the parent's file: the same tensors through ggml_file.write_model without the new argument
    cv, cfg = pkg.convert, m.config
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    tensors = {"vit": lambda: cv.state_dict_to_timm(sd, 2), "dinov2": lambda: cv.dinov2_state_dict_to_timm(sd, cfg), "clip": lambda: cv.clip_state_dict_to_timm(sd, cfg)}[kind]()
    hp = pkg.ggml_file.HParams(128, 2, 2, 24 if kind == "clip" else 10, 14, 56, 1)
    labels = {i: f"dim_{i}" for i in range(24)} if kind == "clip" else {int(k): str(v) for k, v in cfg.id2label.items()}
    parent = str(tmp_path / "parent.gguf")
    pkg.ggml_file.write_model(parent, hp, cv.with_arch(tensors, cv.hf_activation(cfg), cfg.layer_norm_eps), id2label=labels, ftype=1)
    assert open(parent, "rb").read() == open(bare, "rb").read()
    pkg.convert.convert_hf_model(m, nopp, preprocessor_config=PROCESSORS[kind])
    assert open(nopp, "rb").read() == open(out, "rb").read()


def test_converter_refuses_what_it_cannot_honour_by_field_name(pkg):
    base = PROCESSORS["clip"]
    for field, value in (("resample", 1), ("resample", None), ("do_resize", False), ("do_rescale", False), ("rescale_factor", 1.0), ("do_pad", True),
                         ("crop_size", {"height": 48, "width": 48}), ("crop_size", {"height": 56, "width": 48}), ("size", {"shortest_edge": 48}),
                         ("image_std", [0.5, 0.0, 0.5]), ("image_mean", [0.5])):
        with pytest.raises(ValueError, match=field):
            pkg.convert.hf_preproc({**base, field: value}, 56)
    with pytest.raises(ValueError, match="size"):
        pkg.convert.hf_preproc({**PROCESSORS["vit"], "size": {"height": 64, "width": 64}}, 56)
    with pytest.raises(ValueError, match="size"):
        pkg.convert.hf_preproc({**PROCESSORS["vit"], "size": {"shortest_edge": 56}}, 56)
    legacy = {k: v for k, v in base.items() if k != "size"}
    assert np.array_equal(pkg.convert.hf_preproc({**legacy, "size": 56, "crop_size": 56}, 56), pkg.convert.hf_preproc(base, 56))


def test_timm_state_dict_options(binding, pkg, tmp_path):
    hp = pkg.synth.hparams_for(MICRO)
    w = pkg.synth.make_weights(hp, seed=5, head_scale=4.0)
    plain, conv = str(tmp_path / "plain.gguf"), str(tmp_path / "conv.gguf")
    pkg.ggml_file.write_model(plain, hp, dict(w), ftype=1)                     # the same tensors through the writer, without the new argument
    pkg.convert.convert_timm_state_dict(dict(w), conv, ftype=1, heads=2)
    assert open(conv, "rb").read() == open(plain, "rb").read()                # no --pp-* option: the reference's file, byte for byte
    pkg.convert.convert_timm_state_dict(dict(w), conv, ftype=1, heads=2, preproc=dict(resize=0, crop=0, filt="", mean=None, std=None, crop_round=""))
    assert open(conv, "rb").read() == open(plain, "rb").read()
    pkg.convert.convert_timm_state_dict(dict(w), conv, ftype=1, heads=2, preproc=dict(resize=73, crop_round="torchvision"))
    d = binding.Model(conv).preproc().fields()
    assert (d["resize_mode"], d["resize_a"], d["resize_b"], d["filter"], d["crop"], d["crop_round"]) == (1, 73, 0, PD.PP_PIL_BICUBIC, 64, 1)
    assert np.array_equal(d["mean255"], pkg.synth.IMAGENET_MEAN) and np.array_equal(d["std255"], pkg.synth.IMAGENET_STD)
    pkg.convert.convert_timm_state_dict(dict(w), conv, ftype=1, heads=2, preproc=dict(filt="bilinear", mean=[0.5] * 3, std=[0.5] * 3))
    d = binding.Model(conv).preproc().fields()
    assert (d["resize_a"], d["filter"], d["crop"], d["crop_round"]) == (64, PD.PP_PIL_BILINEAR, 64, 0) and d["mean255"] == (127.5,) * 3
    with pytest.raises(ValueError, match="pp-crop"):
        pkg.convert.convert_timm_state_dict(dict(w), conv, heads=2, preproc=dict(crop=48))
    with pytest.raises(ValueError, match="pp-resize"):
        pkg.convert.convert_timm_state_dict(dict(w), conv, heads=2, preproc=dict(resize=48))


# ------------------------------------------------------------------------------------------------ the C++ header
CALLER = r"""
#include <cstdio>
#include "vit.h"
int main(int argc, char **argv) {
    vit_model model;
    image_u8 raw;
    image_f32 out;
    if (argc < 5 || !vit_model_load(argv[1], model) || !load_image_from_file(argv[2], raw)) return 2;
    if (!vit_image_preprocess_model(raw, out, model, atoi(argv[4]))) return 3;
    FILE *f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data.data(), sizeof(float), out.data.size(), f) != out.data.size()) return 4;
    fclose(f);
    printf("%d %d\n", out.nx, out.ny);
    return 0;
}
"""


def test_vit_image_preprocess_model_through_a_cpp_caller(binding, pkg, tmp_path):
    pkgdir = os.path.join(ROOT, "vit.cpp_amd")
    src, exe = tmp_path / "caller.cpp", str(tmp_path / "caller")
    src.write_text("#include <cstdlib>\n" + CALLER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", str(src), "-I" + pkgdir, "-L" + pkgdir, "-lvitx", "-L/opt/rocm/lib", "-Wl,-rpath," + pkgdir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    img = os.path.join(ASSETS, "tench.jpg")
    a = binding.load_image(img)
    with_pp = pkg.synth.cached_synthetic(MICRO, head_scale=4.0, preproc=_clip_slots(pkg, resize=73))
    plain = pkg.synth.cached_synthetic(MICRO, head_scale=4.0)
    for path, size, S in ((with_pp, 0, 64), (with_pp, 96, 96), (plain, 0, 64), (plain, 96, 96)):
        out = str(tmp_path / "out.f32")
        r = subprocess.run([exe, path, img, out, str(size)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.splitlines()[-1] == f"{S} {S}"
        got = np.fromfile(out, np.float32).reshape(S, S, 3)
        if path == with_pp:
            pp = binding.Model(path).preproc()
            want = binding.preprocess_ex(a, binding.preproc_at_size(pp, S) if size else pp)
            assert not np.array_equal(want, binding.preprocess(a, S, binding.BICUBIC))
        else:
            want = binding.preprocess(a, S, binding.BICUBIC)                    # a file without the tensor: vit_image_preprocess, bicubic
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
