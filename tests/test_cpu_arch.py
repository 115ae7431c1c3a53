"""Activation, LayerNorm epsilon and pre-norm on the host (no GPU): the file format's `arch` and `pre_norm.*` extensions, the loader, the file
tools, the converters (HuggingFace ViT, DINOv2, CLIP, timm), and the float64 restatement (tests/arch_data.py) the GPU tests compare with --
pinned here to transformers' ViT, DINOv2 and CLIP with the settings released checkpoints really have."""
import ctypes as C
import hashlib
import struct

import numpy as np
import pytest

import arch_data as AD
import prefix_data as PD
import ref64 as R64

ERR_FORMAT = 2
HF_TOL = 2e-4                        # tests/test_cpu_oracle.py:115 (test_oracle_vs_transformers_vit_f32), as tests/test_cpu_registers.py
KW = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, patch_size=14, image_size=56)        # the micro shape of tests/test_cpu_registers.py


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _redraw(torch, m, seed):
    """Every parameter of a transformers model from a numpy generator (initial values are partly constants, and torch's own draws are not
    what a recorded checksum should depend on); the patch kernel is made fp16-exact: the file stores it in fp16 even at ftype 0."""
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for k, p in m.named_parameters():
            shape = tuple(p.shape)
            if k.endswith("lambda1"):
                v = rng.random(shape) * 1.5 + 0.25                           # LayerScale
            elif k.endswith(".bias"):
                v = rng.standard_normal(shape) * 0.02
            elif p.dim() == 1 and k.endswith(".weight"):
                v = 1.0 + rng.standard_normal(shape) * 0.1                   # LayerNorm weights
            elif p.dim() == 4:
                v = rng.standard_normal(shape) * 0.02                        # the patch kernel
            elif p.dim() == 2 and "position" not in k:
                v = rng.standard_normal(shape) * 0.05                        # every matrix
            else:
                v = rng.standard_normal(shape) * 0.5                         # class token, registers, mask token, position table
            p.copy_(torch.from_numpy(np.asarray(v, np.float32)))
            if p.dim() == 4:
                p.copy_(p.half().float())
    return m


def _hf_model(kind, seed=21, **over):
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    if kind == "vit":
        cfg = tr.ViTConfig(intermediate_size=512, num_labels=10, **{**KW, **dict(hidden_act="gelu", layer_norm_eps=1e-12), **over})
        m = tr.ViTForImageClassification(cfg)
    elif kind == "dinov2":
        cfg = tr.Dinov2Config(num_labels=10, **{**KW, **dict(hidden_act="gelu", layer_norm_eps=1e-6), **over})
        m = tr.Dinov2ForImageClassification(cfg)
    else:
        cfg = tr.CLIPVisionConfig(intermediate_size=512, projection_dim=24, **{**KW, **dict(hidden_act="quick_gelu", layer_norm_eps=1e-5), **over})
        m = tr.CLIPVisionModelWithProjection(cfg)
    return torch, _redraw(torch, m.eval(), seed)


WANT = {"vit": (AD.ACT_ERF, 1e-12, False), "dinov2": (AD.ACT_ERF, 1e-6, False), "clip": (AD.ACT_QUICK, 1e-5, True)}


@pytest.mark.parametrize("kind", ["vit", "dinov2", "clip"])
def test_restatement_and_converter_against_transformers(pkg, binding, tmp_path, kind):
    """convert_hf_model at ftype 0 of a model with the settings its released checkpoints have (HF ViT: erf, 1e-12; DINOv2: erf, 1e-6; CLIP:
    QuickGELU, 1e-5, pre_layrnorm, bias-free convolution and projection), then ref64.forward64 on the file's tensors against the model
    itself: every hidden state and the logits (CLIP: image_embeds) to f32 noise.  The file reports its settings through the loader."""
    torch, m = _hf_model(kind)
    path = str(tmp_path / f"{kind}.gguf")
    hp = pkg.convert.convert_hf_model(m, path, ftype=0)
    C_ = 24 if kind == "clip" else 10
    assert (hp.hidden_size, hp.num_hidden_layers, hp.num_attention_heads, hp.num_classes, hp.patch_size, hp.img_size) == (128, 2, 2, C_, 14, 56)
    t = PD.file_tensors(pkg, path)
    act, eps, pre = WANT[kind]
    names = list(t)
    assert names[0] == "arch" and np.array_equal(_bits(t["arch"]), _bits(np.array([act, eps, 0, 0], np.float32)))
    assert ("pre_norm.weight" in t) == pre
    if pre:
        assert names[1:5] == ["cls_token", "pos_embed", "pre_norm.weight", "pre_norm.bias"]
        assert not t["patch_embed.proj.bias"].any() and not t["head.bias"].any()
        assert pkg.ggml_file.read_model(path).id2label == {i: f"dim_{i}" for i in range(24)}
    mdl = binding.Model(path)
    assert (mdl.activation, mdl.has_pre_norm) == (act, pre) and _bits(mdl.hparams.eps) == _bits(np.float32(eps))
    assert len(mdl.tensors()) == 4 + 24 + 4 + 1 + (2 if pre else 0)
    mdl.close()
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(2, 56, seed=3))
    px = torch.from_numpy(imgs).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        out = m(pixel_values=px, output_hidden_states=True)
    r = R64.forward64(t, imgs, heads=2)
    want_logits = (out.image_embeds if kind == "clip" else out.logits).numpy()
    # every hidden state, stage 0 included: with a pre-norm it is the stream that enters layer 0 (transformers' CLIP encoder starts from the normalised rows)
    assert r["trace"].shape == (3, 2, 17, 128) and len(out.hidden_states) == 3
    if kind == "clip":
        with torch.no_grad():
            e = m.vision_model.embeddings(px).numpy()
        d = float(np.abs(r["embed"] - e).max())
        print(f"clip embedding in front of the pre-norm: max|restatement - transformers| = {d:.3e}")
        assert d <= HF_TOL, d
    for s in range(3):
        d = float(np.abs(r["trace"][s] - out.hidden_states[s].numpy()).max())
        print(f"{kind} hidden state {s}: max|restatement - transformers| = {d:.3e}")
        assert d <= HF_TOL, (s, d)
    d = float(np.abs(r["logits"] - want_logits).max())
    print(f"{kind} logits: max|restatement - transformers| = {d:.3e}  (max|logit| {np.abs(want_logits).max():.3f})")
    assert d <= HF_TOL, d
    # the comparison sees the settings: the reference's arithmetic (tanh, 1e-6, no pre-norm) on the same tensors is NOT the model
    wrong = R64.forward64(t, imgs, heads=2, activation=AD.ACT_TANH, eps=1e-6, pre_norm=False)
    dw = float(np.abs(wrong["logits"] - want_logits).max())
    print(f"{kind} logits with tanh / 1e-6 / no pre-norm: max|d| = {dw:.3e}")
    if kind == "clip":              # erf against tanh alone moves these logits by about the gate itself (max |tanh - erf| = 4.7e-4 per element): printed, not asserted
        assert dw > 100 * HF_TOL, dw


def test_clip_model_and_tower_without_projection(pkg, tmp_path):
    """CLIPModel converts to the bytes of its own vision tower + visual_projection; a CLIPVisionModel needs --no-head semantics."""
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    _, vis = _hf_model("clip")
    full = tr.CLIPModel(tr.CLIPConfig(vision_config=vis.config.to_dict(), text_config=dict(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2,
                                                                                             vocab_size=50, max_position_embeddings=8), projection_dim=24)).eval()
    sd = full.state_dict()
    with torch.no_grad():
        for k, v in vis.state_dict().items():
            sd[k].copy_(v)
    a, b = str(tmp_path / "a.gguf"), str(tmp_path / "b.gguf")
    pkg.convert.convert_hf_model(vis, a, ftype=1)
    pkg.convert.convert_hf_model(full, b, ftype=1)
    assert open(a, "rb").read() == open(b, "rb").read()
    tower = tr.CLIPVisionModel(vis.config).eval()
    with pytest.raises(ValueError, match="no_head"):
        pkg.convert.convert_hf_model(tower, b, ftype=1)
    hp = pkg.convert.convert_hf_model(tower, b, ftype=1, no_head=True)
    t = PD.file_tensors(pkg, b)
    assert hp.num_classes == 1 and pkg.ggml_file.read_model(b).id2label == {0: "(no head)"} and t["head.weight"].shape == (1, 128) and "pre_norm.bias" in t
    # an activation the forward path does not evaluate is refused by name
    vis.config.hidden_act = "relu"
    with pytest.raises(ValueError, match="relu"):
        pkg.convert.convert_hf_model(vis, b, ftype=1)


# sha1 of the files the parent commit's convert.py writes from the same inputs (recorded once, from that commit)
PARENT_SHA1 = {
    "hf_vit_tanh_1e-6_ft1": "c0bffab9de01629cdbb99e3dce951757c078a775",
    "timm_micro_ft1": "d66866692e8fc5b4d3e006ce56d2a56ad8c7c539",
}


def test_conversions_with_the_references_settings_keep_their_bytes(pkg, tmp_path):
    """`arch` is written only when (activation, eps) differs from (tanh, 1e-6): a conversion with the reference's settings is byte for byte the
    file the converter wrote before it knew about either, and the timm path's default still is that file."""
    torch, m = _hf_model("vit", seed=33, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6)
    p = str(tmp_path / "hf.gguf")
    pkg.convert.convert_hf_model(m, p, ftype=1)
    assert "arch" not in PD.file_tensors(pkg, p)
    assert hashlib.sha1(open(p, "rb").read()).hexdigest() == PARENT_SHA1["hf_vit_tanh_1e-6_ft1"]
    hp = pkg.synth.hparams_for("vit_micro_patch16_64")
    w = pkg.synth.make_weights(hp, seed=5, head_scale=4.0)
    q = str(tmp_path / "timm.gguf")
    pkg.convert.convert_timm_state_dict(dict(w), q, ftype=1, heads=2)
    assert hashlib.sha1(open(q, "rb").read()).hexdigest() == PARENT_SHA1["timm_micro_ft1"]
    pkg.convert.convert_timm_state_dict(dict(w), p, ftype=1, heads=2, act="tanh", eps=1e-6)
    assert open(p, "rb").read() == open(q, "rb").read()
    # ... and with timm's own activation the same tensors follow an `arch` record
    pkg.convert.convert_timm_state_dict(dict(w), p, ftype=1, heads=2, act="erf")
    rec = struct.pack("<iii", 1, 4, 0) + struct.pack("<i", 4) + b"arch" + np.array([1, 1e-6, 0, 0], np.float32).tobytes()
    a, b = open(p, "rb").read(), open(q, "rb").read()
    first = b.index(struct.pack("<iii", 3, len("cls_token"), 0))
    assert a == b[:first] + rec + b[first:]
    with pytest.raises(ValueError, match="act"):
        pkg.convert.convert_timm_state_dict(dict(w), p, heads=2, act="relu")


def _record(name, ttype, shape, data):
    nb = name.encode()
    return struct.pack("<iii", len(shape), len(nb), ttype) + b"".join(struct.pack("<i", d) for d in reversed(shape)) + nb + data


def _arch(*vals):
    return _record("arch", 0, (len(vals),), np.array(vals, np.float32).tobytes())


def test_loader_accepts_the_extensions_anywhere_and_rejects_malformed_ones(pkg, binding, tmp_path):
    L = binding.lib()
    plain = pkg.synth.cached_synthetic(AD.MICRO, head_scale=4.0)
    base = open(plain, "rb").read()
    first = base.index(struct.pack("<iii", 3, len("cls_token"), 0))
    D = 128
    ones = np.ones(D, np.float32).tobytes()
    pw, pb = _record("pre_norm.weight", 0, (D,), ones), _record("pre_norm.bias", 0, (D,), ones)

    def load(extra_front=b"", extra_back=b""):
        p = str(tmp_path / "x.gguf")
        open(p, "wb").write(base[:first] + extra_front + base[first:] + extra_back)
        h = C.c_void_p()
        rc = L.vitx_model_load(p.encode(), C.byref(h))
        out = None
        if rc == 0:
            hp = binding.HParams(); L.vitx_model_hparams(h, C.byref(hp))
            out = (L.vitx_model_activation(h), float(hp.eps), L.vitx_model_has_pre_norm(h), L.vitx_model_num_tensors(h))
            L.vitx_model_free(h)
        return rc, out, L.vitx_last_error().decode()

    # absent: today's behaviour
    assert load()[:2] == (0, (0, float(np.float32(1e-6)), 0, 32))
    # present, in front (the converter's place) or at the very end
    for act, eps in ((1, 1e-12), (2, 1e-5), (0, 1e-2)):
        for where in ("front", "back"):
            rc, out, _ = load(**{f"extra_{where}": _arch(act, eps, 0, 0) + pw + pb})
            assert rc == 0 and out == (act, float(np.float32(eps)), 1, 35), (act, eps, where, out)
    assert load(extra_back=pb + pw)[1] == (0, float(np.float32(1e-6)), 1, 34)
    bad = {
        "arch in f16": _record("arch", 1, (4,), np.zeros(4, np.float16).tobytes()),
        "arch of 3": _arch(1, 1e-6, 0),
        "arch of 5": _arch(1, 1e-6, 0, 0, 0),
        "arch with two dims": _record("arch", 0, (1, 4), np.array([1, 1e-6, 0, 0], np.float32).tobytes()),
        "activation 3": _arch(3, 1e-6, 0, 0),
        "activation -1": _arch(-1, 1e-6, 0, 0),
        "activation 1.5": _arch(1.5, 1e-6, 0, 0),
        "activation nan": _arch(np.nan, 1e-6, 0, 0),
        "eps 0": _arch(1, 0.0, 0, 0),
        "eps negative": _arch(1, -1e-6, 0, 0),
        "eps inf": _arch(1, np.inf, 0, 0),
        "eps nan": _arch(1, np.nan, 0, 0),
        "reserved slot 2": _arch(1, 1e-6, 1, 0),
        "reserved slot 3": _arch(1, 1e-6, 0, 1e-30),
        "arch twice": _arch(1, 1e-6, 0, 0) + _arch(1, 1e-6, 0, 0),
        "pre_norm.weight alone": pw,
        "pre_norm.bias alone": pb,
        "pre_norm.weight twice": pw + pw + pb,
        "pre_norm.weight of D / 2": _record("pre_norm.weight", 0, (D // 2,), ones[:D * 2]) + pb,
        "pre_norm.bias in f16": pw + _record("pre_norm.bias", 1, (D,), np.ones(D, np.float16).tobytes()),
    }
    for what, rec in bad.items():
        for where in ("front", "back"):
            rc, _, msg = load(**{f"extra_{where}": rec})
            assert rc == ERR_FORMAT and msg.startswith("vitx_model_load:") and ("arch" in msg or "pre_norm" in msg), (what, where, rc, msg)


def test_quantize_and_resize_carry_arch_and_pre_norm_through(pkg, binding, tmp_path):
    src = AD.fixture_file(pkg, "clip")
    recs0 = {t.name: t for t in pkg.ggml_file.read_model(src).tensors}
    assert list(recs0)[0] == "arch" and list(recs0)[2:5] == ["pos_embed", "pre_norm.weight", "pre_norm.bias"]
    q8 = str(tmp_path / "q8.gguf")
    binding.quantize_file(src, q8, 8)
    big = str(tmp_path / "84.gguf")
    binding.resize_file(src, big, 84, binding.POS_BICUBIC)
    for path, img in ((q8, 56), (big, 84)):
        m = binding.Model(path)
        assert (m.activation, m.has_pre_norm, m.img_size) == (AD.ACT_QUICK, True, img) and _bits(m.hparams.eps) == _bits(np.float32(1e-5))
        m.close()
        recs = {t.name: t for t in pkg.ggml_file.read_model(path).tensors}
        assert list(recs) == list(recs0)
        for k in ("arch", "pre_norm.weight", "pre_norm.bias"):
            assert (recs[k].ttype, recs[k].ne, recs[k].raw) == (recs0[k].ttype, recs0[k].ne, recs0[k].raw), (path, k)
    assert {t.name: t.ttype for t in pkg.ggml_file.read_model(q8).tensors}["blocks.0.mlp.fc1.weight"] == 8


def test_exact_test_inputs_separate_the_activations():
    """The epilogue's exact test (tests/test_gpu_arch.py) can only pin an activation where the float64 references themselves differ by more than
    the tolerance allows: on the grid x = k / 64, k in [-512, 512), count the points where the other activation lies more than two tolerances away."""
    n = {dt: int(AD.separated(AD.ACT_ERF, AD.ACT_TANH, dt).sum()) for dt in (0, 1)}
    nq = {dt: int(AD.separated(AD.ACT_QUICK, AD.ACT_TANH, dt).sum()) for dt in (0, 1)}
    print(f"tanh outside 2 tolerances of erf: fp16 {n[0]}, bf16 {n[1]} of 1024 points; of QuickGELU: fp16 {nq[0]}, bf16 {nq[1]}")
    assert n[0] >= 200 and n[1] >= 150 and nq[0] >= 700 and nq[1] >= 500
    x = AD.grid()[AD.separated(AD.ACT_ERF, AD.ACT_TANH, 0)]
    assert x.min() >= -4.875 and x.max() <= -1.3125           # the negative flank, where tanh-GELU's tail is too thin
    # the tolerance's building blocks
    assert AD.ulp_T(1.0, 0) == 2.0 ** -10 and AD.ulp_T(1.5, 1) == 2.0 ** -7 and AD.ulp_T(0.75, 0) == 2.0 ** -11 and AD.ulp_T(1e-9, 0) == 2.0 ** -24
    assert abs(float(AD.act64(-5.0, AD.ACT_ERF)) - (-5.0 * 2.8665157187919333e-07)) < 1e-18          # x Phi(x): Phi(-5) to its last digits, no cancellation
    assert float(AD.act64(3.0, AD.ACT_QUICK)) == 3.0 / (1.0 + np.exp(-5.106))
