"""Register tokens, folded LayerScale and the cls + mean head on the host (no GPU): the file format's two extensions, the loader, the file
tools, the converters, and the float64 restatement (tests/prefix_data.py) the GPU tests compare with -- pinned here to transformers' DINOv2."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import feature_data as FD
import prefix_data as PD
import ref64 as R64

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_FORMAT = 2
NAME = "vit_micro_patch14_56"        # D 128, 2 layers, 2 heads, patch 14, image 56: 16 patches, N = 17 (R = 0) or 21 (R = 4)
HF_TOL = 2e-4                        # tests/test_cpu_oracle.py:115 (test_oracle_vs_transformers_vit_f32): f32 torch against a no-rounding restatement


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _hf_dinov2(registers, seed):
    """A random-weight Dinov2[WithRegisters]ForImageClassification at the micro shape.  lambda1, the register tokens and the position table are
    re-drawn (their initial values are constants), and the patch kernel is made fp16-exact: the file stores it in fp16 even at ftype 0."""
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    kw = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, patch_size=14, image_size=56, num_labels=10, hidden_act="gelu_pytorch_tanh",
              layer_norm_eps=1e-6)
    torch.manual_seed(seed)
    if registers:
        m = tr.Dinov2WithRegistersForImageClassification(tr.Dinov2WithRegistersConfig(num_register_tokens=registers, **kw)).eval()
    else:
        m = tr.Dinov2ForImageClassification(tr.Dinov2Config(**kw)).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("lambda1"):
                p.copy_(torch.rand(p.shape, generator=g) * 1.5 + 0.25)
            elif k.endswith("register_tokens") or k.endswith("position_embeddings") or k.endswith("cls_token"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif k.endswith("patch_embeddings.projection.weight"):
                p.copy_(p.half().float())
            elif k.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return torch, m


@pytest.mark.parametrize("registers", [4, 0])
def test_restatement_and_converter_against_transformers_dinov2(pkg, tmp_path, registers):
    """convert_hf_model at ftype 0, then the float64 restatement on the file's tensors against the HF model itself: every hidden state (the
    shape of vitx_trace_read) and the logits to f32 noise.  The folded LayerScale, the register rows without a position term, the patch
    positions and the cls + mean head are all in this comparison."""
    torch, m = _hf_dinov2(registers, seed=11 + registers)
    path = str(tmp_path / "dinov2.gguf")
    hp = pkg.convert.convert_hf_model(m, path, ftype=0)
    assert (hp.hidden_size, hp.num_hidden_layers, hp.num_attention_heads, hp.num_classes, hp.patch_size, hp.img_size) == (128, 2, 2, 10, 14, 56)
    t = PD.file_tensors(pkg, path)
    assert ("reg_token" in t) == bool(registers) and t["head.weight"].shape == (10, 256) and t["pos_embed"].shape == (1, 17, 128)
    assert len(t) == 4 + 12 * 2 + 4 + (1 if registers else 0)
    if registers:
        assert list(t)[:3] == ["cls_token", "reg_token", "pos_embed"] and t["reg_token"].shape == (1, 4, 128)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(2, 56, seed=3))
    with torch.no_grad():
        out = m(pixel_values=torch.from_numpy(imgs).permute(0, 3, 1, 2).contiguous(), output_hidden_states=True)
    r = R64.forward64(t, imgs, heads=2)
    N = 17 + registers
    assert r["trace"].shape == (3, 2, N, 128) and len(out.hidden_states) == 3 and tuple(out.hidden_states[0].shape) == (2, N, 128)
    for s in range(3):
        d = float(np.abs(r["trace"][s] - out.hidden_states[s].numpy()).max())
        print(f"R={registers} hidden state {s}: max|restatement - transformers| = {d:.3e}")
        assert d <= HF_TOL, (s, d)
    d = float(np.abs(r["logits"] - out.logits.numpy()).max())
    print(f"R={registers} logits: max|restatement - transformers| = {d:.3e}  (max|logit| {np.abs(r['logits']).max():.3f})")
    assert d <= HF_TOL, d


def test_layer_scale_fold_is_exact_and_mask_token_is_dropped(pkg, tmp_path):
    """File tensors == lambda (.) W and lambda (.) b bitwise at ftype 0 (the fold is one f32 multiplication per element, before the file type's rounding)."""
    torch, m = _hf_dinov2(4, seed=5)
    path = str(tmp_path / "fold.gguf")
    pkg.convert.convert_hf_model(m, path, ftype=0)
    t = PD.file_tensors(pkg, path)
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    assert not any("mask" in k for k in t)
    for i in range(2):
        q = f"dinov2_with_registers.encoder.layer.{i}."
        for lin, src, lam in (("attn.proj", "attention.output.dense", "layer_scale1.lambda1"), ("mlp.fc2", "mlp.fc2", "layer_scale2.lambda1")):
            l = sd[q + lam].astype(np.float32)
            assert not np.allclose(l, 1.0)
            assert np.array_equal(_bits(t[f"blocks.{i}.{lin}.weight"]), _bits(sd[q + src + ".weight"] * l[:, None]))
            assert np.array_equal(_bits(t[f"blocks.{i}.{lin}.bias"]), _bits(sd[q + src + ".bias"] * l))
    assert np.array_equal(_bits(t["reg_token"]), _bits(sd["dinov2_with_registers.embeddings.register_tokens"]))


def test_converter_refusals_and_no_head(pkg, tmp_path):
    torch, m = _hf_dinov2(4, seed=6)
    out = str(tmp_path / "x.gguf")
    m.config.use_swiglu_ffn = True
    with pytest.raises(ValueError, match="use_swiglu_ffn"):
        pkg.convert.convert_hf_model(m, out, ftype=0)
    m.config.use_swiglu_ffn = False
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    for key, what in (("dinov2_with_registers.encoder.layer.0.attention.attention.q_norm.weight", "qk-norm"), ("fc_norm.weight", "fc_norm"),
                      ("dinov2_with_registers.embeddings.dist_token", "distillation")):
        with pytest.raises(ValueError, match=what):
            pkg.convert.dinov2_state_dict_to_timm({**sd, key: np.ones(128, np.float32)}, m.config)
    # a backbone: one class of zeros labelled "(no head)", class-token head
    backbone = m.dinov2_with_registers
    hp = pkg.convert.convert_hf_model(backbone, out, ftype=1, no_head=True)
    mf = pkg.ggml_file.read_model(out)
    t = PD.file_tensors(pkg, out)
    assert hp.num_classes == 1 and mf.id2label == {0: "(no head)"} and t["head.weight"].shape == (1, 128) and not t["head.weight"].any() and not t["head.bias"].any()
    with pytest.raises(ValueError, match="no_head"):
        pkg.convert.convert_hf_model(backbone, out, ftype=1)


def _tensor_record(name, ttype, shape, data):
    import struct
    nb = name.encode()
    return struct.pack("<iii", len(shape), len(nb), ttype) + b"".join(struct.pack("<i", d) for d in reversed(shape)) + nb + data


def _with_tensors(pkg, path_in, path_out, replace):
    """path_in with the records named in `replace` {name: bytes of a whole record, or None to drop} swapped; other records byte for byte."""
    import struct
    mf = pkg.ggml_file.read_model(path_in)
    buf = open(path_in, "rb").read()
    first = buf.index(struct.pack("<iii", 3, len("cls_token"), 0))           # the first tensor record
    out = buf[:first]
    for t in mf.tensors:
        if t.name in replace:
            out += replace[t.name] or b""
        else:
            out += _tensor_record(t.name, t.ttype, tuple(reversed(t.ne)), t.raw)
    open(path_out, "wb").write(out)


def test_loader_accepts_the_extensions_and_rejects_malformed_ones(pkg, binding, tmp_path):
    L = binding.lib()
    good = pkg.synth.cached_synthetic(NAME, head_scale=4.0, registers=4, head_pool=1)
    m = binding.Model(good)
    assert (m.num_registers, m.head_pool) == (4, binding.POOL_CLS_MEAN)
    names = [n for n, *_ in m.tensors()]
    assert names[:3] == ["cls_token", "reg_token", "pos_embed"] and len(names) == 4 + 24 + 4 + 1
    info = {n: (ty, ne) for n, ty, ne, _ in m.tensors()}
    assert info["reg_token"] == (0, (128, 4, 1, 1)) and info["head.weight"][1][:2] == (256, 10) and info["pos_embed"][1][:2] == (128, 17)
    m.close()
    for reg, pool in ((4, 0), (0, 1)):
        mm = binding.Model(pkg.synth.cached_synthetic(NAME, head_scale=4.0, registers=reg, head_pool=pool))
        assert (mm.num_registers, mm.head_pool) == (reg, pool)
        mm.close()
    # files without the extensions report 0 / 0 and keep their bytes
    want = json.load(open(os.path.join(GOLD, "weights_sha1.json")))
    for key in ("vit_micro_patch16_64-h4", "vit_tiny_patch16_224-h4"):
        p = pkg.synth.cached_synthetic(key.rsplit("-", 1)[0], head_scale=4.0)
        assert hashlib.sha1(open(p, "rb").read()).hexdigest() == want[key]
        mm = binding.Model(p)
        assert (mm.num_registers, mm.head_pool) == (0, 0)
        mm.close()
    # malformed extensions: VITX_ERR_FORMAT
    reg = np.zeros((1, 4, 128), np.float32)
    bad = {
        "reg_token of 64 columns": {"reg_token": _tensor_record("reg_token", 0, (1, 4, 64), reg[:, :, :64].tobytes())},
        "reg_token in f16": {"reg_token": _tensor_record("reg_token", 1, (1, 4, 128), reg.astype(np.float16).tobytes())},
        "reg_token with two dims": {"reg_token": _tensor_record("reg_token", 0, (4, 128), reg.tobytes())},
        "reg_token with a leading 2": {"reg_token": _tensor_record("reg_token", 0, (2, 2, 128), reg.tobytes())},
        "reg_token twice": {"reg_token": 2 * _tensor_record("reg_token", 0, (1, 4, 128), reg.tobytes())},
        "head of 3 D columns": {"head.weight": _tensor_record("head.weight", 1, (10, 384), np.zeros((10, 384), np.float16).tobytes())},
    }
    for what, rep in bad.items():
        p = str(tmp_path / "bad.gguf")
        _with_tensors(pkg, good, p, rep)
        h = C.c_void_p()
        assert L.vitx_model_load(p.encode(), C.byref(h)) == ERR_FORMAT, what
    # the same rewrite with nothing replaced is the file itself (the helper is not what makes the loads above fail)
    p = str(tmp_path / "same.gguf")
    _with_tensors(pkg, good, p, {})
    assert open(p, "rb").read() == open(good, "rb").read()


def test_quantize_and_resize_carry_a_register_file_through(pkg, binding, tmp_path):
    src = pkg.synth.cached_synthetic(NAME, head_scale=4.0, registers=4, head_pool=1)
    t0 = PD.file_tensors(pkg, src)
    q8 = str(tmp_path / "q8.gguf")
    binding.quantize_file(src, q8, 8)
    mq = binding.Model(q8)
    assert (mq.num_registers, mq.head_pool) == (4, 1)
    info = {n: ty for n, ty, _ne, _ in mq.tensors()}
    assert info["reg_token"] == 0 and info["head.weight"] == 8 and info["blocks.0.attn.qkv.weight"] == 8 and info["pos_embed"] == 0
    mq.close()
    recs = {t.name: t for t in pkg.ggml_file.read_model(q8).tensors}
    recs0 = {t.name: t for t in pkg.ggml_file.read_model(src).tensors}
    assert recs["reg_token"].raw == recs0["reg_token"].raw and recs["pos_embed"].raw == recs0["pos_embed"].raw
    assert recs["head.weight"].raw == pkg.ggml_file.quantize_q8_0(t0["head.weight"])           # the [C][2 D] head like any 2-D *weight
    # the same file written quantised by the Python writer is the same bytes
    py = str(tmp_path / "q8_py.gguf")
    pkg.synth.write_synthetic(py, NAME, ftype=8, head_scale=4.0, registers=4, head_pool=1)
    assert open(py, "rb").read() == open(q8, "rb").read()
    for interp in (binding.POS_BICUBIC, binding.POS_BICUBIC_AA):
        big = str(tmp_path / "84.gguf")
        binding.resize_file(src, big, 84, interp)
        mb = binding.Model(big)
        assert (mb.img_size, mb.num_registers, mb.head_pool) == (84, 4, 1)
        mb.close()
        tb = PD.file_tensors(pkg, big)
        assert tb["pos_embed"].shape == (1, 37, 128)
        assert np.array_equal(_bits(tb["pos_embed"][0]), _bits(binding.pos_embed_resample(t0["pos_embed"][0], 6, interp)))
        for k in t0:
            if k != "pos_embed":
                assert np.array_equal(_bits(tb[k]), _bits(t0[k])), k


def test_timm_state_dict_with_registers_layer_scale_and_no_embed_class(pkg, tmp_path):
    """A hand-made timm state dict of the reg4 DINOv2 layout (reg_token, ls1 / ls2 gamma, a pos_embed of g^2 rows) converts to the same tensors
    as the equivalent HF model; the zero row in front of pos_embed is exact because the class token gets no position term there."""
    torch, m = _hf_dinov2(4, seed=21)
    e = "dinov2_with_registers.embeddings."
    with torch.no_grad():
        m.state_dict()[e + "position_embeddings"][:, 0].zero_()
    hf = str(tmp_path / "hf.gguf"); tm = str(tmp_path / "timm.gguf")
    pkg.convert.convert_hf_model(m, hf, ftype=1)
    sd = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    t = {"cls_token": sd[e + "cls_token"], "reg_token": sd[e + "register_tokens"], "pos_embed": sd[e + "position_embeddings"][:, 1:],
         "patch_embed.proj.weight": sd[e + "patch_embeddings.projection.weight"], "patch_embed.proj.bias": sd[e + "patch_embeddings.projection.bias"]}
    for i in range(2):
        q, p = f"dinov2_with_registers.encoder.layer.{i}.", f"blocks.{i}."
        a = q + "attention.attention."
        t[p + "norm1.weight"] = sd[q + "norm1.weight"]; t[p + "norm1.bias"] = sd[q + "norm1.bias"]
        t[p + "attn.qkv.weight"] = np.concatenate([sd[a + n + ".weight"] for n in ("query", "key", "value")])
        t[p + "attn.qkv.bias"] = np.concatenate([sd[a + n + ".bias"] for n in ("query", "key", "value")])
        t[p + "attn.proj.weight"] = sd[q + "attention.output.dense.weight"]; t[p + "attn.proj.bias"] = sd[q + "attention.output.dense.bias"]
        t[p + "ls1.gamma"] = sd[q + "layer_scale1.lambda1"]
        t[p + "norm2.weight"] = sd[q + "norm2.weight"]; t[p + "norm2.bias"] = sd[q + "norm2.bias"]
        t[p + "mlp.fc1.weight"] = sd[q + "mlp.fc1.weight"]; t[p + "mlp.fc1.bias"] = sd[q + "mlp.fc1.bias"]
        t[p + "mlp.fc2.weight"] = sd[q + "mlp.fc2.weight"]; t[p + "mlp.fc2.bias"] = sd[q + "mlp.fc2.bias"]
        t[p + "ls2.gamma"] = sd[q + "layer_scale2.lambda1"]
    t["norm.weight"] = sd["dinov2_with_registers.layernorm.weight"]; t["norm.bias"] = sd["dinov2_with_registers.layernorm.bias"]
    t["head.weight"] = sd["classifier.weight"]; t["head.bias"] = sd["classifier.bias"]
    assert t["pos_embed"].shape == (1, 16, 128)
    hp = pkg.convert.convert_timm_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in t.items()}, tm, ftype=1, heads=2)
    assert (hp.img_size, hp.patch_size, hp.num_classes) == (56, 14, 10)
    a, b = pkg.ggml_file.read_model(hf), pkg.ggml_file.read_model(tm)
    assert [x.name for x in a.tensors] == [x.name for x in b.tensors]
    for x, y in zip(a.tensors, b.tensors):
        assert (x.ttype, x.ne, x.raw) == (y.ttype, y.ne, y.raw), x.name
    # other unsupported timm components stay refused, by name
    for key, what in (("fc_norm.weight", "fc_norm"), ("dist_token", "distillation"), ("blocks.0.attn.q_norm.weight", "qk-norm")):
        with pytest.raises(ValueError, match=what):
            pkg.convert.convert_timm_state_dict({**t, key: np.ones(128, np.float32)}, tm, heads=2)


# The gates the GPU tests apply to the three quantities (tests/test_gpu_registers.py), evaluated on the restatement:
def gpu_gates(pkg, t, r, T):
    x0 = r["trace"][0]
    stage0 = 2e-5 * max(1.0, float(np.abs(x0).max()))                                  # tests/test_gpu_parity_r02.py:266
    y64, bound = FD.features64(r["trace"][-1].astype(np.float32), t["norm.weight"], t["norm.bias"], PD.EPS)
    mean = bound[:, T:].mean(axis=1) + FD.U24 * ((y64.shape[1] - T) * np.abs(y64[:, T:]).mean(axis=1) + 2 * np.abs(y64[:, T:].mean(axis=1)))      # tests/test_gpu_features.py:232-235
    z = np.concatenate([r["final"][:, 0], r["mean"]], 1)
    logits = (np.abs(z) @ np.abs(t["head.weight"].astype(np.float64)).T) * 2e-6 + 1e-6   # tests/test_gpu_parity_r02.py:60 (head-GEMM noise)
    return stage0, float(mean.max()), float(logits.max())


def test_each_layout_mistake_moves_its_quantity_by_100_gates(pkg):
    """The GPU tests compare trace stage 0, the mean feature and the logits with the restatement.  Each of the four mistakes a prefix-token
    implementation can make must move the quantity that test compares by at least 100 x the gate applied to it -- on the very file and
    images the GPU tests use: otherwise a GPU test could pass on a wrong layout."""
    t = PD.file_tensors(pkg, pkg.synth.cached_synthetic(NAME, head_scale=4.0, registers=4, head_pool=1))
    imgs = PD.exact_images(3, 56, seed=1)
    good = R64.forward64(t, imgs, heads=2)
    g0, gm, gl = gpu_gates(pkg, t, good, 5)
    moved = {}
    for mut in PD.MUTANTS:
        bad = R64.forward64(t, imgs, heads=2, mutant=mut)
        moved[mut] = (float(np.abs(bad["trace"][0] - good["trace"][0]).max()), float(np.abs(bad["mean"] - good["mean"]).max()),
                      float(np.abs(bad["logits"] - good["logits"]).max()))
        print(f"{mut}: stage 0 moves {moved[mut][0]:.3e} (gate {g0:.1e}), mean {moved[mut][1]:.3e} (gate {gm:.1e}), logits {moved[mut][2]:.3e} (gate {gl:.1e})")
    for mut in ("pos_on_registers", "patch_pos_shifted"):
        assert moved[mut][0] >= 100 * g0, (mut, moved[mut], g0)
    for mut in ("registers_in_mean", "mean_over_n_minus_1"):
        assert moved[mut][0] == 0.0
        assert moved[mut][1] >= 100 * gm, (mut, moved[mut], gm)
        assert moved[mut][2] >= 100 * gl, (mut, moved[mut], gl)
