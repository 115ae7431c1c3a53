"""The converter's output, byte for byte (no GPU): every case below writes one model file with vit.cpp_amd/convert.py, and the file's sha1 is the
one recorded in tests/golden/convert_sha1.json.  The record is made by tests/golden/make_convert_golden.py, which imports CASES from here, on a
commit whose converter is known good -- the JSON names it -- and never on the code under test.

Between them the cases cover every model family, every head kind, a file with and without `arch`, the place of `preproc`, f32, f16 and block-quantised
payloads, and every placement the timm path makes.  The models are the micro configuration of tests/test_cpu_arch.py with every parameter drawn
by its _redraw(seed 21): the bytes depend on numpy's generator alone."""
import hashlib
import json
import os

import numpy as np
import pytest

import map_data as MD
from test_cpu_arch import KW, _hf_model, _redraw
from test_cpu_map_head import _siglip
from test_cpu_preproc import PROCESSORS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convert_sha1.json")
SEED = 21
MICRO = "vit_micro_patch16_64"


def _dinov2_registers():
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    cfg = tr.Dinov2WithRegistersConfig(num_labels=10, num_register_tokens=4, hidden_act="gelu", layer_norm_eps=1e-6, **KW)
    return _redraw(torch, tr.Dinov2WithRegistersForImageClassification(cfg).eval(), SEED)


def _clip_tower():
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    cfg = tr.CLIPVisionConfig(intermediate_size=512, projection_dim=24, hidden_act="quick_gelu", layer_norm_eps=1e-5, **KW)
    return _redraw(torch, tr.CLIPVisionModel(cfg).eval(), SEED)


def _vitstr():
    """The one-channel ViT of tests/test_cpu_vitstr.py (test_vitstr_graph_vs_transformers_f32_and_converter)."""
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    cfg = tr.ViTConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, hidden_act="gelu_pytorch_tanh",
                       layer_norm_eps=1e-6, image_size=96, patch_size=16, num_channels=1, num_labels=96, hidden_dropout_prob=0.0,
                       attention_probs_dropout_prob=0.0, qkv_bias=True)
    return _redraw(torch, tr.ViTForImageClassification(cfg).eval(), SEED)


HF_MODELS = {
    "vit": lambda: _hf_model("vit", SEED)[1],
    "dinov2": lambda: _hf_model("dinov2", SEED)[1],
    "dinov2_reg4": _dinov2_registers,
    "dinov2_backbone": lambda: _hf_model("dinov2", SEED)[1].dinov2,
    "clip": lambda: _hf_model("clip", SEED)[1],
    "clip_tower": _clip_tower,
    "siglip": lambda: _siglip(SEED)[1],
    "vitstr": _vitstr,
}
_models = {}


def _model(name):
    """Each model is built once per process: no case changes it."""
    if name not in _models:
        _models[name] = HF_MODELS[name]()
    return _models[name]


def _hf(name, ftype, **kw):
    return lambda pkg, path: pkg.convert.convert_hf_model(_model(name), path, ftype=ftype, **kw)


def _timm_registers_dict():
    """The reg4 DINOv2 layout of timm as tests/test_cpu_registers.py builds it (test_timm_state_dict_with_registers_layer_scale_and_no_embed_class):
    reg_token, ls1 / ls2 gamma in every block, a pos_embed of g^2 rows."""
    sd = {k: v.detach().numpy().copy() for k, v in _model("dinov2_reg4").state_dict().items()}
    e = "dinov2_with_registers.embeddings."
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
    return t


def _micro(pkg, name=MICRO, **kw):
    return dict(pkg.synth.make_weights(pkg.synth.hparams_for(name), **kw))


def _map(pkg, head):
    t = dict(MD.fixture_tensors(pkg)[1])
    if not head:           # a num_classes 0 checkpoint: the converter supplies the one-class head of zeros
        del t["head.weight"], t["head.bias"]
    return t


def _timm(make, **kw):
    return lambda pkg, path: pkg.convert.convert_timm_state_dict(make(pkg), path, ftype=1, heads=2, **kw)


CASES = {}
for _ft in (0, 1, 2):
    CASES[f"hf_vit_ft{_ft}"] = _hf("vit", _ft)
    CASES[f"hf_dinov2_ft{_ft}"] = _hf("dinov2", _ft)
    CASES[f"hf_dinov2_reg4_ft{_ft}"] = _hf("dinov2_reg4", _ft)
    CASES[f"hf_dinov2_backbone_no_head_ft{_ft}"] = _hf("dinov2_backbone", _ft, no_head=True)
    CASES[f"hf_clip_ft{_ft}"] = _hf("clip", _ft)
    CASES[f"hf_clip_tower_no_head_ft{_ft}"] = _hf("clip_tower", _ft, no_head=True)
    CASES[f"hf_siglip_ft{_ft}"] = _hf("siglip", _ft)
for _kind in ("vit", "dinov2", "clip"):
    CASES[f"hf_{_kind}_preproc_ft1"] = _hf(_kind, 1, preprocessor_config=PROCESSORS[_kind])
CASES["hf_vitstr_ft1"] = _hf("vitstr", 1, vitstr=True)
CASES["timm_micro_ft1"] = _timm(_micro)
CASES["timm_micro_erf_ft1"] = _timm(_micro, act="erf")
CASES["timm_reg4_layer_scale_no_embed_class_ft1"] = _timm(lambda pkg: _timm_registers_dict())
CASES["timm_map_head_ft1"] = _timm(lambda pkg: _map(pkg, True))
CASES["timm_map_no_head_ft1"] = _timm(lambda pkg: _map(pkg, False))
CASES["timm_vitstr_ft1"] = _timm(lambda pkg: _micro(pkg, "vitstr_micro_patch16_64", in_chans=1))
CASES["timm_micro_preproc_ft1"] = _timm(_micro, preproc=dict(resize=73, crop_round="torchvision"))


def sha1_of(pkg, name, path):
    CASES[name](pkg, path)
    with open(path, "rb") as f:
        return hashlib.sha1(f.read()).hexdigest()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_record_holds_exactly_these_cases(recorded):
    assert sorted(recorded["sha1"]) == sorted(CASES) and len(recorded["commit"]) == 40


@pytest.mark.parametrize("name", list(CASES))
def test_converted_file_keeps_its_bytes(pkg, tmp_path, recorded, name):
    assert sha1_of(pkg, name, str(tmp_path / "out.gguf")) == recorded["sha1"][name]
