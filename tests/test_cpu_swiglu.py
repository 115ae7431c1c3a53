"""The gated (SwiGLU) MLP without a GPU (include/vitx.h "gated MLP"): the loader's rules for the `glu` tensor, the file tools, the converter's opt-in
path and the float64 restatement of tests/ref64.py against transformers' Dinov2Model (use_swiglu_ffn) and DINOv3ViTModel (use_gated_mlp), the
separation of the micro fixtures' mutants from operand rounding, and the share of the kernel test's exact grid at which each mutant shows."""
import ctypes as C
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import arch_data as AD
import map_data as MD
import prefix_data as PD
import ref64 as R64
import rope_data as RD
import swiglu_data as SD
import text_data as TD
from test_cpu_rope import _hf_dinov3
from ref64 import PROB_TOL, stage_errors, stage_ok
from test_gpu_arch import ROUND, _apart

ERR_FORMAT = 2
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# The transformers fixtures draw their Linear weights at 0.02 and _hf_dinov3 its biases at 0.02: the gate arguments stay within a few tenths, where
# silu(g) u and silu(u) g nearly coincide, and the up bias moves nothing.  As tests/test_cpu_rope.py does with QK_FACTOR, the MLP is scaled: the fc1
# weights (weights_in / gate_proj, up_proj) by MLP_FACTOR[0], the fc1 biases by [1], the fc2 weight (weights_out / down_proj) by [2].  Measured with
# these factors (max|d| against transformers' last hidden state, features of magnitude 3.9 .. 4.6): the restatement agrees to 5.8e-6 .. 7.7e-6; the
# nearest mutant is gelu_gate at 0.50 (Dinov2) / 0.54 / 0.70 (DINOv3 with / without biases), up_bias_dropped lies at 1.7 / 1.9, every other beyond 3.
MLP_FACTOR = (8.0, 25.0, 4.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _record(name, ttype, shape, data):
    nb = name.encode()
    return struct.pack("<iii", len(shape), len(nb), ttype) + b"".join(struct.pack("<i", d) for d in reversed(shape)) + nb + data


def _glu(*vals):
    return _record("glu", 0, (len(vals),), np.array(vals, np.float32).tobytes())


# ------------------------------------------------------------------------------------------------ the loader
def _load(binding, tmp_path, data):
    L = binding.lib()
    p = str(tmp_path / "x.gguf")
    open(p, "wb").write(data)
    h = C.c_void_p()
    rc = L.vitx_model_load(p.encode(), C.byref(h))
    out = None
    if rc == 0:
        k, w = C.c_int(-1), C.c_int(-1)
        has = L.vitx_model_glu(h, C.byref(k), C.byref(w))
        out = (has, k.value, w.value, L.vitx_model_num_tensors(h))
        assert L.vitx_model_glu(h, None, None) == has
        L.vitx_model_free(h)
    return rc, out, L.vitx_last_error().decode()


def _first_block(data):
    return data.index(struct.pack("<iii", 1, len("blocks.0.norm1.weight"), 0) + struct.pack("<i", 128) + b"blocks.0.norm1.weight")


@pytest.mark.parametrize("kind", SD.FIXTURES)
def test_fixtures_load_and_say_their_width(pkg, binding, kind):
    path = SD.fixture_file(pkg, kind)
    names = [t.name for t in pkg.ggml_file.read_model(path).tensors]
    assert names[:names.index("cls_token")] == (["arch", "rope", "glu"] if kind == "hplus" else ["arch", "glu"])
    m = binding.Model(path)
    assert m.glu == (1, SD.F) == (1, 320)
    assert (m.rope is not None) == (kind == "hplus") and m.num_registers == (4 if kind == "hplus" else 0)
    m.close()
    t = PD.file_tensors(pkg, path)
    assert SD.glu_of(t) == 320
    for i in range(2):
        assert t[f"blocks.{i}.mlp.fc1.weight"].shape == (640, 128) and t[f"blocks.{i}.mlp.fc1.bias"].shape == (640,) and t[f"blocks.{i}.mlp.fc2.weight"].shape == (128, 320)


def test_loader_rules_for_the_glu_tensor(pkg, binding, tmp_path):
    L = binding.lib()
    assert L.vitx_model_glu(None, None, None) == 0
    # a file without `glu`: the getter says 0 and touches nothing; its bytes are what they were (synth.make_weights draws nothing new without glu=)
    plain = pkg.synth.cached_synthetic(AD.MICRO, head_scale=4.0)
    base = open(plain, "rb").read()
    assert _load(binding, tmp_path, base)[:2] == (0, (0, -1, -1, 32))
    want = json.load(open(os.path.join(GOLD, "weights_sha1.json")))
    micro = pkg.synth.cached_synthetic("vit_micro_patch16_64", head_scale=4.0)
    assert hashlib.sha1(open(micro, "rb").read()).hexdigest() == want["vit_micro_patch16_64-h4"]
    # the plain file with a `glu` record: its 4 D-wide MLP tensors no longer have the shapes the record asks for
    first = base.index(struct.pack("<iii", 3, len("cls_token"), 0))
    rc, _, msg = _load(binding, tmp_path, base[:first] + _glu(1, 320, 0, 0) + base[first:])
    assert rc == ERR_FORMAT and "mlp.fc1" in msg, msg
    # the fixture: `glu` where the converter writes it, directly in front of the first block, or at the very front
    good = open(SD.fixture_file(pkg, "g"), "rb").read()
    assert _load(binding, tmp_path, good)[:2] == (0, (1, 1, 320, 34))
    rec = _glu(1, 320, 0, 0)
    at = good.index(rec)
    bare = good[:at] + good[at + len(rec):]
    fb, front = _first_block(bare), bare.index(struct.pack("<iii", 1, len("arch"), 0))
    assert _load(binding, tmp_path, bare[:fb] + rec + bare[fb:])[:2] == (0, (1, 1, 320, 34))
    assert _load(binding, tmp_path, bare[:front] + rec + bare[front:])[:2] == (0, (1, 1, 320, 34))
    # without the record the 2 F-row tensors are the wrong shape for a plain file
    rc, _, msg = _load(binding, tmp_path, bare)
    assert rc == ERR_FORMAT and "mlp.fc1" in msg, msg
    bad = {
        "kind 0": _glu(0, 320, 0, 0), "kind 2": _glu(2, 320, 0, 0), "kind 1.5": _glu(1.5, 320, 0, 0), "kind nan": _glu(np.nan, 320, 0, 0),
        "F 0": _glu(1, 0, 0, 0), "F 32": _glu(1, 32, 0, 0), "F negative": _glu(1, -320, 0, 0), "F 320.5": _glu(1, 320.5, 0, 0), "F nan": _glu(1, np.nan, 0, 0),
        "F inf": _glu(1, np.inf, 0, 0), "F 328 (no multiple of 64)": _glu(1, 328, 0, 0), "F 352 (a multiple of 32 only)": _glu(1, 352, 0, 0),
        "reserved slot 2": _glu(1, 320, 1, 0), "reserved slot 3": _glu(1, 320, 0, 1e-30),
        "glu of 3": _glu(1, 320, 0), "glu of 5": _glu(1, 320, 0, 0, 0), "glu in f16": _record("glu", 1, (4,), np.array([1, 320, 0, 0], np.float16).tobytes()),
        "glu with two dims": _record("glu", 0, (1, 4), np.array([1, 320, 0, 0], np.float32).tobytes()),
        "glu twice": rec + rec,
    }
    for what, r in bad.items():
        rc, _, msg = _load(binding, tmp_path, bare[:fb] + r + bare[fb:])
        assert rc == ERR_FORMAT and msg.startswith("vitx_model_load:") and "glu" in msg, (what, rc, msg)
    # behind a block record: after the first one, and after the last one in front of blocks.0.mlp.fc1.weight (the first record `glu` resizes)
    second = bare.index(b"blocks.0.norm1.bias") - 16
    fc1 = bare.index(b"blocks.0.mlp.fc1.weight") - 20
    for where in (second, fc1):
        rc, _, msg = _load(binding, tmp_path, bare[:where] + rec + bare[where:])
        assert rc == ERR_FORMAT and "glu" in msg and "behind a blocks.* record" in msg, (where, msg)
    # ... and anywhere later the records in front of it already have the wrong shapes for a file without `glu`
    for where in (bare.index(b"blocks.1.norm1.weight") - 16, len(bare)):
        rc, _, msg = _load(binding, tmp_path, bare[:where] + rec + bare[where:])
        assert rc == ERR_FORMAT and "blocks.0.mlp.fc1.weight" in msg, (where, msg)
    # a text-tower file
    text = open(TD.text_file(pkg, "siglip"), "rb").read()
    assert _load(binding, tmp_path, text)[0] == 0
    tb = text.index(b"blocks.0.norm1.weight") - 16
    rc, _, msg = _load(binding, tmp_path, text[:tb] + _glu(1, 320, 0, 0) + text[tb:])
    assert rc == ERR_FORMAT and "glu" in msg and "text" in msg, msg
    # together with the attention-pooling head: a pooled file whose blocks carry the gated shapes
    hp, t = MD.fixture_tensors(pkg)
    assert _load(binding, tmp_path, open(MD.fixture_file(pkg), "rb").read())[0] == 0
    D = hp.hidden_size
    rng = np.random.default_rng(3)
    gt = {}
    for k, v in t.items():
        if k == "pos_embed":
            gt["glu"] = np.array([1, 320, 0, 0], np.float32)
        if k.startswith("blocks.") and k.endswith("mlp.fc1.weight"):
            v = (rng.standard_normal((640, D)) * 0.02).astype(np.float32)
        elif k.startswith("blocks.") and k.endswith("mlp.fc1.bias"):
            v = np.zeros(640, np.float32)
        elif k.startswith("blocks.") and k.endswith("mlp.fc2.weight"):
            v = (rng.standard_normal((D, 320)) * 0.02).astype(np.float32)
        gt[k] = v
    pg = str(tmp_path / "pool_glu.gguf")
    pkg.ggml_file.write_model(pg, hp, gt)
    rc, _, msg = _load(binding, tmp_path, open(pg, "rb").read())
    assert rc == ERR_FORMAT and "glu" in msg and "attn_pool" in msg, msg


@pytest.mark.parametrize("kind", SD.FIXTURES)
def test_quantize_and_resize_carry_glu_through(pkg, binding, tmp_path, kind):
    src = SD.fixture_file(pkg, kind)
    recs0 = {t.name: t for t in pkg.ggml_file.read_model(src).tensors}
    q8, q4, big = str(tmp_path / "q8.gguf"), str(tmp_path / "q4.gguf"), str(tmp_path / "84.gguf")
    binding.quantize_file(src, q8, 8)
    binding.quantize_file(src, q4, 2)
    binding.resize_file(src, big, 84, binding.POS_BICUBIC)
    for path, img in ((q8, 56), (q4, 56), (big, 84)):
        m = binding.Model(path)
        assert m.glu == (1, SD.F) and m.img_size == img
        m.close()
        recs = {t.name: t for t in pkg.ggml_file.read_model(path).tensors}
        assert list(recs) == list(recs0)
        for k in ("arch", "glu"):
            assert (recs[k].ttype, recs[k].ne, recs[k].raw) == (recs0[k].ttype, recs0[k].ne, recs0[k].raw), (path, k)
    for path, ft in ((q8, 8), (q4, 2)):                                # fc1 and fc2 quantise like any matrix
        types = {t.name: (t.ttype, t.ne) for t in pkg.ggml_file.read_model(path).tensors}
        assert types["blocks.0.mlp.fc1.weight"] == (ft, (128, 640)) and types["blocks.1.mlp.fc2.weight"] == (ft, (320, 128))
        assert types["blocks.0.mlp.fc1.bias"] == (0, (640,))


def test_synth_counts_the_gated_mlp(pkg):
    hp = pkg.synth.hparams_for(AD.MICRO)
    plain = pkg.synth.gflop_per_image(hp)
    assert pkg.synth.gflop_per_image(hp, glu=0) == plain
    N, D = 17, 128
    assert abs((pkg.synth.gflop_per_image(hp, glu=320) - plain) * 1e9 - 2.0 * 2 * (3 * N * D * 320 - 8 * N * D * D)) < 1.0
    w0, w1 = pkg.synth.make_weights(hp), pkg.synth.make_weights(hp, glu=0)
    assert list(w0) == list(w1) and all(np.array_equal(_bits(w0[k]), _bits(w1[k])) for k in w0) and "glu" not in w0
    wg = pkg.synth.make_weights(hp, glu=320)
    assert list(wg)[0] == "glu" and wg["blocks.1.mlp.fc1.weight"].shape == (640, 128) and wg["blocks.1.mlp.fc2.weight"].shape == (128, 320)
    with pytest.raises(ValueError, match="glu"):
        pkg.ggml_file.write_model(os.devnull, hp, {**w0, "glu": np.array([1, 320, 0, 0], np.float32)})
    with pytest.raises(ValueError, match="multiple of 64"):
        pkg.ggml_file.write_model(os.devnull, hp, pkg.synth.make_weights(hp, glu=328))


# ------------------------------------------------------------------------------------------------ the converter and the restatement
def _scale_mlp(torch, m, factor=MLP_FACTOR):
    with torch.no_grad():
        for k, p in m.named_parameters():
            if ".mlp." not in k:
                continue
            fc2 = "weights_out" in k or "down_proj" in k
            if k.endswith(".weight"):
                p.mul_(factor[2] if fc2 else factor[0])
            elif not fc2:
                p.mul_(factor[1])


def _hf_dinov2_giant(seed=41):
    """A tiny Dinov2Model with the SwiGLU MLP: D 192, 3 heads of 64, mlp_ratio 4 -- HuggingFace's rounding (int(768 * 2 / 3) up to a multiple of 8)
    gives F = 512 --, lambda1 and the biases re-drawn, the MLP scaled by MLP_FACTOR, the patch kernel fp16-exact."""
    import torch
    import transformers
    torch.manual_seed(seed)
    cfg = transformers.Dinov2Config(hidden_size=192, num_hidden_layers=2, num_attention_heads=3, mlp_ratio=4, patch_size=14, image_size=56, use_swiglu_ffn=True,
                                    hidden_act="gelu", layer_norm_eps=1e-6)
    m = transformers.Dinov2Model(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("lambda1"):
                p.copy_(torch.rand(p.shape, generator=g) * 1.5 + 0.25)
            elif k.endswith("position_embeddings") or k.endswith("cls_token"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif k.endswith("patch_embeddings.projection.weight"):
                p.copy_(p.half().float())
            elif k.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    _scale_mlp(torch, m)
    return torch, m


def _hf_dinov3_hplus(mlp_bias=True, **over):
    """tests/test_cpu_rope.py's DINOv3ViTModel with use_gated_mlp, intermediate_size 320 and the silu gate, the MLP scaled by MLP_FACTOR."""
    torch, m = _hf_dinov3(use_gated_mlp=True, intermediate_size=320, hidden_act="silu", mlp_bias=mlp_bias, **over)
    _scale_mlp(torch, m)
    return torch, m


def _against_transformers(pkg, binding, tmp_path, torch, m, heads, what, mutants):
    path = str(tmp_path / "gated.gguf")
    hp = pkg.convert.convert_hf_model(m, path, ftype=0, no_head=True, gated_mlp=True)
    t = PD.file_tensors(pkg, path)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(2, 56, seed=3))
    with torch.no_grad():
        out = m(pixel_values=torch.from_numpy(imgs).permute(0, 3, 1, 2).contiguous())
    want = out.last_hidden_state.numpy()
    r = R64.forward64(t, imgs, heads=heads)
    assert r["final"].shape == want.shape
    d = float(np.abs(r["final"] - want).max())
    print(f"{what}: max|restatement - transformers| = {d:.3e} on features of magnitude {np.abs(want).max():.2f}")
    assert d <= 1e-4, d                                                  # tests/test_cpu_rope.py's bound for the same comparison
    assert np.abs(r["final"][:, 0] - out.pooler_output.numpy()).max() <= 1e-4
    for mut in mutants:
        dm = float(np.abs(R64.forward64(t, imgs, heads=heads, mutant=mut)["final"] - want).max())
        print(f"{what}: mutant {mut}: max|d| = {dm:.3f}")
        assert dm > 0.1, (mut, dm)
    mdl = binding.Model(path)
    glu = mdl.glu
    mdl.close()
    return hp, t, glu


def test_dinov2_giant_converter_and_restatement_against_transformers(pkg, binding, tmp_path):
    torch, m = _hf_dinov2_giant()
    hp, t, glu = _against_transformers(pkg, binding, tmp_path, torch, m, 3, "Dinov2Model use_swiglu_ffn", SD.MUTANTS)
    assert (hp.hidden_size, hp.num_hidden_layers, hp.num_attention_heads, hp.num_classes, hp.patch_size, hp.img_size) == (192, 2, 3, 1, 14, 56)
    assert glu == (1, 512) and list(t)[:3] == ["arch", "glu", "cls_token"]
    assert np.array_equal(_bits(t["arch"]), _bits(np.array([AD.ACT_ERF, 1e-6, 0, 0], np.float32)))      # hidden_act is carried, not applied
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    for i in range(2):
        q = f"encoder.layer.{i}."
        lam = sd[q + "layer_scale2.lambda1"].astype(np.float32)
        assert t[f"blocks.{i}.mlp.fc1.weight"].shape == (1024, 192) and t[f"blocks.{i}.mlp.fc2.weight"].shape == (192, 512)
        assert np.array_equal(_bits(t[f"blocks.{i}.mlp.fc1.weight"]), _bits(sd[q + "mlp.weights_in.weight"]))
        assert np.array_equal(_bits(t[f"blocks.{i}.mlp.fc1.bias"]), _bits(sd[q + "mlp.weights_in.bias"]))
        assert np.array_equal(_bits(t[f"blocks.{i}.mlp.fc2.weight"]), _bits(sd[q + "mlp.weights_out.weight"] * lam[:, None]))
        assert np.array_equal(_bits(t[f"blocks.{i}.mlp.fc2.bias"]), _bits(sd[q + "mlp.weights_out.bias"] * lam))


@pytest.mark.parametrize("mlp_bias", [True, False])
def test_dinov3_hplus_converter_and_restatement_against_transformers(pkg, binding, tmp_path, mlp_bias):
    torch, m = _hf_dinov3_hplus(mlp_bias)
    mutants = SD.MUTANTS if mlp_bias else SD.OP_MUTANTS                 # without biases there is no up bias to drop
    hp, t, glu = _against_transformers(pkg, binding, tmp_path, torch, m, 2, f"DINOv3ViTModel use_gated_mlp, mlp_bias {mlp_bias}", mutants)
    assert (hp.hidden_size, hp.num_hidden_layers, hp.num_attention_heads, hp.num_classes, hp.patch_size, hp.img_size) == (128, 2, 2, 1, 14, 56)
    assert glu == (1, 320) and list(t)[:5] == ["arch", "rope", "glu", "cls_token", "reg_token"]
    assert np.array_equal(_bits(t["arch"]), _bits(np.array([AD.ACT_TANH, 1e-5, 0, 0], np.float32)))     # silu is the gate, not a slot of `arch`
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    pre = "model." if "model.layer.0.mlp.gate_proj.weight" in sd else ""
    for i in range(2):
        q = f"{pre}layer.{i}.mlp."
        w1 = t[f"blocks.{i}.mlp.fc1.weight"]
        assert w1.shape == (640, 128) and np.array_equal(_bits(w1[:320]), _bits(sd[q + "gate_proj.weight"])) and np.array_equal(_bits(w1[320:]), _bits(sd[q + "up_proj.weight"]))
        b1 = t[f"blocks.{i}.mlp.fc1.bias"]
        if mlp_bias:
            assert np.array_equal(_bits(b1[:320]), _bits(sd[q + "gate_proj.bias"])) and np.array_equal(_bits(b1[320:]), _bits(sd[q + "up_proj.bias"]))
        else:
            assert q + "gate_proj.bias" not in sd and not b1.any() and not t[f"blocks.{i}.mlp.fc2.bias"].any()


def test_default_refusals_and_the_switch(pkg, tmp_path):
    out = str(tmp_path / "x.gguf")
    _, giant = _hf_dinov2_giant()
    with pytest.raises(ValueError, match="use_swiglu_ffn") as ei:
        pkg.convert.convert_hf_model(giant, out, no_head=True)
    assert "gated_mlp=True" in str(ei.value) and "--gated-mlp" in str(ei.value) and "reference" in str(ei.value)
    _, hplus = _hf_dinov3_hplus()
    with pytest.raises(ValueError, match="use_gated_mlp") as ei:
        pkg.convert.convert_hf_model(hplus, out)
    assert "gated_mlp=True" in str(ei.value) and "--gated-mlp" in str(ei.value) and "reference" in str(ei.value)
    # the switch on a model without a gated MLP, a gate that is not silu, a width that is no multiple of 64, and a plain MLP that is not 4 x hidden
    _, plain = _hf_dinov3()
    with pytest.raises(ValueError, match="gated_mlp"):
        pkg.convert.convert_hf_model(plain, out, gated_mlp=True)
    _, gelu = _hf_dinov3(use_gated_mlp=True, intermediate_size=320, hidden_act="gelu")
    with pytest.raises(ValueError, match="silu"):
        pkg.convert.convert_hf_model(gelu, out, gated_mlp=True)
    _, odd = _hf_dinov3(use_gated_mlp=True, intermediate_size=328, hidden_act="silu")
    with pytest.raises(ValueError, match="multiples of 64"):
        pkg.convert.convert_hf_model(odd, out, gated_mlp=True)
    _, narrow = _hf_dinov3(intermediate_size=384)
    with pytest.raises(ValueError, match="4 x hidden"):
        pkg.convert.convert_hf_model(narrow, out)
    assert not os.path.exists(out)


# ------------------------------------------------------------------------------------------------ the micro fixtures
@pytest.mark.parametrize("kind", SD.FIXTURES)
def test_fixtures_separate_the_mutants_from_operand_rounding(pkg, kind):
    """Computed, not assumed (swiglu_data.GLU_SCALE): on each micro fixture and the images of the GPU tests, the operand-rounded restatement lies
    inside HALF of tests/ref64.py's stage and probability gates of the unrounded one, and every mutant lies more than TWICE a gate from the
    real thing -- so a GPU result inside the gates of the restatement is outside those of every mutant."""
    imgs = PD.exact_images(17, 56, seed=1)
    t = PD.file_tensors(pkg, SD.fixture_file(pkg, kind))
    assert SD.glu_of(t) == SD.F and (RD.rope_of(t) is not None) == (kind == "hplus")
    exact = R64.forward64(t, imgs, SD.HEADS)
    for dtype in (0, 1):
        ref = R64.forward64(t, imgs, SD.HEADS, wround=ROUND[dtype], uround=ROUND[dtype])
        se = stage_errors(ref["trace"], exact["trace"])
        dp = float(np.abs(ref["probs"] - exact["probs"]).max())
        print(f"{kind} dtype {dtype}: rounded against unrounded: stages (e_max, e_rms) {[(round(a, 5), round(b, 5)) for a, b in se]}, max|dprob| {dp:.2e}")
        assert all(stage_ok(a, b, dtype, 0.5) for a, b in se) and dp <= 0.5 * PROB_TOL[dtype]
        for mut in SD.MUTANTS:
            m = R64.forward64(t, imgs, SD.HEADS, mutant=mut, wround=ROUND[dtype], uround=ROUND[dtype])
            sm = stage_errors(m["trace"], ref["trace"])
            dm = float(np.abs(ref["probs"] - m["probs"]).max())
            print(f"{kind} dtype {dtype}: mutant {mut}: stages {[(round(a, 4), round(b, 4)) for a, b in sm]}, max|dprob| {dm:.3f}")
            assert _apart(ref, m, dtype), (kind, dtype, mut)


# ------------------------------------------------------------------------------------------------ the exact grid of the kernel test
# Share of the grid's points (g = k / 64 in [-8, 8), u cycling through swiglu_data.U_VALUES) where the mutant lies more than 2 act_tol from the truth,
# computed by swiglu_data.separated_share; (fp16, bf16) floors of the measured shares.
# Measured 99.7 / 98.99 %, 99.9 / 99.9 %, 91.7 / 76.8 %, 83.3 / 83.3 % (no_up: u = 1 in one column of six), 100 / 99.9 %; the floors are those
# shares cut off after two digits.
GRID_SHARE = {"gate_up_swapped": (0.99, 0.98), "gate_is_sigmoid": (0.99, 0.99), "gelu_gate": (0.91, 0.76), "no_up": (0.83, 0.83), "halves_interleaved": (0.99, 0.99)}


@pytest.mark.parametrize("dtype", [0, 1])
def test_every_mutant_shows_on_the_exact_grid(dtype):
    for mut in SD.OP_MUTANTS:
        share = SD.separated_share(mut, dtype)
        print(f"dtype {dtype}: {mut} lies more than 2 act_tol from silu(g) u at {100 * share:.1f} % of the grid")
        assert share >= GRID_SHARE[mut][dtype], (mut, dtype, share)
