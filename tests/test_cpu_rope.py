"""Rotary position embeddings without a GPU (include/vitx.h "rotary position embeddings"): the host table against transformers'
DINOv3ViTRopePositionEmbedding, the converter and the float64 restatement of tests/ref64.py against DINOv3ViTModel, the separation of the micro
fixture's mutants from operand rounding, and the loader's rules for the `rope` tensor."""
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
import text_data as TD
from ref64 import PROB_TOL, stage_errors, stage_ok
from test_gpu_arch import ROUND, _apart

ERR_FORMAT, ERR_ARG = 2, 3
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QK_FACTOR = 6.0                       # the issue's F for the transformers fixture


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _record(name, ttype, shape, data):
    nb = name.encode()
    return struct.pack("<iii", len(shape), len(nb), ttype) + b"".join(struct.pack("<i", d) for d in reversed(shape)) + nb + data


def _rope(*vals):
    return _record("rope", 0, (len(vals),), np.array(vals, np.float32).tobytes())


# ------------------------------------------------------------------------------------------------ the table
def _tiny_rope_file(pkg, tmp_path, hd, theta=100.0):
    """The smallest loadable file with head dim hd: one head, one layer, a 2 x 2 grid of 2 x 2 patches."""
    hp = pkg.ggml_file.HParams(hd, 1, 1, 2, 2, 4, 0)
    t = {"rope": np.array([1, theta, 0, 0], np.float32)}
    t.update(pkg.synth.make_weights(hp))
    path = str(tmp_path / f"hd{hd}.gguf")
    pkg.ggml_file.write_model(path, hp, t, ftype=0)
    return path


@pytest.mark.parametrize("hd", [16, 24, 32, 64, 128])
def test_table_against_transformers(pkg, binding, tmp_path, hd):
    """vitx_model_rope_table (double, rounded once) against DINOv3ViTRopePositionEmbedding in eval mode (f32 angles).  The issue measured 7.9e-7
    between HF and the double formula -- HF's own f32 angle arithmetic -- and sets the gate at 5 x that, 4e-6.  HF's two tiled halves are equal."""
    import torch
    import transformers
    from transformers.models.dinov3_vit.modeling_dinov3_vit import DINOv3ViTRopePositionEmbedding
    m = binding.Model(_tiny_rope_file(pkg, tmp_path, hd))
    assert m.rope == (1, 100.0)
    cfg = transformers.DINOv3ViTConfig(hidden_size=hd, num_attention_heads=1, intermediate_size=4 * hd, num_hidden_layers=1, patch_size=1, image_size=4, rope_theta=100.0)
    hf = DINOv3ViTRopePositionEmbedding(cfg).eval()
    worst = 0.0
    for gh, gw in ((4, 4), (2, 3), (3, 5), (14, 14), (16, 16), (37, 37), (64, 48)):
        cos, sin = m.rope_table((gh, gw))
        assert cos.shape == sin.shape == (gh * gw, hd // 2) and cos.dtype == np.float32
        with torch.no_grad():
            hc, hs = hf(torch.zeros(1, 3, gh, gw))
        hc, hs = hc.numpy(), hs.numpy()
        assert hc.shape == (gh * gw, hd)
        assert np.array_equal(hc[:, :hd // 2], hc[:, hd // 2:]) and np.array_equal(hs[:, :hd // 2], hs[:, hd // 2:])
        d = max(float(np.abs(cos - hc[:, :hd // 2]).max()), float(np.abs(sin - hs[:, :hd // 2]).max()))
        worst = max(worst, d)
        assert d <= 4e-6, (hd, gh, gw, d)
        # ... and it is the restatement's table, to f32 rounding of a value in [-1, 1]
        c64, s64 = RD.table64(100.0, hd, gh, gw)
        assert np.abs(cos - c64).max() <= 2.0 ** -24 and np.abs(sin - s64).max() <= 2.0 ** -24
    print(f"head dim {hd}: worst |table - transformers| over the grids {worst:.2e}")
    # arguments
    L = binding.lib()
    fp = C.POINTER(C.c_float)
    buf = np.zeros(hd, np.float32)
    assert L.vitx_model_rope_table(m._h, 0, 2, buf.ctypes.data_as(fp), buf.ctypes.data_as(fp)) == ERR_ARG
    assert L.vitx_model_rope_table(m._h, 2, 2, None, buf.ctypes.data_as(fp)) == ERR_ARG
    m.close()
    plain = binding.Model(pkg.synth.cached_synthetic(AD.MICRO, head_scale=4.0))
    assert plain.rope is None
    with pytest.raises(binding.VitxError):
        plain.rope_table(4)
    plain.close()


# ------------------------------------------------------------------------------------------------ the converter and the restatement
def _hf_dinov3(seed=31, factor=QK_FACTOR, **over):
    """A random-init DINOv3ViTModel at the shape of arch_data.MICRO, LayerScale and biases perturbed, the q and k weights times `factor`; the patch
    kernel fp16-exact (the file stores it in fp16 even at ftype 0)."""
    import torch
    import transformers
    torch.manual_seed(seed)
    kw = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, patch_size=14, image_size=56, num_register_tokens=4,
              layer_norm_eps=float(np.float32(1e-5)), key_bias=False, hidden_act="gelu", rope_theta=100.0)
    kw.update(over)
    m = transformers.DINOv3ViTModel(transformers.DINOv3ViTConfig(**kw)).eval()
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("lambda1"):
                p.copy_(torch.from_numpy((rng.random(tuple(p.shape)) * 1.5 + 0.25).astype(np.float32)))
            elif k.endswith(".bias"):
                p.copy_(torch.from_numpy((rng.standard_normal(tuple(p.shape)) * 0.02).astype(np.float32)))
            elif k.endswith("q_proj.weight") or k.endswith("k_proj.weight"):
                p.mul_(factor)
            elif p.dim() == 4:
                p.copy_(p.half().float())
    return torch, m


@pytest.mark.parametrize("S", [56, 84])
def test_converter_and_restatement_against_transformers(pkg, binding, tmp_path, S):
    """convert_hf_model at ftype 0, then ref64.forward64 on the file's tensors against the model's f32 last_hidden_state, at the file's size and on
    an 84 x 84 image (6 x 6 grid, the table from the new grid: nothing is resampled).  The issue's gates: 1e-4 for the restatement, every mutant
    further than 0.1 (it measured 2.5e-6 on features of magnitude 3.9, and 0.58 / 0.51 / 0.68 for no_rope / xy_swapped / sin_negated)."""
    torch, m = _hf_dinov3()
    path = str(tmp_path / "dinov3.gguf")
    hp = pkg.convert.convert_hf_model(m, path, ftype=0)
    assert (hp.hidden_size, hp.num_hidden_layers, hp.num_attention_heads, hp.num_classes, hp.patch_size, hp.img_size) == (128, 2, 2, 1, 14, 56)
    t = PD.file_tensors(pkg, path)
    names = list(t)
    assert names[:5] == ["arch", "rope", "cls_token", "reg_token", "pos_embed"]
    assert np.array_equal(_bits(t["arch"]), _bits(np.array([AD.ACT_ERF, 1e-5, 0, 0], np.float32)))
    assert np.array_equal(_bits(t["rope"]), _bits(np.array([1, 100, 0, 0], np.float32)))
    assert t["pos_embed"].shape == (1, 17, 128) and not t["pos_embed"].any()
    assert t["reg_token"].shape == (1, 4, 128) and not t["head.weight"].any() and not t["head.bias"].any()
    assert "mask_token" not in " ".join(names)
    for i in range(2):                                                 # key_bias=False: a zero k bias between the q and v biases
        b = t[f"blocks.{i}.attn.qkv.bias"]
        assert b[:128].any() and not b[128:256].any() and b[256:].any()
    assert pkg.ggml_file.read_model(path).id2label == {0: "(no head)"}
    mdl = binding.Model(path)
    assert mdl.rope == (1, 100.0) and mdl.num_registers == 4 and mdl.activation == AD.ACT_ERF and len(mdl.tensors()) == 2 + 5 + 24 + 4
    mdl.close()
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(2, S, seed=3))
    with torch.no_grad():
        out = m(pixel_values=torch.from_numpy(imgs).permute(0, 3, 1, 2).contiguous())
    want = out.last_hidden_state.numpy()
    g = S // 14
    pos = None if S == 56 else np.zeros((1 + g * g, 128), np.float32)
    r = R64.forward64(t, imgs, heads=2, pos=pos)
    assert r["final"].shape == want.shape == (2, 5 + g * g, 128)
    d = float(np.abs(r["final"] - want).max())
    print(f"S {S}: max|restatement - transformers| = {d:.3e} on features of magnitude {np.abs(want).max():.2f}")
    assert d <= 1e-4, d
    assert np.abs(r["final"][:, 0] - out.pooler_output.numpy()).max() <= 1e-4
    for mut in RD.MUTANTS:
        dm = float(np.abs(R64.forward64(t, imgs, heads=2, pos=pos, mutant=mut)["final"] - want).max())
        print(f"S {S}: mutant {mut}: max|d| = {dm:.3f}")
        assert dm > 0.1, (mut, dm)


def test_converter_refusals(pkg, tmp_path):
    out = str(tmp_path / "x.gguf")
    _, gated = _hf_dinov3(use_gated_mlp=True)
    with pytest.raises(ValueError, match="use_gated_mlp"):
        pkg.convert.convert_hf_model(gated, out)
    _, narrow = _hf_dinov3(intermediate_size=384)
    with pytest.raises(ValueError, match="4 x hidden"):
        pkg.convert.convert_hf_model(narrow, out)
    assert not os.path.exists(out)
    assert pkg.convert.FAMILIES["dinov3_vit"].name == "DINOv3" and pkg.convert.FAMILIES["dinov3_vit"].head == "never"


# ------------------------------------------------------------------------------------------------ the micro fixture
def test_fixture_separates_the_mutants_from_operand_rounding(pkg):
    """Computed, not assumed (rope_data.QK_SCALE): on the micro fixture and the images of the GPU tests, the operand-rounded restatement lies inside
    HALF of tests/ref64.py's stage and probability gates of the unrounded one, and every mutant lies more than TWICE a gate from the real
    thing -- so a GPU result inside the gates of the restatement is outside those of every mutant."""
    imgs = PD.exact_images(17, 56, seed=1)
    t = PD.file_tensors(pkg, RD.fixture_file(pkg))
    assert RD.rope_of(t) == RD.THETA and t["reg_token"].shape[1] == RD.REGISTERS and not t["pos_embed"].any()
    exact = R64.forward64(t, imgs, 2)
    for dtype in (0, 1):
        ref = R64.forward64(t, imgs, 2, wround=ROUND[dtype], uround=ROUND[dtype])
        se = stage_errors(ref["trace"], exact["trace"])
        dp = float(np.abs(ref["probs"] - exact["probs"]).max())
        print(f"dtype {dtype}: rounded against unrounded: stages (e_max, e_rms) {[(round(a, 5), round(b, 5)) for a, b in se]}, max|dprob| {dp:.2e}")
        assert all(stage_ok(a, b, dtype, 0.5) for a, b in se) and dp <= 0.5 * PROB_TOL[dtype]
        for mut in RD.MUTANTS:
            m = R64.forward64(t, imgs, 2, mutant=mut, wround=ROUND[dtype], uround=ROUND[dtype])
            sm = stage_errors(m["trace"], ref["trace"])
            dm = float(np.abs(ref["probs"] - m["probs"]).max())
            print(f"dtype {dtype}: mutant {mut}: stages {[(round(a, 4), round(b, 4)) for a, b in sm]}, max|dprob| {dm:.3f}")
            assert _apart(ref, m, dtype), (dtype, mut)


def test_rope_f32_restatement_is_the_float64_rotation():
    """rope_data.rope_bits (the numpy-f32 operation order the GPU test holds the kernel to) against rotate64: within the f32 rounding of three operations."""
    rng = np.random.default_rng(5)
    n, N, T, D, H = 2, 9, 3, 32, 2
    x = rng.standard_normal((n * N, 3 * D)).astype(np.float32)
    cos, sin = RD.table64(100.0, D // H, 2, 3)
    got = RD.from_bits16(RD.rope_bits(RD.to_bits16(x, 0), cos.astype(np.float32), sin.astype(np.float32), n, N, T, D, H, 0), 0)
    x16 = RD.from_bits16(RD.to_bits16(x, 0), 0).astype(np.float64).reshape(n, N, 3, H, D // H)
    for s in range(2):
        want = RD.rotate64(x16[:, :, s].transpose(0, 2, 1, 3), cos, sin, T).transpose(0, 2, 1, 3)
        assert np.abs(got.reshape(n, N, 3, H, D // H)[:, :, s] - want).max() <= 2.0 ** -10 * np.abs(want).max()
    assert np.array_equal(got.reshape(n, N, 3, D)[:, :, 2], x16.reshape(n, N, 3, D)[:, :, 2])
    assert np.array_equal(got.reshape(n, N, 3, D)[:, :T], x16.reshape(n, N, 3, D)[:, :T])
    hi, lo = RD.split_hilo(x)
    v = RD.from_bits16(hi, 0).astype(np.float64) + RD.from_bits16(lo, 0).astype(np.float64) / 2048
    assert np.abs(v - x).max() <= 2.0 ** -21 * np.abs(x).max()


# ------------------------------------------------------------------------------------------------ the loader
def test_loader_rules_for_the_rope_tensor(pkg, binding, tmp_path):
    L = binding.lib()
    plain = pkg.synth.cached_synthetic(AD.MICRO, head_scale=4.0)
    base = open(plain, "rb").read()
    first = base.index(struct.pack("<iii", 3, len("cls_token"), 0))

    def load(data):
        p = str(tmp_path / "x.gguf")
        open(p, "wb").write(data)
        h = C.c_void_p()
        rc = L.vitx_model_load(p.encode(), C.byref(h))
        out = None
        if rc == 0:
            k, th = C.c_int(-1), C.c_float(-1)
            has = L.vitx_model_rope(h, C.byref(k), C.byref(th))
            out = (has, k.value, th.value, L.vitx_model_num_tensors(h))
            assert L.vitx_model_rope(h, None, None) == has
            L.vitx_model_free(h)
        return rc, out, L.vitx_last_error().decode()

    # a file without `rope`: the getter says 0 and touches nothing; its bytes are what they were
    assert load(base)[:2] == (0, (0, -1, -1.0, 32))
    want = json.load(open(os.path.join(GOLD, "weights_sha1.json")))
    micro = pkg.synth.cached_synthetic("vit_micro_patch16_64-h4".rsplit("-", 1)[0], head_scale=4.0)
    assert hashlib.sha1(open(micro, "rb").read()).hexdigest() == want["vit_micro_patch16_64-h4"]
    assert L.vitx_model_rope(None, None, None) == 0
    # present, in front (the converter's place) or at the very end
    for theta in (100.0, 10000.0, 0.5):
        assert load(base[:first] + _rope(1, theta, 0, 0) + base[first:])[:2] == (0, (1, 1, theta, 33))
        assert load(base + _rope(1, theta, 0, 0))[:2] == (0, (1, 1, theta, 33))
    bad = {
        "kind 0": _rope(0, 100, 0, 0), "kind 2": _rope(2, 100, 0, 0), "kind 1.5": _rope(1.5, 100, 0, 0), "kind nan": _rope(np.nan, 100, 0, 0),
        "theta 0": _rope(1, 0, 0, 0), "theta negative": _rope(1, -100, 0, 0), "theta inf": _rope(1, np.inf, 0, 0), "theta nan": _rope(1, np.nan, 0, 0),
        "reserved slot 2": _rope(1, 100, 1, 0), "reserved slot 3": _rope(1, 100, 0, 1e-30),
        "rope of 3": _rope(1, 100, 0), "rope of 5": _rope(1, 100, 0, 0, 0), "rope in f16": _record("rope", 1, (4,), np.array([1, 100, 0, 0], np.float16).tobytes()),
        "rope with two dims": _record("rope", 0, (1, 4), np.array([1, 100, 0, 0], np.float32).tobytes()),
        "rope twice": _rope(1, 100, 0, 0) + _rope(1, 100, 0, 0),
    }
    for what, rec in bad.items():
        for data in (base[:first] + rec + base[first:], base + rec):
            rc, _, msg = load(data)
            assert rc == ERR_FORMAT and msg.startswith("vitx_model_load:") and "rope" in msg, (what, rc, msg)
    # a head dim that is no multiple of 4: D 12, 2 heads of 6 (the same file loads without `rope`)
    hp = pkg.ggml_file.HParams(12, 1, 2, 2, 2, 4, 0)
    w = pkg.synth.make_weights(hp)
    p6 = str(tmp_path / "hd6.gguf")
    pkg.ggml_file.write_model(p6, hp, w, ftype=0)
    assert load(open(p6, "rb").read())[0] == 0
    pkg.ggml_file.write_model(p6, hp, {"rope": np.array([1, 100, 0, 0], np.float32), **w}, ftype=0)
    rc, _, msg = load(open(p6, "rb").read())
    assert rc == ERR_FORMAT and "multiple of 4" in msg, msg
    # a text-tower file
    text = open(TD.text_file(pkg, "siglip"), "rb").read()
    assert load(text)[0] == 0
    rc, _, msg = load(text + _rope(1, 100, 0, 0))
    assert rc == ERR_FORMAT and "rope" in msg and "text" in msg, msg
    # together with the attention-pooling head
    pool = open(MD.fixture_file(pkg), "rb").read()
    assert load(pool)[0] == 0
    for data in (pool + _rope(1, 100, 0, 0), pool[:pool.index(struct.pack("<iii", 3, len("pos_embed"), 0))] + _rope(1, 100, 0, 0) + pool[pool.index(struct.pack("<iii", 3, len("pos_embed"), 0)):]):
        rc, _, msg = load(data)
        assert rc == ERR_FORMAT and "rope" in msg and "attn_pool" in msg, msg


def test_quantize_and_resize_carry_rope_through(pkg, binding, tmp_path):
    src = RD.fixture_file(pkg)
    recs0 = {t.name: t for t in pkg.ggml_file.read_model(src).tensors}
    assert list(recs0)[:5] == ["arch", "rope", "cls_token", "reg_token", "pos_embed"]
    q8, big = str(tmp_path / "q8.gguf"), str(tmp_path / "84.gguf")
    binding.quantize_file(src, q8, 8)
    binding.resize_file(src, big, 84, binding.POS_BICUBIC)
    for path, img in ((q8, 56), (big, 84)):
        m = binding.Model(path)
        assert m.rope == (1, RD.THETA) and m.img_size == img and m.num_registers == RD.REGISTERS
        m.close()
        recs = {t.name: t for t in pkg.ggml_file.read_model(path).tensors}
        assert list(recs) == list(recs0)
        for k in ("arch", "rope", "reg_token"):
            assert (recs[k].ttype, recs[k].ne, recs[k].raw) == (recs0[k].ttype, recs0[k].ne, recs0[k].raw), (path, k)
    assert {t.name: t.ttype for t in pkg.ggml_file.read_model(q8).tensors}["blocks.0.attn.qkv.weight"] == 8
    t84 = PD.file_tensors(pkg, big)
    assert t84["pos_embed"].shape == (1, 37, 128) and not t84["pos_embed"].any()          # a resampled zero table is a zero table
