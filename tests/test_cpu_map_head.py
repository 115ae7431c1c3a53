"""A model without a class token and with the attention-pooling (MAP) head on the host (no GPU): the file format's `attn_pool.*` extension, the
loader, vitx_model_pool_query, the file tools, the converter (transformers' SiglipVisionModel / SiglipModel, timm state dicts), the preprocessing
description of a SiglipImageProcessor, and the float64 restatement (tests/map_data.py) the GPU tests compare with -- pinned here to transformers."""
import hashlib
import struct

import numpy as np
import pytest

import arch_data as AD
import map_data as MD
import prefix_data as PD
import ref64 as R64
from test_cpu_arch import HF_TOL, KW, _redraw

ERR_FORMAT, ERR_ARG, ERR_UNSUPPORTED = 2, 3, 5
# sha1 of convert_hf_model(ViTForImageClassification, test_cpu_arch's micro config redrawn with seed 21, ftype 1), recorded on the commit before the
# attention-pooling head existed: a class-token file keeps its bytes
VIT_FT1_SHA1 = "808b1a12ec681113ab83016ff8de42efb6ac8c88"


def _siglip(seed=21, full=False, **over):
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    cfg = tr.SiglipVisionConfig(**{**dict(intermediate_size=512), **KW, **over})
    if full:
        m = tr.SiglipModel(tr.SiglipConfig(vision_config=cfg.to_dict(), text_config=dict(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2,
                                                                                      vocab_size=50, max_position_embeddings=8)))
    else:
        m = tr.SiglipVisionModel(cfg)
    return torch, _redraw(torch, m.eval(), seed)


def _write_raw(pkg, path, mf, drop=(), rename=None, extra=()):
    """Re-emit a parsed model file record by record (no validation): the malformed files of the loader test."""
    G = pkg.ggml_file
    hp = mf.hparams
    with open(path, "wb") as f:
        f.write(struct.pack("<i", G.GGML_MAGIC))
        for v in (hp.hidden_size, hp.num_hidden_layers, hp.num_attention_heads, hp.num_classes, hp.patch_size, hp.img_size, hp.ftype):
            f.write(struct.pack("<i", v))
        f.write(struct.pack("<i", len(mf.id2label)))
        for k, v in mf.id2label.items():
            b = v.encode(); f.write(struct.pack("<ii", k, len(b))); f.write(b)
        for t in [t for t in mf.tensors if t.name not in drop] + list(extra):
            name = (rename or {}).get(t.name, t.name).encode()
            f.write(struct.pack("<iii", len(t.ne), len(name), t.ttype))
            for d in t.ne:
                f.write(struct.pack("<i", d))
            f.write(name); f.write(t.raw)


def _load_fails(binding, path, code=ERR_FORMAT, word=None):
    with pytest.raises(binding.VitxError) as ei:
        binding.Model(path)
    assert ei.value.code == code, str(ei.value)
    if word:
        assert word in str(ei.value), str(ei.value)


@pytest.mark.parametrize("full", [False, True], ids=["SiglipVisionModel", "SiglipModel"])
def test_converter_and_restatement_against_transformers(pkg, binding, tmp_path, full):
    """convert_hf_model at ftype 0 of a SiglipVisionModel (and of a SiglipModel: its vision tower), then ref64.forward64 on the file's tensors
    against the model itself: last_hidden_state and pooler_output to f32 noise, textbook and folded."""
    torch, m = _siglip(full=full)
    vis = m.vision_model if full else m
    path = str(tmp_path / "siglip.gguf")
    hp = pkg.convert.convert_hf_model(m, path, ftype=0)
    assert (hp.hidden_size, hp.num_hidden_layers, hp.num_attention_heads, hp.num_classes, hp.patch_size, hp.img_size) == (128, 2, 2, 1, 14, 56)
    t = PD.file_tensors(pkg, path)
    names = list(t)
    assert "cls_token" not in t and "reg_token" not in t and "arch" not in t          # tanh-GELU, 1e-6: the reference's arithmetic
    assert t["pos_embed"].shape == (1, 16, 128)
    i0 = names.index("norm.bias")
    assert names[i0 + 1:i0 + 14] == ["attn_pool." + k for k in MD.POOL_NAMES] and names[i0 + 14:] == ["head.weight", "head.bias"]
    assert t["attn_pool.latent"].shape == (1, 1, 128) and t["attn_pool.kv.weight"].shape == (256, 128)
    assert not t["head.weight"].any() and pkg.ggml_file.read_model(path).id2label == {0: "(no head)"}
    mdl = binding.Model(path)
    assert len(mdl.tensors()) == 3 + 24 + 2 + 13 + 2
    assert (mdl.head_pool, mdl.num_prefix, mdl.num_registers) == (binding.POOL_MAP, 0, 0)
    mdl.close()
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(2, 56, seed=3))
    px = torch.from_numpy(imgs).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        out = vis(pixel_values=px) if full else m(pixel_values=px)
    for folded in (False, True):
        r = R64.forward64(t, imgs, heads=2, folded=folded)
        d_h = float(np.abs(r["final"] - out.last_hidden_state.numpy()).max())
        d_e = float(np.abs(r["e"] - out.pooler_output.numpy()).max())
        print(f"{'folded' if folded else 'textbook'}: max|restatement - transformers|  last_hidden_state {d_h:.3e}  pooler_output {d_e:.3e}  (max|e| {np.abs(r['e']).max():.3f})")
        assert r["final"].shape == (2, 16, 128) and d_h <= HF_TOL and d_e <= HF_TOL, (d_h, d_e)
    if full:        # a SiglipModel converts to the bytes of its own vision tower
        p2 = str(tmp_path / "tower.gguf")
        tr = pytest.importorskip("transformers")
        tower = tr.SiglipVisionModel(m.config.vision_config).eval()
        tower.load_state_dict(vis.state_dict())
        pkg.convert.convert_hf_model(tower, p2, ftype=0, no_head=True)               # the flag is accepted and not required
        assert open(p2, "rb").read() == open(path, "rb").read()


def test_fold_identity_and_fixture_separates_the_mutants(pkg):
    """Folded and textbook restatements agree in float64 to 1e-12 relative on e, with a non-zero K bias; on the fixture the scores spread over a
    few units, so the flat-softmax mutant moves e by more than twice the gate the GPU test applies; the wrong activation (QuickGELU: erf-GELU lies
    within 5e-4 of tanh-GELU everywhere, 1 - cos 6e-9 here) mostly rescales e, so it is the mean length of e that sees it, under both operand types
    (tests/map_data.py LEN).  The operand-rounding figures recorded beside the GPU gates are recomputed here."""
    hp, t = MD.fixture_tensors(pkg)
    assert np.abs(t["attn_pool.kv.bias"][:128]).max() > 0.01
    imgs = PD.exact_images(17, 56, seed=1)              # the images of tests/test_gpu_map_head.py
    a, b = R64.forward64(t, imgs, heads=2, folded=False), R64.forward64(t, imgs, heads=2, folded=True)
    rel = float(np.abs(a["e"] - b["e"]).max() / np.abs(a["e"]).max())
    print(f"fold identity: max|e_folded - e_textbook| / max|e| = {rel:.3e};  max|p_folded - p_textbook| = {np.abs(a['p'] - b['p']).max():.3e}")
    assert rel <= 1e-12
    u, _ = MD.u64(t, 2)
    s = np.einsum("hk,ntk->nht", u, b["final"])
    spread = float((s.max(-1) - s.min(-1)).min())
    print(f"score spread (max - min over tokens, smallest over images and heads): {spread:.2f};  largest p: {b['p'].max():.3f}")
    assert spread > 2.0
    t = PD.file_tensors(pkg, MD.fixture_file(pkg))          # the file the GPU test runs (f16 matrices): the figures recorded in map_data.py are its
    b = R64.forward64(t, imgs, heads=2)
    flat, quick = R64.forward64(t, imgs, heads=2, flat=True), R64.forward64(t, imgs, heads=2, activation=AD.ACT_QUICK)
    for dtype in (0, 1):
        gate, lgate = MD.cos_gate(dtype), MD.len_gate(dtype)
        rnd = PD.f16_round if dtype == 0 else PD.bf16_round
        r = R64.forward64(t, imgs, heads=2, wround=rnd, uround=rnd)
        noise, lnoise = float(MD.one_minus_cos(r["e"], b["e"]).max()), MD.mean_length(r["e"], b["e"])
        c_flat, l_quick = float(MD.one_minus_cos(flat["e"], b["e"]).min()), MD.mean_length(quick["e"], b["e"])
        print(f"dtype {dtype}: operand rounding: 1 - cos(e) {noise:.3e} (recorded {MD.COS_CPU[dtype]:.2e}, gate {gate:.3e}), mean length {lnoise:+.3e} (recorded "
              f"{MD.LEN_CPU[dtype]:.2e}, gate {lgate:.3e});  flat softmax 1 - cos {c_flat:.3e};  QuickGELU for tanh: 1 - cos "
              f"{MD.one_minus_cos(quick['e'], b['e']).min():.3e}, mean length {l_quick:+.3e}, max|dprob| {np.abs(quick['probs'] - b['probs']).max():.3e}")
        assert abs(noise / MD.COS_CPU[dtype] - 1) <= 0.05 and abs(abs(lnoise) / MD.LEN_CPU[dtype] - 1) <= 0.05      # the recorded CPU values are these
        assert c_flat > 2 * gate and abs(l_quick) > 2 * lgate, (c_flat, gate, l_quick, lgate)


@pytest.mark.parametrize("ftype", [0, 1], ids=["f32", "f16"])
def test_pool_query_against_float64(pkg, binding, ftype):
    """vitx_model_pool_query against float64 Wk_h^T q_h / sqrt(d) on the FILE's decode (the f16 file: its f16 matrices): every element within one
    f32 ulp of the float64 value + 1e-12 * sum|terms|."""
    path = MD.fixture_file(pkg, ftype=ftype)
    t = PD.file_tensors(pkg, path)
    if ftype == 1:
        _, t32 = MD.fixture_tensors(pkg)
        assert not np.array_equal(t["attn_pool.kv.weight"], t32["attn_pool.kv.weight"])         # the f16 decode really differs
    want, mag = MD.u64(t, 2)
    mdl = binding.Model(path)
    got = mdl.pool_query()
    mdl.close()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    tol = ulp + 1e-12 * mag
    r = float((np.abs(got.astype(np.float64) - want) / tol).max())
    print(f"ftype {ftype}: worst |u - u64| / (1 ulp + 1e-12 sum|terms|) = {r:.3f}  (max|u| {np.abs(want).max():.3f})")
    assert got.shape == (2, 128) and r <= 1.0


def test_loader_accepts_reports_and_rejects(pkg, binding, tmp_path):
    path = MD.fixture_file(pkg, ftype=1)
    mdl = binding.Model(path)
    assert (mdl.head_pool, mdl.num_prefix, mdl.num_registers, mdl.num_classes) == (binding.POOL_MAP, 0, 0, 10)
    assert len(mdl.tensors()) == 3 + 24 + 2 + 13 + 2
    types = {n: ty for n, ty, _, _ in mdl.tensors()}
    assert types["attn_pool.latent"] == 0 and types["attn_pool.kv.weight"] == 1 and types["attn_pool.kv.bias"] == 0
    mdl.close()
    plain = binding.Model(pkg.synth.cached_synthetic(MD.MICRO, head_scale=4.0))
    assert (plain.head_pool, plain.num_prefix) == (binding.POOL_CLS, 1)
    with pytest.raises(binding.VitxError) as ei:
        plain.pool_query()
    assert ei.value.code == ERR_ARG
    plain.close()
    reg = binding.Model(pkg.synth.cached_synthetic(MD.MICRO, head_scale=4.0, registers=4))
    assert reg.num_prefix == 5
    reg.close()

    G = pkg.ggml_file
    mf = G.read_model(path)
    cls_mf = G.read_model(pkg.synth.cached_synthetic(MD.MICRO, head_scale=4.0))
    reg_mf = G.read_model(pkg.synth.cached_synthetic(MD.MICRO, head_scale=4.0, registers=4))
    rec = lambda m, name: next(t for t in m.tensors if t.name == name)
    bad = str(tmp_path / "bad.gguf")
    # attn_pool.* together with a class token, and with a register token
    _write_raw(pkg, bad, mf, extra=[rec(cls_mf, "cls_token")]); _load_fails(binding, bad, word="cls_token")
    _write_raw(pkg, bad, mf, extra=[rec(reg_mf, "reg_token")]); _load_fails(binding, bad, word="reg_token")
    # no class token and no attn_pool.*
    _write_raw(pkg, bad, cls_mf, drop=("cls_token",)); _load_fails(binding, bad, word="cls_token")
    _write_raw(pkg, bad, mf, drop=tuple("attn_pool." + k for k in MD.POOL_NAMES)); _load_fails(binding, bad, word="cls_token")
    # a partial set: each of the thirteen missing in turn
    for k in MD.POOL_NAMES:
        _write_raw(pkg, bad, mf, drop=("attn_pool." + k,)); _load_fails(binding, bad, word="attn_pool." + k)
    # wrong shapes: kv with D rows, a latent of two rows, a class-row position table beside attn_pool.*
    q = rec(mf, "attn_pool.q.weight")
    _write_raw(pkg, bad, mf, drop=("attn_pool.kv.weight",), extra=[G.TensorRec("attn_pool.kv.weight", q.ttype, q.ne, q.raw)]); _load_fails(binding, bad, word="attn_pool.kv.weight")
    lat = rec(mf, "attn_pool.latent")
    _write_raw(pkg, bad, mf, drop=("attn_pool.latent",), extra=[G.TensorRec("attn_pool.latent", 0, (128, 2, 1), lat.raw * 2)]); _load_fails(binding, bad, word="attn_pool.latent")
    _write_raw(pkg, bad, mf, drop=("pos_embed",), extra=[rec(cls_mf, "pos_embed")]); _load_fails(binding, bad, word="pos_embed")
    _write_raw(pkg, bad, cls_mf, drop=("pos_embed",), extra=[rec(mf, "pos_embed")]); _load_fails(binding, bad, word="pos_embed")
    # a vector that is not f32, a duplicate
    kb = rec(mf, "attn_pool.kv.bias")
    _write_raw(pkg, bad, mf, drop=("attn_pool.kv.bias",), extra=[G.TensorRec("attn_pool.kv.bias", 1, kb.ne, np.frombuffer(kb.raw, "<f4").astype("<f2").tobytes())]); _load_fails(binding, bad)
    _write_raw(pkg, bad, mf, extra=[rec(mf, "attn_pool.norm.bias")]); _load_fails(binding, bad, word="duplicate")


def test_quantize_carries_the_pool_byte_for_byte(pkg, binding, tmp_path):
    src = MD.fixture_file(pkg, ftype=1)
    dst = str(tmp_path / "q8.gguf")
    binding.quantize_file(src, dst, 8)
    a = {t.name: t for t in pkg.ggml_file.read_model(src).tensors}
    b = {t.name: t for t in pkg.ggml_file.read_model(dst).tensors}
    assert list(a) == list(b)
    for k in MD.POOL_NAMES:
        ta, tb = a["attn_pool." + k], b["attn_pool." + k]
        assert (ta.ttype, ta.ne, ta.raw) == (tb.ttype, tb.ne, tb.raw), k
    assert b["blocks.0.attn.qkv.weight"].ttype == 8 and b["head.weight"].ttype == 8        # the selection over the reference's tensors stays
    # the Python writer makes the same file
    hp, t = MD.fixture_tensors(pkg)
    py = str(tmp_path / "q8py.gguf")
    pkg.ggml_file.write_model(py, hp, t, ftype=8)
    assert open(py, "rb").read() == open(dst, "rb").read()
    mdl = binding.Model(dst)
    assert mdl.head_pool == binding.POOL_MAP
    mdl.close()
    with pytest.raises(binding.VitxError) as ei:       # the second part of the feature is not here: a g^2-row table has no resampling path yet
        binding.resize_file(src, str(tmp_path / "r.gguf"), 70)
    assert ei.value.code == ERR_UNSUPPORTED and "class row" in str(ei.value)


def test_class_token_file_keeps_its_bytes(pkg, tmp_path):
    """A class-token model converts to the bytes it converted to before the attention-pooling head existed."""
    from test_cpu_arch import _hf_model
    _, m = _hf_model("vit")
    path = str(tmp_path / "vit.gguf")
    pkg.convert.convert_hf_model(m, path, ftype=1)
    assert hashlib.sha1(open(path, "rb").read()).hexdigest() == VIT_FT1_SHA1


def test_converter_refusals(pkg, tmp_path):
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    out = str(tmp_path / "x.gguf")
    _, so = _siglip(intermediate_size=432)
    with pytest.raises(ValueError, match="intermediate_size"):
        pkg.convert.convert_hf_model(so, out, ftype=0)
    nohead = tr.SiglipVisionModel(tr.SiglipVisionConfig(intermediate_size=512, vision_use_head=False, **KW)).eval()
    with pytest.raises(ValueError, match="vision_use_head"):
        pkg.convert.convert_hf_model(nohead, out, ftype=0)
    cfg = tr.SiglipConfig(vision_config=dict(intermediate_size=512, **KW), text_config=dict(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, vocab_size=50))
    cfg.num_labels = 3
    with pytest.raises(ValueError, match="SiglipForImageClassification"):
        pkg.convert.convert_hf_model(tr.SiglipForImageClassification(cfg).eval(), out, ftype=0)
    s2 = tr.Siglip2VisionModel(tr.Siglip2VisionConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=512, patch_size=14, num_patches=16)).eval()
    with pytest.raises(ValueError, match="Siglip2VisionModel"):
        pkg.convert.convert_hf_model(s2, out, ftype=0)
    # timm state dicts: attn_pool.* is taken without cls_token only; its qk-norm and position embedding are refused by name; no head.* -> the zero head
    hp, t = MD.fixture_tensors(pkg)
    sd = dict(t)
    del sd["head.weight"], sd["head.bias"]
    got = pkg.convert.convert_timm_state_dict(sd, out, ftype=0, heads=2)
    assert got.num_classes == 1 and pkg.ggml_file.read_model(out).id2label == {0: "(no head)"}
    tt = PD.file_tensors(pkg, out)
    assert list(tt)[-15:-2] == ["attn_pool." + k for k in MD.POOL_NAMES] and not tt["head.weight"].any()
    assert np.array_equal(tt["attn_pool.kv.weight"], t["attn_pool.kv.weight"])
    with pytest.raises(ValueError, match="cls_token"):
        pkg.convert.convert_timm_state_dict({**t, "cls_token": np.zeros((1, 1, 128), np.float32)}, out, ftype=0, heads=2)
    for name in ("attn_pool.q_norm.weight", "attn_pool.k_norm.weight", "attn_pool.pos_embed"):
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            pkg.convert.convert_timm_state_dict({**t, name: np.zeros((128,), np.float32)}, out, ftype=0, heads=2)


def test_siglip_image_processor_description(pkg):
    """A SiglipImageProcessor-shaped preprocessor_config gives the `preproc` tensor: stretch to the model's size, PIL bicubic, no crop, 127.5 / 127.5."""
    cfg = {"do_convert_rgb": None, "do_normalize": True, "do_rescale": True, "do_resize": True, "image_mean": [0.5, 0.5, 0.5], "image_std": [0.5, 0.5, 0.5],
           "image_processor_type": "SiglipImageProcessor", "processor_class": "SiglipProcessor", "resample": 3, "rescale_factor": 0.00392156862745098,
           "size": {"height": 56, "width": 56}}
    G = pkg.ggml_file
    f = G.preproc_fields(pkg.convert.hf_preproc(cfg, 56))
    assert (f["resize_mode"], f["resize_a"], f["resize_b"], f["filter"], f["crop"], f["crop_round"]) == (G.PP_STRETCH, 56, 56, G.PP_PIL_BICUBIC, 0, 0)
    assert f["mean255"] == (127.5, 127.5, 127.5) and f["std255"] == (127.5, 127.5, 127.5)
