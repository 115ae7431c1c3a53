"""The text tower without a GPU (include/vitx.h "the text tower"): tests/text_data.py's restatement pinned to transformers' CLIPTextModelWithProjection
and SiglipTextModel in float64, the converter, the loader and every error of the C ABI that is raised before a device call, and the conditions
the GPU tests' data must meet (the pattern of tests/test_cpu_exact_data.py)."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

import arch_data as AD
import exact_data as X
import prefix_data as PD
import text_data as TD
import zs_data as Z

FAMILIES = ("clip", "siglip")


def _rel(a, b):            # tests/test_cpu_zeroshot.py's measure
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _hf_embeds(family, ids):
    import torch
    with torch.no_grad():
        o = TD.hf_model(family)(input_ids=torch.from_numpy(np.asarray(ids)).long())
    return (o.text_embeds if family == "clip" else o.pooler_output).numpy()


# ------------------------------------------------------------------------------------------------ the restatement pinned to transformers
@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_against_transformers(pkg, family, tmp_path):
    """forward64 of the converted f32 file against the float64 model: 1e-12 relative, the tolerance of the transformers pin in
    tests/test_cpu_zeroshot.py (both sides float64; the model's parameters are f32 values, so the f32 file holds them exactly)."""
    path = TD.text_file(pkg, family, ftype=0)
    t = PD.file_tensors(pkg, path)
    ids = TD.prompts(family)
    if family == "clip":
        at = TD.pooled_positions(ids, TD.CLIP_CFG["eos_token_id"])
        assert at[0] == 5 and at[1] == ids.shape[1] - 1 and 5 < len(set(at.tolist()))            # EOS at 5, at T - 1 and mid-row
        assert (ids[0, 6:] == TD.CLIP_CFG["pad_token_id"]).all()
    got, want = TD.forward64(t, ids), _hf_embeds(family, ids)
    r = _rel(got, want)
    print(f"{family}: forward64 against transformers {r:.2e} relative")
    assert want.shape == got.shape and r < 1e-12


def test_pad_ids_behind_eos_do_not_reach_the_clip_embedding(pkg):
    """Under the causal mask nothing behind the pooled (EOS) row reaches it: changing the pad ids there leaves transformers' and the
    restatement's embedding where it was, to the pin's tolerance.  This is why the engine takes no attention mask."""
    t = PD.file_tensors(pkg, TD.text_file(pkg, "clip", ftype=0))
    ids = TD.prompts("clip")
    other = ids.copy()
    other[0, 6:] = 17; other[2, TD.pooled_positions(ids, 95)[2] + 1:] = 33
    assert (other != ids).any()
    assert _rel(TD.forward64(t, other), TD.forward64(t, ids)) < 1e-12
    assert _rel(_hf_embeds("clip", other), _hf_embeds("clip", ids)) < 1e-12
    moved = ids.copy(); moved[0, 3] = 40                                      # a token IN FRONT of EOS does reach it
    assert _rel(TD.forward64(t, moved)[0], TD.forward64(t, ids)[0]) > 1e-3


# ------------------------------------------------------------------------------------------------ converter, loader, ABI
@pytest.mark.parametrize("ftype", [0, 1])
@pytest.mark.parametrize("family", FAMILIES)
def test_file_round_trip(pkg, binding, family, ftype):
    path = TD.text_file(pkg, family, ftype)
    cfg = TD.CLIP_CFG if family == "clip" else TD.SIGLIP_CFG
    V, D, T = cfg["vocab_size"], cfg["hidden_size"], cfg["max_position_embeddings"]
    E = 64 if family == "clip" else D
    m = binding.Model(path)
    hp = m.hparams
    assert m.kind == binding.KIND_TEXT and (hp.hidden_size, hp.num_hidden_layers, hp.num_attention_heads, hp.num_classes, hp.patch_size, hp.img_size) == (D, 2, 2, E, 0, T)
    assert m.text_info == dict(vocab=V, tokens=T, causal=1 if family == "clip" else 0, eos=95 if family == "clip" else -1) and m.text_zs is None
    shapes = {name: (ttype, ne) for name, ttype, ne, _ in m.tensors()}
    assert shapes["token_embed.weight"][1][:2] == (D, V) and shapes["token_embed.weight"][0] == (1 if ftype else 0)
    assert shapes["pos_embed"] == (0, shapes["pos_embed"][1]) and shapes["pos_embed"][1][:2] == (D, T)
    assert shapes["head.weight"][1][:2] == (D, E) and shapes["blocks.1.mlp.fc2.weight"][1][:2] == (4 * D, D) and "cls_token" not in shapes
    t = PD.file_tensors(pkg, path)
    act, eps, causal, eos = TD.text_arch(t)
    assert (act, causal, eos) == ((2, 1, 95) if family == "clip" else (0, 0, -1)) and np.float32(eps) == np.float32(cfg["layer_norm_eps"])
    assert list(t)[0] == "arch"
    m.close()
    img = binding.Model(Z.model_file(pkg, family))
    assert img.kind == binding.KIND_IMAGE
    with pytest.raises(binding.VitxError) as ei:
        img.text_info
    assert ei.value.code == binding.ERR_ARG
    img.close()


def _two_towers(family):
    import torch
    import transformers
    torch.manual_seed(3)
    if family == "clip":
        cfg = transformers.CLIPConfig(text_config={k: v for k, v in TD.CLIP_CFG.items() if k != "projection_dim"},
                                      vision_config=dict(hidden_size=64, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, image_size=32, patch_size=16), projection_dim=64)
        return transformers.CLIPModel(cfg).eval()
    cfg = transformers.SiglipConfig(text_config=dict(TD.SIGLIP_CFG), vision_config=dict(hidden_size=128, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2, image_size=32, patch_size=16))
    m = transformers.SiglipModel(cfg).eval()
    with torch.no_grad():
        m.logit_scale.fill_(float(np.log(112.0))); m.logit_bias.fill_(-12.5)
    return m


@pytest.mark.parametrize("family", FAMILIES)
def test_two_tower_model_writes_zs_and_leaves_the_vision_file_alone(pkg, binding, family, tmp_path):
    """A CLIPModel / SiglipModel: the text file carries zs = {kind, exp(logit_scale), logit_bias, 0}; converting the vision half writes the same bytes
    before and after the text half was converted."""
    import torch
    m = _two_towers(family)
    sha = lambda p: hashlib.sha1(open(p, "rb").read()).hexdigest()
    v1, v2, tp = (str(tmp_path / n) for n in ("v1.gguf", "v2.gguf", "t.gguf"))
    pkg.convert.convert_hf_model(m, v1, 1)
    hp = pkg.convert.convert_hf_text_model(m, tp, 1)
    pkg.convert.convert_hf_model(m, v2, 1)
    assert sha(v1) == sha(v2) and hp.patch_size == 0
    tm = binding.Model(tp)
    kind, scale, bias = tm.text_zs
    assert kind == (Z.SOFTMAX if family == "clip" else Z.SIGMOID)
    assert scale == np.float32(np.exp(np.float64(m.logit_scale.detach().double().reshape(-1)[0].item()))) and bias == (0.0 if family == "clip" else -12.5)
    ids = TD.prompts(family, n=4)
    with torch.no_grad():
        f = m.double().get_text_features(input_ids=torch.from_numpy(ids).long())
    f = f if torch.is_tensor(f) else f.pooler_output
    tf = PD.file_tensors(pkg, str(tmp_path / "t0.gguf")) if pkg.convert.convert_hf_text_model(m, str(tmp_path / "t0.gguf"), 0) else None
    assert _rel(TD.forward64(tf, ids), f.numpy()) < 1e-12
    tm.close()


def test_image_files_keep_their_recorded_hashes(pkg, tmp_path):
    """tests/golden/convert_sha1.json is what it was, and every image file of tests/test_cpu_convert_pins.py still hashes to it."""
    import test_cpu_convert_pins as CP
    with open(CP.GOLDEN) as f:
        rec = json.load(f)
    assert sorted(rec["sha1"]) == sorted(CP.CASES)
    for name in CP.CASES:
        assert CP.sha1_of(pkg, name, str(tmp_path / "o.gguf")) == rec["sha1"][name], name


def test_legacy_eos_and_refusals(pkg, binding, tmp_path):
    """eos_token_id == 2 (legacy CLIP configs pool at argmax(ids)) writes vocab_size - 1; an MLP that is not 4 D, a width without LayerNorm
    instantiation and a model that is no text tower are refused."""
    import torch
    import transformers
    mk = lambda **kw: transformers.CLIPTextModelWithProjection(transformers.CLIPTextConfig(**{**TD.CLIP_CFG, **kw})).eval()
    p = str(tmp_path / "legacy.gguf")
    pkg.convert.convert_hf_text_model(mk(eos_token_id=2), p, 1)
    m = binding.Model(p)
    assert m.text_info["eos"] == TD.CLIP_CFG["vocab_size"] - 1
    m.close()
    with pytest.raises(ValueError, match="4 x hidden MLP"):
        pkg.convert.convert_hf_text_model(mk(intermediate_size=500), p, 1)
    with pytest.raises(ValueError, match="no LayerNorm instantiation"):
        pkg.convert.convert_hf_text_model(mk(hidden_size=96, intermediate_size=384), p, 1)
    with pytest.raises(ValueError, match="text tower"):
        pkg.convert.convert_hf_text_model(transformers.CLIPVisionModel(transformers.CLIPVisionConfig(hidden_size=64, intermediate_size=256, num_hidden_layers=1,
                                                                                                 num_attention_heads=2, image_size=32, patch_size=16)), p, 1)
    with pytest.raises(ValueError, match="convert_hf_text_model"):
        pkg.convert.convert_hf_model(mk(), p, 1)                              # the image path refuses a text tower by name
    assert pkg.convert.FAMILIES["clip_text_model"].name == "CLIP text" and pkg.convert.FAMILIES["siglip_text_model"].name == "SigLIP text"


def test_loader_errors(pkg, binding, tmp_path):
    """VITX_ERR_FORMAT: a wrong shape, a missing block tensor, a missing arch, eos >= V, causal or kind outside its enum."""
    t = PD.file_tensors(pkg, TD.text_file(pkg, "clip", ftype=0))
    V, D = t["token_embed.weight"].shape
    T, E = t["pos_embed"].shape[0], t["head.weight"].shape[0]
    hp = pkg.ggml_file.HParams(D, 2, 2, E, 0, T, 0)

    def load(tensors, name):
        p = str(tmp_path / f"{name}.gguf")
        pkg.ggml_file.write_model(p, hp, tensors, id2label={}, ftype=0)
        return binding.Model(p)

    load(t, "good").close()
    arch = lambda *a: np.array(a, np.float32)
    bad = {
        "pos_rows": {**t, "pos_embed": t["pos_embed"][:-1]},
        "tok_width": {**t, "token_embed.weight": t["token_embed.weight"][:, :-8]},
        "head_width": {**t, "head.weight": np.concatenate([t["head.weight"]] * 2, 1)},          # [E][2 D]: the pooled head of image files
        "missing_block": {k: v for k, v in t.items() if k != "blocks.1.mlp.fc1.bias"},
        "missing_arch": {k: v for k, v in t.items() if k != "arch"},
        "missing_tok": {k: v for k, v in t.items() if k != "token_embed.weight"},
        "eos_ge_V": {**t, "arch": arch(2, 1e-5, 1, V + 1)},
        "eos_fraction": {**t, "arch": arch(2, 1e-5, 1, 3.5)},
        "causal_2": {**t, "arch": arch(2, 1e-5, 2, 96)},
        "zs_kind_2": {"arch": t["arch"], "zs": arch(2, 100, 0, 0), **{k: v for k, v in t.items() if k != "arch"}},
        "zs_slot": {"arch": t["arch"], "zs": arch(0, 100, 0, 1), **{k: v for k, v in t.items() if k != "arch"}},
        "cls_token": {**t, "cls_token": np.zeros((1, 1, D), np.float32)},
    }
    for name, tensors in bad.items():
        with pytest.raises(binding.VitxError) as ei:
            load(tensors, name)
        assert ei.value.code == binding.ERR_FORMAT, (name, str(ei.value))
    ok = load({"arch": t["arch"], "zs": arch(1, 112, -12.5, 0), **{k: v for k, v in t.items() if k != "arch"}}, "zs_ok")
    assert ok.text_zs == (1, 112.0, -12.5)
    ok.close()
    # an image file keeps its rule: the last two arch slots are reserved
    ipath = Z.model_file(pkg, "clip")
    img = PD.file_tensors(pkg, ipath)
    img["patch_embed.proj.bias"] = img["patch_embed.proj.bias"].reshape(-1)          # (the file holds it as [1][D][1][1]; write_model reshapes it itself)
    p = str(tmp_path / "img_arch.gguf")
    pkg.ggml_file.write_model(p, pkg.ggml_file.read_model(ipath).hparams, {**img, "arch": np.array([img["arch"][0], img["arch"][1], 1, 0], np.float32)}, ftype=1)
    with pytest.raises(binding.VitxError) as ei:
        binding.Model(p)
    assert ei.value.code == binding.ERR_FORMAT and b"reserved" in binding.lib().vitx_last_error()


def test_argument_errors_without_a_device(pkg, binding, tmp_path):
    """Everything of vitx_text_* and the image entry points that is refused before a device call."""
    L = binding.lib()
    tp = TD.text_file(pkg, "clip")
    text, image = binding.Model(tp), binding.Model(Z.model_file(pkg, "clip"))
    h = C.c_void_p()
    assert L.vitx_text_create(image._h, 0, 4, binding.F16, C.byref(h)) == binding.ERR_ARG and not h
    assert L.vitx_text_create(text._h, 0, 0, binding.F16, C.byref(h)) == binding.ERR_ARG
    assert L.vitx_text_create(text._h, 0, 4, 7, C.byref(h)) == binding.ERR_ARG
    assert L.vitx_text_create(text._h, 0, 4, binding.MXFP8, C.byref(h)) == binding.ERR_UNSUPPORTED and not h
    assert L.vitx_text_create(None, 0, 4, binding.F16, C.byref(h)) == binding.ERR_ARG
    assert L.vitx_ctx_create(text._h, 0, 1, binding.F16, C.byref(h)) == binding.ERR_ARG and b"text" in L.vitx_last_error()
    dev = (C.c_int * 1)(0)
    assert L.vitx_group_create(text._h, dev, 1, 1, binding.F16, C.byref(h)) == binding.ERR_ARG
    with pytest.raises(binding.VitxError) as ei:
        binding.resize_file(tp, str(tmp_path / "r.gguf"), 32)
    assert ei.value.code == binding.ERR_ARG
    t = PD.file_tensors(pkg, tp)
    for name, change in (("T129", dict(T=129)), ("hd136", dict(D=272))):
        p = str(tmp_path / f"{name}.gguf")
        TD.write_variant(pkg, t, p, **change)
        m = binding.Model(p)
        assert L.vitx_text_create(m._h, 0, 4, binding.F16, C.byref(h)) == binding.ERR_UNSUPPORTED and not h, name
        m.close()
    ids = (C.c_int32 * 24)()
    out = (C.c_float * 64)()
    assert L.vitx_text_embed(None, ids, 1, 0, out) == binding.ERR_ARG
    assert L.vitx_text_embed_device(None, ids, 1, 0, 4096, None) == binding.ERR_ARG
    assert L.vitx_text_shares_weights(None) == 0
    L.vitx_text_free(None)
    p = 4096
    for call in (lambda: binding.op_attention_text(0, 0, p, 1, 8, 64, 1, True), lambda: binding.op_attention_text(2, p, p, 1, 8, 64, 1, True),
                 lambda: binding.op_text_embed(True, p, p, p, p, 1, 8, 60), lambda: binding.op_text_embed(True, p + 2, p, p, p, 1, 8, 64),
                 lambda: binding.op_text_pool(0, p, 0, p, p, p, 1, 8, 64)):
        with pytest.raises(binding.VitxError) as ei:
            call()
        assert ei.value.code == binding.ERR_ARG
    for call in (lambda: binding.op_attention_text(0, p, p, 1, 129, 64, 1, True), lambda: binding.op_attention_text(0, p, p, 1, 8, 136, 1, True),
                 lambda: binding.op_attention_text(0, p, p, 1, 8, 68, 1, False), lambda: binding.op_text_pool(0, p, p, p, p, p, 1, 8, 96)):
        with pytest.raises(binding.VitxError) as ei:
            call()
        assert ei.value.code == binding.ERR_UNSUPPORTED
    text.close(); image.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_quantize_copies_the_front_byte_for_byte(pkg, binding, family, tmp_path):
    src, dst = TD.text_file(pkg, family), str(tmp_path / "q8.gguf")
    binding.quantize_file(src, dst, 8)
    a, b = pkg.ggml_file.read_model(src), pkg.ggml_file.read_model(dst)
    ta, tb = {t.name: t for t in a.tensors}, {t.name: t for t in b.tensors}
    assert list(ta) == list(tb)
    for name in ("token_embed.weight", "pos_embed", "arch"):
        assert ta[name].ttype == tb[name].ttype and bytes(ta[name].raw) == bytes(tb[name].raw), name
    for name in ("blocks.0.attn.qkv.weight", "blocks.1.attn.proj.weight", "blocks.0.mlp.fc1.weight", "blocks.1.mlp.fc2.weight", "head.weight"):
        assert tb[name].ttype == 8 and ta[name].ttype == 1, name
    m = binding.Model(dst)
    assert m.kind == binding.KIND_TEXT and m.text_info == binding.Model(src).text_info
    # the converter's own quantised file selects the same tensors
    p2 = str(tmp_path / "conv_q8.gguf")
    pkg.convert.convert_hf_text_model(TD.hf_model(family), p2, 8)
    tc = {t.name: t.ttype for t in pkg.ggml_file.read_model(p2).tensors}
    assert tc == {n: t.ttype for n, t in tb.items()}


# ------------------------------------------------------------------------------------------------ conditions of the GPU data
@pytest.mark.parametrize("case", TD.ATTN_CASES, ids=TD.case_id)
def test_staircase_conditions(case):
    """The expected value is exact: representable in bf16 and fp16, and what the schedule gives (partial sums (t + 1)^2 u exact in f32, the product
    with fl(1 / (t + 1)) rounded to the output type is (t + 1) u).  One leaked future key and one dropped past key each move the row by at least two output ulps."""
    import torch
    n, T, H, hd = case
    for sign in X.FLAT_SIGNS:
        qkv, u = TD.staircase_qkv(n, T, H, hd, sign, X.attn_seed(n, T, H, hd) + 17 * sign)
        for tdt in (torch.float16, torch.bfloat16):
            assert torch.equal(torch.from_numpy(qkv).to(tdt).float(), torch.from_numpy(qkv))                  # the operands are exact in both types
        s = qkv.reshape(n, T, 3, H, hd)
        raw = np.einsum("nthd,njhd->nhtj", s[:, :, 0].astype(np.float64), s[:, :, 1].astype(np.float64))
        assert (raw == raw[..., :1]).all()                                                                     # every score of a row is the same number
        for causal in (True, False):
            want = TD.staircase_expected(u, T, causal)
            for tdt in (torch.float16, torch.bfloat16):
                assert torch.equal(torch.from_numpy(want).to(tdt).float(), torch.from_numpy(want))
            got = TD.staircase_f32(qkv, n, T, H, hd, causal)
            # the f32 product (t + 1)^2 u * fl(1 / (t + 1)) may lie one f32 ulp beside (t + 1) u (225 * fl(1 / 15) = 15.000001): 2^-23 relative, far
            # inside half an output ulp (2^-9 / 2^-12) of a value of at most 8 significant bits -- the rounding to the output type returns it exactly
            assert (np.abs(got - want) <= np.abs(want) * 2.0 ** -23).all()
            for tdt in (torch.float16, torch.bfloat16):
                assert torch.equal(torch.from_numpy(got).to(tdt).float(), torch.from_numpy(want))
            x = qkv.astype(np.float64).reshape(n, T, 3, H, hd)
            w = np.tril(np.ones((T, T))) if causal else np.ones((T, T))
            assert np.array_equal(np.einsum("tj,njhd->nthd", w / w.sum(1, keepdims=True), x[:, :, 2]).reshape(n * T, H * hd).astype(np.float32), want)
        if T >= 3:
            t = T // 2
            want = TD.staircase_expected(u, T, True).reshape(n, T, H * hd)[:, t]
            ulp = AD.ulp_T(want, 1)                                                                              # one bf16 ulp of the row (the coarser type)
            for fault in (dict(leak=(t, t + 1)), dict(drop=(t, 0)), dict(drop=(t, t))):
                got = TD.staircase_f32(qkv, n, T, H, hd, True, **fault).reshape(n, T, H * hd)
                assert (np.abs(got[:, t] - want) >= 2 * ulp).all(), fault
                rest = lambda a: torch.from_numpy(np.delete(a, t, 1)).to(torch.float16).float()
                assert torch.equal(rest(got), rest(TD.staircase_expected(u, T, True).reshape(n, T, H * hd)))            # every other row is untouched


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "nomask"])
@pytest.mark.parametrize("case", [c for c in TD.ATTN_CASES if c[1] >= X.SPREAD_MIN_N], ids=TD.case_id)
def test_spread_conditions(case, causal, dtype_name):
    """On every spread / peaked case the emulation stays below half of the bound, and one leaked future key, one dropped past key and a 2 % scale
    error each break a gate."""
    import torch
    n, T, H, hd = case
    tdt = torch.float16 if dtype_name == "f16" else torch.bfloat16
    scale = 1.0 / np.sqrt(hd)
    for kind in X.spread_kinds(T):
        x = torch.from_numpy(X.spread_qkv(n, T, H, hd, X.attn_seed(n, T, H, hd), kind))
        q, k, v = X.heads_of(x.to(tdt).float(), n, T, H, hd)
        ref, cond = TD.masked_ref(q, k, v, scale, causal, want_bound=True)
        bound = X.attention_bound(ref, cond, dtype_name)
        emu = TD.masked_emu(q, k, v, scale, dtype_name, causal)
        worst, mean = X.attention_gate_ratios(emu, ref, bound, emu)
        assert worst <= 0.5 and mean == 1.0, (kind, worst)
        for fault, out in TD.masked_faults(q, k, v, scale, causal, n, H).items():
            w, m = X.attention_gate_ratios(out, ref, bound, emu)
            assert w > 1.0 or m > X.ATTN_MEAN_FACTOR, f"{case} {kind} {dtype_name}: fault '{fault}' passes both gates ({w:.2f}, {m:.2f})"


@pytest.mark.parametrize("family", FAMILIES)
def test_zero_shot_margins_of_the_restatement(pkg, family):
    """The condition of the GPU zero-shot test, on the float64 restatement alone: at least half of the 17 images have a top-2 margin above twice
    zs_data.COS_BOUND * scale, both operand types."""
    t = PD.file_tensors(pkg, TD.text_file(pkg, family))
    r64 = TD.forward64(t, TD.prompts(family))
    kind, scale, bias = TD.zs_constants(family)
    emb = Z.embedding64(pkg, family)
    assert emb.shape[1] == r64.shape[1]
    r = Z.restate(Z.normalise64(emb), TD.bank64(r64, TD.zs_groups()), kind, scale, bias)
    top, mar = Z.margins(r["logits"])
    for dtype in (0, 1):
        need = 2 * Z.COS_BOUND[dtype](emb.shape[1]) * scale
        print(f"{family} dtype {dtype}: margins {np.sort(mar)[:3]} .. {mar.max():.3f}, needed {need:.3f}: {(mar > need).sum()} of {len(mar)}")
        assert (mar > need).sum() * 2 >= Z.N_IMAGES


def test_text_bank_rule_is_zeroshot_banks(pkg):
    """text_data.bank64 (what the GPU test compares binding.text_bank with) is convert.zeroshot_bank's ensembling"""
    e = np.random.default_rng(0).standard_normal((17, 64))
    g = TD.zs_groups()
    b = TD.bank64(e, g)
    en = Z.normalise64(e)
    for k in range(int(g.max()) + 1):
        mean = en[g == k].mean(0)
        assert np.abs(b[k] - mean / np.linalg.norm(mean)).max() < 1e-15


def test_command_line_arguments(pkg):
    """vit_cli.py and convert.py refuse inconsistent text options while parsing: no model is loaded, no device touched."""
    from vitcpp_amd import cli
    a = cli.make_parser().parse_args(["-m", "clip.gguf", "-i", "x.jpg", "--text-model", "t.gguf", "--zero-shot-ids", "ids.npy", "--zero-shot-labels", "l.txt", "--text-embed", "e.npy"])
    assert (a.text_model, a.zero_shot_ids, a.zero_shot_labels, a.text_embed) == ("t.gguf", "ids.npy", "l.txt", "e.npy")
    for argv in (["--text-model", "t.gguf"], ["--zero-shot-ids", "i.npy"], ["--zero-shot-labels", "l.txt"], ["--text-embed", "e.npy"],
                 ["--text-model", "t.gguf", "--zero-shot-ids", "i.npy", "--zero-shot", "b.npz"], ["--text-model", "t.gguf", "--zero-shot-ids", "i.npy", "--dir", "d"],
                 ["--text-model", "t.gguf", "--zero-shot-ids", "i.npy", "--dtype", "mxfp8"]):
        with pytest.raises(SystemExit) as ei:
            cli.main(argv)
        assert ei.value.code == 2, argv
    with pytest.raises(SystemExit) as ei:
        pkg.convert.main(["m.pth", "o.gguf", "--timm-state-dict", "--text-out", "t.gguf"])
    assert ei.value.code == 2


def test_id_checks_on_the_host(pkg, binding):
    """Every VITX_ERR_ARG of vitx_text_embed about its ids, through vitx_text_check_ids -- the host function vitx_text_embed and
    vitx_text_embed_device call before their first device call: an id < 0, an id >= V (both at the first and the last position, in the first and
    the last prompt), a row without EOS in a file with eos; and the pooled positions: the FIRST EOS of a CLIP row, T - 1 of a SigLIP row."""
    L = binding.lib()
    i32p = C.POINTER(C.c_int32)
    for family in FAMILIES:
        m = binding.Model(TD.text_file(pkg, family))
        info = m.text_info
        V, T, eos = info["vocab"], info["tokens"], info["eos"]
        ids = TD.prompts(family)
        want = TD.pooled_positions(ids, eos)
        assert np.array_equal(binding.text_check_ids(m, ids), want)
        assert np.array_equal(binding.text_check_ids(m, ids[3:4]), want[3:4])
        assert L.vitx_text_check_ids(m._h, ids.ctypes.data_as(i32p), len(ids), None) == 0                   # pooled may be NULL
        if family == "clip":
            twice = ids.copy(); twice[0, 7] = eos                                                           # a second EOS behind the first changes nothing
            assert binding.text_check_ids(m, twice)[0] == 5
        bad = []
        for row in (0, len(ids) - 1):
            for col in (0, T - 1):
                for val in (-1, V, V + 1000, -2 ** 31, 2 ** 31 - 1):
                    x = ids.copy(); x[row, col] = val
                    bad.append(x)
        if eos >= 0:
            for row in (0, 8, len(ids) - 1):
                x = ids.copy(); x[row][x[row] == eos] = 1
                bad.append(x)
        for x in bad:
            with pytest.raises(binding.VitxError) as ei:
                binding.text_check_ids(m, x)
            assert ei.value.code == binding.ERR_ARG
        edge = ids.copy(); edge[0, 0] = 0; edge[1, 1] = V - 1 if eos < 0 else V - 2                        # 0 and the largest id are fine
        binding.text_check_ids(m, edge)
        assert L.vitx_text_check_ids(m._h, ids.ctypes.data_as(i32p), 0, None) == binding.ERR_ARG
        assert L.vitx_text_check_ids(m._h, None, 1, None) == binding.ERR_ARG
        assert L.vitx_text_check_ids(None, ids.ctypes.data_as(i32p), 1, None) == binding.ERR_ARG
        m.close()
    img = binding.Model(Z.model_file(pkg, "clip"))
    x = np.zeros((1, 24), np.int32)
    assert L.vitx_text_check_ids(img._h, x.ctypes.data_as(i32p), 1, None) == binding.ERR_ARG
    img.close()


def test_layernorm_widths_are_the_kernels_table(pkg):
    """convert.LN_WIDTHS (what convert_hf_text_model refuses by) is VITX_LN_WIDTHS of kernels.h, read out of the header; exact_data's copy too."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(pkg.convert.__file__), "csrc", "kernels.h")).read()
    body = src[src.index("#define VITX_LN_WIDTHS(X)"):]
    body = body[:body.index("// The table's one dispatcher")]
    widths = [int(w) for w in re.findall(r"X\((\d+), \d+, \d+\)", body)]
    assert len(widths) == 19 and sorted(widths) == sorted(pkg.convert.LN_WIDTHS) == sorted(X.LN_WIDTHS)
    assert pkg.convert.TEXT_MAX_TOKENS == int(re.search(r"#define VITX_TEXT_MAX_TOKENS (\d+)", open(os.path.join(os.path.dirname(pkg.convert.__file__), "..", "include", "vitx.h")).read()).group(1))


@pytest.mark.parametrize("family", FAMILIES)
def test_quantize_copies_zs_byte_for_byte(pkg, binding, family, tmp_path):
    """A two-tower model's text file carries `zs`: vitx_quantize_file copies it, with the token table, pos_embed and arch, byte for byte."""
    src, dst = str(tmp_path / "t.gguf"), str(tmp_path / "q.gguf")
    pkg.convert.convert_hf_text_model(_two_towers(family), src, 1)
    binding.quantize_file(src, dst, 2)
    ta = {t.name: t for t in pkg.ggml_file.read_model(src).tensors}
    tb = {t.name: t for t in pkg.ggml_file.read_model(dst).tensors}
    assert list(ta) == list(tb) and "zs" in ta
    for name in ("zs", "arch", "token_embed.weight", "pos_embed"):
        assert ta[name].ttype == tb[name].ttype and bytes(ta[name].raw) == bytes(tb[name].raw), name
    assert tb["head.weight"].ttype == 2 and tb["blocks.0.attn.qkv.weight"].ttype == 2
    a, b = binding.Model(src), binding.Model(dst)
    assert a.text_zs == b.text_zs and a.text_zs is not None and a.text_info == b.text_info
    a.close(); b.close()
