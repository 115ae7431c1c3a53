"""Zero-shot classification without a GPU: tests/zs_data.py's restatement and convert.zeroshot_bank pinned to transformers' CLIPModel and
SiglipModel in float64, prompt ensembling, the bank file, the command lines, the end-to-end fixtures' margins, and the argument errors of the C
ABI that need no device."""
import ctypes as C

import numpy as np
import pytest

import zs_data as Z


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _tiny(family):
    import torch
    import transformers
    torch.manual_seed(7 if family == "clip" else 8)
    if family == "clip":
        cfg = transformers.CLIPConfig(
            text_config=dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, vocab_size=100, max_position_embeddings=16,
                             eos_token_id=99, bos_token_id=98, pad_token_id=0),
            vision_config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, image_size=32, patch_size=16), projection_dim=64)
        m = transformers.CLIPModel(cfg)
    else:
        cfg = transformers.SiglipConfig(
            text_config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, vocab_size=100, max_position_embeddings=8),
            vision_config=dict(hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=32, patch_size=16))
        m = transformers.SiglipModel(cfg)
        with torch.no_grad():              # the released values' order of magnitude; a fresh model has 0 and 0
            m.logit_scale.fill_(float(np.log(112.0))); m.logit_bias.fill_(-12.5)
    m = m.double().eval()
    T = 16 if family == "clip" else 8
    ids = torch.randint(1, 97, (6, T))
    if family == "clip":
        ids[:, -1] = 99                    # CLIP pools at the end-of-text token
    pv = torch.randn(5, 3, 32, 32, dtype=torch.float64)
    return torch, m, ids, pv


@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_restatement_and_bank_against_transformers(pkg, family):
    """Fed the model's own image_embeds and OUR bank, the restatement gives transformers' logits_per_image and softmax / sigmoid of it to 1e-10
    relative: both sides are float64 and a few thousand operations."""
    torch, m, ids, pv = _tiny(family)
    with torch.no_grad():
        out = m(input_ids=ids, pixel_values=pv)
    embeds, kind, scale, bias = pkg.convert.zeroshot_bank(m, ids.numpy())
    assert embeds.shape == (6, 64) and embeds.dtype == np.float64
    assert np.abs(np.linalg.norm(embeds, axis=1) - 1).max() < 1e-14
    assert kind == (Z.SOFTMAX if family == "clip" else Z.SIGMOID)
    assert scale == pytest.approx(float(m.logit_scale.detach().exp().reshape(-1)[0]), rel=1e-14) and bias == (0.0 if family == "clip" else -12.5)
    assert _rel(embeds, out.text_embeds.numpy()) < 1e-12
    cos = Z.normalise64(out.image_embeds.numpy()) @ embeds.T
    logits = cos * scale + bias                                    # restate() rounds scale and bias to f32, as the C ABI takes them: not here
    want = out.logits_per_image.numpy()
    assert want.shape == (5, 6) and np.ptp(want) > 0.05
    r_l = _rel(logits, want)
    ref_p = torch.softmax(out.logits_per_image, dim=-1) if family == "clip" else torch.sigmoid(out.logits_per_image)
    r_p = _rel(Z.probs64(logits, kind), ref_p.numpy())
    print(f"{family}: logits {r_l:.2e}, probabilities {r_p:.2e} relative")
    assert r_l < 1e-10 and r_p < 1e-10
    # restate() itself, with an f32-exact scale and bias
    r = Z.restate(Z.normalise64(out.image_embeds.numpy()), embeds, kind, np.float32(scale), np.float32(bias))
    assert _rel(r["logits"], cos * float(np.float32(scale)) + float(np.float32(bias))) < 1e-15


@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_prompt_ensembles_are_mean_then_renormalise(pkg, family):
    torch, m, ids, _ = _tiny(family)
    single, kind, scale, bias = pkg.convert.zeroshot_bank(m, ids.numpy())
    groups = [0, 2, 2, 1, 0, 2]
    ens, kind2, scale2, bias2 = pkg.convert.zeroshot_bank(m, ids.numpy(), groups=groups)
    assert ens.shape == (3, 64) and (kind2, scale2, bias2) == (kind, scale, bias)
    for k in range(3):
        mean = single[[i for i, g in enumerate(groups) if g == k]].mean(0)
        assert np.abs(ens[k] - mean / np.linalg.norm(mean)).max() < 1e-15
    assert np.abs(np.linalg.norm(ens, axis=1) - 1).max() < 1e-14
    assert np.abs(ens[1] - single[3]).max() < 1e-15                 # a class of one prompt is that prompt
    with pytest.raises(ValueError):
        pkg.convert.zeroshot_bank(m, ids.numpy(), groups=[0, 0, 0, 2, 2, 2])       # class 1 has no prompt
    with pytest.raises(ValueError):
        pkg.convert.zeroshot_bank(m.vision_model, ids.numpy())                     # a tower alone has no text side


def test_attention_mask_reaches_the_text_tower(pkg):
    torch, m, ids, _ = _tiny("clip")
    mask = np.ones(ids.shape, np.int64); mask[:, :3] = 0
    a = pkg.convert.zeroshot_bank(m, ids.numpy())[0]
    b = pkg.convert.zeroshot_bank(m, ids.numpy(), attention_mask=mask)[0]
    with torch.no_grad():
        want = m(input_ids=ids, attention_mask=torch.from_numpy(mask), pixel_values=torch.zeros(1, 3, 32, 32, dtype=torch.float64)).text_embeds.numpy()
    assert _rel(b, want) < 1e-12 and np.abs(a - b).max() > 1e-4


def test_bank_file_round_trip(pkg, tmp_path):
    rng = np.random.default_rng(3)
    e = Z.unit_rows(rng.standard_normal((5, 64)))
    path = str(tmp_path / "bank.npz")
    pkg.convert.save_bank(path, e.astype(np.float64), Z.SIGMOID, 112.5, -12.25, labels=["a cat", "a dog", "naïve café", "x", "y"])
    b = pkg.convert.load_bank(path)
    assert b["embeds"].dtype == np.float32 and np.array_equal(b["embeds"], e)
    assert b["labels"] == ["a cat", "a dog", "naïve café", "x", "y"] and (b["kind"], b["scale"], b["bias"]) == (Z.SIGMOID, 112.5, -12.25)
    pkg.convert.save_bank(path, e, Z.SOFTMAX, 100.0, 0.0)
    assert pkg.convert.load_bank(path)["labels"] == [f"class_{k}" for k in range(5)]
    with pytest.raises(ValueError):
        pkg.convert.save_bank(path, e, Z.SOFTMAX, 100.0, 0.0, labels=["too", "few"])
    other = str(tmp_path / "other.npz")
    np.savez(other, embeds=e)
    with pytest.raises(ValueError, match="labels"):
        pkg.convert.load_bank(other)


def test_vit_cli_arguments(pkg, tmp_path):
    from vitcpp_amd import cli
    ap = cli.make_parser()
    a = ap.parse_args(["-m", "clip.gguf", "-i", "image.jpg", "-k", "5", "--zero-shot", "bank.npz"])
    assert (a.model, a.inp, a.topk, a.zero_shot, a.dir) == ("clip.gguf", "image.jpg", 5, "bank.npz", None)
    assert ap.parse_args(["-m", "m.gguf"]).zero_shot is None
    with pytest.raises(SystemExit) as ei:                           # refused while parsing: no model is loaded, no device touched
        cli.main(["-m", "m.gguf", "--dir", "d", "--zero-shot", "bank.npz"])
    assert ei.value.code == 2


def test_convert_arguments(pkg):
    for argv in (["m", "o.gguf", "--zero-shot-ids", "ids.npy"],                               # no --zero-shot-out
                 ["m", "o.gguf", "--zero-shot-out", "b.npz"],                                 # nothing to make it from
                 ["m", "o.gguf", "--zero-shot-out", "b.npz", "--zero-shot-ids", "i.npy", "--zero-shot-prompts", "p.txt"],
                 ["m.pth", "o.gguf", "--timm-state-dict", "--zero-shot-ids", "i.npy", "--zero-shot-out", "b.npz"]):
        with pytest.raises(SystemExit) as ei:
            pkg.convert.main(argv)
        assert ei.value.code == 2, argv


@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_fixture_margins(pkg, family):
    """The end-to-end test compares top-1 only where the restatement's top-2 margin exceeds twice the logit bound: at least 3 of every 4 images
    must have such a margin, both operand types -- here on the files' float64 embeddings (the GPU test asserts it again on the engine's own)."""
    emb = Z.embedding64(pkg, family)
    t, kind, scale, bias = Z.bank(family, emb)
    assert t.shape == (Z.BANK_K, emb.shape[1]) and np.abs(np.linalg.norm(t.astype(np.float64), axis=1) - 1).max() < 1e-7
    r = Z.restate(Z.normalise64(emb), t, kind, scale, bias)
    top, mar = Z.margins(r["logits"])
    for dtype in (0, 1):
        need = 2 * Z.COS_BOUND[dtype](emb.shape[1]) * scale
        frac = float((mar > need).mean())
        print(f"{family} dtype {dtype}: margins {mar.min():.3f} .. {mar.max():.3f} logits, needed {need:.3f}: {frac:.2f} of the images; {len(set(top.tolist()))} distinct top-1 classes")
        assert frac >= 0.75
    if family == "siglip":
        assert len(set(top.tolist())) == Z.N_IMAGES


def test_device_operand_is_the_f32_rule():
    """device_operand(): exact on the kernel test's data (z = +-2^k: ss = E 4^k, a = +-1/sqrt(E) exactly), zero stays zero, and within f32 rounding
    of the float64 rule on random rows."""
    rng = np.random.default_rng(1)
    sign = rng.choice([-1.0, 1.0], (4, 64)).astype(np.float32)
    for k in (-20, 0, 7, 40):
        z = sign * np.float32(2.0 ** k)
        assert np.array_equal(Z.device_sumsq(z), np.full(4, 64 * 4.0 ** k, np.float32))
        for dtype in (0, 1):
            assert np.array_equal(Z.device_operand(z, dtype), sign / 8)
    assert not Z.device_operand(np.zeros((2, 128), np.float32), 1).any()
    z = rng.standard_normal((6, 512)).astype(np.float32)
    assert np.abs(Z.device_sumsq(z) / (z.astype(np.float64) ** 2).sum(1) - 1).max() < 512 * 2.0 ** -24
    for dtype, u in ((0, 2.0 ** -11), (1, 2.0 ** -8)):
        a, want = Z.device_operand(z, dtype).astype(np.float64), Z.normalise64(z)
        tol = np.maximum(np.abs(want), 2.0 ** -14 if dtype == 0 else 0) * u * 1.001 + (2.0 ** -25 if dtype == 0 else 0) + 1e-9
        assert (np.abs(a - want) <= tol).all()


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_errors_that_need_no_device(binding):
    """vitx_zeroshot_* on a NULL context and every argument error of vitx_op_zeroshot: all raised before any device call."""
    L = binding.lib()
    fp = C.POINTER(C.c_float)
    bank = (C.c_float * 64)(*([0.125] * 64))
    assert L.vitx_zeroshot_set(None, bank, 1, 64, 0, 1.0, 0.0) == binding.ERR_ARG
    assert L.vitx_zeroshot_read(None, bank, None, 64) == binding.ERR_ARG
    assert L.vitx_zeroshot_classes(None) == 0 and L.vitx_zeroshot_images(None) == 0 and L.vitx_zeroshot_device(None) is None
    assert binding.zeroshot_max_classes(512) == 0xf0000000 // 1024 and binding.zeroshot_max_classes(512) % 128 == 0
    assert binding.zeroshot_max_classes(64) == 0xf0000000 // 128 and binding.zeroshot_max_classes(100) == 0 and binding.zeroshot_max_classes(0) == 0
    p = 4096                                    # a pointer that is never followed
    ok = dict(dtype=1, d_z=p, z_stride=64, d_bank=p, d_a=p, d_acc=p, d_probs=p, d_logits=p, n=1, K=1, E=64, kind=0, scale=2.0, bias=0.0)
    cases = [(dict(d_z=0), binding.ERR_ARG), (dict(d_bank=0), binding.ERR_ARG), (dict(d_a=0), binding.ERR_ARG), (dict(d_acc=0), binding.ERR_ARG),
             (dict(d_probs=0), binding.ERR_ARG), (dict(d_logits=0), binding.ERR_ARG), (dict(n=0), binding.ERR_ARG), (dict(K=0), binding.ERR_ARG),
             (dict(dtype=2), binding.ERR_ARG), (dict(kind=2), binding.ERR_ARG), (dict(kind=-1), binding.ERR_ARG),
             (dict(scale=float("inf")), binding.ERR_ARG), (dict(scale=float("nan")), binding.ERR_ARG), (dict(bias=float("-inf")), binding.ERR_ARG),
             (dict(z_stride=60), binding.ERR_ARG), (dict(z_stride=66), binding.ERR_ARG), (dict(d_z=p + 4), binding.ERR_ARG), (dict(d_bank=p + 8), binding.ERR_ARG),
             (dict(E=96, z_stride=96), binding.ERR_UNSUPPORTED), (dict(E=32, z_stride=32), binding.ERR_UNSUPPORTED),
             (dict(K=binding.zeroshot_max_classes(64) + 1), binding.ERR_UNSUPPORTED)]
    for change, code in cases:
        with pytest.raises(binding.VitxError) as ei:
            binding.op_zeroshot(**{**ok, **change})
        assert ei.value.code == code, (change, str(ei.value))
