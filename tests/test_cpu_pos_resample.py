"""Position-embedding resampling on the host (vitx_pos_embed_resample, vitx_model_resize_file; the contract: include/vitx.h).

  1. the resampler against CPU torch F.interpolate in float64, both conventions, under the gate torch's own f32 error sets
     (tests/resolution_data.py), and far from the other convention;
  2. vitx_model_resize_file: only the header's img_size and pos_embed change, f16 and q4_0 files, errors;
  3. an independent end-to-end pin of the BICUBIC convention: the oracle on resized files against HuggingFace ViT called with
     interpolate_pos_encoding=True on the 64^2 weights;
  4. ABI: exports, and a vitx_ctx_options of the size it had before img_size / pos_interp were appended."""
import ctypes
import os

import numpy as np
import pytest

import resolution_data as RD

ERR_IO, ERR_ARG, ERR_HIP, ERR_UNSUPPORTED = 1, 3, 4, 5
MICRO = "vit_micro_patch16_64"


# ------------------------------------------------------------------------------------------------ 1. the resampler
@pytest.mark.parametrize("D", RD.WIDTHS)
@pytest.mark.parametrize("case", RD.CASES, ids=RD.case_id)
@pytest.mark.parametrize("interp", [RD.BICUBIC, RD.BICUBIC_AA], ids=["bicubic", "bicubic_aa"])
def test_host_resampler_matches_torch_float64(binding, interp, case, D):
    grid_in, grid_out = case
    pos = RD.table(grid_in, D)
    ours = binding.pos_embed_resample(pos, grid_out, interp, grid_in)
    RD.check_against_torch(ours, pos, grid_in, grid_out, interp, "host")


@pytest.mark.parametrize("D", RD.WIDTHS)
@pytest.mark.parametrize("interp", [RD.BICUBIC, RD.BICUBIC_AA])
def test_equal_grids_are_an_exact_copy(binding, interp, D):
    grid_in, grid_out = RD.IDENTITY
    pos = RD.table(grid_in, D)
    assert RD.bits_equal(binding.pos_embed_resample(pos, grid_out, interp, grid_in), pos)


def test_resampler_argument_errors(binding):
    L = binding.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    pos = RD.table((4, 4), 8)
    out = np.zeros((1 + 36, 8), np.float32)
    p, o = pos.ctypes.data_as(fp), out.ctypes.data_as(fp)
    assert L.vitx_pos_embed_resample(p, 4, 4, 8, 6, 6, 0, o) == 0
    assert L.vitx_pos_embed_resample(None, 4, 4, 8, 6, 6, 0, o) == ERR_ARG
    assert L.vitx_pos_embed_resample(p, 4, 4, 8, 6, 6, 0, None) == ERR_ARG
    for args in ((0, 4, 8, 6, 6), (4, -1, 8, 6, 6), (4, 4, 0, 6, 6), (4, 4, 8, 0, 6), (4, 4, 8, 6, -3)):
        assert L.vitx_pos_embed_resample(p, *args, 0, o) == ERR_ARG, args
    for interp in (-1, 2, 7):
        assert L.vitx_pos_embed_resample(p, 4, 4, 8, 6, 6, interp, o) == ERR_ARG, interp
    with pytest.raises(binding.VitxError):
        binding.pos_embed_resample(pos, 6, 2)


# ------------------------------------------------------------------------------------------------ 2. the file
def _tensors(pkg, path):
    mf = pkg.ggml_file.read_model(path)
    return mf, {t.name: t for t in mf.tensors}


def _pos_of(rec):
    return np.frombuffer(rec.raw, np.float32).reshape(rec.ne[1], rec.ne[0])


@pytest.mark.parametrize("ftype", [1, 2], ids=["f16", "q4_0"])
@pytest.mark.parametrize("interp", [RD.BICUBIC, RD.BICUBIC_AA])
def test_resize_file_changes_img_size_and_pos_embed_only(pkg, binding, tmp_path, ftype, interp):
    src = pkg.synth.cached_synthetic(MICRO, head_scale=4.0)
    if ftype == 2:
        q = str(tmp_path / "micro_q4_0.gguf")
        binding.quantize_file(src, q, 2)
        src = q
    mf0, t0 = _tensors(pkg, src)
    pos0 = _pos_of(t0["pos_embed"])
    for S in (32, 96, 128):
        dst = str(tmp_path / f"micro_{S}.gguf")
        binding.resize_file(src, dst, S, interp)
        mf1, t1 = _tensors(pkg, dst)
        g = S // 16
        assert mf1.hparams.img_size == S
        assert [getattr(mf1.hparams, k) for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "num_classes", "patch_size", "ftype")] == \
               [getattr(mf0.hparams, k) for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "num_classes", "patch_size", "ftype")]
        assert mf1.id2label == mf0.id2label and list(mf1.id2label) == list(mf0.id2label)
        assert [t.name for t in mf1.tensors] == [t.name for t in mf0.tensors]
        for name, rec in t1.items():
            if name == "pos_embed":
                assert rec.ttype == 0 and tuple(rec.ne[:2]) == (128, g * g + 1) and len(rec.ne) == len(t0[name].ne)
                assert RD.bits_equal(_pos_of(rec), binding.pos_embed_resample(pos0, g, interp))
            else:
                assert (rec.ttype, tuple(rec.ne), bytes(rec.raw)) == (t0[name].ttype, tuple(t0[name].ne), bytes(t0[name].raw)), name
        m = binding.Model(dst)
        assert m.img_size == S and m.label(3) == binding.Model(src).label(3)
        m.close()
    # a resized file is an ordinary file: it resizes again, and back to its own size it is the same bytes
    again = str(tmp_path / "micro_again.gguf")
    binding.resize_file(str(tmp_path / "micro_96.gguf"), again, 48, interp)
    _, t2 = _tensors(pkg, again)
    assert RD.bits_equal(_pos_of(t2["pos_embed"]), binding.pos_embed_resample(_pos_of(_tensors(pkg, str(tmp_path / "micro_96.gguf"))[1]["pos_embed"]), 3, interp))
    same = str(tmp_path / "micro_same.gguf")
    binding.resize_file(src, same, 64, interp)
    assert open(same, "rb").read() == open(src, "rb").read()


def test_resize_file_errors(pkg, binding, tmp_path):
    L = binding.lib()
    src = pkg.synth.cached_synthetic(MICRO, head_scale=4.0).encode()
    dst = str(tmp_path / "out.gguf").encode()
    for S in (40, 1, 100):
        assert L.vitx_model_resize_file(src, dst, S, 0) == ERR_ARG, S
    for S in (0, -64):
        assert L.vitx_model_resize_file(src, dst, S, 0) == ERR_ARG, S
    assert L.vitx_model_resize_file(src, dst, 96, 2) == ERR_ARG
    assert L.vitx_model_resize_file(None, dst, 96, 0) == ERR_ARG and L.vitx_model_resize_file(src, None, 96, 0) == ERR_ARG
    assert L.vitx_model_resize_file(src, src, 96, 0) == ERR_ARG
    assert not os.path.exists(dst.decode())
    assert L.vitx_model_resize_file(str(tmp_path / "missing.gguf").encode(), dst, 96, 0) == ERR_IO
    vitstr = pkg.synth.cached_synthetic("vitstr_micro_patch16_64", head_scale=4.0).encode()
    assert L.vitx_model_resize_file(vitstr, dst, 96, 0) == ERR_UNSUPPORTED
    assert b"ViTSTR" in L.vitx_last_error()
    assert not os.path.exists(dst.decode())


# ------------------------------------------------------------------------------------------------ 3. HuggingFace pin
def _hf_micro(pkg):
    """HuggingFace ViTForImageClassification on the micro model's 64^2 weights (the mapping of test_cpu_oracle.test_oracle_vs_transformers_vit_f32)."""
    import torch
    import transformers as tr
    hp = pkg.synth.hparams_for(MICRO)
    w = pkg.synth.make_weights(hp, head_scale=4.0)
    def f16(x): return x.astype(np.float16).astype(np.float32)
    cfg = tr.ViTConfig(hidden_size=hp.hidden_size, num_hidden_layers=hp.num_hidden_layers, num_attention_heads=hp.num_attention_heads,
                       intermediate_size=4 * hp.hidden_size, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6, image_size=hp.img_size,
                       patch_size=hp.patch_size, num_labels=hp.num_classes, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, qkv_bias=True)
    m = tr.ViTForImageClassification(cfg).eval()
    D = hp.hidden_size
    sd = {"vit.embeddings.cls_token": w["cls_token"], "vit.embeddings.position_embeddings": w["pos_embed"],
          "vit.embeddings.patch_embeddings.projection.weight": f16(w["patch_embed.proj.weight"]),
          "vit.embeddings.patch_embeddings.projection.bias": w["patch_embed.proj.bias"]}
    new_names = "vit.layers.0.attention.q_proj.weight" in set(m.state_dict().keys())          # transformers >= 5 renamed the ViT sub-modules
    for i in range(hp.num_hidden_layers):
        p = f"blocks.{i}."
        q = f"vit.layers.{i}." if new_names else f"vit.encoder.layer.{i}."
        qkv_w, qkv_b = f16(w[p + "attn.qkv.weight"]), w[p + "attn.qkv.bias"]
        for j, nm in enumerate(("q_proj", "k_proj", "v_proj") if new_names else ("attention.query", "attention.key", "attention.value")):
            sd[q + f"attention.{nm}.weight"] = qkv_w[j * D:(j + 1) * D]
            sd[q + f"attention.{nm}.bias"] = qkv_b[j * D:(j + 1) * D]
        o = "attention.o_proj" if new_names else "attention.output.dense"
        f1 = "mlp.fc1" if new_names else "intermediate.dense"
        f2 = "mlp.fc2" if new_names else "output.dense"
        sd[q + o + ".weight"] = f16(w[p + "attn.proj.weight"]); sd[q + o + ".bias"] = w[p + "attn.proj.bias"]
        sd[q + "layernorm_before.weight"] = w[p + "norm1.weight"]; sd[q + "layernorm_before.bias"] = w[p + "norm1.bias"]
        sd[q + "layernorm_after.weight"] = w[p + "norm2.weight"]; sd[q + "layernorm_after.bias"] = w[p + "norm2.bias"]
        sd[q + f1 + ".weight"] = f16(w[p + "mlp.fc1.weight"]); sd[q + f1 + ".bias"] = w[p + "mlp.fc1.bias"]
        sd[q + f2 + ".weight"] = f16(w[p + "mlp.fc2.weight"]); sd[q + f2 + ".bias"] = w[p + "mlp.fc2.bias"]
    sd["vit.layernorm.weight"] = w["norm.weight"]; sd["vit.layernorm.bias"] = w["norm.bias"]
    sd["classifier.weight"] = f16(w["head.weight"]); sd["classifier.bias"] = w["head.bias"]
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    assert not [k for k in missing if "pooler" not in k], missing
    assert not unexpected, unexpected
    return m


@pytest.mark.parametrize("S", [32, 96, 128])
def test_oracle_on_resized_file_matches_huggingface_interpolate_pos_encoding(pkg, binding, oracle, tmp_path, S):
    """max |dlogit| <= 2e-4, the gate of test_oracle_vs_transformers_vit_f32 for this model pair; the AA convention reads 5e-4 .. 2e-3 on the
    same comparison, so the gate pins the convention too."""
    import torch
    m = _hf_micro(pkg)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(3, S))
    with torch.no_grad():
        hf = m(pixel_values=torch.from_numpy(imgs).permute(0, 3, 1, 2).contiguous(), interpolate_pos_encoding=True).logits.numpy()
    src = pkg.synth.cached_synthetic(MICRO, head_scale=4.0)
    got = {}
    for interp in (RD.BICUBIC, RD.BICUBIC_AA):
        dst = str(tmp_path / f"micro_{S}_{interp}.gguf")
        binding.resize_file(src, dst, S, interp)
        lg, _ = oracle.OracleModel(dst).forward(imgs, oracle.IDEAL)
        got[interp] = float(np.abs(lg - hf).max())
    print(f"img_size {S}: max|dlogit| oracle(resized file) vs HuggingFace: bicubic {got[RD.BICUBIC]:.2e}, bicubic_aa {got[RD.BICUBIC_AA]:.2e}")
    assert got[RD.BICUBIC] <= 2e-4, got
    assert got[RD.BICUBIC_AA] > 2e-4, got


# ------------------------------------------------------------------------------------------------ 4. ABI
def test_new_names_are_exported(binding):
    L = binding.lib()
    for name in ("vitx_ctx_img_size", "vitx_ctx_tokens", "vitx_pos_embed_resample", "vitx_op_pos_embed_resample", "vitx_model_resize_file"):
        assert name in binding.EXPORTS and hasattr(L, name), name
    names = [f for f, _ in binding.CtxOptions._fields_]
    assert names[-2:] == ["img_size", "pos_interp"] and ctypes.sizeof(binding.CtxOptions) == 48
    assert L.vitx_ctx_img_size(None) == 0 and L.vitx_ctx_tokens(None) == 0


def test_options_struct_of_the_old_size_is_still_accepted(pkg, binding):
    """Host-side argument checks only: they run before any device is touched, so without a GPU a well-formed call ends in VITX_ERR_HIP."""
    L = binding.lib()
    model = binding.Model(pkg.synth.cached_synthetic(MICRO, head_scale=4.0))

    def create(**kw):
        size = kw.pop("struct_size")
        opt = binding.CtxOptions(**kw); opt.struct_size = size
        h = ctypes.c_void_p()
        rc = L.vitx_ctx_create_ex(model._h, 0, 1, binding.F16, ctypes.byref(opt), ctypes.byref(h))
        geometry = (L.vitx_ctx_img_size(h), L.vitx_ctx_tokens(h)) if rc == 0 else None
        if rc == 0:
            L.vitx_ctx_free(h)
        return rc, geometry

    OLD = 40                        # sizeof(vitx_ctx_options) before img_size and pos_interp
    rc, geo = create(struct_size=OLD)
    assert rc in (0, ERR_HIP) and geo in (None, (64, 17))
    # what lies behind an old caller's struct is not read
    rc, geo = create(struct_size=OLD, img_size=-5, pos_interp=9)
    assert rc in (0, ERR_HIP) and geo in (None, (64, 17))
    rc, geo = create(struct_size=48, img_size=96)
    assert rc in (0, ERR_HIP) and geo in (None, (96, 37))
    for kw in (dict(img_size=-16), dict(img_size=40), dict(img_size=96, pos_interp=2), dict(pos_interp=-1)):
        assert create(struct_size=48, **kw)[0] == ERR_ARG, kw
    assert create(struct_size=52)[0] == ERR_ARG
    vitstr = binding.Model(pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0))
    opt = binding.CtxOptions(img_size=384); opt.struct_size = 48
    h = ctypes.c_void_p()
    assert L.vitx_ctx_create_ex(vitstr._h, 0, 1, binding.F16, ctypes.byref(opt), ctypes.byref(h)) == ERR_UNSUPPORTED
    vitstr.close(); model.close()


def test_converter_writes_the_checkpoint_at_another_size(pkg, binding, tmp_path):
    """convert.py --img-size N [--pos-interp ...]: the file vitx_model_resize_file writes from the plainly converted one."""
    import torch
    hp = pkg.synth.hparams_for(MICRO)
    w = pkg.synth.make_weights(hp, seed=5, head_scale=4.0)
    pth = str(tmp_path / "m.pth"); torch.save({k: torch.from_numpy(v.copy()) for k, v in w.items()}, pth)
    plain, out, want = str(tmp_path / "plain.gguf"), str(tmp_path / "at96.gguf"), str(tmp_path / "want.gguf")
    assert pkg.convert.main(["--timm-state-dict", pth, plain, "--heads", "2"]) == 0
    for flag, interp in ((["--pos-interp", "bicubic-aa"], RD.BICUBIC_AA), ([], RD.BICUBIC)):
        assert pkg.convert.main(["--timm-state-dict", pth, out, "--heads", "2", "--img-size", "96"] + flag) == 0
        binding.resize_file(plain, want, 96, interp)
        assert open(out, "rb").read() == open(want, "rb").read()
        assert binding.Model(out).img_size == 96
    assert sorted(os.listdir(tmp_path)) == ["at96.gguf", "m.pth", "plain.gguf", "want.gguf"]
    with pytest.raises(binding.VitxError):
        pkg.convert.main(["--timm-state-dict", pth, out, "--heads", "2", "--img-size", "100"])
