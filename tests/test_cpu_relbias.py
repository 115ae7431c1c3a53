"""The relative position bias without a GPU (include/vitx.h): host index rule, quantize copy, every refusal that needs no device, what the op's gate sees, the converter."""
import numpy as np
import pytest

import prefix_data as PD
import relbias_data as RB


def _write(pkg, tmp_path, edit=None, shared=False, pool=False):
    hp, t = RB.tensors(pkg, shared, pool)
    t = edit(t) or t if edit else t
    pkg.ggml_file.write_model(str(tmp_path / "m.gguf"), hp, t)
    return str(tmp_path / "m.gguf"), t


@pytest.mark.parametrize("shared", [False, True])
def test_dense_accessor_quantize_copy_and_refusals_without_a_device(pkg, binding, tmp_path, shared):
    path, t = _write(pkg, tmp_path, shared=shared)
    m = binding.Model(path)
    assert m.rel_bias() == (1 if shared else RB.LAYERS, 52) and binding.Model(pkg.synth.cached_synthetic(RB.NAME)).rel_bias() is None
    for layer in range(RB.LAYERS):
        tab = t["rel_bias"][0 if shared else layer]
        assert np.array_equal(m.rel_bias_dense(layer, 4), tab[:, RB.index(4, 4)]) and np.array_equal(m.rel_bias_dense(layer, (2, 3)), tab[:, RB.index(2, 3, g=4)])
    L, C, q, out = binding.lib(), binding.C, path + ".q8", binding.C.c_void_p()
    assert L.vitx_quantize_file(path.encode(), q.encode(), 8) == 0
    assert {x.name: x.raw for x in pkg.ggml_file.read_model(q).tensors}["rel_bias"] == t["rel_bias"].astype("<f4").tobytes() and binding.Model(q).rel_bias() == m.rel_bias()
    grey = binding.Model(_write(pkg, tmp_path, lambda t: t.update({"patch_embed.proj.weight": t["patch_embed.proj.weight"][:, :1]}))[0])       # one channel: ViTSTR
    opt = binding.CtxOptions(struct_size=C.sizeof(binding.CtxOptions), img_size=128)
    calls = {"resize": lambda: L.vitx_model_resize_file(q.encode(), (q + ".rs").encode(), 128, 0),
             "mxfp8": lambda: L.vitx_ctx_create_ex(m._h, 0, 1, binding.MXFP8, None, C.byref(out)),
             "vitstr": lambda: L.vitx_ctx_create_ex(grey._h, 0, 1, binding.BF16, None, C.byref(out)),
             "img_size": lambda: L.vitx_ctx_create_ex(m._h, 0, 1, binding.BF16, C.byref(opt), C.byref(out)),
             "rect": lambda: L.vitx_ctx_create_rect(m._h, 0, 1, binding.BF16, None, 64, 32, C.byref(out)),
             "pack": lambda: L.vitx_pack_create(m._h, 0, 64, 2, binding.BF16, None, C.byref(out)),
             "op head dim 32": lambda: L.vitx_op_attention_bias(binding.BF16, 16, 16, 16, 1, 4, 4, 128, 4),
             "op 41 x 41: table beyond the LDS": lambda: L.vitx_op_attention_bias(binding.BF16, 16, 16, 16, 1, 41, 41, 64, 1)}
    for name, call in calls.items():
        assert call() == binding.ERR_UNSUPPORTED and "relative position bias" in L.vitx_last_error().decode(), name


REFUSALS = {   # edit of relbias_data.tensors -> words of the refusal behind the file's path (a file with attn_pool.* has no cls_token: the first case)
    "no_cls": (lambda t: {k: v[:, 1:] if k == "pos_embed" else v for k, v in t.items() if k != "cls_token"}, "'rel_bias' in a file without cls_token"),
    "registers": (lambda t: {k2: v2 for k, v in t.items() for k2, v2 in [(k, v)] + [("reg_token", np.zeros((1, 2, 128), np.float32))] * (k == "cls_token")}, "'rel_bias' together with reg_token"),
    "rotary": (lambda t: {"rope": np.array([1, 100, 0, 0], np.float32), **t}, "'rel_bias' together with rope"),
    "layers": (lambda t: t.update(rel_bias=np.concatenate([t["rel_bias"], t["rel_bias"][:1]])), "3 dims [52, 2, 3]"),
    "length": (lambda t: t.update(rel_bias=t["rel_bias"][:, :, :-1]), "3 dims [51, 2, 2]"),
    "nan": (lambda t: t["rel_bias"].__setitem__((1, 1, 7), np.nan), "entry 163 is not finite"),
    "inf": (lambda t: t["rel_bias"].__setitem__((0, 0, 51), np.inf), "entry 51 is not finite"),
    "behind": (lambda t: {**{k: v for k, v in t.items() if k != "rel_bias"}, "rel_bias": t["rel_bias"]}, "'rel_bias' stands behind a blocks.* record"),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_loader_refuses(pkg, binding, tmp_path, what):
    path, _ = _write(pkg, tmp_path, REFUSALS[what][0], pool=what == "no_cls")
    with pytest.raises(binding.VitxError) as ei:
        binding.Model(path)
    assert ei.value.code == binding.ERR_FORMAT and REFUSALS[what][1] in str(ei.value).split(path)[-1], str(ei.value)


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("grid", RB.OP_GRIDS, ids=lambda g: "%dx%d" % g)
def test_the_ops_gate_sees_a_dropped_swapped_negated_or_misassigned_bias(grid, dtype_name):
    """On the op test's own data, float64 alone: each mistake moves an element by more than twice RB.GATE of the largest reference value."""
    qkv, table = RB.op_case(dtype_name, *grid)
    B = table[:, RB.index(*grid)]
    ref = RB.attention64(qkv, B, RB.OP_IMG, RB.OP_H)
    wrong = {"dropped": 0 * B, "negated": -B, "other head": np.roll(B, 1, 0), "dy/dx swapped": table[:, RB.index(*grid, swap=True)]}
    for name, Bw in wrong.items():
        moved = np.abs(RB.attention64(qkv, Bw, RB.OP_IMG, RB.OP_H) - ref).max()
        assert moved > 2 * RB.GATE * np.abs(ref).max() or (name, grid) == ("dy/dx swapped", (1, 1)), (name, moved)      # one patch has no offset to swap


@pytest.mark.parametrize("mean_pool,shared", [(False, False), (True, True)])
def test_converter_pinned_to_transformers_beit(pkg, binding, tmp_path, mean_pool, shared):
    tr, torch = pytest.importorskip("transformers"), pytest.importorskip("torch")
    torch.manual_seed(3)
    cfg = tr.BeitConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, image_size=64, patch_size=16, num_labels=5,
                        use_mean_pooling=mean_pool, use_relative_position_bias=not shared, use_shared_relative_position_bias=shared, layer_scale_init_value=0.1,
                        hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6)
    model = tr.BeitForImageClassification(cfg).eval()
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "relative_position_bias_table" in k or "lambda_" in k:
                p.copy_(torch.randn_like(p))
    out = str(tmp_path / "beit.gguf")
    if mean_pool:
        with pytest.raises(ValueError, match="mean_pool=True"):
            pkg.convert.convert_hf_model(model, out, ftype=0)
    pkg.convert.convert_hf_model(model, out, ftype=0, mean_pool=mean_pool)
    assert binding.Model(out).rel_bias() == (1 if shared else 2, 52) and binding.Model(out).head_pool == (binding.POOL_MEAN_NORM if mean_pool else 0)
    imgs = PD.exact_images(2, 64, seed=5)
    with torch.no_grad():
        want = torch.softmax(model(pixel_values=torch.from_numpy(imgs).permute(0, 3, 1, 2)).logits.double(), -1).numpy()
    assert np.abs(RB.forward64(PD.file_tensors(pkg, out), imgs) - want).max() < 2e-4


@pytest.mark.parametrize("shared", [False, True])
def test_timm_beit_state_dict(pkg, binding, tmp_path, shared):
    """timm's Beit names: q_bias / v_bias, gamma_1 / gamma_2, the tables [num][H] per block or shared, the index buffers, fc_norm, no pos_embed."""
    _, t = RB.tensors(pkg, shared, True)
    sd = {k.replace("norm.", "fc_norm.") if k.startswith("norm.") else k: v for k, v in t.items() if k not in ("pool", "rel_bias", "pos_embed")}
    for i in range(RB.LAYERS):
        p, b = f"blocks.{i}.", sd.pop(f"blocks.{i}.attn.qkv.bias")
        sd.update({p + "attn.q_bias": b[:128], p + "attn.v_bias": b[256:], p + "gamma_1": np.full(128, 0.5, np.float32), p + "gamma_2": np.full(128, 2.0, np.float32),
                   p + "attn.relative_position_index": RB.index(4, 4), **({} if shared else {p + "attn.relative_position_bias_table": t["rel_bias"][i].T})})
    if shared:
        sd.update({"rel_pos_bias.relative_position_bias_table": t["rel_bias"][0].T, "rel_pos_bias.relative_position_index": RB.index(4, 4)})
    with pytest.raises(ValueError, match="fc_norm"):
        pkg.convert.convert_timm_state_dict(sd, str(tmp_path / "b.gguf"), heads=2)
    pkg.convert.convert_timm_state_dict(sd, str(tmp_path / "b.gguf"), heads=2, mean_pool=True)
    got, b0 = PD.file_tensors(pkg, str(tmp_path / "b.gguf")), t["blocks.0.attn.qkv.bias"]
    assert binding.Model(str(tmp_path / "b.gguf")).head_pool == binding.POOL_MEAN_NORM and np.array_equal(got["rel_bias"], t["rel_bias"]) and not got["pos_embed"].any()
    assert np.array_equal(got["blocks.0.attn.qkv.bias"], np.concatenate([b0[:128], np.zeros(128, np.float32), b0[256:]]))
    assert np.array_equal(got["blocks.1.mlp.fc2.bias"], 2 * t["blocks.1.mlp.fc2.bias"]) and np.array_equal(got["norm.weight"], t["norm.weight"])
