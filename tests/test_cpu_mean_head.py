"""The mean-pool head without a GPU (include/vitx.h): loader rules, quantize / resize copy-through, the converter's opt-in and default refusals."""
import numpy as np
import pytest

NAME = "vit_micro_patch14_56"


def _tensors(pkg, order=1, cls=True, R=4):
    hp = pkg.synth.hparams_for(NAME)
    return hp, pkg.synth.make_weights(hp, head_scale=4.0, registers=R, head_pool=3 + order, cls_token=cls)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("cls,R", [(True, 4), (True, 0), (False, 4), (False, 0)])
def test_loader_accepts_and_quantize_resize_copy_through(pkg, binding, tmp_path, order, cls, R):
    path = str(tmp_path / "m.gguf")
    pkg.synth.write_synthetic(path, NAME, registers=R, head_pool=3 + order, cls_token=cls)
    m = binding.Model(path)
    assert (m.head_pool, m.num_prefix, m.num_registers) == (3 + order, int(cls) + R, R)
    assert (binding.POOL_MEAN, binding.POOL_MEAN_NORM) == (3, 4) and "vitx_op_pool_mean" in binding.EXPORTS
    q, r = path + ".q8", path + ".rs"
    assert binding.lib().vitx_quantize_file(path.encode(), q.encode(), 8) == 0
    assert binding.Model(q).head_pool == 3 + order and binding.Model(q).num_prefix == int(cls) + R
    assert binding.lib().vitx_model_resize_file(path.encode(), r.encode(), 112, 0) == (0 if cls else binding.ERR_UNSUPPORTED)
    assert not cls or (binding.Model(r).head_pool, binding.Model(r).hparams.img_size) == (3 + order, 112)


@pytest.mark.parametrize("what,word", [("map", "attn_pool"), ("wide_head", "2 D"), ("order", "order"), ("kind", "kind"), ("pos_cls", "pos_embed"), ("pos_nocls", "pos_embed")])
def test_loader_refuses(pkg, binding, tmp_path, what, word):
    hp, t = _tensors(pkg, cls=what != "pos_nocls")
    marker = {"order": [1, 2, 0, 0], "kind": [2, 0, 0, 0]}.get(what)
    if what == "map":
        import map_data as MD
        t = {"pool": t["pool"], **MD.fixture_tensors(pkg)[1]}
    elif what == "wide_head":
        t["head.weight"] = np.concatenate([t["head.weight"]] * 2, axis=1)
    elif what == "pos_cls":
        t["pos_embed"] = t["pos_embed"][:, 1:]                    # a class token, but no class row
    elif what == "pos_nocls":
        t["pos_embed"] = np.concatenate([t["pos_embed"][:, :1], t["pos_embed"]], axis=1)       # no class token, but a class row
    path = str(tmp_path / "bad.gguf")
    pkg.ggml_file.write_model(path, hp, t)
    if marker:                                                    # the writer refuses such a marker itself: patched into the file, 16 bytes behind the name
        buf = bytearray(open(path, "rb").read())
        at = buf.index(b"pool") + 4
        buf[at:at + 16] = np.asarray(marker, "<f4").tobytes()
        open(path, "wb").write(bytes(buf))
    with pytest.raises(binding.VitxError) as ei:
        binding.Model(path)
    assert ei.value.code == binding.ERR_FORMAT and word in str(ei.value), str(ei.value)


def test_converter_opt_in_and_default_refusals(pkg, binding, tmp_path):
    out = str(tmp_path / "x.gguf")
    hp, t = _tensors(pkg, cls=False)
    sd = {k.replace("norm.", "fc_norm.") if k.startswith("norm.") else k: v for k, v in t.items() if k != "pool"}
    with pytest.raises(ValueError, match="fc_norm"):
        pkg.convert.convert_timm_state_dict(sd, out, heads=2)
    pkg.convert.convert_timm_state_dict(sd, out, heads=2, mean_pool=True)
    assert (binding.Model(out).head_pool, binding.Model(out).num_prefix, binding.Model(out).num_registers) == (binding.POOL_MEAN_NORM, 4, 4)
    assert {x.name: x.raw for x in pkg.ggml_file.read_model(out).tensors}["norm.weight"] == t["norm.weight"].astype("<f4").tobytes()
    _, t0 = _tensors(pkg, order=0, cls=True, R=0)                  # norm.*, no fc_norm, a class token: order 0 on the explicit flag
    pkg.convert.convert_timm_state_dict({k: v for k, v in t0.items() if k != "pool"}, out, heads=2, mean_pool=True)
    assert (binding.Model(out).head_pool, binding.Model(out).num_prefix) == (binding.POOL_MEAN, 1)
    tr = pytest.importorskip("transformers")
    cfg = tr.SiglipConfig(vision_config=dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, patch_size=14, image_size=56),
                          text_config=dict(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, vocab_size=50))
    cfg.num_labels = 3
    model = tr.SiglipForImageClassification(cfg).eval()
    with pytest.raises(ValueError, match="SiglipForImageClassification"):
        pkg.convert.convert_hf_model(model, out, ftype=0)
    pkg.convert.convert_hf_model(model, out, ftype=0, mean_pool=True)
    m = binding.Model(out)
    assert (m.head_pool, m.num_prefix, m.hparams.num_classes, m.hparams.img_size) == (binding.POOL_MEAN, 0, 3, 56)
