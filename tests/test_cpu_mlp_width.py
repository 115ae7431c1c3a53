"""The `mlp` tensor (include/vitx.h "MLP width") without a GPU: the loader's rules, vitx_model_mlp_width, and the converter's opt-in with a round trip
through vitx_model_resize_file.  mlp_data(): the D 576 / H 8 / F 1000 two-layer model tests/test_gpu_attention_wide.py runs end to end."""
import numpy as np
import pytest

import ref64 as R64

D, H, F = 576, 8, 1000


def mlp_data(pkg, width=F, pad_to=0):
    """(hparams, tensors) of pkg.synth.make_weights at D 576, 8 heads (head dim 72), 2 layers, patch 14, image 56, its 4 D MLP cut to `width` rows /
    columns, `mlp` = {width, 0, 0, 0} in front.  pad_to: the same model filed at that width, the pad rows, bias and columns written out as zeros."""
    hp = pkg.ggml_file.HParams(D, 2, H, 10, 14, 56, 1)
    t = dict(pkg.synth.make_weights(hp, head_scale=4.0))
    Fw = pad_to or width
    for i in range(hp.num_hidden_layers):
        p = f"blocks.{i}.mlp."
        w1, b1, w2 = np.zeros((Fw, D), np.float32), np.zeros((Fw,), np.float32), np.zeros((D, Fw), np.float32)
        w1[:width], b1[:width], w2[:, :width] = t[p + "fc1.weight"][:width], t[p + "fc1.bias"][:width], t[p + "fc2.weight"][:, :width]
        t[p + "fc1.weight"], t[p + "fc1.bias"], t[p + "fc2.weight"] = w1, b1, w2
    return hp, {"mlp": np.array([Fw, 0, 0, 0], np.float32), **t}


def mlp_file(pkg, width=F, pad_to=0):
    return R64.cached_file(f"mlp-width-{width}-{pad_to}", lambda tmp: pkg.ggml_file.write_model(tmp, *mlp_data(pkg, width, pad_to)))


def test_width_1000_loads_and_reports_its_width(pkg, binding):
    m = binding.Model(mlp_file(pkg))
    assert m.mlp_width == F and m.hparams.hidden_size == D
    m.close()
    plain = binding.Model(pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0))
    assert plain.mlp_width == 4 * plain.hparams.hidden_size
    plain.close()


def siglip_model():
    """A tiny randomly initialised SiglipVisionModel in SO400M's proportions: D 576, 8 heads of 72, intermediate_size 1000, attention-pooling head."""
    import torch
    import transformers
    torch.manual_seed(3)
    cfg = transformers.SiglipVisionConfig(hidden_size=D, intermediate_size=F, num_hidden_layers=2, num_attention_heads=H, image_size=28, patch_size=14)
    return transformers.SiglipVisionModel(cfg).eval()


def siglip_file(pkg):
    return R64.cached_file("mlp-width-siglip", lambda tmp: pkg.convert.convert_hf_model(siglip_model(), tmp, mlp_width=True))


# what is wrong -> (the tensors, the loader's words for it)
MALFORMED = {
    "F = 12": (lambda pkg, hp, t: {**t, "mlp": np.array([12, 0, 0, 0], np.float32)}, "multiple of 8"),
    "reserved slot": (lambda pkg, hp, t: {**t, "mlp": np.array([F, 0, 1, 0], np.float32)}, "reserved slots"),
    "with glu": (lambda pkg, hp, t: {"mlp": np.array([64, 0, 0, 0], np.float32), **pkg.synth.make_weights(hp, glu=64)}, "together with 'mlp'"),
    # (a 4 D wide model, so that the blocks in front of it have the shapes the loader still expects)
    "behind a block": (lambda pkg, hp, t: {**pkg.synth.make_weights(hp), "mlp": np.array([4 * D, 0, 0, 0], np.float32)}, "behind a blocks.* record"),
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_mlp_tensors_are_refused(pkg, binding, tmp_path, what):
    hp, t = mlp_data(pkg)
    make, words = MALFORMED[what]
    path = str(tmp_path / "bad.gguf")
    pkg.ggml_file.write_model(path, hp, make(pkg, hp, t))
    with pytest.raises(binding.VitxError) as ei:
        binding.Model(path)
    assert ei.value.code == binding.ERR_FORMAT and words in str(ei.value), (what, str(ei.value))


def test_converter_opt_in_and_resize_copy(pkg, binding, tmp_path):
    """siglip_model(): refused with today's message by default, converted with mlp_width=True; the file loads with its width and pooling head.
    vitx_model_resize_file refuses every attention-pooling file (no class row to resample), so the copy-through is shown on mlp_file."""
    with pytest.raises(ValueError, match="4 x hidden MLP"):
        pkg.convert.convert_hf_model(siglip_model(), str(tmp_path / "no.gguf"))
    names = [t.name for t in pkg.ggml_file.read_model(siglip_file(pkg)).tensors]
    assert names.index("mlp") < names.index("blocks.0.norm1.weight")
    m = binding.Model(siglip_file(pkg))
    assert m.mlp_width == F and m.head_pool == binding.POOL_MAP
    m.close()
    small = str(tmp_path / "small.gguf")
    binding.resize_file(mlp_file(pkg), small, 28)
    r = binding.Model(small)
    assert r.mlp_width == F and r.hparams.img_size == 28
    r.close()
