"""Windowed attention without a GPU (include/vitx.h): the float64 reference against a direct restatement of window partition + decomposed relative
position, and the refusals that need no device."""
import numpy as np
import pytest

import prefix_data as PD
import window_data as WD


def test_reference_is_window_partition_plus_decomposed_rel_pos():
    """Pins window_data.attention64, not the kernel: pad behind the (already biased) qkv rows, partition, add the two einsum terms, attend, un-partition, crop."""
    torch = pytest.importorskip("torch")
    F, (grid, win), n = torch.nn.functional, WD.F64_CASES[1], 2
    qkv, Rh, Rw, bias = (torch.from_numpy(a).double() for a in WD.case("f16", grid, win))
    (gh, gw), ws = grid, win[0]
    x = qkv.reshape(n, gh, gw, -1) - bias                   # the qkv GEMM's product without its bias: the pad rows of it are zero
    x = F.pad(x, (0, 0, 0, -gw % ws, 0, -gh % ws)) + bias
    Hp, Wp = x.shape[1:3]
    x = x.view(n, Hp // ws, ws, Wp // ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, 3, WD.H, WD.DH)
    q, k, v = x.permute(2, 0, 3, 1, 4).reshape(3, -1, ws * ws, WD.DH)
    attn = (q * WD.DH ** -0.5) @ k.transpose(-2, -1)
    coords = torch.arange(ws)[:, None] - torch.arange(ws)[None, :] + ws - 1
    r_q = q.reshape(-1, ws, ws, WD.DH)
    rel_h, rel_w = torch.einsum("bhwc,hkc->bhwk", r_q, Rh[coords]), torch.einsum("bhwc,wkc->bhwk", r_q, Rw[coords])
    attn = (attn.view(-1, ws, ws, ws, ws) + rel_h[:, :, :, :, None] + rel_w[:, :, :, None, :]).view(-1, ws * ws, ws * ws)
    o = (attn.softmax(-1) @ v).view(-1, WD.H, ws, ws, WD.DH).permute(0, 2, 3, 1, 4).reshape(n, Hp // ws, Wp // ws, ws, ws, WD.D)
    o = o.permute(0, 1, 3, 2, 4, 5).reshape(n, Hp, Wp, WD.D)[:, :gh, :gw].reshape(-1, WD.D)
    assert np.abs(WD.attention64(*WD.case("f16", grid, win), n, grid, win) - o.numpy()).max() < 1e-12


def test_op_refusals_without_a_device(binding):
    L, p = binding.lib(), 16
    assert "vitx_op_attention_window" in binding.EXPORTS
    assert L.vitx_op_attention_window(binding.BF16, p, p, p, p, None, 1, 4, 4, 4, 4, 128, 2) == binding.ERR_ARG
    assert L.vitx_op_attention_window(binding.MXFP8, p, p, p, p, p, 1, 4, 4, 4, 4, 128, 2) == binding.ERR_ARG
    for gh, gw, wh, ww, D, H in ((4, 4, 4, 4, 128, 4), (4, 80, 4, 65, 128, 2), (65, 65, 65, 65, 64, 1)):      # head dim 32; a window side above 64
        assert L.vitx_op_attention_window(binding.BF16, p, p, p, p, p, 1, gh, gw, wh, ww, D, H) == binding.ERR_UNSUPPORTED
        assert "windowed attention" in L.vitx_last_error().decode()


def _write(pkg, tmp_path, edit=None, heads=WD.H, text=False):
    hp, t = WD.tensors(pkg, heads=heads)
    t = edit(t) or t if edit else t
    if text:                      # a text-tower file is told by patch_size 0; the loader meets `window` first
        hp, t = pkg.synth.HParams(WD.D, WD.LAYERS, heads, 10, 0, 8, ftype=1), {"window": t["window"]}
    pkg.ggml_file.write_model(str(tmp_path / "m.gguf"), hp, t)
    return str(tmp_path / "m.gguf"), t


def test_round_trip_quantize_copy_and_refusals_without_a_device(pkg, binding, tmp_path):
    path, t = _write(pkg, tmp_path)
    m = binding.Model(path)
    assert m.window() == (WD.WS, 1, [True, False, True]) and m.head_pool == binding.POOL_MEAN and binding.Model(pkg.synth.cached_synthetic("vit_micro_patch16_64")).window() is None
    L, C, q, out = binding.lib(), binding.C, path + ".q8", binding.C.c_void_p()
    assert L.vitx_quantize_file(path.encode(), q.encode(), 8) == 0 and binding.Model(q).window() == m.window()
    raw = {x.name: x.raw for x in pkg.ggml_file.read_model(q).tensors}
    for name in ("window", "blocks.0.attn.rel_pos_h", "blocks.1.attn.rel_pos_w"):
        assert raw[name] == np.asarray(t[name], "<f4").tobytes() and np.shape(t[name]) == {"w": (5,), "0": (5, 64), "1": (9, 64)}[name[0] if name[0] == "w" else name[7]]
    opt = binding.CtxOptions(struct_size=C.sizeof(binding.CtxOptions), img_size=80)
    grey = binding.Model(_write(pkg, tmp_path, lambda t: t.update({"patch_embed.proj.weight": t["patch_embed.proj.weight"][:, :1]}))[0])       # one channel: ViTSTR
    hd32 = binding.Model(_write(pkg, tmp_path, heads=4)[0])
    calls = {"resize": lambda: L.vitx_model_resize_file(path.encode(), (path + ".rs").encode(), 80, 0),
             "mxfp8": lambda: L.vitx_ctx_create_ex(m._h, 0, 1, binding.MXFP8, None, C.byref(out)),
             "vitstr": lambda: L.vitx_ctx_create_ex(grey._h, 0, 1, binding.BF16, None, C.byref(out)),
             "head dim 32": lambda: L.vitx_ctx_create_ex(hd32._h, 0, 1, binding.BF16, None, C.byref(out)),
             "img_size": lambda: L.vitx_ctx_create_ex(m._h, 0, 1, binding.BF16, C.byref(opt), C.byref(out)),
             "pack": lambda: L.vitx_pack_create(m._h, 0, 64, 2, binding.BF16, None, C.byref(out))}
    for name, call in calls.items():
        assert call() == binding.ERR_UNSUPPORTED and "windowed attention" in L.vitx_last_error().decode(), name


def _front(extra):
    return lambda t: {**extra, **t}


REFUSALS = {   # edit of window_data.tensors -> words of the refusal behind the file's path
    "cls_token": (lambda t: {**{k: v for k, v in t.items() if k != "pos_embed"}, "cls_token": np.zeros((1, 1, 128), np.float32), "pos_embed": np.zeros((1, 26, 128), np.float32)}, "'window' together with cls_token"),
    "reg_token": (lambda t: {"reg_token": np.zeros((1, 2, 128), np.float32), **t}, "'window' together with reg_token"),
    "rope": (_front({"rope": np.array([1, 100, 0, 0], np.float32)}), "'window' together with rope"),
    "rel_bias": (_front({"rel_bias": np.zeros((1, 2, 84), np.float32)}), "'window' together with rel_bias"),
    "attn_pool": (lambda t: {**t, "attn_pool.latent": np.zeros((1, 1, 128), np.float32)}, "together with attn_pool.*"),      # (`pool`'s own check meets it first)
    "text tower": (None, "text-tower file: tensor 'window' belongs to image files"),
    "glu": (lambda t: {"glu": np.array([1, 512, 0, 0], np.float32), **{k: (np.zeros((1024, 128), np.float32) if k.endswith("fc1.weight") else np.zeros(1024, np.float32) if k.endswith("fc1.bias") else v) for k, v in t.items()}}, "'window' together with glu"),
    "no pool": (lambda t: {k: v for k, v in t.items() if k != "pool"}, None),
    "missing table": (lambda t: {k: v for k, v in t.items() if k != "blocks.2.attn.rel_pos_w"}, None),
    "mis-sized table": (lambda t: t.update({"blocks.1.attn.rel_pos_h": t["blocks.1.attn.rel_pos_h"][:5]}), "'blocks.1.attn.rel_pos_h' has wrong size"),
    "nan": (lambda t: t["blocks.0.attn.rel_pos_w"].__setitem__((2, 3), np.nan), "'blocks.0.attn.rel_pos_w' entry 131 is not finite"),
    "ws 0": (lambda t: t["window"].__setitem__(0, 0), "names ws 0"),
    "flag 2": (lambda t: t["window"].__setitem__(3, 2), "slot 3 is 2"),
    "norm flag": (lambda t: t["window"].__setitem__(1, 0.5), "slot 1 is 0.5"),
    "behind": (lambda t: {**{k: v for k, v in t.items() if k != "window"}, "window": t["window"]}, None),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_loader_refuses(pkg, binding, tmp_path, what):
    path, _ = _write(pkg, tmp_path, REFUSALS[what][0], text=what == "text tower")
    with pytest.raises(binding.VitxError) as ei:
        binding.Model(path)
    assert ei.value.code == binding.ERR_FORMAT and (REFUSALS[what][1] or "") in str(ei.value).split(path)[-1], str(ei.value)


def test_converter_against_a_state_dict_under_segment_anythings_names(pkg, binding, tmp_path, capsys):
    """image_encoder.* names, pos_embed [1][g][g][D], mlp.lin1 / lin2, neck.* and the other modules beside them: the file's tensors one by one."""
    _, t = WD.tensors(pkg)
    sd = {"prompt_encoder.pe": np.zeros(4, np.float32), "image_encoder.neck.0.weight": np.zeros((8, 128, 1, 1), np.float32)}
    for k, v in t.items():
        if k.startswith(("blocks.", "patch_embed.")) or k == "pos_embed":
            sd["image_encoder." + k.replace("mlp.fc1", "mlp.lin1").replace("mlp.fc2", "mlp.lin2")] = v.reshape(1, WD.GRID, WD.GRID, WD.D) if k == "pos_embed" else v
    out = str(tmp_path / "sam.gguf")
    hp = pkg.convert.convert_sam_state_dict(sd, out, ftype=0, heads=WD.H)
    notes = capsys.readouterr().out
    assert "neck.*" in notes and "prompt_encoder" in notes and (hp.img_size, hp.patch_size, hp.num_classes) == (WD.IMG, WD.IMG // WD.GRID, 1)
    got, m = PD.file_tensors(pkg, out), binding.Model(out)
    assert m.window() == (WD.WS, 1, [True, False, True]) and m.head_pool == binding.POOL_MEAN and m.activation == binding.ACT_GELU_ERF
    for k, v in t.items():
        want = {"norm.weight": np.ones(128), "norm.bias": np.zeros(128), "head.weight": np.zeros((1, 128)), "head.bias": np.zeros(1),
                "patch_embed.proj.weight": PD.f16_round(v)}.get(k, v)      # (the file format keeps the patch kernel in f16 at every ftype)
        assert np.array_equal(got[k].reshape(np.shape(want)), want), k
    assert list(got)[:3] == ["arch", "window", "pool"] and set(got) == set(t) | {"arch"} and np.array_equal(got["arch"], np.array([1, 1e-6, 0, 0], np.float32))
