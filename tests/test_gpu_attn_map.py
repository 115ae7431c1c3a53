"""Attention maps and attention rollout (vitx_attn_enable / vitx_attn_read / vitx_op_attention_map, include/vitx.h).

The maps are f32 softmaxes of the context's own q, k: s = (q . k) / sqrt(hd), A_h = expf(s - max) / sum.  Checked
  - op level against float64 numpy on the same operands (bf16, f16, and the F16 parity mode's two planes),
  - end to end against a float64 recompute from the residual-stream trace and the weights (every layer, wired in order; the rollout chain),
  - for bits: the forward's own outputs do not move with maps on, an image's maps do not depend on its batch, the class-rows-only last layer
    and the graph cache give the same maps,
  - for its errors, and through the CLI's --attn-map picture."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = 3, 5


def _dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _softmax64(s):
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _maps64(q, k, H):
    """q, k [N][D] f64 of one image -> A [H][N][N] f64."""
    N, D = q.shape
    hd = D // H
    qh = q.reshape(N, H, hd).transpose(1, 0, 2)
    kh = k.reshape(N, H, hd).transpose(1, 0, 2)
    return _softmax64(qh @ kh.transpose(0, 2, 1) / np.sqrt(hd))


# ------------------------------------------------------------------------------------------------ op level
OP_SHAPES = [(7, 197, 768, 12), (3, 577, 1024, 16), (5, 50, 192, 3), (4, 65, 256, 8), (2, 197, 256, 2), (3, 17, 64, 4), (9, 1, 128, 2),
             # head dims 24, 40, 56, 72: hd / 8 = 3, 5, 7, 9 pieces of 16 bytes per key row, the class-token map's lane groups of 4, 8, 8, 16 with idle lanes
             (3, 50, 72, 3), (2, 65, 80, 2), (2, 33, 112, 2), (2, 197, 144, 2)]


@pytest.mark.parametrize("mode", ["bf16", "f16", "f16_planes"])
@pytest.mark.parametrize("n_img,N,D,H,mean", [s + (True,) for s in OP_SHAPES] + [(2, 785, 64, 8, False)])
def test_op_attention_map_against_float64(binding, torch_gpu, mode, n_img, N, D, H, mean):
    """Head dims 8 .. 128 (1, 2, 3, 4, 5, 7, 8, 9 and 16 pieces of 16 bytes per key row), 1 .. 785 tokens.  Scores drawn with a spread of several units: peaked rows, not uniform ones."""
    torch = torch_gpu
    rows = n_img * N
    rng = np.random.default_rng(n_img * 7 + N * 13 + D + H)
    x = (rng.standard_normal((rows, 3 * D)) * 1.6).astype(np.float32)
    if mode == "bf16":
        dt, buf = binding.BF16, _dev(torch, x, torch.bfloat16)
        vals, lo_off = buf.float().cpu().numpy().astype(np.float64), 0
    elif mode == "f16":
        dt, buf = binding.F16, _dev(torch, x, torch.float16)
        vals, lo_off = buf.float().cpu().numpy().astype(np.float64), 0
    else:
        dt = binding.F16
        xt = _dev(torch, x)
        hi = xt.to(torch.float16); lo = ((xt - hi.float()) * 2048.0).to(torch.float16)
        pad = 8
        buf = torch.full((2 * (rows + pad), 3 * D), float("nan"), dtype=torch.float16, device="cuda")     # NaN rows behind each plane: never read
        buf[:rows] = hi; buf[rows + pad:2 * rows + pad] = lo
        lo_off = (rows + pad) * 3 * D
        vals = hi.double().cpu().numpy() + lo.double().cpu().numpy() * 2.0 ** -11
    cls = torch.full((n_img, H, N), float("nan"), dtype=torch.float32, device="cuda")
    mn = torch.full((n_img, N, N), float("nan"), dtype=torch.float32, device="cuda") if mean else None
    binding.op_attention_map(dt, buf.data_ptr(), cls.data_ptr(), mn.data_ptr() if mean else 0, n_img, N, D, H, lo_off=lo_off)
    torch.cuda.synchronize()
    g_cls = cls.cpu().numpy().astype(np.float64)
    g_mn = mn.cpu().numpy().astype(np.float64) if mean else None
    spread = []
    for b in range(n_img):
        v = vals[b * N:(b + 1) * N]
        A = _maps64(v[:, :D], v[:, D:2 * D], H)
        spread.append(A[:, 0].max())
        assert np.abs(g_cls[b] - A[:, 0, :]).max() <= 1e-5, (b, float(np.abs(g_cls[b] - A[:, 0, :]).max()))
        if mean:
            assert np.abs(g_mn[b] - A.mean(axis=0)).max() <= 1e-5, (b, float(np.abs(g_mn[b] - A.mean(axis=0)).max()))
    assert np.abs(g_cls.sum(axis=-1) - 1.0).max() <= 1e-5
    if mean:
        assert np.abs(g_mn.sum(axis=-1) - 1.0).max() <= 1e-5
    if N >= 17:
        assert np.median(spread) > 5.0 / N           # the rows are peaked (a uniform row would have max 1 / N)


def test_op_attention_map_argument_checks(binding, torch_gpu):
    torch = torch_gpu
    L = binding.lib()
    q = torch.zeros((4 * 1025 * 3 * 128,), dtype=torch.float16, device="cuda")
    o = torch.zeros((4 * 1025 * 1025,), dtype=torch.float32, device="cuda")
    assert L.vitx_op_attention_map(binding.F16, q.data_ptr(), 0, None, None, 4, 10, 128, 2, None) == ERR_ARG              # nothing to write
    assert L.vitx_op_attention_map(binding.F16, q.data_ptr(), 0, o.data_ptr(), None, 4, 10, 100, 4, None) == ERR_UNSUPPORTED   # head dim 25
    assert L.vitx_op_attention_map(binding.F16, q.data_ptr(), 0, o.data_ptr(), None, 4, 10, 512, 2, None) == ERR_UNSUPPORTED   # head dim 256
    assert L.vitx_op_attention_map(binding.F16, q.data_ptr(), 0, None, o.data_ptr(), 4, 1025, 128, 2, None) == ERR_UNSUPPORTED  # mean above 1024 tokens
    assert L.vitx_op_attention_map(binding.BF16, q.data_ptr(), 4 * 10 * 384, o.data_ptr(), None, 4, 10, 128, 2, None) == ERR_ARG  # planes: F16 only
    assert L.vitx_op_attention_map(binding.F16, q.data_ptr(), 100, o.data_ptr(), None, 4, 10, 128, 2, None) == ERR_ARG           # lo inside hi
    assert L.vitx_op_attention_map(7, q.data_ptr(), 0, o.data_ptr(), None, 4, 10, 128, 2, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------ end to end, against the trace
MODES = {"bf16": (1, {}), "f16": (0, {}), "f16_fast": (0, {"f16_fast_attention": 1})}
# test-only toys (registered at run time): three layers, so that rollout runs its in-place step (layers 1 .. L-2), at 401 and 785 tokens
# (the step's and the head mean's 8- and 16-tile builds); and one beyond rollout's 1024 tokens
EXTRA_CONFIGS = {"vit_micro3_patch8_160": (128, 3, 2, 10, 8, 160), "vit_micro3_patch8_224": (128, 3, 2, 10, 8, 224),
                 "vit_micro_patch4_128": (128, 2, 2, 10, 4, 128),
                 # 122 tokens: the step's 2-tile build, N % 4 == 2;  26 tokens in one layer: rollout is the row kernel without r;  in two
                 # layers: head mean, then the row kernel, no step;  25 patches + class token + 2 registers = 28 tokens: N % 4 == 0
                 "vit_micro3_patch8_88": (128, 3, 2, 10, 8, 88), "vit_micro1_patch16_80": (128, 1, 2, 10, 16, 80),
                 "vit_micro_patch16_80": (128, 2, 2, 10, 16, 80), "vit_micro3_patch8_40": (128, 3, 2, 10, 8, 40)}
EXTRA_REGISTERS = {"vit_micro3_patch8_40": 2}


def _synthetic(pkg, name):
    if name in EXTRA_CONFIGS:
        pkg.synth.CONFIGS.setdefault(name, EXTRA_CONFIGS[name])
    return pkg.synth.cached_synthetic(name, head_scale=4.0, registers=EXTRA_REGISTERS.get(name, 0))


def _round(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.float16 if dtype == 0 else torch.bfloat16).float().numpy().astype(np.float64)


def _layer_maps_from_trace(torch, model, trace, dtype, round_qkv, n_img):
    """Per layer l, per image: the f64 maps [H][N][N] recomputed from the residual stream entering layer l."""
    hp = model.hparams
    D, H, L = hp.hidden_size, hp.num_attention_heads, hp.num_hidden_layers
    idx = {name: i for i, (name, *_rest) in enumerate(model.tensors())}
    out = []
    for l in range(L):
        p = f"blocks.{l}."
        vec = lambda name: model.tensor_f32(idx[p + name]).reshape(-1).astype(np.float64)
        lw, lb = vec("norm1.weight"), vec("norm1.bias")
        W = _round(torch, model.tensor_f32(idx[p + "attn.qkv.weight"]).reshape(3 * D, D), dtype)
        bias = vec("attn.qkv.bias")
        per = []
        for b in range(n_img):
            xx = trace[l, b].astype(np.float64)
            mu = xx.mean(axis=1, keepdims=True); var = ((xx - mu) ** 2).mean(axis=1, keepdims=True)
            u = _round(torch, ((xx - mu) / np.sqrt(var + hp.eps)) * lw + lb, dtype)
            qkv = u @ W.T + bias
            if round_qkv:
                qkv = _round(torch, qkv, dtype)
            per.append(_maps64(qkv[:, :D], qkv[:, D:2 * D], H))
        out.append(per)
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,n_img", [("vit_tiny_patch16_224", 3), ("vit_base_patch16_224", 2), ("vit_micro3_patch8_160", 3), ("vit_micro3_patch8_224", 2),
                                        ("vit_micro3_patch8_88", 3), ("vit_micro1_patch16_80", 3), ("vit_micro_patch16_80", 3), ("vit_micro3_patch8_40", 3)])
def test_maps_and_rollout_match_a_float64_recompute_from_the_trace(pkg, binding, torch_gpu, mode, name, n_img):
    torch = torch_gpu
    dtype, opts = MODES[mode]
    path = _synthetic(pkg, name)
    model = binding.Model(path)
    hp = model.hparams
    L, H = hp.num_hidden_layers, hp.num_attention_heads
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n_img, hp.img_size, seed=77))
    ctx = binding.Context(model, device=0, max_batch=n_img, dtype=dtype, **opts)
    ctx.trace_enable(list(range(n_img)))
    ctx.attn_enable(None, rollout=True)
    ctx.forward(imgs)
    trace = ctx.trace_read()
    cls, roll = ctx.attn_read()
    assert cls.shape == (n_img, L, H, trace.shape[2]) and roll.shape == (n_img, trace.shape[2])
    parity = mode == "f16"
    ref = _layer_maps_from_trace(torch, model, trace, dtype, round_qkv=not parity, n_img=n_img)
    tol = 2e-3 if parity else 3e-2
    for b in range(n_img):
        refc = [ref[l][b][:, 0, :] for l in range(L)]           # [H][N] class rows of every layer
        for l in range(L):
            g = cls[b, l].astype(np.float64)
            err = np.abs(g - refc[l]).max(axis=1)
            assert (err <= tol * refc[l].max(axis=1)).all(), (b, l, err.tolist())
            others = [np.abs(g - refc[m]).max() for m in range(L) if m != l]
            if others:                                                  # a one-layer model has no other layer to be confused with
                assert np.abs(g - refc[l]).max() <= 0.1 * min(others), (b, l, float(np.abs(g - refc[l]).max()), min(others))
        N = refc[0].shape[1]
        eye = np.eye(N)
        fac = [0.5 * ref[l][b].mean(axis=0) + 0.5 * eye for l in range(L)]
        R, Rrev = eye, eye
        for l in range(L):
            R = fac[l] @ R
            Rrev = Rrev @ fac[l]
        r = roll[b].astype(np.float64)
        assert (r >= 0).all() and abs(r.sum() - 1.0) <= 1e-4, float(r.sum())
        assert np.abs(r - R[0]).max() <= tol * R[0].max(), (b, float(np.abs(r - R[0]).max()), float(R[0].max()))
        if L > 1:
            assert np.abs(r - R[0]).max() <= 0.1 * np.abs(r - Rrev[0]).max()   # the factors are chained in layer order
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ bits
def _forward_dev(torch, ctx, imgs):
    d = _dev(torch, imgs)
    n = imgs.shape[0]
    C = ctx.model.num_classes
    p = torch.empty((n, C), dtype=torch.float32, device="cuda"); lg = torch.empty((n, C), dtype=torch.float32, device="cuda")
    ctx.forward_device(d.data_ptr(), n, p.data_ptr(), lg.data_ptr(), 0)
    ctx.synchronize()
    return p.cpu().numpy(), lg.cpu().numpy()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("all_rows", [0, 1])
@pytest.mark.parametrize("n", [1, 5, 256])
def test_probabilities_and_logits_are_the_same_bits_with_maps_on(pkg, binding, torch_gpu, dtype, all_rows, n):
    torch = torch_gpu
    path = pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0)
    model = binding.Model(path)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, 224, seed=5))
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, last_layer_all_rows=all_rows)
    p0, l0 = _forward_dev(torch, ctx, imgs)
    ctx.attn_enable(None, rollout=True)
    p1, l1 = _forward_dev(torch, ctx, imgs)
    cls, roll = ctx.attn_read(n)
    assert np.isfinite(cls).all() and np.isfinite(roll).all()
    ctx.attn_disable()
    p2, l2 = _forward_dev(torch, ctx, imgs)
    for p, lg in ((p1, l1), (p2, l2)):
        assert np.array_equal(p.view(np.uint32), p0.view(np.uint32)) and np.array_equal(lg.view(np.uint32), l0.view(np.uint32))
    ctx.close(); model.close()


def test_probabilities_are_the_same_bits_with_maps_on_for_a_q4_0_file(pkg, binding, torch_gpu, tmp_path):
    torch = torch_gpu
    src = pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0)
    q4 = str(tmp_path / "tiny-q4_0.gguf")
    binding.quantize_file(src, q4, 2)
    model = binding.Model(q4)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(5, 224, seed=6))
    ctx = binding.Context(model, device=0, max_batch=5, dtype=binding.BF16)
    p0, l0 = _forward_dev(torch, ctx, imgs)
    ctx.attn_enable([0, 5, 11], rollout=True)
    p1, l1 = _forward_dev(torch, ctx, imgs)
    assert np.array_equal(p1.view(np.uint32), p0.view(np.uint32)) and np.array_equal(l1.view(np.uint32), l0.view(np.uint32))
    ctx.close(); model.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_map_bits_of_an_image_do_not_depend_on_its_batch(pkg, binding, torch_gpu, dtype):
    from conftest import boundary_rows
    torch = torch_gpu
    path = pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0)
    ids = boundary_rows(binding, path, 256, dtype)
    model = binding.Model(path)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(256, 224, seed=8))
    ctx = binding.Context(model, device=0, max_batch=256, dtype=dtype)
    ctx.attn_enable([0, 6, 11], rollout=True)
    _forward_dev(torch, ctx, imgs)
    cls, roll = ctx.attn_read(256)
    for i in ids:
        _forward_dev(torch, ctx, imgs[i:i + 1])
        c1, r1 = ctx.attn_read(1)
        assert np.array_equal(c1[0].view(np.uint32), cls[i].view(np.uint32)), i
        assert np.array_equal(r1[0].view(np.uint32), roll[i].view(np.uint32)), i
    ctx.close(); model.close()


@pytest.mark.parametrize("dtype,opts", [(0, {}), (1, {}), (0, {"f16_fast_attention": 1})])
def test_last_layer_map_and_rollout_are_the_same_bits_with_the_class_rows_only_tail(pkg, binding, torch_gpu, dtype, opts):
    torch = torch_gpu
    path = pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0)
    model = binding.Model(path)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(20, 224, seed=9))
    got = []
    for all_rows in (0, 1):
        ctx = binding.Context(model, device=0, max_batch=20, dtype=dtype, last_layer_all_rows=all_rows, **opts)
        ctx.attn_enable([11], rollout=True)
        _forward_dev(torch, ctx, imgs)
        got.append(ctx.attn_read(20))
        ctx.close()
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))
    assert np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))
    model.close()


def test_graph_context_gives_the_same_bits_and_replays_its_graph_after_maps_are_off(pkg, binding, torch_gpu):
    path = pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0)
    model = binding.Model(path)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(4, 224, seed=10))
    ref = binding.Context(model, device=0, max_batch=4, dtype=binding.F16, graph=0)
    p_ref = ref.forward(imgs)
    ref.attn_enable(None, rollout=True)
    ref.forward(imgs)
    m_ref = ref.attn_read()
    ctx = binding.Context(model, device=0, max_batch=4, dtype=binding.F16, graph=1)
    for _ in range(2):                       # the second identical call is captured and launched as a graph
        assert np.array_equal(ctx.forward(imgs).view(np.uint32), p_ref.view(np.uint32))
    assert ctx.graph_launches() == 1
    ctx.attn_enable(None, rollout=True)
    for _ in range(2):                       # maps on: direct launches, the cached graph is left alone
        assert np.array_equal(ctx.forward(imgs).view(np.uint32), p_ref.view(np.uint32))
        m = ctx.attn_read()
        assert np.array_equal(m[0].view(np.uint32), m_ref[0].view(np.uint32)) and np.array_equal(m[1].view(np.uint32), m_ref[1].view(np.uint32))
    assert ctx.graph_launches() == 1
    ctx.attn_disable()
    for i in range(3):                       # replays the graph captured before the maps were on
        assert np.array_equal(ctx.forward(imgs).view(np.uint32), p_ref.view(np.uint32))
        assert ctx.graph_launches() == 2 + i
    ctx.close(); ref.close(); model.close()


# ------------------------------------------------------------------------------------------------ errors
def test_attention_map_errors(pkg, binding, torch_gpu):
    L = binding.lib()
    path = pkg.synth.cached_synthetic("vit_micro_patch16_64")
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=4, dtype=binding.F16)
    assert L.vitx_attn_enable(ctx._h, 1 << 2, 0) == ERR_ARG                  # the model has 2 layers
    assert L.vitx_attn_enable(ctx._h, 1, 2) == ERR_ARG                       # unknown flag
    assert L.vitx_attn_floats(ctx._h) == 0
    ctx.attn_enable([1], rollout=True)
    assert L.vitx_attn_floats(ctx._h) == 2 * 17 + 17
    buf = np.empty(4 * 51, np.float32)
    fp = buf.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_float))
    assert L.vitx_attn_read(ctx._h, fp, buf.size) == ERR_ARG                 # before any forward with maps on
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(3, 64))
    ctx.forward(imgs)
    assert L.vitx_attn_read(ctx._h, fp, 3 * 51 - 1) == ERR_ARG               # too small
    assert L.vitx_attn_read(ctx._h, fp, 3 * 51) == 0
    assert L.vitx_attn_images(ctx._h) == 3
    with pytest.raises(ValueError):
        ctx.attn_read(4)                                                     # the last forward had 3 images
    assert ctx.attn_read()[0].shape == (3, 1, 2, 17)
    ctx.attn_enable([0])                                                     # re-enabling forgets the last forward
    assert L.vitx_attn_read(ctx._h, fp, buf.size) == ERR_ARG
    ctx.attn_disable()
    assert L.vitx_attn_floats(ctx._h) == 0 and L.vitx_attn_read(ctx._h, fp, buf.size) == ERR_ARG
    ctx.close(); model.close()

    st = binding.Model(pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0))
    sctx = binding.Context(st, device=0, max_batch=1, dtype=binding.F16)
    assert L.vitx_attn_enable(sctx._h, 1, 0) == ERR_UNSUPPORTED
    sctx.close(); st.close()

    big = binding.Model(_synthetic(pkg, "vit_micro_patch4_128"))                       # 32 x 32 patches + 1 = 1025 tokens
    bctx = binding.Context(big, device=0, max_batch=1, dtype=binding.F16)
    assert L.vitx_attn_enable(bctx._h, 0, binding.ATTN_ROLLOUT) == ERR_UNSUPPORTED
    bctx.attn_enable([0, 1])                                                 # class-token maps have no token limit
    bctx.forward(pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(1, 128)))
    cls, _ = bctx.attn_read()
    assert cls.shape == (1, 2, 2, 1025) and np.abs(cls.sum(-1) - 1).max() <= 1e-5
    bctx.close(); big.close()


def test_maps_take_one_pass(pkg, binding, torch_gpu):
    """A forward of more images than one pass of the kernels takes (F16 parity ViT-B: about 2200) is refused with maps on, before anything runs."""
    torch = torch_gpu
    L = binding.lib()
    model = binding.Model(pkg.synth.cached_synthetic("vit_base_patch16_224", head_scale=4.0))
    ctx = binding.Context(model, device=0, max_batch=2300, dtype=binding.F16, streams=1)
    limit = ctx.split(2300)[0]                   # the first pass of a larger batch = one pass's worth
    assert limit < 2300
    ctx.attn_enable([0])
    n = limit + 1
    x = torch.zeros((n, 224, 224, 3), dtype=torch.float32, device="cuda")        # sized for the call: memory-safe even if the check were gone
    p = torch.zeros((n, model.num_classes), dtype=torch.float32, device="cuda")
    assert L.vitx_forward_device(ctx._h, x.data_ptr(), n, p.data_ptr(), None, None) == ERR_ARG
    assert L.vitx_attn_images(ctx._h) == 0
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ CLI
@pytest.mark.parametrize("kind", ["rollout", "last"])
def test_cli_writes_the_attention_map_as_pgm(pkg, binding, torch_gpu, tmp_path, kind):
    path = pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0)
    img = pkg.synth.synthetic_images_u8(1, 224, seed=11)[0]
    ppm = tmp_path / "img.ppm"
    ppm.write_bytes(b"P6\n224 224\n255\n" + np.ascontiguousarray(img, np.uint8).tobytes())
    out = tmp_path / "map.pgm"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "vit_cli.py"), "-m", path, "-i", str(ppm), "--attn-map", str(out), "--attn-kind", kind],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    data = out.read_bytes()
    head = b"P5\n224 224\n255\n"
    assert data.startswith(head) and len(data) == len(head) + 224 * 224
    pic = np.frombuffer(data[len(head):], np.uint8).reshape(224, 224)
    # the same map through the binding (the CLI's context: F16, batch 1)
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=1, dtype=binding.F16)
    x = binding.preprocess(img, 224)[None]
    ctx.attn_enable([] if kind == "rollout" else [11], rollout=kind == "rollout")
    ctx.forward(x)
    cls, roll = ctx.attn_read()
    grid = ctx.attn_grid(roll[0] if kind == "rollout" else cls[0, 0].mean(axis=0))
    gi, gj = np.unravel_index(int(np.argmax(grid)), grid.shape)
    assert pic[gi * 16:(gi + 1) * 16, gj * 16:(gj + 1) * 16].min() == 255 == pic.max()
    ctx.close(); model.close()


def test_a_refused_enable_leaves_the_maps_on(pkg, binding, torch_gpu):
    """A vitx_attn_enable that is refused for its arguments (unknown flags) leaves the maps as they were enabled: the next forward gives the same bits."""
    L = binding.lib()
    model = binding.Model(pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0))
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(4, 224, seed=10))
    ctx = binding.Context(model, device=0, max_batch=4, dtype=binding.F16)
    ctx.attn_enable([2, 11], rollout=True)
    ctx.forward(imgs)
    cls, roll = ctx.attn_read(4)
    fpi = L.vitx_attn_floats(ctx._h)
    assert L.vitx_attn_enable(ctx._h, 1, 0x100) == binding.ERR_ARG
    ctx.forward(imgs)
    assert L.vitx_attn_images(ctx._h) == 4 and L.vitx_attn_floats(ctx._h) == fpi
    cls2, roll2 = ctx.attn_read(4)
    assert np.array_equal(cls2.view(np.uint32), cls.view(np.uint32)) and np.array_equal(roll2.view(np.uint32), roll.view(np.uint32))
    ctx.close(); model.close()
