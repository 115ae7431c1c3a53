"""MXFP8 operand mode on the GPU (include/vitx.h VITX_MXFP8; gemm_mx8.hip).

  - the block-scaled GEMM's operand and scale lane maps, with integer-valued elements, distinct power-of-two block scales and an
    asymmetric W, small enough that every f32 partial sum is exact: the result must equal float64 bit for bit;
  - each epilogue on random data against float64 on the decoded operands (the GELU -> MX output against the reference encoder);
  - the device encoder and the LayerNorm -> MX kernel against the host / reference encoders;
  - the forward: agreement with the BF16 context, bits independent of the batch, the sub-batch cut and graph replay, the class-rows tail,
    attention maps and the trace in an MX context, a q4_0 file, LayerNorm fusion off."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID = 0, 1, 2


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bf16(torch, x64):
    return torch.from_numpy(np.asarray(x64, np.float32)).to(torch.bfloat16).float().numpy()


def _gelu64(v):
    return 0.5 * v * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * v * (1.0 + 0.044715 * v * v)))


def _int_operand(rng, rows, K, salt):
    """Integer elements in [-4, 4] (exact e4m3 codes), scale bytes 125..129 distinct between neighbouring blocks."""
    from vitcpp_amd import mxfp8
    kp = mxfp8.k_pad_of(K)
    vals = rng.integers(-4, 5, (rows, K)).astype(np.float32)
    q = np.zeros((rows, kp), np.uint8)
    q[:, :K] = _codes(vals)
    nb = kp // 32
    s = (125 + (np.arange(rows)[:, None] * 3 + np.arange(nb)[None, :] + salt) % 5).astype(np.uint8)
    s[:, (K + 31) // 32:] = 127
    return q, s, kp


def _codes(vals):
    import torch
    return torch.from_numpy(np.ascontiguousarray(vals, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


@pytest.mark.parametrize("K", [192, 768, 3072])
@pytest.mark.parametrize("N", [768, 2304, 3072])
@pytest.mark.parametrize("M", [1, 37, 300])
def test_gemm_lane_maps_exact(binding, torch_gpu, M, N, K):
    torch = torch_gpu
    from vitcpp_amd import mxfp8
    rng = np.random.default_rng(M * 7 + N + K)
    qa, sa, kp = _int_operand(rng, M, K, 0)
    n_pad = (N + 127) // 128 * 128
    qw, sw, _ = _int_operand(rng, n_pad, K, 2)
    qw[N:] = 0; sw[N:] = 127
    qw[:N, :K] = _codes(rng.integers(-4, 5, (N, K)).astype(np.float32) + (np.arange(N)[:, None] % 3 == 0))   # W is not A's transpose pattern
    bias = rng.integers(-8, 9, N).astype(np.float32)
    ref = mxfp8.decode(qa, sa, K) @ mxfp8.decode(qw[:N], sw[:N], K).T + bias          # exact in float64 and in f32
    assert np.abs(ref).max() < 2.0 ** 23
    d = [_dev(torch, a) for a in (qa, sa, qw, sw, bias)]
    x0 = rng.integers(-16, 17, (M, N)).astype(np.float32)
    out = _dev(torch, x0.copy())
    binding.op_gemm_mxfp8(EPI_BIAS_RESID, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), out.data_ptr(), 0, M, N, K)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), (ref + x0).astype(np.float32))
    ob = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
    binding.op_gemm_mxfp8(EPI_BIAS, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), ob.data_ptr(), 0, M, N, K)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ob.float().cpu().numpy(), _bf16(torch, ref))


def _random_operands(rng, M, N, K, spread=True):
    from vitcpp_amd import mxfp8
    a = rng.standard_normal((M, K)).astype(np.float32)
    if spread:
        a *= np.exp2(rng.integers(-3, 4, (M, K // 32 if K % 32 == 0 else K // 32 + 1))).repeat(32, axis=1)[:, :K].astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    n_pad = (N + 127) // 128 * 128
    wp = np.zeros((n_pad, K), np.float32); wp[:N] = w
    qa, sa = mxfp8.encode(a); qw, sw = mxfp8.encode(wp)
    return qa, sa, qw, sw, mxfp8.decode(qa, sa, K), mxfp8.decode(qw[:N], sw[:N], K)


def _near_boundary(amax, rel=1e-6):
    """Blocks whose maximum lies within `rel` (relative) of a scale boundary (m = 1.75 or a power of two)."""
    amax = np.asarray(amax, np.float64)
    m = amax / np.exp2(np.floor(np.log2(np.maximum(amax, 1e-300))))
    return (np.abs(m - 1.75) <= 1.75 * rel) | (np.abs(m - 2.0) <= 2 * rel) | (np.abs(m - 1.0) <= rel)


@pytest.mark.parametrize("M,N,K", [(37, 768, 768), (300, 2304, 768), (513, 3072, 768), (300, 768, 3072), (129, 384, 192), (45, 200, 320), (70, 2320, 768)])
def test_gemm_epilogues_against_float64(binding, torch_gpu, M, N, K):
    torch = torch_gpu
    from vitcpp_amd import mxfp8
    rng = np.random.default_rng(M + N + K)
    qa, sa, qw, sw, a64, w64 = _random_operands(rng, M, N, K)     # N = 200, 2320: a partial column tile and partial 32-column blocks
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    acc = a64 @ w64.T
    scale = np.abs(a64) @ np.abs(w64).T                       # sum |a w| per element
    # the block-scaled MFMA does not accumulate like an f32 fma chain: measured up to 1.6e-5 sum|a w| at K = 768 (8x an f32 chain)
    tol = 5e-5 * scale + 1e-30
    d = [_dev(torch, x) for x in (qa, sa, qw, sw, bias)]
    ptrs = [t.data_ptr() for t in d]
    # fc2: f32 residual in place
    x0 = rng.standard_normal((M, N)).astype(np.float32)
    out = _dev(torch, x0.copy())
    binding.op_gemm_mxfp8(EPI_BIAS_RESID, *ptrs, out.data_ptr(), 0, M, N, K)
    torch.cuda.synchronize()
    err = np.abs(out.cpu().numpy() - ((acc + bias) + x0))
    print(f"MX GEMM M {M} N {N} K {K}: max |err| / sum|a w| = {float((err / scale).max()):.2e}")
    assert (err <= tol + 2 * np.abs(x0) * 2.0 ** -24 + 1e-6).all(), float((err / scale).max())
    # qkv: bf16 out
    ob = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
    binding.op_gemm_mxfp8(EPI_BIAS, *ptrs, ob.data_ptr(), 0, M, N, K)
    torch.cuda.synchronize()
    v = acc + bias
    err = np.abs(ob.float().cpu().numpy() - v)
    assert (err <= tol + np.abs(v) * 2.0 ** -8).all(), "bf16 out"
    # fc1: GELU -> MX elements + scales against the reference encoder of the float64 GELU
    kn = mxfp8.k_pad_of(N)
    oq = torch.full((M, kn), 0x55, dtype=torch.uint8, device="cuda"); os_ = torch.full((M, kn // 32), 0x55, dtype=torch.uint8, device="cuda")
    binding.op_gemm_mxfp8(EPI_BIAS_GELU, *ptrs, oq.data_ptr(), os_.data_ptr(), M, N, K)
    torch.cuda.synchronize()
    g = _gelu64(v)
    qr, sr = mxfp8.encode(g.astype(np.float32), kn)
    qg, sg = oq.cpu().numpy(), os_.cpu().numpy()
    gp = np.zeros((M, kn)); gp[:, :N] = g
    amax = np.abs(gp).reshape(M, kn // 32, 32).max(axis=2)
    # the GELU's input carries the GEMM's error (tol, relative to sum|a w|, not to the value); |gelu'| <= 1.13.  A block's maximum can move
    # by at most 1.13 x the largest tol of the block: that, relative to the maximum, is how close to a scale boundary a block may differ
    tp = np.zeros((M, kn)); tp[:, :N] = 1.13 * tol
    blk_rel = tp.reshape(M, kn // 32, 32).max(axis=2) / np.maximum(amax, 1e-30)
    _check_encoded(qg, sg, qr, sr, amax, N, tol_rel=blk_rel, slack=1.13 * tol)


def _check_encoded(qg, sg, qr, sr, amax, K, tol_rel, slack=0.0):
    """Device encoding of values that differ from float64 by the producer's own error against the reference encoder of float64:
    scales equal except on blocks whose maximum lies within that error of a scale boundary; elements within one e4m3 step of the
    coarser of the two scales plus the producer's absolute error `slack`; padding zero with scale 127."""
    from vitcpp_amd import mxfp8
    rows = qg.shape[0]
    assert (qg[:, K:] == 0).all() and (sg[:, (K + 31) // 32:] == 127).all()
    diff = sg != sr
    near = _near_boundary(amax, np.maximum(tol_rel, 1e-6))
    assert not (diff & ~near).any(), f"{int((diff & ~near).sum())} scales differ away from a boundary"
    print(f"  scale check: {float(1 - near.mean()):.4f} of the blocks must match exactly")
    assert near.mean() < 0.05                                  # the exemption is narrow: almost every block's scale is checked
    dec, ref_dec = mxfp8.decode(qg, sg, K), mxfp8.decode(qr, sr, K)
    assert np.isfinite(dec).all()
    s_hi = np.repeat(np.maximum(sg, sr).astype(np.float64) - 127, 32, axis=1)[:, :K]
    mag = np.maximum(np.abs(dec), np.abs(ref_dec)) * np.exp2(-s_hi)
    step = np.exp2(s_hi) * np.where(mag < 2.0 ** -6, 2.0 ** -9, np.exp2(np.floor(np.log2(np.maximum(mag, 2.0 ** -6))) - 3))
    bad = np.argwhere(np.abs(dec - ref_dec) > step * 1.0001 + slack)
    for r, k in bad[:6]:
        print(f"  row {r} col {k}: device {dec[r, k]:.6e} ref {ref_dec[r, k]:.6e} step {step[r, k]:.3e} scales {sg[r, k // 32]} {sr[r, k // 32]}")
    assert len(bad) == 0, f"{len(bad)} elements more than one e4m3 step apart"
    same = float(np.mean(qg[:, :K] == qr[:, :K]))
    print(f"  encoded: {same:.4f} of the elements and {1 - float(diff.mean()):.5f} of the scales equal the reference encoder's")
    assert same > 0.95


def test_device_encoder_matches_host_bit_for_bit(binding, torch_gpu):
    torch = torch_gpu
    import importlib.util
    spec = importlib.util.spec_from_file_location("tcm", os.path.join(ROOT, "tests", "test_cpu_mxfp8.py"))
    tcm = importlib.util.module_from_spec(spec); spec.loader.exec_module(tcm)
    rng = np.random.default_rng(11)
    for x in (tcm.adversarial_rows(), (rng.standard_normal((65, 1000)) * np.exp2(rng.integers(-40, 40, (65, 1)))).astype(np.float32)):
        rows, K = x.shape
        for kp in (binding.mx_k_pad(K), binding.mx_k_pad(K) + 128):
            q, s = binding.mxfp8_quantize(x, kp)
            dx = _dev(torch, x)
            dq = torch.full((rows, kp), 0x55, dtype=torch.uint8, device="cuda"); ds = torch.full((rows, kp // 32), 0x55, dtype=torch.uint8, device="cuda")
            binding.op_quantize_mxfp8(dx.data_ptr(), rows, K, kp, dq.data_ptr(), ds.data_ptr())
            torch.cuda.synchronize()
            np.testing.assert_array_equal(ds.cpu().numpy(), s)
            np.testing.assert_array_equal(dq.cpu().numpy(), q)


@pytest.mark.parametrize("D", [192, 384, 768, 1024, 64, 1280])
def test_layernorm_mx_against_float64(binding, torch_gpu, D):
    torch = torch_gpu
    from vitcpp_amd import mxfp8
    M = 203
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((M, D)) * 3 + rng.standard_normal((M, 1))).astype(np.float32)
    w = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32); b = (0.2 * rng.standard_normal(D)).astype(np.float32)
    kp = binding.mx_k_pad(D)
    dx, dw, db = _dev(torch, x), _dev(torch, w), _dev(torch, b)
    dq = torch.full((M, kp), 0x55, dtype=torch.uint8, device="cuda"); ds = torch.full((M, kp // 32), 0x55, dtype=torch.uint8, device="cuda")
    binding.op_layernorm_mxfp8(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), dq.data_ptr(), ds.data_ptr(), M, D, 1e-6)
    torch.cuda.synchronize()
    x64 = x.astype(np.float64)
    y = (x64 - x64.mean(1, keepdims=True)) / np.sqrt(x64.var(1, keepdims=True) + 1e-6) * w + b
    qr, sr = mxfp8.encode(y.astype(np.float32), kp)
    qg, sg = dq.cpu().numpy(), ds.cpu().numpy()
    yp = np.zeros((M, kp)); yp[:, :D] = y
    _check_encoded(qg, sg, qr, sr, np.abs(yp).reshape(M, kp // 32, 32).max(axis=2), D, tol_rel=1e-5)


# ------------------------------------------------------------------------------------------------ forward
def _decided(p, margin=0.02):
    s = np.sort(p, axis=1)
    return (s[:, -1] - s[:, -2]) > margin


# measured on these 48 images: 0.072 (ViT-B) and 0.0027 (ViT-tiny); on 256 ViT-B images tools/mxfp8_cost.py saw 0.106, so the ViT-B bound
# is set at 0.15: 2.1x the 48-image value, 1.4x the 256-image one
@pytest.mark.parametrize("name,n,dp_max", [("vit_base_patch16_224", 48, 0.15), ("vit_tiny_patch16_224", 48, 0.01)])
def test_forward_agrees_with_bf16(pkg, binding, torch_gpu, name, n, dp_max):
    """Synthetic random-init files: their class probabilities are nearly flat, so a top-1 flip needs only a small change; rows whose
    BF16 top-2 gap exceeds twice the bound on max |dp| cannot flip and are checked."""
    path = pkg.synth.cached_synthetic(name, head_scale=4.0)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, 224))
    model = binding.Model(path)
    p_mx = binding.Context(model, device=0, max_batch=n, dtype=binding.MXFP8).forward(imgs)
    p_bf = binding.Context(model, device=0, max_batch=n, dtype=binding.BF16).forward(imgs)
    assert np.isfinite(p_mx).all()
    dp = float(np.abs(p_mx - p_bf).max())
    dec = _decided(p_bf, 2 * dp_max)
    print(f"{name}: MXFP8 vs BF16 max|dp| = {dp:.3e}, top-1 equal on {int(dec.sum())} decided rows of {n}, overall {np.mean(p_mx.argmax(1) == p_bf.argmax(1)):.3f}")
    assert dp < dp_max
    assert (p_mx.argmax(1)[dec] == p_bf.argmax(1)[dec]).all()


def test_bits_independent_of_batch_split_and_graph(pkg, binding, torch_gpu):
    path = pkg.synth.cached_synthetic("vit_base_patch16_224", head_scale=4.0)
    model = binding.Model(path)
    n = 256
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, 224))
    ctx = binding.Context(model, device=0, max_batch=n, dtype=binding.MXFP8)
    assert ctx.ln_fusion_active() == 0
    assert len(ctx.split(n)) == 2
    p = ctx.forward(imgs)
    one = binding.Context(model, device=0, max_batch=1, dtype=binding.MXFP8)
    for i in ctx.boundary_rows(n):
        np.testing.assert_array_equal(one.forward(imgs[i:i + 1])[0], p[i])
    g = binding.Context(model, device=0, max_batch=4, dtype=binding.MXFP8, graph=1)
    ref = g.forward(imgs[:4])
    for _ in range(3):
        np.testing.assert_array_equal(g.forward(imgs[:4]), ref)
    assert g.graph_launches() >= 1
    np.testing.assert_array_equal(ref, p[:4])
    full = binding.Context(model, device=0, max_batch=n, dtype=binding.MXFP8, last_layer_all_rows=1).forward(imgs)
    assert float(np.abs(full - p).max()) < 5e-3
    dec = _decided(p, 0.02)
    assert (full.argmax(1)[dec] == p.argmax(1)[dec]).all()


def test_attention_maps_and_trace_in_mx_context(pkg, binding, torch_gpu):
    path = pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0)
    model = binding.Model(path)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(6, 224))
    ctx = binding.Context(model, device=0, max_batch=6, dtype=binding.MXFP8)
    p0 = ctx.forward(imgs)
    ctx.attn_enable(layers=[0, 11], rollout=True)
    p1 = ctx.forward(imgs)
    np.testing.assert_array_equal(p0, p1)
    cls, roll = ctx.attn_read()
    assert cls.shape[:2] == (6, 2) and np.isfinite(cls).all() and np.isfinite(roll).all()
    np.testing.assert_allclose(cls.sum(axis=-1), 1.0, rtol=1e-4)
    ctx.attn_disable()
    ctx.trace_enable([0, 5])
    ctx.forward(imgs)
    tr = ctx.trace_read()
    assert tr.shape[0] == 13 and np.isfinite(tr).all()


def test_q4_0_file_runs_in_mx_context(pkg, binding, torch_gpu, tmp_path):
    src = pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0)
    q4 = str(tmp_path / "q4_0.gguf")
    binding.quantize_file(src, q4, 2)
    model = binding.Model(q4)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(32, 224))
    p_mx = binding.Context(model, device=0, max_batch=32, dtype=binding.MXFP8).forward(imgs)
    p_bf = binding.Context(model, device=0, max_batch=32, dtype=binding.BF16).forward(imgs)
    dp = float(np.abs(p_mx - p_bf).max())
    assert dp < 0.01
    dec = _decided(p_bf, 2 * dp)
    print(f"q4_0: max|dp| {dp:.2e}: top-1 equal on {int(dec.sum())} decided rows of 32, overall {np.mean(p_mx.argmax(1) == p_bf.argmax(1)):.3f}")
    assert (p_mx.argmax(1)[dec] == p_bf.argmax(1)[dec]).all()


def test_mfma_probe_mx(binding, torch_gpu):
    tf_bf, _ = binding.probe_mfma(0, binding.BF16, 2, 50.0)
    tf_mx, _ = binding.probe_mfma(0, binding.MXFP8, 2, 50.0)
    print(f"probe: bf16 {tf_bf:.0f} TF/s, MXFP8 {tf_mx:.0f} TF/s")
    assert tf_mx > tf_bf


def test_hidden_size_not_a_multiple_of_32_is_unsupported(pkg, binding, torch_gpu, tmp_path):
    from vitcpp_amd.ggml_file import HParams, write_model
    hp = HParams(80, 1, 2, 10, 16, 64, ftype=1)           # hidden 80: 2.5 MX blocks per row
    path = str(tmp_path / "h80.gguf")
    write_model(path, hp, pkg.synth.make_weights(hp))
    model = binding.Model(path)
    h = __import__("ctypes").c_void_p()
    assert binding.lib().vitx_ctx_create(model._h, 0, 4, binding.MXFP8, __import__("ctypes").byref(h)) == 5     # VITX_ERR_UNSUPPORTED


def test_group_in_mx_context_matches_the_context(pkg, binding, torch_gpu):
    path = pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0)
    model = binding.Model(path)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(8, 224))
    grp = binding.Group(model, [0], 8, binding.MXFP8)
    np.testing.assert_array_equal(grp.forward(imgs).reshape(8, -1), binding.Context(model, device=0, max_batch=8, dtype=binding.MXFP8).forward(imgs))


# ------------------------------------------------------------------------------------------------ rounding points, teacher-forced
def _weights(binding, model):
    return {name: model.tensor_f32(i).astype(np.float64).reshape(-1) for i, (name, _, _, _) in enumerate(model.tensors())}


def _ln64(x, w, b, eps=1e-6):
    m = x.mean(-1, keepdims=True)
    return (x - m) / np.sqrt(((x - m) ** 2).mean(-1, keepdims=True) + eps) * w + b


def _layer64(torch, x, W, il, H, mx_points):
    """Layer il of the encoder in float64 from its input x [N][D], rounded where a context of either kind rounds: the MX rounding points
    (norm1, norm2, fc1 output encoded; qkv, fc1, fc2 weights MX-decoded) or BF16's (the same activations and weights rounded to bf16).
    Shared: q, k, v rounded to bf16, the attention output rounded to bf16, proj weights bf16, f32 residual."""
    from vitcpp_amd import mxfp8
    N, D = x.shape
    bf = lambda a: _bf16(torch, a).astype(np.float64)
    p = f"blocks.{il}."
    def mat(n, rows, cols):
        w = W[p + n].reshape(rows, cols)
        if not mx_points:
            return bf(w)
        q, s = mxfp8.encode(w.astype(np.float32))
        return mxfp8.decode(q, s, cols)
    act = (lambda a: mxfp8.decode(*mxfp8.encode(a.astype(np.float32)), a.shape[1])) if mx_points else bf
    h = act(_ln64(x, W[p + "norm1.weight"], W[p + "norm1.bias"]))
    qkv = bf(h @ mat("attn.qkv.weight", 3 * D, D).T + W[p + "attn.qkv.bias"])
    hd = D // H
    o = np.empty((N, D))
    for hh in range(H):
        q, k, v = (qkv[:, j * D + hh * hd: j * D + (hh + 1) * hd] for j in range(3))
        o[:, hh * hd:(hh + 1) * hd] = _softmax64(q @ k.T / np.sqrt(hd)) @ v
    x1 = x + (bf(o) @ bf(W[p + "attn.proj.weight"].reshape(D, D)).T + W[p + "attn.proj.bias"])
    h2 = act(_ln64(x1, W[p + "norm2.weight"], W[p + "norm2.bias"]))
    f = act(_gelu64(h2 @ mat("mlp.fc1.weight", 4 * D, D).T + W[p + "mlp.fc1.bias"]))
    return x1 + (f @ mat("mlp.fc2.weight", D, 4 * D).T + W[p + "mlp.fc2.bias"])


def _softmax64(s):
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


# the engine's layer output must lie within LAYER_GATE (relative to the layer's own update) of the MX recompute; the BF16 recompute must not.
# Measured (2 images): against the MX recompute 2.6e-3 .. 5.1e-3 (ViT-tiny, 12 layers) and 1.0e-2 .. 1.1e-2 (ViT-B, layers 0-1); against the
# BF16 recompute 4.8e-2 .. 5.4e-2.  The gate sits 1.8x above the worst MX value and 2.4x below the best BF16 value.
LAYER_GATE = 0.02


def _layer_gate(err):
    return err <= LAYER_GATE


@pytest.mark.parametrize("name,layers", [("vit_tiny_patch16_224", range(12)), ("vit_base_patch16_224", range(2))])
def test_layers_follow_the_mx_rounding_points(pkg, binding, torch_gpu, name, layers):
    """Teacher-forced from vitx_trace_read: each layer is recomputed in float64 from the engine's own traced input, once with the MX
    rounding points and once with BF16's.  err = |engine - recompute| / |recompute - input| (the layer's update).  The engine's output
    passes the gate against the MX recompute, and the same gate FAILS with the BF16 recompute as the expected value: the test tells the
    two sets of rounding points apart (a context that rounded norm1 / norm2 / the fc1 output to bf16, or took bf16 weights, fails it)."""
    torch = torch_gpu
    path = pkg.synth.cached_synthetic(name, head_scale=4.0)
    model = binding.Model(path)
    W = _weights(binding, model)
    H = model.hparams.num_attention_heads
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(2, 224))
    ctx = binding.Context(model, device=0, max_batch=2, dtype=binding.MXFP8)
    ctx.trace_enable([0, 1])
    ctx.forward(imgs)
    tr = ctx.trace_read().astype(np.float64)
    ratios = []
    for il in layers:
        for i in range(2):
            x, out = tr[il, i], tr[il + 1, i]
            errs = {}
            for kind in ("mx", "bf16"):
                rec = _layer64(torch, x, W, il, H, kind == "mx")
                errs[kind] = float(np.linalg.norm(out - rec) / np.linalg.norm(rec - x))
            ratios.append(errs["bf16"] / errs["mx"])
            print(f"{name} layer {il} image {i}: err vs MX recompute {errs['mx']:.3e}, vs BF16 recompute {errs['bf16']:.3e}")
            assert _layer_gate(errs["mx"]), errs
            assert not _layer_gate(errs["bf16"]), errs          # the discriminating half: BF16's rounding points as the expected value fail
    print(f"{name}: err(BF16) / err(MX) min {min(ratios):.2f}, median {float(np.median(ratios)):.2f}")


# ------------------------------------------------------------------------------------------------ end to end against the oracle
def _mx_weight_file(pkg, name, path):
    """f32 file whose qkv, fc1 and fc2 weights are MX-decoded values (exact in bf16): the oracle's GPU_BF16 mode then differs from an
    MXFP8 context only at the three activation rounding points."""
    from vitcpp_amd import mxfp8
    from vitcpp_amd.ggml_file import write_model
    hp = pkg.synth.hparams_for(name, ftype=0)
    t = pkg.synth.make_weights(hp, head_scale=8.0)
    for il in range(hp.num_hidden_layers):
        for n in ("attn.qkv.weight", "mlp.fc1.weight", "mlp.fc2.weight"):
            w = t[f"blocks.{il}.{n}"]
            q, s = mxfp8.encode(w)
            t[f"blocks.{il}.{n}"] = mxfp8.decode(q, s, w.shape[1]).astype(np.float32)
    write_model(path, hp, t, ftype=0)


# max |dp| of an MXFP8 context against the oracle's GPU_BF16 mode on these files, 48 images: measured 0.119 (ViT-B/8) and 0.024 (ViT-tiny);
# the gates leave a margin of 2.1x.  The difference is the three MX activation rounding points (the bf16 context tracks this oracle to 5e-3).
ORACLE_DP = {"vit_base_patch8_224": 0.25, "vit_tiny_patch16_224": 0.05}


@pytest.mark.parametrize("name,n", [("vit_base_patch8_224", 48), ("vit_tiny_patch16_224", 48)])
def test_forward_against_the_bf16_oracle_on_mx_weights(pkg, binding, oracle, torch_gpu, tmp_path, name, n):
    import time
    path = str(tmp_path / f"{name}-mxw.gguf")
    _mx_weight_file(pkg, name, path)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, 224))
    model = binding.Model(path)
    p = binding.Context(model, device=0, max_batch=n, dtype=binding.MXFP8).forward(imgs)
    t0 = time.time()
    _, ref = oracle.OracleModel(path).forward(imgs, oracle.GPU_BF16)
    dp = float(np.abs(p - ref).max())
    dec = _decided(ref, 2 * ORACLE_DP[name])
    print(f"{name} x{n}: MXFP8 vs oracle GPU_BF16 max|dp| = {dp:.3e} (gate {ORACLE_DP[name]}), top-1 equal on {int(dec.sum())} decided rows, "
          f"overall {np.mean(p.argmax(1) == ref.argmax(1)):.3f}; oracle {time.time() - t0:.0f} s")
    assert dp <= ORACLE_DP[name]
    assert (p.argmax(1)[dec] == ref.argmax(1)[dec]).all()
