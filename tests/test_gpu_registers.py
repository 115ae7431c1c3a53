"""Register tokens and the cls + mean head on the GPU: the patch-embedding kernel's prefix rows, the forward end to end against the float64
restatement of tests/ref64.py (pinned to transformers' DINOv2 by tests/test_cpu_registers.py, which also shows that each layout
mistake moves what is compared here by more than 100 gates), the pooled-head kernel's operand, the last layer, maps, sizes and q8_0.

Synthetic model: D 128, 2 layers, 2 heads, patch 14, image 56 (16 patches; N = 17, or 21 with 4 registers), head scale 4 as the other micro
fixtures.  Images are multiples of 1/16 (exact in both operand types).  Every tolerance is the one the existing test of the same quantity
applies; the line is cited where it is used."""
import functools

import numpy as np
import pytest

import feature_data as FD
import prefix_data as PD
import ref64 as R64

pytestmark = pytest.mark.gpu

NAME = "vit_micro_patch14_56"
D, L, H, P, S = 128, 2, 2, 14, 56
ROUND = {0: PD.f16_round, 1: PD.bf16_round}
CASES = [(0, 1), (4, 0), (4, 1)]            # (registers, head_pool); (0, 0) is every existing test


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _file(pkg, R, pool, ftype=1):
    return pkg.synth.cached_synthetic(NAME, ftype=ftype, head_scale=4.0, registers=R, head_pool=pool)


@functools.lru_cache(maxsize=None)
def _images():
    return PD.exact_images(17, S, seed=1)


_REF = {}


def _ref(pkg, R, pool, dtype):
    """The restatement of all 17 images, computed once per (file, operand type) and shared (an image's result does not depend on its batch)."""
    key = (R, pool, dtype)
    if key not in _REF:
        t = PD.file_tensors(pkg, _file(pkg, R, pool))
        _REF[key] = (t, R64.forward64(t, _images(), H, wround=ROUND[dtype], uround=ROUND[dtype]))
    return _REF[key]


def _check_trace(x, ref, dtype, where):
    """x, ref [L + 1][n][N][D].  Stage 0: tests/test_gpu_parity_r02.py:266.  Later stages, F16: :271-272; BF16: :304 (the bound against a
    reference without bf16 rounding points)."""
    d0 = float(np.abs(x[0] - ref[0]).max()); g0 = 2e-5 * max(1.0, float(np.abs(ref[0]).max()))
    print(f"{where} stage 0: max|d| {d0:.3e} (gate {g0:.3e})")
    assert d0 <= g0, (where, d0, g0)
    for il, (e_max, e_rms) in enumerate(R64.stage_errors(x, ref), 1):
        print(f"{where} stage {il}: max|d| / rms {e_max:.3e}, rms(d) / rms {e_rms:.3e}")
        assert R64.stage_ok(e_max, e_rms, dtype), (where, il, e_max, e_rms)


PROB_TOL = R64.PROB_TOL                    # tests/test_gpu_parity_r02.py:262 (F16), :292 (BF16)


# ------------------------------------------------------------------------------------------------ the patch-embedding kernel
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("size,n_img", [(28, 3), (42, 15)])          # 4 patches x 3 images; 9 x 15 = 135 patch rows: a 128-row tile ends inside image 14
def test_op_patch_embed_writes_class_register_and_patch_rows(binding, torch_gpu, dtype, size, n_img):
    torch = torch_gpu
    R, g = 4, size // P
    tpi, N = g * g, g * g + 1 + R
    rng = np.random.default_rng(100 * size + dtype)
    rnd = ROUND[dtype]
    w = rnd((rng.standard_normal((D, 3 * P * P)) * 0.05).astype(np.float32))
    bias = (rng.standard_normal(D) * 0.1).astype(np.float32)
    pos = (rng.standard_normal((1 + tpi, D)) * 0.5).astype(np.float32)
    cls = (rng.standard_normal(D) * 0.5).astype(np.float32)
    reg = (rng.standard_normal((R, D)) * 0.5).astype(np.float32)
    imgs = PD.exact_images(n_img, size, seed=size)
    tail = 300                                                        # rows behind the last image: beyond the padded M of the GEMM too
    SENT = np.float32(-12345.5)
    X = torch.full((n_img * N + tail, D), float(SENT), dtype=torch.float32, device="cuda")
    dv = [_dev(torch, a) for a in (imgs, w, bias, pos, cls, reg)]
    binding.op_patch_embed(dtype, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(), dv[5].data_ptr(), R,
                           X.data_ptr(), n_img, size, P, 3, D)
    x = X.cpu().numpy()
    assert (x[n_img * N:] == SENT).all(), "rows behind the last token row were written"
    x = x[:n_img * N].reshape(n_img, N, D)
    assert np.array_equal(_bits(x[:, 0]), _bits(np.broadcast_to(cls + pos[0], (n_img, D)))), "class rows are not cls + pos[0] bit for bit"
    assert np.array_equal(_bits(x[:, 1:1 + R]), _bits(np.broadcast_to(reg, (n_img, R, D)))), "register rows are not reg_token bit for bit"
    a64 = imgs.astype(np.float64).reshape(n_img, g, P, g, P, 3).transpose(0, 1, 3, 5, 2, 4).reshape(n_img, tpi, -1)
    want = a64 @ w.astype(np.float64).T + bias + pos[1:]
    tol = (np.abs(a64) @ np.abs(w.astype(np.float64)).T) * 2e-6 + 1e-6 + np.abs(want) * 2e-7 + 1e-7          # tests/test_gpu_parity_r02.py:60, :80 (EPI_PATCH)
    err = np.abs(x[:, 1 + R:] - want)
    print(f"patch rows, size {size}, dtype {dtype}: worst err / tol {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), float((err / tol).max())


@pytest.mark.parametrize("dtype", [0, 1])
def test_op_patch_embed_without_registers_is_the_contexts_patch_embedding(pkg, binding, torch_gpu, dtype):
    """R = 0: the bits of stage 0 of a context of a file without registers (the forward's own launch)."""
    torch = torch_gpu
    path = pkg.synth.cached_synthetic(NAME, head_scale=4.0)
    t = PD.file_tensors(pkg, path)
    imgs = _images()[:3]
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=dtype)
    ctx.trace_enable([0, 1, 2]); ctx.forward(imgs)
    x0 = ctx.trace_read()[0]
    ctx.close(); model.close()
    X = torch.zeros((3 * 17, D), dtype=torch.float32, device="cuda")
    dv = [_dev(torch, a) for a in (imgs, t["patch_embed.proj.weight"].reshape(D, -1), t["patch_embed.proj.bias"].reshape(-1), t["pos_embed"][0], t["cls_token"].reshape(-1))]
    binding.op_patch_embed(dtype, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(), 0, 0, X.data_ptr(), 3, S, P, 3, D)
    assert np.array_equal(_bits(X.cpu().numpy().reshape(3, 17, D)), _bits(x0))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("R,pool", CASES)
def test_forward_with_registers_and_pooled_head_against_the_restatement(pkg, binding, torch_gpu, R, pool, dtype):
    """Batches 1, 3 and 17 (17 runs as two sub-batch streams): the trace after the patch embedding and after each layer, and the probabilities."""
    t, ref = _ref(pkg, R, pool, dtype)
    imgs = _images()
    N = 17 + R
    model = binding.Model(_file(pkg, R, pool))
    assert (model.num_registers, model.head_pool) == (R, pool)
    ctx = binding.Context(model, device=0, max_batch=17, dtype=dtype)
    assert (ctx.tokens, ctx.registers, ctx.prefix) == (N, R, 1 + R) and len(ctx.split(17)) == 2
    plain = {n: ctx.forward(imgs[:n]) for n in (1, 3, 17)}            # untraced: the class-rows-only last layer where the model keeps it
    for n in (1, 3, 17):
        p = plain[n]
        d = float(np.abs(p - ref["probs"][:n]).max())
        print(f"R={R} pool={pool} dtype={dtype} batch {n}: max|dprob| {d:.3e}")
        assert np.isfinite(p).all() and np.abs(p.sum(1) - 1).max() < 1e-4
        assert d <= PROB_TOL[dtype], (n, d)
        assert (p.argmax(1) == ref["probs"][:n].argmax(1)).all()
    # an image's probability bits do not depend on its batch, its position or the stream it ran on
    assert np.array_equal(_bits(plain[17][:3]), _bits(plain[3])) and np.array_equal(_bits(plain[17][:1]), _bits(plain[1]))
    for i in ctx.boundary_rows(17):
        assert np.array_equal(_bits(ctx.forward(imgs[i:i + 1])), _bits(plain[17][i:i + 1])), i
    for n in (1, 3, 17):
        ids = list(range(n)) if n <= 3 else ctx.boundary_rows(17)
        ctx.trace_enable(ids)
        p = ctx.forward(imgs[:n])
        x = ctx.trace_read()
        assert x.shape == (L + 1, len(ids), N, D)
        _check_trace(x, ref["trace"][:, ids], dtype, f"R={R} pool={pool} dtype={dtype} batch {n}")
        assert np.abs(p - ref["probs"][:n]).max() <= PROB_TOL[dtype]
    ctx.close(); model.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_features_cover_the_patch_rows_and_are_the_pooled_heads_operand(pkg, binding, torch_gpu, dtype):
    torch = torch_gpu
    R, T, N, n = 4, 5, 21, 3
    path = _file(pkg, R, 1)
    t = PD.file_tensors(pkg, path)
    imgs = _images()[:n]
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype)
    ctx.feat_enable(cls=True, mean=True, tokens=True)
    ctx.trace_enable(list(range(n)))
    probs, logits = ctx.forward(imgs, want_logits=True)
    f = ctx.feat_read(n)[L - 1]
    x_last = ctx.trace_read()[L]
    assert binding.lib().vitx_feat_floats(ctx._h) == D * (2 + N - T) and f["tokens"].shape == (n, N - T, D)
    # the restatement's final norm and pooling on the context's own last residual stream, under the bounds of tests/test_gpu_features.py:219-231
    y64, bound = FD.features64(x_last, t["norm.weight"], t["norm.bias"], PD.EPS)
    assert (np.abs(f["cls"] - y64[:, 0]) <= bound[:, 0]).all()
    assert (np.abs(f["tokens"] - y64[:, T:]) <= bound[:, T:]).all()
    m64, mb = FD.mean_bound(f["tokens"])
    assert (np.abs(f["mean"] - m64) <= mb).all()
    assert (np.abs(f["mean"] - PD.pooled64(y64, T)) <= mb + bound[:, T:].mean(axis=1)).all()                 # tests/test_gpu_features.py:232-235
    for mut in ("registers_in_mean", "mean_over_n_minus_1"):
        assert np.abs(f["mean"] - PD.pooled64(y64, T, mut)).max() > 100 * float(mb.max()), mut
    # RNE(cls) ‖ RNE(mean) through the head weights in float64 against the engine's logits: head-GEMM noise (tests/test_gpu_parity_r02.py:60, :96)
    rnd = ROUND[dtype]
    z = np.concatenate([rnd(f["cls"]), rnd(f["mean"])], 1).astype(np.float64)
    hw = rnd(t["head.weight"]).astype(np.float64)
    want = z @ hw.T + t["head.bias"]
    tol = (np.abs(z) @ np.abs(hw).T) * 2e-6 + 1e-6
    print(f"dtype {dtype}: logits vs host head on RNE(features): worst err / tol {float((np.abs(logits - want) / tol).max()):.3f}")
    assert (np.abs(logits - want) <= tol).all()
    # the operand itself, through the kernel's op entry on the same rows: RNE(feature) == operand bit for bit, and the op's features are the context's
    dx = _dev(torch, x_last); dw = _dev(torch, t["norm.weight"]); db = _dev(torch, t["norm.bias"])
    oc = torch.zeros((n, D), device="cuda"); om = torch.zeros((n, D), device="cuda")
    oz = torch.zeros((n, 2 * D), dtype=torch.float16 if dtype == 0 else torch.bfloat16, device="cuda")
    binding.op_features_ex(dx.data_ptr(), D, N * D, dw.data_ptr(), db.data_ptr(), oc.data_ptr(), om.data_ptr(), 0, D, n, N, T, D, PD.EPS, False, oz.data_ptr(), dtype)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(oc.cpu().numpy()), _bits(f["cls"])) and np.array_equal(_bits(om.cpu().numpy()), _bits(f["mean"]))
    assert np.array_equal(_bits(oz.float().cpu().numpy()), _bits(np.concatenate([rnd(f["cls"]), rnd(f["mean"])], 1)))
    # the operand alone (what a forward without features launches), and with VITX_FEAT_L2 on the features: the same operand bits
    oz2 = torch.zeros_like(oz)
    binding.op_features_ex(dx.data_ptr(), D, N * D, dw.data_ptr(), db.data_ptr(), 0, 0, 0, D, n, N, T, D, PD.EPS, False, oz2.data_ptr(), dtype)
    oz3 = torch.zeros_like(oz)
    binding.op_features_ex(dx.data_ptr(), D, N * D, dw.data_ptr(), db.data_ptr(), oc.data_ptr(), om.data_ptr(), 0, D, n, N, T, D, PD.EPS, True, oz3.data_ptr(), dtype)
    torch.cuda.synchronize()
    assert torch.equal(oz2, oz) and torch.equal(oz3, oz)
    # features off: the same probabilities and logits, bit for bit (one launch serves both; without features it writes the operand only)
    ctx.feat_disable()
    p2, l2 = ctx.forward(imgs, want_logits=True)
    assert np.array_equal(_bits(p2), _bits(probs)) and np.array_equal(_bits(l2), _bits(logits))
    ctx.close(); model.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_last_layer_of_pooled_and_class_token_heads(pkg, binding, torch_gpu, dtype):
    imgs = _images()
    # pooled head: every row of the last layer, bit-identical to last_layer_all_rows = 1
    model = binding.Model(_file(pkg, 4, 1))
    out = []
    for opts in ({}, {"last_layer_all_rows": 1}):
        ctx = binding.Context(model, device=0, max_batch=17, dtype=dtype, **opts)
        out.append(ctx.forward(imgs, want_logits=True)); ctx.close()
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))
    model.close()
    # class-token head with registers: the class-rows-only shortcut stays, within the bound of tests/test_gpu_cls_tail.py:131-135
    model = binding.Model(_file(pkg, 4, 0))
    res = {}
    for label, opts in (("cls", {}), ("all", {"last_layer_all_rows": 1})):
        ctx = binding.Context(model, device=0, max_batch=17, dtype=dtype, **opts)
        ctx.profile_enable(True); res[label] = ctx.forward(imgs)
        names = [p["name"] for p in ctx.profile_read()]
        assert ("attention_cls" in names) == (label == "cls"), names
        ctx.close()
    model.close()
    d = float(np.abs(res["cls"] - res["all"]).max())
    print(f"dtype {dtype}: class rows only vs every row, R = 4: max|dprob| {d:.3e}")
    assert d <= (1e-3 if dtype == 0 else 6e-3) and (res["cls"].argmax(1) == res["all"].argmax(1)).all()


@pytest.mark.parametrize("dtype", [0, 1])
def test_attention_maps_include_the_registers(pkg, binding, torch_gpu, dtype):
    R, N, n = 4, 21, 3
    path = _file(pkg, R, 1)
    t = PD.file_tensors(pkg, path)
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype)
    ctx.trace_enable(list(range(n)))
    ctx.attn_enable(None, rollout=True)
    ctx.forward(_images()[:n])
    assert binding.lib().vitx_attn_floats(ctx._h) == L * H * N + N            # popcount . H . N (+ the rollout row), N with the registers
    cls, roll = ctx.attn_read()
    trace = ctx.trace_read()
    assert cls.shape == (n, L, H, N) and roll.shape == (n, N)
    assert np.abs(cls.sum(-1) - 1).max() <= 1e-5 and np.abs(roll.sum(-1) - 1).max() <= 1e-4      # tests/test_gpu_attn_map.py:82, :182
    assert ctx.attn_grid(cls).shape == (n, L, H, 4, 4) and np.array_equal(ctx.attn_grid(cls).reshape(n, L, H, 16), cls[..., 1 + R:])
    parity = dtype == 0
    tol = 2e-3 if parity else 3e-2                                             # tests/test_gpu_attn_map.py:165, :171
    rnd = ROUND[dtype]
    for l in range(L):
        q, k, _v = R64.qk64(t, trace[l], l, H, wround=rnd, uround=rnd)          # the restatement's q, k from the stream that enters layer l
        if not parity:
            q, k = rnd(q).astype(np.float64), rnd(k).astype(np.float64)       # the context holds q, k in the operand type (the parity mode: f32 grade)
        ref = PD.cls_maps64(q, k)
        err = np.abs(cls[:, l] - ref).max(axis=-1)
        print(f"dtype {dtype} layer {l}: worst map err / row max {float((err / ref.max(axis=-1)).max()):.3e} (tol {tol})")
        assert (err <= tol * ref.max(axis=-1)).all(), l
    ctx.close(); model.close()


def test_context_at_another_image_size_keeps_the_registers_untouched(pkg, binding, torch_gpu):
    """img_size 84 from the 56 file: 36 patches + 5 prefix tokens, on the host-resampled table [1 + 36]."""
    R, dtype, n = 4, 0, 3
    path = _file(pkg, R, 1)
    t = PD.file_tensors(pkg, path)
    imgs = PD.exact_images(n, 84, seed=84)
    pos = binding.pos_embed_resample(t["pos_embed"][0], 6, binding.POS_BICUBIC)
    ref = R64.forward64(t, imgs, H, pos=pos, wround=ROUND[dtype], uround=ROUND[dtype])
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, img_size=84)
    assert (ctx.tokens, ctx.registers, ctx.grid) == (41, 4, 6)
    ctx.trace_enable(list(range(n)))
    p = ctx.forward(imgs)
    x = ctx.trace_read()
    assert np.array_equal(_bits(x[0][:, 1:5]), _bits(np.broadcast_to(t["reg_token"][0], (n, 4, D))))
    _check_trace(x, ref["trace"], dtype, "img_size 84")
    assert np.abs(p - ref["probs"]).max() <= PROB_TOL[dtype]
    ctx.close(); model.close()


def test_q8_0_register_file_matches_the_restatement_on_dequantised_weights(pkg, binding, torch_gpu, tmp_path):
    src = _file(pkg, 4, 1)
    q8 = str(tmp_path / "q8.gguf")
    binding.quantize_file(src, q8, 8)
    t = PD.file_tensors(pkg, q8)
    imgs = _images()[:3]
    ref = R64.forward64(t, imgs, H, wround=PD.f16_round, uround=PD.f16_round)
    model = binding.Model(q8)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=0)
    p = ctx.forward(imgs)
    ctx.close(); model.close()
    d = float(np.abs(p - ref["probs"]).max())
    print(f"q8_0, R = 4, pooled head: max|dprob| {d:.3e}")
    assert d <= 1e-3 and (p.argmax(1) == ref["probs"].argmax(1)).all()          # tests/test_gpu_quant.py:137-138


def test_unsupported_combinations_are_refused_at_context_creation(pkg, binding, torch_gpu, tmp_path):
    import ctypes as C
    ERR_UNSUPPORTED = 5
    L_ = binding.lib()
    model = binding.Model(_file(pkg, 4, 1))
    h = C.c_void_p()
    assert L_.vitx_ctx_create(model._h, 0, 1, binding.MXFP8, C.byref(h)) == ERR_UNSUPPORTED
    model.close()
    # a one-channel (ViTSTR) file with registers
    hp = pkg.synth.hparams_for("vitstr_tiny_patch16_224")
    w = pkg.synth.make_weights(hp, head_scale=4.0, in_chans=1, registers=2)
    p = str(tmp_path / "vitstr_reg.gguf")
    pkg.ggml_file.write_model(p, hp, w, id2label=dict(pkg.synth.VITSTR_LABELS))
    model = binding.Model(p)
    assert (model.in_channels, model.num_registers) == (1, 2)
    assert L_.vitx_ctx_create(model._h, 0, 1, binding.F16, C.byref(h)) == ERR_UNSUPPORTED
    model.close()
