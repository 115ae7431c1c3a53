"""Rectangular contexts on the GPU (include/vitx.h "rectangular contexts"): the patch-embedding kernel bit for bit on exact data at rectangular
grids, the forward of vitx_ctx_create_rect against the float64 restatement of tests/ref64.py under its gates with
every mutant outside them, bit-equality with the square path, the persistent attention band, batch invariance, the outputs, the device
preprocessing against the host's, the refusals, and vit_cli.py --img-fit and examples/embed_main.cpp --img-shape against the binding path."""
import ctypes as C
import functools

import numpy as np
import pytest

import arch_data as AD
import feature_data as FD
import prefix_data as PD
import preproc_data as PPD
import rect_data as XD
import ref64 as R64
import rope_data as RD
from ref64 import PROB_TOL
from test_gpu_arch import ROUND, _check_trace, _outside

pytestmark = pytest.mark.gpu

D, L, H = 128, 2, 2
SENT = np.float32(-12345.5)
MODES = {"f16_parity": 0, "bf16": 1}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the patch embedding alone, on exact data
def _exact_case(P, gh, gw, n, R, with_cls, Dn=36):
    """Images whose pixel (b, y, x, c) holds the small integer ((y W + x) 3 + c + 17 b) mod 253 - 126, a selector matrix (row d is one-hot on k_d; the
    k_d include the patch's four corners and its last element), zero bias, an integer table distinct per (row, d), integer class and register rows:
    every product and sum is exact in bf16, fp16 and f32, so X is known to the bit."""
    Hh, Ww, K = gh * P, gw * P, 3 * P * P
    b, y, x, c = np.meshgrid(np.arange(n), np.arange(Hh), np.arange(Ww), np.arange(3), indexing="ij")
    imgs = ((((y * Ww + x) * 3 + c + 17 * b) % 253) - 126).astype(np.float32)
    corners = [0, P - 1, (P - 1) * P, P * P - 1, K - 1]                       # file order [c][ky][kx]: channel 0's corners, the last element
    rest = np.random.default_rng(P * 100 + gh * 10 + gw).choice(np.setdiff1d(np.arange(K), corners), Dn - len(corners), replace=False)
    ks = np.concatenate([corners, rest])
    w = np.zeros((Dn, K), np.float32); w[np.arange(Dn), ks] = 1.0
    tpi, T = gh * gw, (1 + R if with_cls else 0)
    pos = (np.arange((tpi + (1 if with_cls else 0)) * Dn).reshape(-1, Dn) % 2039 - 1000).astype(np.float32)
    cls = (np.arange(Dn) * 3 - 50).astype(np.float32)
    reg = (np.arange(max(R, 1) * Dn).reshape(-1, Dn) * 5 - 400).astype(np.float32)
    patches = imgs.reshape(n, gh, P, gw, P, 3).transpose(0, 1, 3, 5, 2, 4).reshape(n, tpi, K)
    want = np.empty((n, tpi + T, Dn), np.float32)
    if with_cls:
        want[:, 0] = cls + pos[0]
        want[:, 1:T] = reg[:R]
        want[:, T:] = patches[:, :, ks] + pos[1:]
    else:
        want[:] = patches[:, :, ks] + pos
    return imgs, w, pos, cls, reg, want.reshape(n * (tpi + T), Dn)


def _run_embed(binding, torch, dtype, imgs, w, pos, cls, reg, R, with_cls, P, rows, rect=True):
    n, Hh, Ww = imgs.shape[:3]
    Dn = w.shape[0]
    X = torch.full((rows + 300, Dn), float(SENT), dtype=torch.float32, device="cuda")
    dv = [_dev(torch, a) for a in (imgs, w, np.zeros(Dn, np.float32), pos, cls, reg)]
    pc, pr = (dv[4].data_ptr() if with_cls else 0), (dv[5].data_ptr() if R else 0)
    if rect:
        binding.op_patch_embed_rect(dtype, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), pc, pr, R, X.data_ptr(), n, Hh, Ww, P, 3, Dn)
    else:
        binding.op_patch_embed(dtype, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), pc, pr, R, X.data_ptr(), n, Hh, P, 3, Dn)
    torch.cuda.synchronize()
    return X.cpu().numpy()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("P", [16, 14])
@pytest.mark.parametrize("grid", [(1, 7), (7, 1), (5, 9), (9, 5)])
def test_patch_embed_rect_is_exact_bit_for_bit(binding, torch_gpu, grid, P, dtype):
    """n = 3 (5 x 9: 135 patch rows, a 128-row tile ends inside the third image), patch 16 (the 16-float gather) and 14 (the per-element gather), with 0
    and 4 register rows, with a class row and without one.  Every row of X is the numpy result bit for bit and the rows behind the last token keep
    the sentinel."""
    gh, gw = grid
    for R, with_cls in ((0, True), (4, True), (0, False)):
        imgs, w, pos, cls, reg, want = _exact_case(P, gh, gw, 3, R, with_cls)
        x = _run_embed(binding, torch_gpu, dtype, imgs, w, pos, cls, reg, R, with_cls, P, want.shape[0])
        what = (grid, P, dtype, R, with_cls)
        assert (x[want.shape[0]:] == SENT).all(), (what, "rows behind the last token row were written")
        got = x[:want.shape[0]]
        assert np.array_equal(_bits(got), _bits(want)), (what, np.argwhere(_bits(got) != _bits(want))[:5].tolist())


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("P", [16, 14])
def test_patch_embed_rect_on_a_square_is_the_square_entry_point(binding, torch_gpu, P, dtype):
    """Grid (4, 4): vitx_op_patch_embed_rect and vitx_op_patch_embed give the same bits, on the exact data and on random data."""
    imgs, w, pos, cls, reg, want = _exact_case(P, 4, 4, 3, 4, True)
    rng = np.random.default_rng(P + dtype)
    cases = [(imgs, w, pos, cls, reg), (PD.exact_images(3, 4 * P, seed=P), (rng.standard_normal(w.shape) * 0.05).astype(np.float32),
                                        (rng.standard_normal(pos.shape) * 0.5).astype(np.float32), rng.standard_normal(cls.shape).astype(np.float32),
                                        rng.standard_normal(reg.shape).astype(np.float32))]
    for i, (a, ww, pp, cc, rr) in enumerate(cases):
        r = _run_embed(binding, torch_gpu, dtype, a, ww, pp, cc, rr, 4, True, P, want.shape[0], rect=True)
        s = _run_embed(binding, torch_gpu, dtype, a, ww, pp, cc, rr, 4, True, P, want.shape[0], rect=False)
        assert np.array_equal(_bits(r), _bits(s)), (P, dtype, i)
        if i == 0:
            assert np.array_equal(_bits(r[:want.shape[0]]), _bits(want))


# ------------------------------------------------------------------------------------------------ 2. the forward against the restatement
@functools.lru_cache(maxsize=None)
def _images(h, w, n=17):
    return XD.images(n, h, w)


_REF, _T = {}, {}


def _tensors(pkg, kind):
    if kind not in _T:
        _T[kind] = PD.file_tensors(pkg, XD.fixture_file(pkg, kind))
    return _T[kind]


def _ref(pkg, binding, kind, shape, dtype, mutant=None, n=17):
    """The restatement of the images of a (fixture, shape), once per (operand type, mutant)."""
    key = (kind, shape, dtype, mutant, n)
    if key not in _REF:
        _REF[key] = R64.forward64(_tensors(pkg, kind), _images(*shape, n), XD.HEADS, mutant=mutant, wround=ROUND[dtype], uround=ROUND[dtype], binding=binding)
    return _REF[key]


def _geometry(t, shape):
    P = t["patch_embed.proj.weight"].shape[-1]
    gh, gw = shape[0] // P, shape[1] // P
    T = 1 + (t["reg_token"].shape[1] if "reg_token" in t else 0)
    return gh, gw, T, gh * gw + T


@pytest.mark.parametrize("all_rows", [0, 1])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind,shape", XD.CASES, ids=[f"{k}-{h}x{w}" for k, (h, w) in XD.CASES])
def test_forward_against_the_restatement_and_every_mutant(pkg, binding, torch_gpu, kind, shape, mode, all_rows):
    """Batch 17 (two sub-batch streams) and batch 3: probabilities and the trace layer by layer inside the gates of the rounded restatement, every
    mutant of rect_data outside them."""
    dtype = MODES[mode]
    t = _tensors(pkg, kind)
    gh, gw, T, N = _geometry(t, shape)
    ref = _ref(pkg, binding, kind, shape, dtype)
    imgs = _images(*shape)
    model = binding.Model(XD.fixture_file(pkg, kind))
    ctx = binding.Context(model, device=0, max_batch=17, dtype=dtype, img_shape=shape, last_layer_all_rows=all_rows)
    assert (ctx.tokens, ctx.img_shape, ctx.grid_hw, ctx.img_size) == (N, shape, (gh, gw), 0) and len(ctx.split(17)) == 2
    p17, p3 = ctx.forward(imgs), ctx.forward(imgs[:3])
    for n, p in ((17, p17), (3, p3)):
        d = float(np.abs(p - ref["probs"][:n]).max())
        print(f"{kind} {shape} {mode} all_rows {all_rows} batch {n}: max|dprob| {d:.3e} (gate {PROB_TOL[dtype]})")
        assert np.isfinite(p).all() and d <= PROB_TOL[dtype], (n, d)
    assert np.array_equal(_bits(p17[:3]), _bits(p3))
    ids = ctx.boundary_rows(17)
    ctx.trace_enable(ids)
    p = ctx.forward(imgs)
    x = ctx.trace_read()
    assert x.shape == (L + 1, len(ids), N, D)
    _check_trace(x, ref["trace"][:, ids], dtype, f"{kind} {shape} {mode} all_rows {all_rows}")
    assert np.abs(p - ref["probs"]).max() <= PROB_TOL[dtype]
    for mut in XD.mutants_of(t):
        assert _outside(x, p, _ref(pkg, binding, kind, shape, dtype, mut), dtype, ids), (kind, shape, mode, mut)
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 3. square equivalence
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("S", [56, 84])
def test_square_rect_context_is_the_square_context_bit_for_bit(pkg, binding, torch_gpu, S, dtype):
    """create_rect(S, S) against create_ex(img_size = S) at the file's own size and at 84: probabilities, logits, trace, features and class-token maps
    have the same bits, the graph cache replays as often, and the weight set is shared."""
    n = 3
    imgs = PD.exact_images(n, S, seed=S)
    model = binding.Model(XD.fixture_file(pkg, "p14r4"))
    got = {}
    ctxs = []
    for label, kw in (("ex", dict(img_size=S)), ("rect", dict(img_shape=(S, S)))):
        ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, graph=1, **kw)
        ctxs.append(ctx)
        assert (ctx.img_size, ctx.img_shape, ctx.grid_hw, ctx.tokens) == (S, (S, S), (S // 14, S // 14), (S // 14) ** 2 + 5)
        plain = [ctx.forward(imgs, want_logits=True) for _ in range(4)]
        for pr in plain[1:]:
            assert np.array_equal(_bits(pr[0]), _bits(plain[0][0])) and np.array_equal(_bits(pr[1]), _bits(plain[0][1]))
        launches = ctx.graph_launches()
        ctx.trace_enable(list(range(n))); ctx.attn_enable(None, rollout=True); ctx.feat_enable(cls=True, mean=True, tokens=True)
        p, lg = ctx.forward(imgs, want_logits=True)
        cls, roll = ctx.attn_read()
        f = ctx.feat_read(n)[L - 1]
        got[label] = (plain[0][0], plain[0][1], p, lg, ctx.trace_read(), cls, roll, f["cls"], f["mean"], f["tokens"], launches)
    assert ctxs[1].shares_weights()
    for a, b in zip(got["ex"][:-1], got["rect"][:-1]):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
    assert got["ex"][-1] == got["rect"][-1] and got["ex"][-1] >= 1
    for c in ctxs:
        c.close()
    model.close()


# ------------------------------------------------------------------------------------------------ 4. the persistent attention band
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", [(192, 272), (16, 3104)])
def test_token_counts_of_the_persistent_attention_band(pkg, binding, torch_gpu, shape, mode):
    """The patch-16 fixture at 192 x 272 (a 12 x 17 grid: 205 tokens, inside 193 .. 224) and at 16 x 3104 (194 patches in ONE row: 195 tokens), batch
    3, against the restatement inside the gates."""
    dtype, n = MODES[mode], 3
    t = _tensors(pkg, "p16")
    gh, gw, T, N = _geometry(t, shape)
    assert N in (205, 195)
    ref = _ref(pkg, binding, "p16", shape, dtype, n=n)
    model = binding.Model(XD.fixture_file(pkg, "p16"))
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, img_shape=shape)
    assert (ctx.tokens, ctx.grid_hw) == (N, (gh, gw))
    ctx.trace_enable(list(range(n)))
    p = ctx.forward(_images(*shape, n))
    x = ctx.trace_read()
    _check_trace(x, ref["trace"], dtype, f"p16 {shape} {mode}")
    d = float(np.abs(p - ref["probs"]).max())
    print(f"p16 {shape} {mode}: max|dprob| {d:.3e} (gate {PROB_TOL[dtype]})")
    assert d <= PROB_TOL[dtype]
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 5. batch invariance
@pytest.mark.parametrize("dtype", [0, 1])
def test_batch_invariance_and_graph_replay(pkg, binding, torch_gpu, dtype):
    """Image 11 of 17 has the bits it has alone (probabilities and features), and a hipGraph replay gives the bits of the plain forward."""
    kind, shape = "p14r4", (28, 70)
    imgs = _images(*shape)
    model = binding.Model(XD.fixture_file(pkg, kind))
    ctx = binding.Context(model, device=0, max_batch=17, dtype=dtype, img_shape=shape)
    ctx.feat_enable(cls=True, mean=True, tokens=True)
    p17 = ctx.forward(imgs); f17 = ctx.feat_read(17)[L - 1]
    p1 = ctx.forward(imgs[11:12]); f1 = ctx.feat_read(1)[L - 1]
    assert np.array_equal(_bits(p17[11:12]), _bits(p1))
    for k in ("cls", "mean", "tokens"):
        assert np.array_equal(_bits(f17[k][11:12]), _bits(f1[k])), k
    ctx.close()
    off = binding.Context(model, device=0, max_batch=2, dtype=dtype, img_shape=shape)
    want = off.forward(imgs[:2]); off.close()
    g = binding.Context(model, device=0, max_batch=2, dtype=dtype, img_shape=shape, graph=1)
    for _ in range(4):
        assert np.array_equal(_bits(g.forward(imgs[:2])), _bits(want))
    assert g.graph_launches() >= 1
    assert np.array_equal(_bits(want), _bits(p17[:2]))
    g.close(); model.close()


# ------------------------------------------------------------------------------------------------ 6. outputs
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", ["p14r4", "p14rope"])
def test_token_features_and_class_token_maps(pkg, binding, torch_gpu, kind, mode):
    """VITX_FEAT_TOKENS has gh gw rows in raster order: the float64 final norm of the context's own last stream (feature_data.features64), and within
    the stage gate's form of the restatement's `final` -- which the transposed order is not.  Class-token maps against prefix_data.cls_maps64 of the
    restatement's q and k built from the context's own stream, under the bounds of tests/test_gpu_rope.py.  The grid helper returns [gh, gw]."""
    dtype, n, shape = MODES[mode], 3, (28, 70)
    t = _tensors(pkg, kind)
    gh, gw, T, N = _geometry(t, shape)
    ref = _ref(pkg, binding, kind, shape, dtype)
    model = binding.Model(XD.fixture_file(pkg, kind))
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, img_shape=shape)
    ctx.trace_enable(list(range(n))); ctx.attn_enable(None, rollout=True); ctx.feat_enable(cls=True, tokens=True)
    ctx.forward(_images(*shape)[:n])
    cls, roll = ctx.attn_read()
    trace = ctx.trace_read()
    f = ctx.feat_read(n)[L - 1]
    assert cls.shape == (n, L, H, N) and roll.shape == (n, N) and f["tokens"].shape == (n, gh * gw, D)
    assert np.abs(cls.sum(-1) - 1).max() <= 1e-5 and np.abs(roll.sum(-1) - 1).max() <= 1e-4
    assert ctx.attn_grid(cls).shape == (n, L, H, gh, gw) and np.array_equal(ctx.attn_grid(roll)[:, 1, 2], roll[:, T + gw + 2])
    _, eps, _ = AD.arch_of(t)
    y64, bound = FD.features64(trace[L], t["norm.weight"], t["norm.bias"], eps)
    assert (np.abs(f["cls"] - y64[:, 0]) <= bound[:, 0]).all() and (np.abs(f["tokens"] - y64[:, T:]) <= bound[:, T:]).all()
    want = ref["final"][:n, T:]
    rms = float(np.sqrt((want ** 2).mean()))
    scale = 2.5e-2                                    # the stage gates' form on the final norm's rows: F16 max|d| <= 2.5e-2 rms, bf16 rms(d) <= 2.5e-2 rms
    err = (lambda a: float(np.abs(a - want).max())) if dtype == 0 else (lambda a: float(np.sqrt(((a - want) ** 2).mean())))
    transposed = f["tokens"].reshape(n, gh, gw, D).transpose(0, 2, 1, 3).reshape(n, gh * gw, D)
    print(f"{kind} {mode}: tokens against the restatement's final {err(f['tokens']) / rms:.3e} of the rms (gate {scale}); in transposed order {err(transposed) / rms:.3e}")
    assert err(f["tokens"]) <= scale * rms and err(transposed) > 2 * scale * rms
    two_planes = mode == "f16_parity"
    tol = 2e-3 if two_planes else 3e-2
    rnd = ROUND[dtype]
    hd = D // H
    cos, sin = RD.table64(RD.rope_of(t), hd, gh, gw) if "rope" in t else (np.ones((gh * gw, hd // 2)), np.zeros((gh * gw, hd // 2)))
    for l in range(L):
        q, k, _ = R64.qk64(t, trace[l], l, H, cos, sin, None, wround=rnd, uround=rnd)
        if not two_planes:
            q, k = rnd(q).astype(np.float64), rnd(k).astype(np.float64)
        m = PD.cls_maps64(q, k)
        worst = float((np.abs(cls[:, l] - m).max(axis=-1) / m.max(axis=-1)).max())
        print(f"{kind} {mode} layer {l}: worst map err / row max {worst:.3e} (tol {tol})")
        assert worst <= tol, (l, worst)
    ctx.close(); model.close()


def test_rollout_at_eleven_tokens(pkg, binding, torch_gpu):
    """28 x 42 on the patch-14 fixture with 4 registers: a 2 x 3 grid, N = 11."""
    model = binding.Model(XD.fixture_file(pkg, "p14r4"))
    ctx = binding.Context(model, device=0, max_batch=3, dtype=binding.F16, img_shape=(28, 42))
    assert (ctx.tokens, ctx.grid_hw) == (11, (2, 3))
    ctx.attn_enable(None, rollout=True)
    p = ctx.forward(XD.images(3, 28, 42))
    cls, roll = ctx.attn_read()
    assert cls.shape == (3, L, H, 11) and roll.shape == (3, 11) and np.isfinite(p).all()
    assert np.abs(cls.sum(-1) - 1).max() <= 1e-5 and np.abs(roll.sum(-1) - 1).max() <= 1e-4 and (roll >= 0).all()
    assert ctx.attn_grid(roll).shape == (3, 2, 3)
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 7. preprocessing
@pytest.mark.parametrize("fname", list(PPD.FILTERS))
@pytest.mark.parametrize("g", [(50, 37, 48, 32), (37, 50, 32, 48), (500, 375, 288, 224)], ids=PPD.geo_id)
def test_preprocess_rect_device_equals_the_host_bit_for_bit(binding, torch_gpu, g, fname):
    torch = torch_gpu
    nx, ny, ow, oh = g
    n = 3
    mean, std = PPD.mean_std255(PPD.IMAGENET)
    pp = PPD.make_pp(binding, dict(resize_mode=PPD.PP_STRETCH, resize_a=16, resize_b=16, filter=PPD.FILTERS[fname], crop=0, crop_round=0), mean, std)
    src = np.stack([PPD.image("random" if i != 1 else "checker", nx, ny, seed=i) for i in range(n)])
    want = np.stack([binding.preprocess_rect(a, pp, ow, oh) for a in src])
    assert binding.preprocess_rect_device_supports(pp, nx, ny, ow, oh)
    d_src = torch.from_numpy(src).cuda()
    d_out = torch.full((n * oh * ow * 3 + 64,), float(SENT), dtype=torch.float32, device="cuda")
    binding.preprocess_rect_device(pp, d_src.data_ptr(), n, nx, ny, ow, oh, d_out.data_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[n * oh * ow * 3:] == SENT).all()
    assert np.array_equal(_bits(out[:n * oh * ow * 3].reshape(n, oh, ow, 3)), _bits(want))


def test_preprocess_rect_device_beyond_the_lds_bound(binding, torch_gpu):
    """_supports and the launch agree: a down-scale whose tile does not fit the LDS is VITX_ERR_UNSUPPORTED and nothing is written."""
    torch = torch_gpu
    pp = binding.Preproc.make(resize_a=16, resize_b=16, filter=PPD.PP_PIL_BICUBIC)
    nx, ny, ow, oh = 40000, 4, 8, 16
    assert not binding.preprocess_rect_device_supports(pp, nx, ny, ow, oh)
    d_src = torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.full((oh * ow * 3,), float(SENT), dtype=torch.float32, device="cuda")
    with pytest.raises(binding.VitxError) as ei:
        binding.preprocess_rect_device(pp, d_src.data_ptr(), 1, nx, ny, ow, oh, d_out.data_ptr())
    assert ei.value.code == binding.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d_out == float(SENT)).all())
    assert binding.preprocess_rect(np.zeros((ny, nx, 3), np.uint8), pp, ow, oh).shape == (oh, ow, 3)      # the host path has no bound


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(pkg, binding, torch_gpu):
    model = binding.Model(XD.fixture_file(pkg, "p16"))
    for shape in ((40, 64), (64, 40), (0, 64), (64, 0), (-16, 64)):
        with pytest.raises(binding.VitxError) as ei:
            binding.Context(model, device=0, max_batch=1, img_shape=shape)
        assert ei.value.code == binding.ERR_ARG, shape
    with pytest.raises(ValueError, match="img_shape and img_size"):
        binding.Context(model, device=0, max_batch=1, img_shape=(48, 80), img_size=64)
    Lb = binding.lib()
    opt = binding.CtxOptions(img_size=64); opt.struct_size = 48
    h = C.c_void_p()
    assert Lb.vitx_ctx_create_rect(model._h, 0, 1, binding.F16, C.byref(opt), 48, 80, C.byref(h)) == binding.ERR_ARG
    ctx = binding.Context(model, device=0, max_batch=2, img_shape=(48, 80))
    for bad in (np.zeros((2, 80, 48, 3), np.float32), np.zeros((2, 64, 64, 3), np.float32), np.zeros((2, 48, 80), np.float32)):
        with pytest.raises(ValueError, match="48, 80, 3"):
            ctx.forward(bad)
    assert ctx.forward(np.zeros((2, 48, 80, 3), np.float32)).shape == (2, 10)
    ctx.close(); model.close()
    vitstr = binding.Model(pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0))
    for shape in ((224, 448), (448, 224), (384, 384)):
        with pytest.raises(binding.VitxError, match="unsupported"):
            binding.Context(vitstr, device=0, max_batch=1, img_shape=shape)
    ok = binding.Context(vitstr, device=0, max_batch=1, img_shape=(224, 224))
    assert ok.img_size == 224
    ok.close(); vitstr.close()
    import map_data as MD
    mp = binding.Model(MD.fixture_file(pkg))
    own = mp.img_size
    with pytest.raises(binding.VitxError, match="unsupported"):
        binding.Context(mp, device=0, max_batch=1, img_shape=(own, 2 * own))
    ok = binding.Context(mp, device=0, max_batch=1, img_shape=(own, own))
    ok.close(); mp.close()
    with pytest.raises(binding.VitxError) as ei:
        binding.preprocess_rect(PPD.image("random", 20, 10), binding.Preproc.make(resize_a=16, resize_b=16, filter=PPD.PP_REF_BICUBIC), 12, 8)
    assert ei.value.code == binding.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 9. end to end
def test_cli_img_fit_equals_the_binding_path(pkg, binding, torch_gpu, tmp_path):
    """vit_cli.py --img-fit 64 on tench.jpg: the token features it writes are the binding's -- rect_shape, preprocess_rect (a file without a `preproc`
    tensor: Pillow bicubic, the default mean / std), a rect context -- bit for bit, and --attn-map writes an img_w x img_h picture."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = XD.fixture_file(pkg, "p16")
    img = os.path.join(root, "tests", "golden", "assets", "tench.jpg")
    emb, pgm = tmp_path / "e.npy", tmp_path / "map.pgm"
    r = subprocess.run([sys.executable, os.path.join(root, "vit_cli.py"), "-m", src, "-i", img, "--img-fit", "64", "--embed", str(emb), "--embed-kind", "tokens",
                        "--attn-map", str(pgm)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    from vitcpp_amd import cli
    u8 = cli._decode(img)
    w, h = binding.rect_shape(u8.shape[1], u8.shape[0], 16, 64)
    assert min(w, h) == 64 and max(w, h) > 64 and w % 16 == 0 and h % 16 == 0 and f"({w} x {h})" in r.stderr
    model = binding.Model(src)
    pp = model.preproc()
    assert not model.has_preproc
    pp.filter = binding.PP_PIL_BICUBIC
    ctx = binding.Context(model, device=0, max_batch=1, dtype=binding.F16, img_shape=(h, w))
    ctx.feat_enable(cls=False, tokens=True)
    p = ctx.forward(binding.preprocess_rect(u8, pp, w, h)[None])
    want = ctx.feat_read(1)[L - 1]["tokens"]
    got = np.load(emb)
    assert got.shape == want.shape == (1, (h // 16) * (w // 16), D) and np.array_equal(_bits(got), _bits(want))
    idx, val = binding.topk(p[0], 5)
    assert r.stdout == "".join(f" > {model.label(i)} : {v:.2f}\n" for i, v in zip(idx, val))
    head = f"P5\n{w} {h}\n255\n".encode()
    assert pgm.read_bytes().startswith(head) and len(pgm.read_bytes()) == len(head) + w * h
    ctx.close(); model.close()
    both = subprocess.run([sys.executable, os.path.join(root, "vit_cli.py"), "-m", src, "-i", img, "--img-fit", "64", "--img-shape", "64x80"], capture_output=True, text=True, timeout=300)
    assert both.returncode == 2 and "give one" in both.stderr
    bad = subprocess.run([sys.executable, os.path.join(root, "vit_cli.py"), "-m", src, "-i", img, "--img-shape", "64x72"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "patch size" in bad.stderr


def test_cpp_example_embed_main_at_an_img_shape(pkg, binding, torch_gpu, tmp_path):
    """examples/embed_main.cpp --img-shape through vit.cpp_amd/vit.h (vit_state::img_h, img_w; vit_image_preprocess_rect): the embedding it writes is
    the binding's."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkgdir = os.path.join(root, "vit.cpp_amd")
    exe = str(tmp_path / "embed_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(root, "examples", "embed_main.cpp"), "-I" + pkgdir, "-L" + pkgdir, "-lvitx", "-L/opt/rocm/lib",
                        "-Wl,-rpath," + pkgdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assets = os.path.join(root, "tests", "golden", "assets")
    a, b = os.path.join(assets, "tench.jpg"), os.path.join(assets, "kiwi.jpg")
    path = XD.fixture_file(pkg, "p16")
    out = tmp_path / "emb.bin"
    r = subprocess.run([exe, path, a, b, "--img-shape", "48x80", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "embedding: 128 floats per image" in r.stdout
    model = binding.Model(path)
    pp = model.preproc(); pp.filter = binding.PP_PIL_BICUBIC
    ctx = binding.Context(model, device=0, max_batch=2, dtype=binding.F16, img_shape=(48, 80))
    ctx.feat_enable(cls=True, l2=True)
    ctx.forward(np.stack([binding.preprocess_rect(binding.load_image(f), pp, 80, 48) for f in (a, b)]))
    want = ctx.feat_read(2)[L - 1]["cls"][0]
    ctx.close(); model.close()
    assert np.array_equal(_bits(np.fromfile(out, np.float32)), _bits(want))
    for args in (["--img-shape", "48x72"], ["--img-shape", "48x80", "--img-size", "96"], ["--img-shape", "48"]):
        r = subprocess.run([exe, path, a, b] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0, args
