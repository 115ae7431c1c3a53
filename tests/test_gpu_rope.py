"""Rotary position embeddings on the GPU (include/vitx.h "rotary position embeddings"): vitx_op_rope bit for bit against the numpy-f32 restatement
of its operation order (tests/rope_data.py::rope_bits) on the three operand forms, exact tables that name a fault, batch invariance, and the
forward of the micro RoPE fixture (N = 21) against the float64 restatement that tests/test_cpu_rope.py pins to transformers' DINOv3ViTModel, under
the gates of tests/ref64.py -- with every mutant of rope_data.MUTANTS outside them."""
import ctypes as C
import functools

import numpy as np
import pytest

import feature_data as FD
import prefix_data as PD
import ref64 as R64
import rope_data as RD
from ref64 import PROB_TOL
from test_gpu_arch import ROUND, _check_trace, _outside

pytestmark = pytest.mark.gpu

D, L, H, P, S, N, T = 128, 2, 2, 14, 56, 21, 5
ERR_ARG, ERR_UNSUPPORTED = 3, 5
FORMS = ("bf16", "f16", "planes")                  # bf16; one fp16 plane (f16_fast_attention); the parity mode's two fp16 planes
CANARY = 2                                         # rows behind the last image that no launch may touch
# the forward's three operand modes: (dtype, context options, the restatement's rounding)
MODES = {"bf16": (1, {}), "f16_parity": (0, {}), "f16_fast": (0, {"f16_fast_attention": 1})}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _form_dtype(form):
    return 1 if form == "bf16" else 0


def _quiet_f32(rng, shape):
    """f32 values h + k ulp(h) / 64, h an fp16 number in [1/4, 4) with a random sign, |k| <= 15: the two-plane split of such a value is exact and no
    split lands on a rounding tie, so a rotation by the identity or by a quarter turn must give back the very same planes."""
    h = (rng.integers(1024, 2048, shape) * 2.0 ** -10 * 2.0 ** rng.integers(-2, 2, shape)).astype(np.float32)
    ulp = (2.0 ** (np.floor(np.log2(h)) - 10)).astype(np.float32)
    return ((h + rng.integers(-15, 16, shape).astype(np.float32) * ulp / 64) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _planes_of(x, form):
    """f32 [rows][3 D] -> the input plane(s) as uint16 bits."""
    if form == "planes":
        return RD.split_hilo(x)
    return RD.to_bits16(x, _form_dtype(form)), None


def _run(binding, torch, form, hi, lo, cos, sin, n_img, N_, prefix, D_, H_):
    """One vitx_op_rope launch on device copies of the plane(s) [rows][3 D] (rows >= n_img * N_); returns them as they come back."""
    rows = hi.shape[0]
    buf = np.stack([hi, lo]) if lo is not None else hi[None]
    d = torch.from_numpy(np.ascontiguousarray(buf).view(np.int16)).cuda()
    dc, ds = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (cos, sin))
    binding.op_rope(_form_dtype(form), d.data_ptr(), dc.data_ptr(), ds.data_ptr(), n_img, N_, prefix, D_, H_, lo_off=rows * 3 * D_ if lo is not None else 0)
    torch.cuda.synchronize()
    out = d.cpu().numpy().view(np.uint16)
    return out[0], (out[1] if lo is not None else None)


def _table(hd, gh, gw):
    c, s = RD.table64(100.0, hd, gh, gw)
    return c.astype(np.float32), s.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the kernel, bit for bit
@pytest.mark.parametrize("hd,heads", [(16, 3), (24, 2), (32, 2), (64, 2), (128, 1)])
@pytest.mark.parametrize("form", FORMS)
def test_op_rope_is_the_f32_restatement_bit_for_bit(binding, torch_gpu, form, hd, heads):
    """n = 3, prefix 0 / 1 / 5, grids 2 x 3, 4 x 4 and 14 x 14 (more than one workgroup), head dims on the 16-byte path (32, 64, 128: hd / 2 a multiple
    of 8) and on the scalar one (16, 24).  Every bit of the buffer is compared: q and k of the patch rows are the restatement's, and the v columns,
    the prefix rows and two canary rows behind the last image are the input's."""
    n, D_ = 3, hd * heads
    rng = np.random.default_rng(hd * 7 + heads)
    for prefix in (0, 1, 5):
        for gh, gw in ((2, 3), (4, 4), (14, 14)):
            N_ = prefix + gh * gw
            rows = n * N_ + CANARY
            x = rng.standard_normal((rows, 3 * D_)).astype(np.float32)
            hi, lo = _planes_of(x, form)
            cos, sin = _table(hd, gh, gw)
            want = RD.rope_bits(hi, cos, sin, n, N_, prefix, D_, heads, _form_dtype(form), lo)
            want_hi, want_lo = want if lo is not None else (want, None)
            got_hi, got_lo = _run(binding, torch_gpu, form, hi, lo, cos, sin, n, N_, prefix, D_, heads)
            what = (form, hd, heads, prefix, gh, gw)
            for got, w, src in ((got_hi, want_hi, hi), (got_lo, want_lo, lo)):
                if src is None:
                    continue
                assert np.array_equal(got, w), (what, int((got != w).sum()))
                g3, s3 = got[:n * N_].reshape(n, N_, 3, D_), src[:n * N_].reshape(n, N_, 3, D_)
                assert np.array_equal(g3[:, :, 2], s3[:, :, 2]), (what, "v columns")
                assert np.array_equal(g3[:, :prefix], s3[:, :prefix]), (what, "prefix rows")
                assert np.array_equal(got[n * N_:], src[n * N_:]), (what, "canary rows")
                assert (g3[:, prefix:, :2] != s3[:, prefix:, :2]).mean() > 0.5, (what, "q and k of the patch rows did not change")


@pytest.mark.parametrize("hd,heads", [(24, 2), (64, 2)])
@pytest.mark.parametrize("form", FORMS)
def test_exact_tables_name_the_fault(binding, torch_gpu, form, hd, heads):
    """cos = 1, sin = 0: the output is the input, bit for bit.  cos = 0, sin = 1: an exact (-b, a) swap of every pair.  A table that differs from the
    identity at ONE patch p changes exactly rows b N + T + p of q and k, in every image and head."""
    n, prefix, gh, gw, D_ = 3, 5, 4, 4, hd * heads
    N_, half = prefix + gh * gw, hd // 2
    rng = np.random.default_rng(hd)
    x = _quiet_f32(rng, (n * N_ + CANARY, 3 * D_))
    hi, lo = _planes_of(x, form)
    if form != "planes":
        x = RD.from_bits16(hi, _form_dtype(form))
        hi, lo = _planes_of(x, form)
    one, zero = np.ones((gh * gw, half), np.float32), np.zeros((gh * gw, half), np.float32)
    got_hi, got_lo = _run(binding, torch_gpu, form, hi, lo, one, zero, n, N_, prefix, D_, heads)
    assert np.array_equal(got_hi, hi) and (lo is None or np.array_equal(got_lo, lo)), "the identity table changed bits"
    # a quarter turn: (a, b) -> (-b, a); a sign flip is bit 15 in both types, and in both planes
    got_hi, got_lo = _run(binding, torch_gpu, form, hi, lo, zero, one, n, N_, prefix, D_, heads)
    for got, src in ((got_hi, hi), (got_lo, lo)):
        if src is None:
            continue
        g5 = got[:n * N_].reshape(n, N_, 3, heads, hd)[:, prefix:, :2]
        s5 = src[:n * N_].reshape(n, N_, 3, heads, hd)[:, prefix:, :2]
        flipped = np.where((s5[..., half:] & 0x7FFF) == 0, s5[..., half:], s5[..., half:] ^ 0x8000)      # 0 - (+0) = +0: a zero lo keeps its sign
        assert np.array_equal(g5[..., :half], flipped), "a' is not -b"
        assert np.array_equal(g5[..., half:], s5[..., :half]), "b' is not a"
    # one patch
    p = 6
    cos, sin = one.copy(), zero.copy()
    cos[p], sin[p] = _table(hd, gh, gw)[0][11], _table(hd, gh, gw)[1][11]
    got_hi, _ = _run(binding, torch_gpu, form, hi, lo, cos, sin, n, N_, prefix, D_, heads)
    changed = (got_hi != hi)[:n * N_].reshape(n, N_, 3, heads, hd)
    assert not (got_hi != hi)[n * N_:].any()
    rows = changed.any(axis=(2, 3, 4))
    want_rows = np.zeros((n, N_), bool); want_rows[:, prefix + p] = True
    assert np.array_equal(rows, want_rows), np.argwhere(rows != want_rows)
    assert changed[:, prefix + p, :2].any(axis=-1).all(), "some image, q / k or head of the patch's row did not change"
    assert not changed[:, :, 2].any()


@pytest.mark.parametrize("form", FORMS)
def test_batch_invariance(binding, torch_gpu, form):
    """Image 0 of a batch of 17 has the bits of a batch of 1 (every element has one writer: nothing depends on the grid's size)."""
    hd, heads, prefix, gh, gw = 64, 2, 5, 4, 4
    D_, N_ = hd * heads, prefix + gh * gw
    x = np.random.default_rng(17).standard_normal((17 * N_, 3 * D_)).astype(np.float32)
    hi, lo = _planes_of(x, form)
    cos, sin = _table(hd, gh, gw)
    all_hi, all_lo = _run(binding, torch_gpu, form, hi, lo, cos, sin, 17, N_, prefix, D_, heads)
    one_hi, one_lo = _run(binding, torch_gpu, form, hi[:N_], None if lo is None else lo[:N_], cos, sin, 1, N_, prefix, D_, heads)
    assert np.array_equal(all_hi[:N_], one_hi) and (lo is None or np.array_equal(all_lo[:N_], one_lo))
    assert (all_hi[N_:] != hi[N_:]).any()


def test_bad_op_arguments_are_refused_before_any_launch(binding, torch_gpu):
    torch = torch_gpu
    Lb = binding.lib()
    n, N_, prefix, D_, H_ = 2, 9, 1, 32, 2
    buf = torch.full((2, n * N_, 3 * D_), 0x3C00, dtype=torch.int16, device="cuda")
    tab = torch.zeros((2, N_ - prefix, D_ // H_ // 2), dtype=torch.float32, device="cuda")
    q, c, s, hi_elems = buf.data_ptr(), tab[0].data_ptr(), tab[1].data_ptr(), n * N_ * 3 * D_
    call = lambda dtype=0, q=q, lo=0, c=c, s=s, n=n, N=N_, prefix=prefix, D=D_, H=H_: Lb.vitx_op_rope(dtype, q, lo, c, s, n, N, prefix, D, H, None)
    bad_arg = [call(q=None), call(c=None), call(s=None), call(n=0), call(N=0), call(D=0), call(H=0), call(prefix=-1), call(prefix=N_ + 1), call(dtype=2), call(dtype=-1),
               call(dtype=1, lo=hi_elems), call(lo=hi_elems - 8), call(lo=hi_elems + 4), call(lo=-8), call(q=q + 1)]
    assert bad_arg == [ERR_ARG] * len(bad_arg), bad_arg
    assert "vitx_op_rope" in Lb.vitx_last_error().decode()
    assert call(D=30, H=4) == ERR_UNSUPPORTED and call(D=6, H=2) == ERR_UNSUPPORTED       # D no multiple of H; an odd head dim
    torch.cuda.synchronize()
    assert bool((buf == 0x3C00).all()), "a refused call wrote to the buffer"
    assert call(prefix=N_) == 0                                                          # no patch row: nothing to do, nothing written
    torch.cuda.synchronize()
    assert bool((buf == 0x3C00).all())


# ------------------------------------------------------------------------------------------------ end to end on the micro fixture
@functools.lru_cache(maxsize=None)
def _images():
    return PD.exact_images(17, S, seed=1)


_REF = {}


def _ref(pkg, dtype, mutant=None):
    """The restatement of all 17 images, once per (operand type, mutant)."""
    if (dtype, mutant) not in _REF:
        t = PD.file_tensors(pkg, RD.fixture_file(pkg))
        _REF[(dtype, mutant)] = (t, R64.forward64(t, _images(), H, mutant=mutant, wround=ROUND[dtype], uround=ROUND[dtype]))
    return _REF[(dtype, mutant)]


@pytest.mark.parametrize("all_rows", [0, 1])
@pytest.mark.parametrize("mode", list(MODES))
def test_forward_against_the_restatement_and_every_mutant(pkg, binding, torch_gpu, mode, all_rows):
    """Batch 17 (two sub-batch streams) and batch 3: probabilities and the trace layer by layer inside the gates of the rounded restatement, every
    mutant outside them, image 0 alone bit-identical to image 0 of the batch, and one `rope` launch per layer and sub-batch in the profile."""
    dtype, opts = MODES[mode]
    t, ref = _ref(pkg, dtype)
    imgs = _images()
    model = binding.Model(RD.fixture_file(pkg))
    assert model.rope == (1, RD.THETA) and model.num_registers == RD.REGISTERS
    ctx = binding.Context(model, device=0, max_batch=17, dtype=dtype, last_layer_all_rows=all_rows, **opts)
    assert (ctx.tokens, ctx.registers, ctx.grid) == (N, 4, 4) and len(ctx.split(17)) == 2
    p17 = ctx.forward(imgs)
    p3, p1 = ctx.forward(imgs[:3]), ctx.forward(imgs[:1])
    for n, p in ((17, p17), (3, p3)):
        d = float(np.abs(p - ref["probs"][:n]).max())
        print(f"{mode} all_rows {all_rows} batch {n}: max|dprob| {d:.3e} (gate {PROB_TOL[dtype]})")
        assert np.isfinite(p).all() and d <= PROB_TOL[dtype], (n, d)
    assert np.array_equal(_bits(p17[:3]), _bits(p3)) and np.array_equal(_bits(p3[:1]), _bits(p1))
    ctx.profile_enable(True)
    ctx.forward(imgs)
    prof = {e["name"]: e for e in ctx.profile_read()}
    ctx.profile_enable(False)
    assert prof["rope"]["launches"] == 2 * L and prof["rope"]["bytes"] == L * 17 * (N - T) * 2 * D * 2 * 2 * (2 if mode == "f16_parity" else 1)
    assert ("attention_cls" in prof) == (not all_rows)
    ids = ctx.boundary_rows(17)
    ctx.trace_enable(ids)
    p = ctx.forward(imgs)
    x = ctx.trace_read()
    assert x.shape == (L + 1, len(ids), N, D)
    _check_trace(x, ref["trace"][:, ids], dtype, f"{mode} all_rows {all_rows}")
    assert np.abs(p - ref["probs"]).max() <= PROB_TOL[dtype]
    for mut in RD.MUTANTS:
        _, m = _ref(pkg, dtype, mut)
        assert _outside(x, p, m, dtype, ids), (mode, mut)
    ctx.close(); model.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_features_and_class_token_maps_read_rotated_q_and_k(pkg, binding, torch_gpu, mode):
    """The class-token attention maps of both layers against prefix_data.cls_maps64 on the restatement's ROTATED q and k (built from the context's own
    stream that enters the layer), under the bounds of tests/test_gpu_registers.py::test_attention_maps_include_the_registers -- and outside them for
    the unrotated q and k.  The final features against the float64 final norm of the context's own last stream (tests/test_gpu_arch.py)."""
    dtype, opts = MODES[mode]
    n = 3
    t, _ = _ref(pkg, dtype)
    model = binding.Model(RD.fixture_file(pkg))
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, **opts)
    ctx.trace_enable(list(range(n)))
    ctx.attn_enable(None, rollout=True)
    ctx.feat_enable(cls=True, tokens=True)
    ctx.forward(_images()[:n])
    cls, roll = ctx.attn_read()
    trace = ctx.trace_read()
    f = ctx.feat_read(n)[L - 1]
    assert cls.shape == (n, L, H, N) and roll.shape == (n, N)
    assert np.abs(cls.sum(-1) - 1).max() <= 1e-5 and np.abs(roll.sum(-1) - 1).max() <= 1e-4
    two_planes = mode == "f16_parity"
    tol = 2e-3 if two_planes else 3e-2
    rnd = ROUND[dtype]
    cos, sin = RD.table64(RD.THETA, D // H, 4, 4)
    for l in range(L):
        worst = {}
        for mut in (None, "no_rope"):
            q, k, _ = R64.qk64(t, trace[l], l, H, cos, sin, mut, wround=rnd, uround=rnd)
            if not two_planes:
                q, k = rnd(q).astype(np.float64), rnd(k).astype(np.float64)
            ref = PD.cls_maps64(q, k)
            worst[mut] = float((np.abs(cls[:, l] - ref).max(axis=-1) / ref.max(axis=-1)).max())
        print(f"{mode} layer {l}: worst map err / row max {worst[None]:.3e} (tol {tol}); against unrotated q, k {worst['no_rope']:.3e}")
        assert worst[None] <= tol and worst["no_rope"] > 2 * tol, (l, worst)
    _, eps, _ = RD.AD.arch_of(t)
    y64, bound = FD.features64(trace[L], t["norm.weight"], t["norm.bias"], eps)
    assert (np.abs(f["cls"] - y64[:, 0]) <= bound[:, 0]).all() and (np.abs(f["tokens"] - y64[:, T:]) <= bound[:, T:]).all()
    ctx.close(); model.close()


def test_graph_replay_gives_the_same_bits(pkg, binding, torch_gpu):
    """The rotation is an ordinary launch: captured into the hipGraph cache with the rest (batch 2, single stream)."""
    imgs = _images()[:2]
    model = binding.Model(RD.fixture_file(pkg))
    for dtype in (binding.BF16, binding.F16):
        off = binding.Context(model, device=0, max_batch=2, dtype=dtype)
        want = off.forward(imgs); off.close()
        g = binding.Context(model, device=0, max_batch=2, dtype=dtype, graph=1)
        for _ in range(4):
            assert np.array_equal(_bits(g.forward(imgs)), _bits(want))
        assert g.graph_launches() >= 1
        g.close()
    model.close()


def test_q8_0_file_matches_the_restatement_on_dequantised_weights(pkg, binding, torch_gpu, tmp_path):
    q8 = str(tmp_path / "q8.gguf")
    binding.quantize_file(RD.fixture_file(pkg), q8, 8)
    t = PD.file_tensors(pkg, q8)
    assert RD.rope_of(t) == RD.THETA
    imgs = _images()[:3]
    ref = R64.forward64(t, imgs, H, wround=PD.f16_round, uround=PD.f16_round)
    unrotated = R64.forward64(t, imgs, H, mutant="no_rope", wround=PD.f16_round, uround=PD.f16_round)
    model = binding.Model(q8)
    assert model.rope == (1, RD.THETA)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=0)
    p = ctx.forward(imgs)
    ctx.close(); model.close()
    d = float(np.abs(p - ref["probs"]).max())
    print(f"q8_0 with rope: max|dprob| {d:.3e}; the unrotated restatement is {float(np.abs(unrotated['probs'] - ref['probs']).max()):.3e} away")
    assert d <= 1e-3 and (p.argmax(1) == ref["probs"].argmax(1)).all()          # tests/test_gpu_registers.py:303
    assert np.abs(p - unrotated["probs"]).max() > 1e-3


def test_context_at_another_image_size(pkg, binding, torch_gpu, tmp_path):
    """img_size 84 from the 56 file: 41 tokens, the table of the 6 x 6 grid -- against the restatement at that grid, and bit-identical to an ordinary
    context on the file vitx_model_resize_file writes for 84 (the resolution feature's invariant: the table is a function of the grid)."""
    dtype, n = 0, 3
    path = RD.fixture_file(pkg)
    t = PD.file_tensors(pkg, path)
    imgs = PD.exact_images(n, 84, seed=84)
    ref = R64.forward64(t, imgs, H, pos=np.zeros((37, D), np.float32), wround=ROUND[dtype], uround=ROUND[dtype])
    big = str(tmp_path / "84.gguf")
    binding.resize_file(path, big, 84, binding.POS_BICUBIC)
    got = {}
    for label, file, opts in (("ctx", path, {"img_size": 84}), ("file", big, {})):
        model = binding.Model(file)
        ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, **opts)
        assert (ctx.tokens, ctx.registers, ctx.grid) == (41, 4, 6)
        ctx.trace_enable(list(range(n)))
        p = ctx.forward(imgs)
        got[label] = (p, ctx.trace_read())
        ctx.close(); model.close()
    p, x = got["ctx"]
    _check_trace(x, ref["trace"], dtype, "rope at img_size 84")
    assert np.abs(p - ref["probs"]).max() <= PROB_TOL[dtype]
    wrong = R64.forward64(t, imgs, H, pos=np.zeros((37, D), np.float32), mutant="wrong_grid", wround=ROUND[dtype], uround=ROUND[dtype])
    assert _outside(x, p, wrong, dtype, list(range(n)))
    assert np.array_equal(_bits(p), _bits(got["file"][0])) and np.array_equal(_bits(x), _bits(got["file"][1]))


def test_mxfp8_is_refused_at_context_creation(pkg, binding, torch_gpu, tmp_path):
    """A file that VITX_MXFP8 would take (tanh-GELU, no registers, class-token head) but for its `rope` tensor."""
    hp = pkg.synth.hparams_for(RD.MICRO)
    w = pkg.synth.make_weights(hp, head_scale=4.0)
    plain, rope = str(tmp_path / "plain.gguf"), str(tmp_path / "rope.gguf")
    pkg.ggml_file.write_model(plain, hp, w)
    pkg.ggml_file.write_model(rope, hp, {"rope": np.array([1, 100, 0, 0], np.float32), **w})
    Lb = binding.lib()
    h = C.c_void_p()
    m = binding.Model(plain)
    assert Lb.vitx_ctx_create(m._h, 0, 1, binding.MXFP8, C.byref(h)) == 0
    Lb.vitx_ctx_free(h); m.close()
    m = binding.Model(rope)
    assert Lb.vitx_ctx_create(m._h, 0, 1, binding.MXFP8, C.byref(h)) == ERR_UNSUPPORTED
    assert "rotary" in Lb.vitx_last_error().decode()
    with pytest.raises(binding.VitxError) as ei:
        binding.Context(m, device=0, max_batch=1, dtype=binding.MXFP8)
    assert ei.value.code == binding.ERR_UNSUPPORTED
    ok = binding.Context(m, device=0, max_batch=1, dtype=binding.BF16)          # the same file in an operand type that rotates
    ok.close(); m.close()


def test_converted_dinov3_model_gives_transformers_pooler_output(pkg, binding, torch_gpu, tmp_path):
    """A random-init DINOv3ViTModel (tests/test_cpu_rope.py's, q and k weights times 6) through convert.py at ftype 1 and a VITX_F16 context:
    VITX_FEAT_CLS is transformers' f32 pooler_output, VITX_FEAT_TOKENS its patch rows of last_hidden_state.  The bound is the F16 stage gate's form,
    2.5e-2 of the rms, applied to the final norm's rows; tests/test_cpu_rope.py shows every mutant of the rotation further than 0.1 from the model
    on features of this size."""
    import torch
    from test_cpu_rope import _hf_dinov3
    _, m = _hf_dinov3()
    path = str(tmp_path / "dinov3.gguf")
    pkg.convert.convert_hf_model(m, path, ftype=1)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(3, S, seed=3))
    with torch.no_grad():
        out = m(pixel_values=torch.from_numpy(imgs).permute(0, 3, 1, 2).contiguous())
    want_cls, want_tok = out.pooler_output.numpy(), out.last_hidden_state.numpy()[:, T:]
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=binding.F16)
    ctx.feat_enable(cls=True, tokens=True)
    ctx.forward(imgs)
    f = ctx.feat_read(3)[L - 1]
    ctx.close(); model.close()
    rms = float(np.sqrt((want_tok ** 2).mean()))
    d_cls, d_tok = float(np.abs(f["cls"] - want_cls).max()), float(np.abs(f["tokens"] - want_tok).max())
    print(f"converted DINOv3 micro model, F16: max|cls - pooler_output| {d_cls:.3e}, max|tokens - last_hidden_state| {d_tok:.3e} (rms {rms:.3f}, gate {2.5e-2 * rms:.3e})")
    assert d_cls <= 2.5e-2 * rms and d_tok <= 2.5e-2 * rms
