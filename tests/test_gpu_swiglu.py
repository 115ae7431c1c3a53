"""The gated (SwiGLU) MLP on the GPU (include/vitx.h "gated MLP"): vitx_op_swiglu against float64 on an exact grid and on hostile values, with
sentinels around everything it may not touch; and the forward of the two micro fixtures of tests/swiglu_data.py (F = 320: N = 17 without registers,
N = 21 with four and `rope`) against the float64 restatement that tests/test_cpu_swiglu.py pins to transformers, under the gates of
tests/test_gpu_arch.py -- with every mutant of swiglu_data.MUTANTS outside them."""
import ctypes as C
import functools

import numpy as np
import pytest

import arch_data as AD
import feature_data as FD
import prefix_data as PD
import ref64 as R64
import rope_data as RD
import swiglu_data as SD
from ref64 import PROB_TOL
from test_gpu_arch import ROUND, _check_trace, _outside

pytestmark = pytest.mark.gpu

D, L, H, S, F = 128, 2, 2, 56, SD.F
TOKENS = {"g": (17, 1), "hplus": (21, 5)}          # (N, T) of the two fixtures
ERR_ARG, ERR_UNSUPPORTED = 3, 5
SENT = {0: 0x4700, 1: 0x40E0}                       # 7.0 in fp16 and in bf16: the sentinel of every cell a launch may not touch
CANARY = 2                                          # rows behind the last one
SHAPES = [(1, 8), (5, 72), (300, 320)]              # one thread; rows that share a workgroup; more than one workgroup, the fixtures' width
MODES = {"bf16": (1, {}), "f16_parity": (0, {}), "f16_fast": (0, {"f16_fast_attention": 1})}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _launch(binding, torch, dtype, g, u, pad=8):
    """One vitx_op_swiglu launch on g, u [rows][Fw] (float64 values the operand type holds): the input rows are [gate | up | pad] with ld_in =
    2 Fw + pad, the output rows [Fw | pad] with ld_out = Fw + pad, CANARY rows behind both, every other cell the sentinel.  Returns (values
    [rows][Fw] float64, the whole output buffer's bits, the input buffer's bits before and after)."""
    rows, Fw = g.shape
    ld_in, ld_out = 2 * Fw + pad, Fw + pad
    src = np.full((rows + CANARY, ld_in), SENT[dtype], np.uint16)
    src[:rows, :Fw] = RD.to_bits16(g, dtype); src[:rows, Fw:2 * Fw] = RD.to_bits16(u, dtype)
    d_in = torch.from_numpy(src.view(np.int16)).cuda()
    d_out = torch.full((rows + CANARY, ld_out), SENT[dtype], dtype=torch.int16, device="cuda")
    binding.op_swiglu(dtype, d_in.data_ptr(), ld_in, d_out.data_ptr(), ld_out, rows, Fw)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint16)
    return RD.from_bits16(out[:rows, :Fw], dtype).astype(np.float64), out, src, d_in.cpu().numpy().view(np.uint16)


def _untouched(out, src, after, rows, Fw, dtype, what):
    assert (out[:rows, Fw:] == SENT[dtype]).all(), (what, "padding columns of the output")
    assert (out[rows:] == SENT[dtype]).all(), (what, "canary rows of the output")
    assert np.array_equal(src, after), (what, "the input")


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("rows,Fw", SHAPES)
@pytest.mark.parametrize("dtype", [0, 1])
def test_op_swiglu_against_float64_on_the_exact_grid(binding, torch_gpu, dtype, rows, Fw):
    """g on arch_data.grid() as the operand type holds it, u from swiglu_data.U_VALUES cycled per column: every stored element within
    arch_data.act_tol (one ulp of the output type + 1e-6) of silu64(g) u; the padding columns (ld_in = 2 F + 8, ld_out = F + 8), the two canary
    rows behind both buffers and the input keep their bits.  At the widest shape every mutant a launch could make is outside the bound somewhere."""
    g, u = SD.grid_operands(rows, Fw, dtype)
    got, out, src, after = _launch(binding, torch_gpu, dtype, g, u)
    want = SD.swiglu64(np.concatenate([g, u], 1), Fw)
    err = np.abs(got - want) / AD.act_tol(want, dtype)
    print(f"dtype {dtype} rows {rows} F {Fw}: worst |err| / act_tol {float(err.max()):.3f}")
    assert np.isfinite(got).all() and (err <= 1.0).all(), (dtype, rows, Fw, float(err.max()))
    _untouched(out, src, after, rows, Fw, dtype, (dtype, rows, Fw))
    if Fw == 320:
        for mut in SD.OP_MUTANTS:
            wm = SD.swiglu64(np.concatenate([g, u], 1), Fw, mut)
            share = float((np.abs(got - wm) > AD.act_tol(wm, dtype)).mean())
            assert share > 0.5, (mut, share)


@pytest.mark.parametrize("dtype", [0, 1])
def test_hostile_values_stay_finite_and_inside_the_bound(binding, torch_gpu, dtype):
    """g in {+-0, +-2^-20, +-88, +-89, +-104, +- the type's largest finite} with u in {1, -1}: exp(-g) overflows f32 from g = -89 on and underflows
    from g = 104 on.  No NaN, no inf, the same bound; a large negative g gives a zero, a large positive g gives g u."""
    big = 65504.0 if dtype == 0 else float(np.float32(3.3895313892515355e38))
    vals = np.array([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, big, -big])
    g = np.stack([vals, vals, vals[::-1], vals[::-1]]).reshape(3, 16)
    u = np.stack([np.ones(12), -np.ones(12), np.ones(12), -np.ones(12)]).reshape(3, 16)
    assert np.array_equal(RD.from_bits16(RD.to_bits16(g, dtype), dtype).astype(np.float64), g)
    got, out, src, after = _launch(binding, torch_gpu, dtype, g, u)
    want = SD.silu64(g) * u
    assert np.isfinite(want).all()
    assert np.isfinite(got).all(), got
    err = np.abs(got - want) / AD.act_tol(want, dtype)
    print(f"dtype {dtype}: hostile values: worst |err| / act_tol {float(err.max()):.3f}")
    assert (err <= 1.0).all(), (got, want)
    assert (got[g <= -89.0] == 0).all() and np.array_equal(got[g >= 104.0], (g * u)[g >= 104.0])
    _untouched(out, src, after, 3, 16, dtype, "hostile")


@pytest.mark.parametrize("dtype", [0, 1])
def test_rows_do_not_depend_on_the_launch(binding, torch_gpu, dtype):
    """Rows 100 .. 199 run alone give the bits they have inside the 300-row launch (one writer per element, nothing shared)."""
    rng = np.random.default_rng(300 + dtype)
    g = RD.from_bits16(RD.to_bits16(rng.standard_normal((300, 320)) * 3.0, dtype), dtype).astype(np.float64)
    u = RD.from_bits16(RD.to_bits16(rng.standard_normal((300, 320)) * 2.0, dtype), dtype).astype(np.float64)
    _, all_rows, _, _ = _launch(binding, torch_gpu, dtype, g, u)
    _, part, _, _ = _launch(binding, torch_gpu, dtype, g[100:200], u[100:200])
    assert np.array_equal(all_rows[100:200, :320], part[:100, :320])
    want = SD.silu64(g) * u
    assert (np.abs(RD.from_bits16(all_rows[:300, :320], dtype) - want) <= AD.act_tol(want, dtype)).all()


def test_bad_op_arguments_are_refused_before_any_launch(binding, torch_gpu):
    torch = torch_gpu
    Lb = binding.lib()
    rows, Fw = 4, 16
    src = torch.full((rows, 2 * Fw + 8), 0x3C00, dtype=torch.int16, device="cuda")
    out = torch.full((rows + 1, Fw + 8), SENT[0], dtype=torch.int16, device="cuda")
    i, o = src.data_ptr(), out.data_ptr()
    call = lambda dtype=0, i=i, ld_in=2 * Fw + 8, o=o, ld_out=Fw + 8, rows=rows, Fw=Fw: Lb.vitx_op_swiglu(dtype, i, ld_in, o, ld_out, rows, Fw, None)
    bad = {"F % 8": call(Fw=12), "in off a 16-byte boundary": call(i=i + 2), "in off by 8 bytes": call(i=i + 8), "out off a 16-byte boundary": call(o=o + 2),
           "ld_in % 8": call(ld_in=2 * Fw + 4), "ld_out % 8": call(ld_out=Fw + 4), "ld_in < 2 F": call(ld_in=2 * Fw - 8), "ld_out < F": call(ld_out=Fw - 8),
           "NULL in": call(i=None), "NULL out": call(o=None), "rows 0": call(rows=0), "F 0": call(Fw=0), "dtype 2": call(dtype=2), "dtype -1": call(dtype=-1)}
    assert all(rc == ERR_ARG for rc in bad.values()), bad
    assert "vitx_op_swiglu" in Lb.vitx_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == SENT[0]).all()), "a refused call wrote to the output"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[:rows, :Fw] != SENT[0]).all()) and bool((out[:rows, Fw:] == SENT[0]).all()) and bool((out[rows:] == SENT[0]).all())


# ------------------------------------------------------------------------------------------------ end to end on the micro fixtures
@functools.lru_cache(maxsize=None)
def _images():
    return PD.exact_images(17, S, seed=1)


_REF = {}


def _ref(pkg, kind, dtype, mutant=None):
    """The restatement of all 17 images, once per (fixture, operand type, mutant)."""
    key = (kind, dtype, mutant)
    if key not in _REF:
        t = PD.file_tensors(pkg, SD.fixture_file(pkg, kind))
        _REF[key] = (t, R64.forward64(t, _images(), H, mutant=mutant, wround=ROUND[dtype], uround=ROUND[dtype]))
    return _REF[key]


@pytest.mark.parametrize("all_rows", [0, 1])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", SD.FIXTURES)
def test_forward_against_the_restatement_and_every_mutant(pkg, binding, torch_gpu, kind, mode, all_rows):
    """Batch 17 (two sub-batch streams) and batch 3: probabilities and the trace layer by layer inside the gates of the rounded restatement, every
    mutant outside them, image 0 alone bit-identical to image 0 of the batch, and one `swiglu` launch per layer and sub-batch in the profile."""
    dtype, opts = MODES[mode]
    N, T = TOKENS[kind]
    t, ref = _ref(pkg, kind, dtype)
    imgs = _images()
    model = binding.Model(SD.fixture_file(pkg, kind))
    assert model.glu == (1, F)
    ctx = binding.Context(model, device=0, max_batch=17, dtype=dtype, last_layer_all_rows=all_rows, **opts)
    assert (ctx.tokens, ctx.registers, ctx.grid) == (N, T - 1, 4) and len(ctx.split(17)) == 2
    p17 = ctx.forward(imgs)
    p3, p1 = ctx.forward(imgs[:3]), ctx.forward(imgs[:1])
    for n, p in ((17, p17), (3, p3)):
        d = float(np.abs(p - ref["probs"][:n]).max())
        print(f"{kind} {mode} all_rows {all_rows} batch {n}: max|dprob| {d:.3e} (gate {PROB_TOL[dtype]})")
        assert np.isfinite(p).all() and d <= PROB_TOL[dtype], (n, d)
    assert np.array_equal(_bits(p17[:3]), _bits(p3)) and np.array_equal(_bits(p3[:1]), _bits(p1))
    ctx.profile_enable(True)
    ctx.forward(imgs)
    prof = {e["name"]: e for e in ctx.profile_read()}
    ctx.profile_enable(False)
    tail = "attention_cls" in prof                                      # the class-rows-only last layer: never with the cls + mean head of fixture g
    assert tail == (not all_rows and kind == "hplus")
    rows = (L - 1) * 17 * N + (17 if tail else 17 * N)
    assert prof["swiglu"]["launches"] == 2 * L and prof["swiglu"]["bytes"] == rows * 3 * F * 2
    ids = ctx.boundary_rows(17)
    ctx.trace_enable(ids)
    p = ctx.forward(imgs)
    x = ctx.trace_read()
    assert x.shape == (L + 1, len(ids), N, D)
    _check_trace(x, ref["trace"][:, ids], dtype, f"{kind} {mode} all_rows {all_rows}")
    assert np.abs(p - ref["probs"]).max() <= PROB_TOL[dtype]
    for mut in SD.MUTANTS:
        _, m = _ref(pkg, kind, dtype, mut)
        assert _outside(x, p, m, dtype, ids), (kind, mode, mut)
    ctx.close(); model.close()


def test_a_file_without_glu_launches_nothing_new(pkg, binding, torch_gpu):
    model = binding.Model(AD.fixture_file(pkg, "dinov2_erf"))
    assert model.glu is None
    ctx = binding.Context(model, device=0, max_batch=3, dtype=1)
    ctx.profile_enable(True)
    ctx.forward(_images()[:3])
    assert "swiglu" not in {e["name"] for e in ctx.profile_read()}
    ctx.close(); model.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_features_of_the_hplus_fixture(pkg, binding, torch_gpu, mode):
    """cls, mean and tokens of the last layer: against the float64 final norm of the context's own last residual stream under the bounds of
    tests/test_gpu_arch.py::test_features_of_the_erf_file, and against the restatement's final norm under the stage gate's form (F16: max|d| <=
    2.5e-2 rms; BF16: rms(d) <= 2.5e-2 rms)."""
    dtype, opts = MODES[mode]
    n, (N, T) = 3, TOKENS["hplus"]
    t, ref = _ref(pkg, "hplus", dtype)
    _, eps, _ = AD.arch_of(t)
    model = binding.Model(SD.fixture_file(pkg, "hplus"))
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, **opts)
    ctx.feat_enable(cls=True, mean=True, tokens=True)
    ctx.trace_enable(list(range(n)))
    ctx.forward(_images()[:n])
    f = ctx.feat_read(n)[L - 1]
    x_last = ctx.trace_read()[L]
    ctx.close(); model.close()
    y64, bound = FD.features64(x_last, t["norm.weight"], t["norm.bias"], eps)
    assert (np.abs(f["cls"] - y64[:, 0]) <= bound[:, 0]).all() and (np.abs(f["tokens"] - y64[:, T:]) <= bound[:, T:]).all()
    m64, mb = FD.mean_bound(f["tokens"])
    assert (np.abs(f["mean"] - m64) <= mb).all()
    want = ref["final"][:n]
    rms = float(np.sqrt((want ** 2).mean()))
    for name, got, w in (("cls", f["cls"], want[:, 0]), ("mean", f["mean"], ref["mean"][:n]), ("tokens", f["tokens"], want[:, T:])):
        e_max, e_rms = float(np.abs(got - w).max()) / rms, float(np.sqrt(((got - w) ** 2).mean())) / rms
        print(f"hplus {mode} {name}: max|d| / rms {e_max:.3e}, rms(d) / rms {e_rms:.3e}")
        assert (e_max <= 2.5e-2) if dtype == 0 else (e_rms <= 2.5e-2), (name, e_max, e_rms)


@pytest.mark.parametrize("kind", SD.FIXTURES)
def test_q8_0_file_matches_the_restatement_on_dequantised_weights(pkg, binding, torch_gpu, tmp_path, kind):
    q8 = str(tmp_path / "q8.gguf")
    binding.quantize_file(SD.fixture_file(pkg, kind), q8, 8)
    t = PD.file_tensors(pkg, q8)
    assert SD.glu_of(t) == F
    imgs = _images()[:3]
    ref = R64.forward64(t, imgs, H, wround=PD.f16_round, uround=PD.f16_round)
    swapped = R64.forward64(t, imgs, H, mutant="gate_up_swapped", wround=PD.f16_round, uround=PD.f16_round)
    model = binding.Model(q8)
    assert model.glu == (1, F)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=0)
    p = ctx.forward(imgs)
    ctx.close(); model.close()
    d = float(np.abs(p - ref["probs"]).max())
    print(f"{kind} q8_0: max|dprob| {d:.3e}; the swapped restatement is {float(np.abs(swapped['probs'] - ref['probs']).max()):.3e} away")
    assert d <= 1e-3 and (p.argmax(1) == ref["probs"].argmax(1)).all()          # tests/test_gpu_registers.py:303
    assert np.abs(p - swapped["probs"]).max() > 1e-3


@pytest.mark.parametrize("kind", SD.FIXTURES)
def test_graph_replay_gives_the_same_bits(pkg, binding, torch_gpu, kind):
    """The gate is an ordinary launch: captured into the hipGraph cache with the rest (batch 2, single stream)."""
    imgs = _images()[:2]
    model = binding.Model(SD.fixture_file(pkg, kind))
    for dtype in (binding.BF16, binding.F16):
        off = binding.Context(model, device=0, max_batch=2, dtype=dtype)
        want = off.forward(imgs); off.close()
        g = binding.Context(model, device=0, max_batch=2, dtype=dtype, graph=1)
        for _ in range(4):
            assert np.array_equal(_bits(g.forward(imgs)), _bits(want))
        assert g.graph_launches() >= 1
        g.close()
    model.close()


def test_context_at_another_image_size(pkg, binding, torch_gpu):
    """Fixture g at img_size 84 from the 56 file: 37 tokens, the position table resampled on the device -- against the restatement on the host's
    resampled table (tests/test_gpu_arch.py::test_clip_file_at_another_image_size)."""
    dtype, n = 0, 3
    path = SD.fixture_file(pkg, "g")
    t = PD.file_tensors(pkg, path)
    imgs = PD.exact_images(n, 84, seed=84)
    pos = binding.pos_embed_resample(t["pos_embed"][0], 6, binding.POS_BICUBIC)
    ref = R64.forward64(t, imgs, H, pos=pos, wround=ROUND[dtype], uround=ROUND[dtype])
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, img_size=84)
    assert (ctx.tokens, ctx.grid) == (37, 6)
    ctx.trace_enable(list(range(n)))
    p = ctx.forward(imgs)
    x = ctx.trace_read()
    ctx.close(); model.close()
    _check_trace(x, ref["trace"], dtype, "fixture g at img_size 84")
    assert np.abs(p - ref["probs"]).max() <= PROB_TOL[dtype]
    wrong = R64.forward64(t, imgs, H, pos=pos, mutant="gate_up_swapped", wround=ROUND[dtype], uround=ROUND[dtype])
    assert _outside(x, p, wrong, dtype, list(range(n)))


def test_mxfp8_and_one_channel_files_are_refused_at_context_creation(pkg, binding, torch_gpu, tmp_path):
    """Files that VITX_MXFP8 / a ViTSTR context would take (tanh-GELU, no registers, class-token head) but for their `glu` tensor."""
    Lb = binding.lib()
    h = C.c_void_p()
    hp = pkg.synth.hparams_for(SD.MICRO)
    plain, gated = str(tmp_path / "plain.gguf"), str(tmp_path / "glu.gguf")
    pkg.ggml_file.write_model(plain, hp, pkg.synth.make_weights(hp, head_scale=4.0))
    pkg.ggml_file.write_model(gated, hp, pkg.synth.make_weights(hp, head_scale=4.0, glu=F))
    m = binding.Model(plain)
    assert Lb.vitx_ctx_create(m._h, 0, 1, binding.MXFP8, C.byref(h)) == 0
    Lb.vitx_ctx_free(h); m.close()
    m = binding.Model(gated)
    assert m.glu == (1, F)
    assert Lb.vitx_ctx_create(m._h, 0, 1, binding.MXFP8, C.byref(h)) == ERR_UNSUPPORTED
    assert "gated MLP" in Lb.vitx_last_error().decode() and "MXFP8" in Lb.vitx_last_error().decode()
    with pytest.raises(binding.VitxError) as ei:
        binding.Context(m, device=0, max_batch=1, dtype=binding.MXFP8)
    assert ei.value.code == binding.ERR_UNSUPPORTED
    ok = binding.Context(m, device=0, max_batch=1, dtype=binding.BF16)          # the same file in an operand type that has the gate
    ok.close(); m.close()
    name = "vitstr_tiny_patch16_224"
    hp1 = pkg.synth.hparams_for(name)
    one = str(tmp_path / "one.gguf")
    pkg.ggml_file.write_model(one, hp1, pkg.synth.make_weights(hp1, in_chans=1, glu=F), id2label=dict(pkg.synth.VITSTR_LABELS))
    m = binding.Model(one)
    assert m.in_channels == 1 and m.glu == (1, F)
    assert Lb.vitx_ctx_create(m._h, 0, 1, binding.F16, C.byref(h)) == ERR_UNSUPPORTED
    assert "ViTSTR" in Lb.vitx_last_error().decode() and "gated MLP" in Lb.vitx_last_error().decode()
    m.close()


@pytest.mark.parametrize("family", ["dinov2_giant", "dinov3_hplus"])
def test_converted_models_give_transformers_pooler_output(pkg, binding, torch_gpu, tmp_path, family):
    """The two tiny transformers models of tests/test_cpu_swiglu.py through convert.py (gated_mlp=True) at ftype 1 and a VITX_F16 context:
    VITX_FEAT_CLS is transformers' f32 pooler_output, VITX_FEAT_TOKENS its patch rows of last_hidden_state.  The bound is that of
    tests/test_gpu_rope.py::test_converted_dinov3_model_gives_transformers_pooler_output: 2.5e-2 of the rms of the final norm's rows;
    tests/test_cpu_swiglu.py shows every mutant further than 0.1 from the model on features of this size."""
    import torch
    from test_cpu_swiglu import _hf_dinov2_giant, _hf_dinov3_hplus
    _, m = _hf_dinov2_giant() if family == "dinov2_giant" else _hf_dinov3_hplus()
    T, width = (1, 512) if family == "dinov2_giant" else (5, 320)
    path = str(tmp_path / "gated.gguf")
    pkg.convert.convert_hf_model(m, path, ftype=1, no_head=True, gated_mlp=True)
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(3, S, seed=3))
    with torch.no_grad():
        out = m(pixel_values=torch.from_numpy(imgs).permute(0, 3, 1, 2).contiguous())
    want_cls, want_tok = out.pooler_output.numpy(), out.last_hidden_state.numpy()[:, T:]
    model = binding.Model(path)
    assert model.glu == (1, width)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=binding.F16)
    ctx.feat_enable(cls=True, tokens=True)
    ctx.forward(imgs)
    f = ctx.feat_read(3)[L - 1]
    ctx.close(); model.close()
    rms = float(np.sqrt((want_tok ** 2).mean()))
    d_cls, d_tok = float(np.abs(f["cls"] - want_cls).max()), float(np.abs(f["tokens"] - want_tok).max())
    print(f"converted {family}, F16: max|cls - pooler_output| {d_cls:.3e}, max|tokens - last_hidden_state| {d_tok:.3e} (rms {rms:.3f}, gate {2.5e-2 * rms:.3e})")
    assert d_cls <= 2.5e-2 * rms and d_tok <= 2.5e-2 * rms
