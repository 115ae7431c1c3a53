"""Activation, LayerNorm epsilon and pre-norm on the GPU (include/vitx.h "activation, epsilon and pre-norm"): the two new fc1 epilogues on every
GEMM family, the f32 LayerNorm, and the forward of the three model classes (HuggingFace ViT: erf-GELU, eps 1e-12; DINOv2: erf-GELU, cls + mean
head; CLIP: QuickGELU, eps 1e-5, pre-norm) against the float64 restatement of tests/ref64.py, which tests/test_cpu_arch.py pins to transformers.

What pins each activation.  The exact epilogue tests: their inputs make acc + bias an exact fp16 number on the grid x = k / 64 (+ 1 / 128 on odd rows),
the bound is one ulp of the output type + 1e-6, and tests/test_cpu_arch.py shows that the float64 references themselves lie more than two such
bounds apart on hundreds of grid points.  End to end, QuickGELU against tanh-GELU is visible in the F16 trace of the CLIP fixture (asserted); erf
against tanh drowns in operand rounding on every fixture (max |tanh - erf| = 4.7e-4 per element), and so does QuickGELU under the BF16 gates: those
mutants are asserted only where the restatements themselves lie more than twice the gate apart, which is computed, printed and, on these fixtures,
not the case.  The eps mutant (a file with eps 1e-2 against the restatement with 1e-6) is visible everywhere and asserted in both operand types."""
import ctypes as C
import functools

import numpy as np
import pytest

import arch_data as AD
import feature_data as FD
import prefix_data as PD
import ref64 as R64
from ref64 import PROB_TOL, stage_errors, stage_ok

pytestmark = pytest.mark.gpu

D, L, H, P, S = 128, 2, 2, 14, 56
ROUND = {0: PD.f16_round, 1: PD.bf16_round}
KERNELS = [1, 945, 445, 245, 122, 0, 2]            # tests/test_gpu_parity_r02.py KERNELS: vitx_op_gemm_ex kernel ids
ERR_UNSUPPORTED = 5
F16_ULP, BF16_ULP = 2.0 ** -10, 2.0 ** -7
SENT = 7.0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tdt(torch, dtype):
    return torch.float16 if dtype == 0 else torch.bfloat16


# ------------------------------------------------------------------------------------------------ (a), (b): the epilogues on exact data
def _exact_operands(torch, dtype, M, N, n_pad, K, stride=1):
    """A[m][0] = (m & 1) / 128, W[n][0] = 1, everything else 0; bias[n] = (stride n mod 1024 - 512) / 64: acc + bias = bias[n] + a_m exactly, an fp16
    number (so F16's argument rounding is the identity).  Returns A, W [n_pad][K], bias [n_pad], the q4_0 planes of the same W, and v [2][N] f64."""
    tdt = _tdt(torch, dtype)
    A = torch.zeros((M, K), dtype=tdt, device="cuda"); A[1::2, 0] = 1.0 / 128
    W = torch.zeros((n_pad, K), dtype=tdt, device="cuda"); W[:N, 0] = 1.0
    b = np.zeros(n_pad, np.float32); b[:N] = ((np.arange(N) * stride) % 1024 - 512) / 64.0
    # q4_0: value = (nibble - 8) * d.  d = 1, every nibble 8 (zero) but element 0 of block 0 (the low nibble of byte 0): 9
    qs = np.full((n_pad, K // 32, 16), 0x88, np.uint8); qs[:N, 0, 0] = 0x89
    ds = np.ones((n_pad, K // 32), np.float16)
    v = np.stack([b[:N].astype(np.float64), b[:N].astype(np.float64) + 1.0 / 128])
    return A, W, _dev(torch, b), _dev(torch, qs), _dev(torch, ds.view(np.int16)), v


def _run_epilogue(binding, torch, dtype, epi, kernel, ops, M, M_real, N, K):
    """One launch into a sentinel-filled [M][N] output; kernel "q4" = vitx_op_gemm_q4.  None when the family cannot tile the shape."""
    A, W, bias, qs, ds, _ = ops
    out = torch.full((M, N), SENT, dtype=_tdt(torch, dtype), device="cuda")
    Lb = binding.lib()
    if kernel == "q4":
        rc = Lb.vitx_op_gemm_q4(dtype, epi, A.data_ptr(), qs.data_ptr(), ds.data_ptr(), bias.data_ptr(), out.data_ptr(), M, M_real, N, K, None)
    else:
        rc = Lb.vitx_op_gemm_ex(dtype, epi, kernel, A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), None, M, M_real, N, K, 0, None)
    if rc == ERR_UNSUPPORTED:
        return None
    binding.check(rc, f"epi {epi} kernel {kernel}")
    torch.cuda.synchronize()
    return out


def _check_exact(torch, out, v, act, dtype, M_real, what):
    """|got - act64(v)| <= ulp_T(act64(v)) + 1e-6 on every stored element; rows >= M_real keep the sentinel.  Returns the worst error / tolerance."""
    want = AD.act64(v, act)                                   # [2][N]: even rows, odd rows
    tol = AD.act_tol(want, dtype)
    assert bool((out[M_real:] == SENT).all()), what + ": rows past M_real were written"
    worst = 0.0
    for par in (0, 1):
        ratio = (out[par:M_real:2].double() - _dev(torch, want[par])).abs() / _dev(torch, tol[par])
        col = ratio.max(dim=0).values.cpu().numpy()
        worst = max(worst, float(col.max()))
        assert col.max() <= 1.0, (what, par, float(col.max()), float(v[par][col.argmax()]))
    return worst


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("act", [AD.ACT_ERF, AD.ACT_QUICK])
def test_activation_epilogues_are_exact_on_every_gemm_family(binding, torch_gpu, act, dtype):
    """M = 8192 (128 tiles of 256 x 256: the ping-pong kernel is the automatic choice), the last 100 rows not stored, N = 1024, K = 128: the staged
    whole-line epilogue of every family and the q4_0 kernel.  Every family must also give the same bits."""
    torch = torch_gpu
    M, N, K = 8192, 1024, 128
    M_real = M - 100
    ops = _exact_operands(torch, dtype, M, N, N, K)
    first = None
    for kernel in KERNELS + ["q4"]:
        out = _run_epilogue(binding, torch, dtype, AD.EPI[act], kernel, ops, M, M_real, N, K)
        assert out is not None, f"kernel {kernel} refused M {M} N {N} K {K}"
        worst = _check_exact(torch, out, ops[5], act, dtype, M_real, f"{AD.ACT_NAMES[act]} dtype {dtype} kernel {kernel}")
        print(f"{AD.ACT_NAMES[act]} dtype {dtype} kernel {kernel}: worst err / tol {worst:.3f}")
        if first is None:
            first = out
        else:
            assert torch.equal(out.view(torch.int16), first.view(torch.int16)), f"kernel {kernel} and kernel {KERNELS[0]} differ in bits"
    # the tanh epilogue on the same data is NOT within this activation's bound: the test's inputs tell the activations apart
    tanh = _run_epilogue(binding, torch, dtype, AD.EPI[AD.ACT_TANH], 0, ops, M, M_real, N, K).double().cpu().numpy()
    want = AD.act64(ops[5], act)
    far = np.abs(tanh[0:2] - want) > AD.act_tol(want, dtype)
    print(f"{AD.ACT_NAMES[act]} dtype {dtype}: the tanh epilogue is outside the bound on {int(far.sum())} of {far.size} grid points")
    assert far.sum() >= (150 if act == AD.ACT_ERF else 500)


@pytest.mark.parametrize("stride", [1, 5])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("act", [AD.ACT_ERF, AD.ACT_QUICK])
def test_activation_epilogues_on_ragged_tiles(binding, torch_gpu, act, dtype, stride):
    """M = 256 with 130 rows stored, N = 192 (W and bias padded to 256 rows), K = 64: the tiles that hold row 130 or column 192 are not full and take the per-element edge
    epilogue, on every family that tiles the shape.  stride 1: the data of the test above (bias -8 .. -5); stride 5: the same grid spread over -8 .. 7."""
    torch = torch_gpu
    M, M_real, N, K = 256, 130, 192, 64
    ops = _exact_operands(torch, dtype, M, N, 256, K, stride)
    ran, first = [], None
    for kernel in KERNELS + ["q4"]:
        out = _run_epilogue(binding, torch, dtype, AD.EPI[act], kernel, ops, M, M_real, N, K)
        if out is None:
            continue
        ran.append(kernel)
        worst = _check_exact(torch, out, ops[5], act, dtype, M_real, f"ragged {AD.ACT_NAMES[act]} dtype {dtype} kernel {kernel}")
        print(f"ragged {AD.ACT_NAMES[act]} dtype {dtype} stride {stride} kernel {kernel}: worst err / tol {worst:.3f}")
        if first is None:
            first = out
        else:
            assert torch.equal(out.view(torch.int16), first.view(torch.int16)), f"kernel {kernel} and kernel {ran[0]} differ in bits"
    assert {445, 245, 122, 0, "q4"} <= set(ran), ran


def _act64_t(torch, v, act):
    if act == AD.ACT_ERF:
        q = 0.5 * torch.special.erfc(v.abs() / 2.0 ** 0.5)
        return torch.where(v < 0, v * q, v * (1.0 - q))
    return v / (1.0 + torch.exp(-1.702 * v))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("act", [AD.ACT_ERF, AD.ACT_QUICK])
def test_activation_epilogues_on_random_operands(binding, torch_gpu, act, dtype):
    """M = 8192, N = 1024, K = 256, the automatic kernel: the tolerance of the tanh epilogue (tests/test_gpu_parity_r02.py:60, :91) with the matching
    float64 activation, on every element."""
    torch = torch_gpu
    M, N, K = 8192, 1024, 256
    tdt, ulp = _tdt(torch, dtype), (F16_ULP if dtype == 0 else BF16_ULP)
    g = torch.Generator(device="cuda").manual_seed(77 + act)
    A = (torch.randn((M, K), device="cuda", generator=g) * 0.7).to(tdt)
    W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(tdt)
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    out = torch.full((M, N), SENT, dtype=tdt, device="cuda")
    binding.check(binding.lib().vitx_op_gemm_ex(dtype, AD.EPI[act], 0, A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), None, M, M, N, K, 0, None))
    torch.cuda.synchronize()
    v = A.double() @ W.double().T + bias.double()
    tol_acc = (A.double().abs() @ W.double().abs().T) * 2e-6 + 1e-6
    want = _act64_t(torch, v, act)
    err = (out.double() - want).abs()
    tol = tol_acc * 2 + torch.maximum(want.abs(), v.abs()) * 2 * ulp + 1e-6
    print(f"random {AD.ACT_NAMES[act]} dtype {dtype}: worst err / tol {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())
    # the torch restatement used here is arch_data.act64
    s = v[:4].cpu().numpy()
    assert np.abs(want[:4].cpu().numpy() - AD.act64(s, act)).max() <= 1e-14


def test_new_epilogues_are_refused_where_they_do_not_exist(binding, torch_gpu):
    """vitx_op_gemm takes 0..3, 6 and 7; an id past the table is an argument error."""
    torch = torch_gpu
    A = torch.zeros((128, 64), dtype=torch.float16, device="cuda"); W = torch.zeros((256, 64), dtype=torch.float16, device="cuda")
    b = torch.zeros(256, device="cuda"); out = torch.zeros((128, 256), dtype=torch.float16, device="cuda")
    Lb = binding.lib()
    for epi in (6, 7):
        assert Lb.vitx_op_gemm(0, epi, A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), 128, 256, 64, None) == 0
    torch.cuda.synchronize()
    assert not out.any()                                   # act(0) = 0 for both
    for epi in (4, 5, 8, -1):
        assert Lb.vitx_op_gemm(0, epi, A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), 128, 256, 64, None) == 3
    assert Lb.vitx_op_gemm_ex(0, 8, 0, A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), None, 128, 128, 256, 64, 0, None) == 3


# ------------------------------------------------------------------------------------------------ (d): the f32 LayerNorm
@pytest.mark.parametrize("Dn", [128, 192, 256, 768, 1024])
def test_layernorm_f32(binding, torch_gpu, Dn):
    """vitx_op_layernorm_f32 on 67 rows (17 workgroups, the last with one row): the tiled statistics (256, 768, 1024) and the flat ones (128, 192)."""
    torch = torch_gpu
    M, tail = 67, 5
    rng = np.random.default_rng(Dn)
    x = (rng.standard_normal((M + tail, Dn)) * rng.uniform(0.2, 3.0, (M + tail, 1)) + rng.uniform(-2, 2, (M + tail, 1))).astype(np.float32)
    w = (1.0 + rng.standard_normal(Dn) * 0.2).astype(np.float32); b = (rng.standard_normal(Dn) * 0.3).astype(np.float32)
    dx, dw, db = _dev(torch, x), _dev(torch, w), _dev(torch, b)
    Lb = binding.lib()
    for eps in (1e-6, 1e-5):
        y = torch.full((M + tail, Dn), SENT, device="cuda")
        binding.op_layernorm_f32(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), y.data_ptr(), M, Dn, eps)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        assert (got[M:] == SENT).all(), "rows beyond M were written"
        y64, bound = FD.features64(x[None, :M], w, b, eps)            # the bound tests/test_gpu_features.py applies to the f32 rows F
        err = np.abs(got[:M] - y64[0])
        print(f"D {Dn} eps {eps:g}: worst err / bound {float((err / bound[0]).max()):.3f}")
        assert (err <= bound[0]).all()
        for dtype in (0, 1):                                          # RNE(y) is the 16-bit LayerNorm's output, bit for bit
            y16 = torch.zeros((M, Dn), dtype=_tdt(torch, dtype), device="cuda")
            binding.check(Lb.vitx_op_layernorm(dtype, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), y16.data_ptr(), M, Dn, eps, None))
            torch.cuda.synchronize()
            assert torch.equal(y[:M].to(_tdt(torch, dtype)).view(torch.int16), y16.view(torch.int16)), (Dn, eps, dtype)
        z = dx.clone()                                                # in place
        binding.op_layernorm_f32(z.data_ptr(), dw.data_ptr(), db.data_ptr(), z.data_ptr(), M, Dn, eps)
        torch.cuda.synchronize()
        assert torch.equal(z[:M], y[:M]) and torch.equal(z[M:], dx[M:])
    # rows of one value: variance 0, y = b exactly, at both ends of the eps range the format carries
    c = torch.full((M, Dn), 1.5, device="cuda")
    for eps in (1e-12, 1e-5):
        y = torch.zeros((M, Dn), device="cuda")
        binding.op_layernorm_f32(c.data_ptr(), dw.data_ptr(), db.data_ptr(), y.data_ptr(), M, Dn, eps)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(np.broadcast_to(b, (M, Dn)))), (Dn, eps)
    # argument errors are vitx_op_layernorm's
    assert Lb.vitx_op_layernorm_f32(None, dw.data_ptr(), db.data_ptr(), c.data_ptr(), M, Dn, 1e-6, None) == 3
    assert Lb.vitx_op_layernorm_f32(c.data_ptr(), dw.data_ptr(), db.data_ptr(), c.data_ptr(), 0, Dn, 1e-6, None) == 3
    assert Lb.vitx_op_layernorm_f32(c.data_ptr(), dw.data_ptr(), db.data_ptr(), c.data_ptr(), M, Dn + 8, 1e-6, None) == ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ (e): end to end
@functools.lru_cache(maxsize=None)
def _images():
    return PD.exact_images(17, S, seed=1)


_REF = {}


def _ref(pkg, kind, dtype, **mutant):
    """The restatement of all 17 images, once per (file, operand type, mutant)."""
    key = (kind, dtype, tuple(sorted(mutant.items())))
    if key not in _REF:
        t = PD.file_tensors(pkg, AD.fixture_file(pkg, kind))
        _REF[key] = (t, R64.forward64(t, _images(), H, wround=ROUND[dtype], uround=ROUND[dtype], **mutant))
    return _REF[key]


def _check_trace(x, ref, dtype, where, stage0=True):
    if stage0:
        d0 = float(np.abs(x[0] - ref[0]).max()); g0 = 2e-5 * max(1.0, float(np.abs(ref[0]).max()))      # tests/test_gpu_registers.py:56
        print(f"{where} stage 0: max|d| {d0:.3e} (gate {g0:.3e})")
        assert d0 <= g0, (where, d0, g0)
    for il, (e_max, e_rms) in enumerate(stage_errors(x, ref), 1):
        print(f"{where} stage {il}: max|d| / rms {e_max:.3e}, rms(d) / rms {e_rms:.3e}")
        assert stage_ok(e_max, e_rms, dtype), (where, il, e_max, e_rms)


def _outside(x, p, mut, dtype, ids):
    """The GPU result (trace x of images `ids`, probabilities p of the first len(p) images) fails at least one gate against the restatement `mut`."""
    if np.abs(p - mut["probs"][:len(p)]).max() > PROB_TOL[dtype]:
        return True
    return any(not stage_ok(a, b, dtype) for a, b in stage_errors(x, mut["trace"][:, ids]))


def _apart(ref, mut, dtype):
    """The two restatements lie more than TWICE a gate apart: a result inside the gates of `ref` is then outside those of `mut`, whatever it is."""
    if np.abs(ref["probs"] - mut["probs"]).max() > 2 * PROB_TOL[dtype]:
        return True
    return any(not stage_ok(a, b, dtype, 2.0) for a, b in stage_errors(mut["trace"], ref["trace"]))


MUTANT = {"vit_erf": dict(activation=AD.ACT_TANH), "dinov2_erf": dict(activation=AD.ACT_TANH), "clip": dict(activation=AD.ACT_TANH), "eps_1e-2": dict(eps=1e-6)}


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("kind", ["vit_erf", "dinov2_erf", "clip", "eps_1e-2"])
def test_forward_of_each_model_class_against_the_restatement(pkg, binding, torch_gpu, kind, dtype):
    """Batches 1, 3 and 17 (17 runs as two sub-batch streams): probabilities, the trace layer by layer, batch independence bit for bit, and the
    mutant of the file's own setting (module docstring: which of them an end-to-end gate can see)."""
    torch = torch_gpu
    t, ref = _ref(pkg, kind, dtype)
    act, eps, pre = AD.arch_of(t)
    imgs = _images()
    model = binding.Model(AD.fixture_file(pkg, kind))
    assert (model.activation, model.has_pre_norm) == (act, pre) and _bits(model.hparams.eps) == _bits(np.float32(eps))
    ctx = binding.Context(model, device=0, max_batch=17, dtype=dtype)
    assert ctx.tokens == 17 and len(ctx.split(17)) == 2
    plain = {n: ctx.forward(imgs[:n]) for n in (1, 3, 17)}
    for n in (1, 3, 17):
        p = plain[n]
        d = float(np.abs(p - ref["probs"][:n]).max())
        print(f"{kind} dtype {dtype} batch {n}: max|dprob| {d:.3e}")
        assert np.isfinite(p).all() and np.abs(p.sum(1) - 1).max() < 1e-4
        assert d <= PROB_TOL[dtype], (n, d)
    assert np.array_equal(_bits(plain[17][:3]), _bits(plain[3])) and np.array_equal(_bits(plain[17][:1]), _bits(plain[1]))
    for i in range(17):                                                # image i alone is image i of the batch of 17, bit for bit
        assert np.array_equal(_bits(ctx.forward(imgs[i:i + 1])), _bits(plain[17][i:i + 1])), i
    traced = {}
    for n in (1, 3, 17):
        ids = list(range(n)) if n <= 3 else ctx.boundary_rows(17)
        ctx.trace_enable(ids)
        p = ctx.forward(imgs[:n])
        x = ctx.trace_read()
        assert x.shape == (L + 1, len(ids), 17, D)
        _check_trace(x, ref["trace"][:, ids], dtype, f"{kind} dtype {dtype} batch {n}", stage0=not pre)
        assert np.abs(p - ref["probs"][:n]).max() <= PROB_TOL[dtype]
        traced[n] = (ids, x, p)
    if pre:
        # stage 0 = float64 pre-norm of the patch embedding: the embedding rows come from the patch-embedding kernel itself (its bits are the
        # context's, tests/test_gpu_registers.py), the pre-norm of those f32 rows is held to the f32 LayerNorm bound of test_layernorm_f32
        ids, x, _ = traced[3]
        X = torch.zeros((3 * 17, D), dtype=torch.float32, device="cuda")
        dv = [_dev(torch, a) for a in (imgs[:3], t["patch_embed.proj.weight"].reshape(D, -1), t["patch_embed.proj.bias"].reshape(-1), t["pos_embed"][0], t["cls_token"].reshape(-1))]
        binding.op_patch_embed(dtype, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(), 0, 0, X.data_ptr(), 3, S, P, 3, D)
        emb = X.cpu().numpy().reshape(3, 17, D)
        gate = 2e-5 * max(1.0, float(np.abs(ref["embed"][:3]).max()))
        assert np.abs(emb - ref["embed"][:3]).max() <= gate                      # the rows in front of the pre-norm: the stage-0 gate of a file without one
        y64, bound = FD.features64(emb, t["pre_norm.weight"], t["pre_norm.bias"], eps)
        err = np.abs(x[0] - y64)
        print(f"{kind} dtype {dtype}: trace stage 0 against float64 pre-norm(patch embedding): worst err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        assert np.abs(x[0] - ref["embed"][:3]).max() > 100 * gate                # ... and it is not the un-normalised embedding
    # the mutant
    _, mut = _ref(pkg, kind, dtype, **MUTANT[kind])
    apart = _apart(ref, mut, dtype)
    ids, x, p = traced[17]
    outside = _outside(x, p, mut, dtype, ids)
    print(f"{kind} dtype {dtype}: mutant {MUTANT[kind]}: restatements more than twice a gate apart: {apart}; GPU result outside the mutant's gates: {outside}")
    if kind == "eps_1e-2" or (kind == "clip" and dtype == 0):
        assert apart and outside
    elif apart:
        assert outside
    ctx.close(); model.close()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("kind", ["vit_erf", "clip"])
def test_class_rows_only_last_layer(pkg, binding, torch_gpu, kind, dtype):
    """The class-rows-only last layer (fc1 of the class rows runs the model's epilogue too) against last_layer_all_rows = 1: tests/test_gpu_registers.py:237."""
    imgs = _images()
    model = binding.Model(AD.fixture_file(pkg, kind))
    res = {}
    for label, opts in (("cls", {}), ("all", {"last_layer_all_rows": 1})):
        ctx = binding.Context(model, device=0, max_batch=17, dtype=dtype, **opts)
        ctx.profile_enable(True); res[label] = ctx.forward(imgs)
        names = [p["name"] for p in ctx.profile_read()]
        assert ("attention_cls" in names) == (label == "cls"), names
        ctx.close()
    model.close()
    d = float(np.abs(res["cls"] - res["all"]).max())
    print(f"{kind} dtype {dtype}: class rows only vs every row: max|dprob| {d:.3e}")
    assert d <= (1e-3 if dtype == 0 else 6e-3)
    _, ref = _ref(pkg, kind, dtype)
    assert np.abs(res["all"] - ref["probs"]).max() <= PROB_TOL[dtype]


# ------------------------------------------------------------------------------------------------ (f): combinations, once each
def test_q8_0_erf_file_matches_the_restatement_on_dequantised_weights(pkg, binding, torch_gpu, tmp_path):
    q8 = str(tmp_path / "q8.gguf")
    binding.quantize_file(AD.fixture_file(pkg, "vit_erf"), q8, 8)
    t = PD.file_tensors(pkg, q8)
    assert AD.arch_of(t) == (AD.ACT_ERF, float(np.float32(1e-12)), False)
    imgs = _images()[:3]
    ref = R64.forward64(t, imgs, H, wround=PD.f16_round, uround=PD.f16_round)
    model = binding.Model(q8)
    assert model.activation == AD.ACT_ERF
    ctx = binding.Context(model, device=0, max_batch=3, dtype=0)
    p = ctx.forward(imgs)
    ctx.close(); model.close()
    d = float(np.abs(p - ref["probs"]).max())
    print(f"q8_0, erf: max|dprob| {d:.3e}")
    assert d <= 1e-3 and (p.argmax(1) == ref["probs"].argmax(1)).all()          # tests/test_gpu_registers.py:303


def test_clip_file_at_another_image_size(pkg, binding, torch_gpu):
    """img_size 84 from the 56 file (1.5 x): 36 patches, the pre-norm over the 37 rows of the resampled table."""
    dtype, n = 0, 3
    path = AD.fixture_file(pkg, "clip")
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
    # stage 0 here is held to the loose form of its gate: the pre-norm divides the embedding's f32 noise by the row's standard deviation
    d0 = float(np.abs(x[0] - ref["trace"][0]).max())
    print(f"img_size 84 stage 0: max|d| {d0:.3e}")
    _check_trace(x, ref["trace"], dtype, "clip at img_size 84", stage0=False)
    assert np.abs(p - ref["probs"]).max() <= PROB_TOL[dtype]
    ctx.close(); model.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_features_of_the_erf_file(pkg, binding, torch_gpu, dtype):
    """CLS | MEAN of the erf file against the restatement's final norm on the context's own last residual stream: tests/test_gpu_registers.py:177-181."""
    n, T = 3, 1
    path = AD.fixture_file(pkg, "vit_erf")
    t = PD.file_tensors(pkg, path)
    _, eps, _ = AD.arch_of(t)
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype)
    ctx.feat_enable(cls=True, mean=True, tokens=True)
    ctx.trace_enable(list(range(n)))
    ctx.forward(_images()[:n])
    f = ctx.feat_read(n)[L - 1]
    x_last = ctx.trace_read()[L]
    y64, bound = FD.features64(x_last, t["norm.weight"], t["norm.bias"], eps)
    assert (np.abs(f["cls"] - y64[:, 0]) <= bound[:, 0]).all()
    assert (np.abs(f["tokens"] - y64[:, T:]) <= bound[:, T:]).all()
    m64, mb = FD.mean_bound(f["tokens"])
    assert (np.abs(f["mean"] - m64) <= mb).all()
    assert (np.abs(f["mean"] - PD.pooled64(y64, T)) <= mb + bound[:, T:].mean(axis=1)).all()
    ctx.close(); model.close()


def test_graph_replay_of_the_clip_file_gives_the_same_bits(pkg, binding, torch_gpu):
    """The pre-norm is an ordinary launch: captured into the hipGraph cache with the rest (batch 2, single stream)."""
    imgs = _images()[:2]
    model = binding.Model(AD.fixture_file(pkg, "clip"))
    off = binding.Context(model, device=0, max_batch=2, dtype=binding.BF16)
    want = off.forward(imgs); off.close()
    g = binding.Context(model, device=0, max_batch=2, dtype=binding.BF16, graph=1)
    for _ in range(4):
        assert np.array_equal(_bits(g.forward(imgs)), _bits(want))
    assert g.graph_launches() >= 1
    g.close(); model.close()


# ------------------------------------------------------------------------------------------------ (g): refusals at context creation
def test_unsupported_combinations_are_refused_at_context_creation(pkg, binding, torch_gpu):
    Lb = binding.lib()
    h = C.c_void_p()
    for kind in ("vit_erf", "clip"):                               # VITX_MXFP8 evaluates tanh-GELU only
        model = binding.Model(AD.fixture_file(pkg, kind))
        assert Lb.vitx_ctx_create(model._h, 0, 1, binding.MXFP8, C.byref(h)) == ERR_UNSUPPORTED
        assert "MXFP8" in Lb.vitx_last_error().decode()
        with pytest.raises(binding.VitxError) as ei:
            binding.Context(model, device=0, max_batch=1, dtype=binding.MXFP8)
        assert ei.value.code == binding.ERR_UNSUPPORTED
        model.close()
    for kind in ("vitstr_erf", "vitstr_pre"):                      # a one-channel (ViTSTR) file with either extension
        model = binding.Model(AD.fixture_file(pkg, kind, name="vitstr_tiny_patch16_224", in_chans=1))
        assert model.in_channels == 1 and (model.activation != 0 or model.has_pre_norm)
        assert Lb.vitx_ctx_create(model._h, 0, 1, binding.F16, C.byref(h)) == ERR_UNSUPPORTED
        assert "ViTSTR" in Lb.vitx_last_error().decode()
        model.close()


def test_mxfp8_takes_eps_and_pre_norm_of_a_tanh_file(pkg, binding, torch_gpu):
    """eps and the pre-norm are plain arguments and launches: a tanh file with eps 1e-5 and pre_norm.* runs under VITX_MXFP8 and agrees with its
    BF16 context within the bound tests/test_gpu_mxfp8.py::test_forward_agrees_with_bf16 applies to this model size (ViT-tiny: 0.01)."""
    name, n = "vit_tiny_patch16_224", 8
    model = binding.Model(AD.fixture_file(pkg, "tanh_pre", name=name))
    assert (model.activation, model.has_pre_norm) == (0, True) and _bits(model.hparams.eps) == _bits(np.float32(1e-5))
    imgs = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, 224))
    p_mx = binding.Context(model, device=0, max_batch=n, dtype=binding.MXFP8).forward(imgs)
    p_bf = binding.Context(model, device=0, max_batch=n, dtype=binding.BF16).forward(imgs)
    dp = float(np.abs(p_mx - p_bf).max())
    print(f"tanh + eps 1e-5 + pre-norm, {name}: MXFP8 vs BF16 max|dp| = {dp:.3e}")
    assert np.isfinite(p_mx).all() and dp < 0.01
    # the pre-norm is really applied: the same tensors without it are another model
    t = PD.file_tensors(pkg, AD.fixture_file(pkg, "tanh_pre", name=name))
    assert "pre_norm.weight" in t and AD.arch_of(t)[1] == float(np.float32(1e-5))
    model.close()
