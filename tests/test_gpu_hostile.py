"""Kernels on data shaped like a trained model's activations instead of randn, against plain float64 (tests/exact_data.py).

  * LayerNorm, every path (stand-alone tiled and flat statistics at every width, LayerNorm -> MX, fused into the residual GEMM, the fix-up
    launch) on rows with outlier channels, outlier tokens, a large common offset, constant and zero (padding) rows, a vanishing variance, a
    step between the 256-column tiles, and very large and very small magnitudes.  The tolerance is
        |y - y64| <= |y64| * ulp_out + |w| * rstd64 * max|x_row| * 2^-21 + 1e-6:
    one output ulp plus the conditioning of the problem (an f32 mean carries an error of a few 2^-24 max|x|, which rstd magnifies).  It is
    pinned by an f32 emulation of the kernels' definition, which needs less than half of the middle term (test_cpu_exact_data.py), not by
    what the kernels give.  Inputs beyond 1e18 are out of scope: the f32 square of a deviation overflows.
  * the GELU epilogue over its whole domain (+-0, 2^-24 .. 60000, bf16 to 1e30) on every GEMM family;
  * attention with one dominant key and one dominant query per image (scores in the hundreds, both signs) on every family.
"""
import ctypes

import numpy as np
import pytest

import exact_data as X
import test_gpu_exact as TE

pytestmark = pytest.mark.gpu


def _hostile(torch, D, rows_per_kind=64):
    x, kind = X.hostile_matrix(D, rows_per_kind)
    w, b = X.ln_params(D)
    return torch.from_numpy(x).cuda(), kind, torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()


def _report(ratio, kind, what):
    r = ratio.amax(1).cpu().numpy()
    print("  " + what + ": " + ", ".join(f"{name} {r[kind == i].max():.2f}" for i, name in enumerate(X.ROW_KINDS)))


# ------------------------------------------------------------------------------------------------------------------
# 2a. LayerNorm, every path
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("D", X.LN_WIDTHS)
def test_layernorm_hostile_rows(binding, torch_gpu, D, dtype_name):
    """vitx_op_layernorm at every instantiated width (256 .. 1024: tiled statistics; the others: flat)."""
    torch = torch_gpu
    dt, tdt, ulp = TE._types(binding, torch, dtype_name)
    x, kind, w, b = _hostile(torch, D)
    M = x.shape[0]
    y = torch.full((M, D), float("nan"), dtype=tdt, device="cuda")
    binding.check(binding.lib().vitx_op_layernorm(dt, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, D, X.LN_EPS, None), "vitx_op_layernorm")
    torch.cuda.synchronize()
    y64, rstd, xmax = TE.ln64(torch, x, w, b)
    assert bool(torch.isfinite(y.float()).all())
    tol = y64.abs() * ulp + w.double().abs() * rstd * xmax * 2.0 ** -21 + 1e-6
    ratio = (y.double() - y64).abs() / tol
    _report(ratio, kind, f"D {D} {dtype_name} |y - y64| / bound")
    assert float(ratio.max()) <= 1.0, (D, dtype_name, X.ROW_KINDS[kind[int(ratio.amax(1).argmax())]], float(ratio.max()))


@pytest.mark.parametrize("D", [64, 192, 384, 768, 1024, 1280])
def test_layernorm_mx_hostile_rows(binding, torch_gpu, D):
    """vitx_op_layernorm_mxfp8: the decoded value against the reference encoding of the float64 LayerNorm, within one e4m3 step of the coarser
    of the two block scales (the tolerance of test_gpu_mxfp8.test_layernorm_mx_against_float64) plus the conditioning term and 1e-6."""
    torch = torch_gpu
    from vitcpp_amd import mxfp8
    x, kind, w, b = _hostile(torch, D)
    M, kp = x.shape[0], binding.mx_k_pad(D)
    dq = torch.full((M, kp), 0x55, dtype=torch.uint8, device="cuda"); ds = torch.full((M, kp // 32), 0x55, dtype=torch.uint8, device="cuda")
    binding.op_layernorm_mxfp8(x.data_ptr(), w.data_ptr(), b.data_ptr(), dq.data_ptr(), ds.data_ptr(), M, D, X.LN_EPS)
    torch.cuda.synchronize()
    y64, rstd, xmax = X.layernorm64(x.cpu().numpy(), w.cpu().numpy(), b.cpu().numpy())
    slack = X.ln_cond(w.cpu().numpy(), rstd, xmax) + 1e-6
    qg, sg = dq.cpu().numpy(), ds.cpu().numpy()
    qr, sr = mxfp8.encode(y64.astype(np.float32), kp)
    assert (qg[:, D:] == 0).all() and (sg[:, (D + 31) // 32:] == 127).all()          # padding: zero elements, scale 127
    dec, ref_dec = mxfp8.decode(qg, sg, D), mxfp8.decode(qr, sr, D)
    assert np.isfinite(dec).all()
    s_hi = np.repeat(np.maximum(sg, sr).astype(np.float64) - 127, 32, axis=1)[:, :D]
    mag = np.maximum(np.abs(dec), np.abs(ref_dec)) * np.exp2(-s_hi)
    step = np.exp2(s_hi) * np.where(mag < 2.0 ** -6, 2.0 ** -9, np.exp2(np.floor(np.log2(np.maximum(mag, 2.0 ** -6))) - 3))
    ratio = np.abs(dec - ref_dec) / (step * 1.0001 + slack)
    print(f"  D {D}: worst |decoded - reference| / (one e4m3 step + conditioning) = {ratio.max():.3f}")
    assert ratio.max() <= 1.0, (D, X.ROW_KINDS[kind[ratio.max(axis=1).argmax()]], float(ratio.max()))


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("N,K", [(256, 256), (512, 256), (768, 768), (1024, 128)])
def test_gemm_ln_hostile_residual(binding, torch_gpu, N, K, dtype_name):
    """vitx_op_gemm_ln with the hostile rows as the incoming residual and an exact integer GEMM on top: X is the f32 sum of the exact product
    and the residual (one rounding: compared bit for bit with that sum); Y within the bound of the float64 LayerNorm of that X; fused,
    forced fall-back, timed-out and stand-alone outputs bit-identical."""
    torch = torch_gpu
    dt, tdt, ulp = TE._types(binding, torch, dtype_name)
    tiles = N // 256
    M = 256 * ((128 + tiles - 1) // tiles + 2)                      # a little above the 128 tiles the fusing kernel needs
    x0, kind, lw, lb = _hostile(torch, N, rows_per_kind=M // len(X.ROW_KINDS) + 1)
    x0, kind = x0[:M].contiguous(), kind[:M]
    a, w, bias, _, _ = X.gemm_operands(M, N, K, 1, seed=N + K)
    A, W, B = torch.from_numpy(a).cuda().to(tdt), torch.from_numpy(w).cuda().to(tdt), torch.from_numpy(bias).cuda()
    v = (A.double() @ W.double().T + B.double()).float()            # exact
    want_x = v + x0                                                 # (acc + bias) + x: one f32 rounding, the kernel's order
    L = binding.lib()
    ys = []
    for test in (0, 1, 3):
        what = f"{dtype_name} N {N} K {K} test {test}"
        x = x0.clone(); y = torch.full((M, N), 9.0, dtype=tdt, device="cuda"); fb = ctypes.c_int(-1)
        binding.check(L.vitx_op_gemm_ln(dt, A.data_ptr(), W.data_ptr(), B.data_ptr(), x.data_ptr(), lw.data_ptr(), lb.data_ptr(), y.data_ptr(),
                                        M, N, K, X.LN_EPS, test, 50 if test else 200, fb, None), what)
        torch.cuda.synchronize()
        assert fb.value >= (1 if test else 0), what
        TE._same(torch, x, want_x, what + " X")
        ys.append(y)
    y2 = torch.empty_like(ys[0])
    binding.check(L.vitx_op_layernorm(dt, want_x.data_ptr(), lw.data_ptr(), lb.data_ptr(), y2.data_ptr(), M, N, X.LN_EPS, None))
    torch.cuda.synchronize()
    TE._same(torch, ys[0], y2, "fused against stand-alone")
    TE._same(torch, ys[1], y2, "forced fall-back against stand-alone")
    TE._same(torch, ys[2], y2, "timed-out peers against stand-alone")
    ratio = TE.ln_check(torch, ys[0], want_x, lw, lb, ulp, f"{dtype_name} N {N} K {K}")
    _report(ratio, kind, "|y - y64| / bound")


# ------------------------------------------------------------------------------------------------------------------
# 2b. GELU epilogue over its whole domain
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("kernel", X.KERNELS)
def test_gelu_epilogue_whole_domain(binding, torch_gpu, kernel, dtype_name):
    """A one-hot selector times a zero W plus bias[n] = v_n: epilogue 1 computes gelu(v_n) of chosen values.  Reference: float64 tanh-GELU of
    the value after the rounding the epilogue applies to its argument (F16: to fp16, as the reference's table; BF16: none).  2 ulp of
    max(|x|, |y|) + 1e-6; no NaN; the negative tail is 0 or -0, never positive."""
    torch = torch_gpu
    dt, tdt, ulp = TE._types(binding, torch, dtype_name)
    vals = X.gelu_sweep(dtype_name == "bf16")
    M, N, K = 256, vals.size, 128
    A = torch.zeros((M, K), dtype=tdt, device="cuda"); A[torch.arange(M), torch.arange(M) % K] = 1.0
    W = torch.zeros((N, K), dtype=tdt, device="cuda")
    B = torch.from_numpy(vals).cuda()
    out = torch.full((M, N), float("nan"), dtype=tdt, device="cuda")
    binding.check(binding.lib().vitx_op_gemm_ex(dt, 1, kernel, A.data_ptr(), W.data_ptr(), B.data_ptr(), out.data_ptr(), None, M, M, N, K, 0, None), f"kernel {kernel}")
    torch.cuda.synchronize()
    got = out.double()
    assert bool(torch.isfinite(got).all()), "NaN or inf"
    arg = B.to(torch.float16).double() if dtype_name == "f16" else B.double()
    want = TE._gelu64(torch, arg)
    tol = torch.maximum(want.abs(), arg.abs()) * 2 * ulp + 1e-6
    err = (got - want).abs()
    worst = int((err / tol).amax(0).argmax())
    assert bool((err <= tol).all()), f"kernel {kernel} {dtype_name}: gelu({vals[worst]!r}) = {out[0, worst].item()!r}, float64 {want[worst].item()!r}"
    TE._same(torch, out, out[:1].expand(M, N), "every row computes the same values")
    assert bool((got[:, arg < 0] <= 0).all()), "a negative argument gave a positive result"
    assert bool((got[:, arg < -20] == 0).all()), "the negative tail is not 0"


# ------------------------------------------------------------------------------------------------------------------
# 2c. attention with a dominant token
# ------------------------------------------------------------------------------------------------------------------
DOMINANT_PARAMS = [(f, dn, c) for f in X.ATTN_CASES if f != "map" for dn in ("f16", "bf16") for c in X.ATTN_CASES[f] if not (f == "precise" and dn == "bf16")]


@pytest.mark.parametrize("family,dtype_name,case", DOMINANT_PARAMS, ids=lambda p: p if isinstance(p, str) else "n%d_N%d_H%d_hd%d" % p)
def test_attention_dominant_token(binding, torch_gpu, family, dtype_name, case):
    """randn * 0.8 q, k, v with one key and one query per image scaled by 30.  Reference: float64 softmax attention of the operands the kernel
    multiplies (rounded to the operand type; the precise entry points take the f32 values).  Tolerances: those the existing test of each
    family states: f16 3e-3 max / 3e-4 mean, bf16 2.5e-2 / 2.5e-3; the class row (test_gpu_cls_tail.py) 2 ulp max / a quarter ulp mean."""
    torch = torch_gpu
    n_img, N, H, hd = case
    _, tdt, ulp = TE._types(binding, torch, dtype_name)
    qkv = X.dominant_qkv(n_img, N, H, hd, seed=N * 3 + H + hd)
    ops = qkv if family == "precise" else torch.from_numpy(qkv).to(tdt).float().numpy()
    ref = X.attention64(ops, n_img, N, H, hd)
    if family == "cls":
        ref = ref[::N]
    tmax, tmean = (2 * ulp, ulp / 4) if family == "cls" else (3e-3, 3e-4) if dtype_name == "f16" else (2.5e-2, 2.5e-3)
    for name, out in TE.attention_run(binding, torch, family, dtype_name, qkv, n_img, N, H, hd).items():
        got = out.float().cpu().numpy()
        assert np.isfinite(got).all(), (name, case)
        d = np.abs(got - ref)
        print(f"  {name} {dtype_name} {case}: max {d.max():.2e} mean {d.mean():.2e}")
        assert d.max() <= tmax and d.mean() <= tmean, (name, case, float(d.max()), float(d.mean()))
