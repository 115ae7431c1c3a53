"""Kernels checked element for element on data that leaves ONE correct result (tests/exact_data.py; conditions: test_cpu_exact_data.py).

  * GEMM (every family, epilogue and operand type; the LayerNorm-fusing and the q4_0 entry points; the patch embedding): operands are small
    integers, possibly times a power of two, so every partial sum is exact in f32 in any order.  The WHOLE output buffer -- pad rows,
    class-token slots, the lo plane, everything behind M_real -- is compared with torch.equal against a buffer built from the float64
    product (exact: every value is an integer far below 2^53) on top of the same sentinel fill.
  * attention (every family and entry point): every query is routed to one key by a score gap of at least 40, so row i of the output is
    v[p(i)] bit for bit.

Reach for these when a change touches tiling, staging, lane maps, epilogue stores or dispatch: a wrong lane, a dropped column, a stale
register or a store past M_real changes some element, and no tolerance hides it.  They say nothing about rounding behaviour on generic
data: that is what the float64 comparisons of the other files are for.
"""
import ctypes

import numpy as np
import pytest

import exact_data as X

pytestmark = pytest.mark.gpu

VITX_OK, VITX_ERR_UNSUPPORTED = 0, 5
# what a FORCED family tiles (vitx_op_gemm_ex kernel id -> M % , K % , K >=); kernels 0 and 2 (automatic) accept every shape
FAMILY_RULES = {1: (256, 128, 128), 445: (256, 64, 64), 945: (256, 64, 128), 245: (128, 64, 64), 122: (64, 64, 64)}
TPI = 50                                   # "tokens per image" of the patch epilogue: patch row m -> token row m + m / TPI + 1


def family_takes(kernel: int, M: int, K: int) -> bool:
    if kernel in (0, 2):
        return True
    mm, km, kmin = FAMILY_RULES[kernel]
    return M % mm == 0 and K % km == 0 and K >= kmin


def _types(binding, torch, dtype_name):
    return (binding.F16, torch.float16, 2.0 ** -10) if dtype_name == "f16" else (binding.BF16, torch.bfloat16, 2.0 ** -7)


def _same(torch, out, ref, what):
    """torch.equal with a message that names the first differing element."""
    if torch.equal(out, ref):
        return
    bad = (out != ref).nonzero()
    at = tuple(bad[0].tolist())
    pytest.fail(f"{what}: {bad.shape[0]} of {out.numel()} elements differ; first at {at}: got {out[at].item()!r}, want {ref[at].item()!r}")


def _gelu64(torch, x):
    return 0.5 * x * (1.0 + torch.tanh(0.79788456080286535588 * x * (1.0 + 0.044715 * x * x)))


def ln64(torch, x, w, b, eps=X.LN_EPS):
    """float64 LayerNorm on the device: (y, rstd, max|x| per row)."""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd * w.double() + b.double(), rstd, x.abs().amax(1, keepdim=True)


def ln_check(torch, y, x, w, b, ulp, what):
    """|y - y64| <= |y64| * ulp_out + |w| * rstd64 * max|x_row| * 2^-21 + 1e-6 (exact_data.ln_bound) against the float64 LayerNorm of x."""
    y64, rstd, xmax = ln64(torch, x, w, b)
    assert bool(torch.isfinite(y.float()).all()), what
    tol = y64.abs() * ulp + w.double().abs() * rstd * xmax * 2.0 ** -21 + 1e-6
    ratio = (y.double() - y64).abs() / tol
    worst = float(ratio.max())
    print(f"  {what}: worst |y - y64| / bound = {worst:.3f}")
    assert worst <= 1.0, (what, worst, int(ratio.argmax()))
    return ratio


# ------------------------------------------------------------------------------------------------------------------
# 1a. vitx_op_gemm_ex: every family, epilogue, type
# ------------------------------------------------------------------------------------------------------------------
def _gemm_case(binding, torch, dtype_name, case):
    dt, tdt, ulp = _types(binding, torch, dtype_name)
    M, M_real, N, K = case
    Np = X.round_up(N, 256)
    a, w, bias, resid, pos = X.gemm_operands(M, N, K, TPI, seed=M * 7 + M_real * 5 + N * 3 + K)
    L = binding.lib()
    idx = torch.arange(M_real, device="cuda")
    for variant, (sa, sw) in X.VARIANTS.items():
        assert X.gemm_bound(K, variant) < 2 ** 24
        A = (torch.from_numpy(a).cuda() * 2.0 ** sa).to(tdt)
        W = torch.zeros((Np, K), dtype=tdt, device="cuda"); W[:N] = (torch.from_numpy(w).cuda() * 2.0 ** sw).to(tdt)
        B = torch.zeros(Np, device="cuda"); B[:N] = torch.from_numpy(bias).cuda()
        R, P = torch.from_numpy(resid).cuda(), torch.from_numpy(pos).cuda()
        v = A.double() @ W[:N].double().T + B[:N].double()                   # exact: integers (times 2^-8) below 2^53
        v32 = v.float()
        assert torch.equal(v32.double(), v)
        for epi in X.EPILOGUES:
            if epi in (0, 1):
                init = torch.full((M, N), 7.0, dtype=tdt, device="cuda"); ref = init.clone()
                if epi == 0:
                    ref[:M_real] = v32[:M_real].to(tdt)                      # rounded once, to nearest even
            elif epi == 2:
                init = R.clone(); ref = R.clone(); ref[:M_real] = (v + R.double())[:M_real].float()
            elif epi == 3:
                init = torch.full((M, N), 7.0, device="cuda"); ref = init.clone(); ref[:M_real] = v32[:M_real]
            elif epi == 4:
                init = torch.full((M + M // TPI + 2, N), 7.0, device="cuda"); ref = init.clone()
                ref[idx + idx // TPI + 1] = (v[:M_real] + P.double()[idx % TPI + 1]).float()
            else:
                init = torch.full((2 * M, N), 7.0, dtype=tdt, device="cuda"); ref = init.clone()
                hi = v32.to(tdt); lo = ((v32 - hi.float()) * 2048.0).to(tdt)
                ref[:M_real] = hi[:M_real]; ref[M:M + M_real] = lo[:M_real]
            for kernel in X.KERNELS:
                what = f"{dtype_name} M {M} M_real {M_real} N {N} K {K} {variant} epi {epi} kernel {kernel}"
                out = init.clone()
                rc = L.vitx_op_gemm_ex(dt, epi, kernel, A.data_ptr(), W.data_ptr(), B.data_ptr(), out.data_ptr(), P.data_ptr(), M, M_real, N, K, TPI, None)
                torch.cuda.synchronize()
                if not family_takes(kernel, M, K):
                    assert rc == VITX_ERR_UNSUPPORTED, f"{what}: the family does not tile this shape, status {rc}"
                    _same(torch, out, init, what + " (refused, so nothing may be stored)")
                    continue
                assert rc == VITX_OK, f"{what}: status {rc}: {L.vitx_last_error().decode()}"
                if epi == 1:                                                 # not exact: float64 tanh-GELU of the exact v
                    want = _gelu64(torch, v[:M_real])
                    tol = torch.maximum(want.abs(), v[:M_real].abs()) * 2 * ulp + 1e-6
                    err = (out[:M_real].double() - want).abs()
                    assert bool((err <= tol).all()), f"{what}: worst {float((err / tol).max()):.2f} of the tolerance"
                    _same(torch, out[M_real:], init[M_real:], what + " rows past M_real")
                    continue
                _same(torch, out, ref, what)
                if epi == 5:
                    _same(torch, out[:M_real].float() + out[M:M + M_real].float() / 2048.0, v32[:M_real], what + " hi + lo / 2048")


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("case", X.gemm_small_cases(), ids=lambda c: "M%d_%d_N%d_K%d" % c)
def test_gemm_exact_small_shapes(binding, torch_gpu, case, dtype_name):
    """Every M_real in 1 .. 513 around the 64 / 128 / 256-row tile edges, every N from 4 to 2304 around the 64 / 256-column edges, K from one
    64-deep step to 3072: whole output buffer of every epilogue on every kernel family; a forced family refuses exactly what its tiles
    cannot cover."""
    _gemm_case(binding, torch_gpu, dtype_name, case)


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("case", X.gemm_wide_cases(), ids=lambda c: "M%d_%d_N%d_K%d" % c)
def test_gemm_exact_wide_shapes(binding, torch_gpu, case, dtype_name):
    """Tile counts on both sides of the 128-tile threshold of the wide kernels and of whole rounds of the CU count (255, 256, 257, 258, 339,
    513 tiles): a fault that sits only in the partial last round of a persistent kernel, in one raster group or in the second launch of the
    tail split is in rows a sample may not hold; here every row is compared."""
    M, M_real, N, K = case
    n_cu = torch_gpu.cuda.get_device_properties(0).multi_processor_count
    if (M, N) == (113 * 256, 768) and n_cu == 256:
        assert X.tail_split_rows(M, N, n_cu) == 85 * 256             # kernel 2 takes its two-launch path here
    _gemm_case(binding, torch_gpu, dtype_name, case)


# ------------------------------------------------------------------------------------------------------------------
# 1b. the other GEMM entry points on the same data
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("M,N,K", [(256 * 48, 768, 768), (256 * 44, 768, 3072), (256 * 33, 1024, 1024), (256 * 130, 256, 256), (256 * 67, 512, 256)])
def test_gemm_ln_exact(binding, torch_gpu, M, N, K, dtype_name):
    """vitx_op_gemm_ln: X equals the exact sum over the whole buffer; Y equals the stand-alone LayerNorm of that X bit for bit and the float64
    LayerNorm within the bound of the hostile-row tests; all-fused (test 0), forced fall-backs (1) and real time-outs (3) alike."""
    torch = torch_gpu
    dt, tdt, ulp = _types(binding, torch, dtype_name)
    a, w, bias, resid, _ = X.gemm_operands(M, N, K, 1, seed=M + N + K)
    lw, lb = (torch.from_numpy(t).cuda() for t in X.ln_params(N))
    L = binding.lib()
    for variant, (sa, sw) in X.VARIANTS.items():
        A = (torch.from_numpy(a).cuda() * 2.0 ** sa).to(tdt); W = (torch.from_numpy(w).cuda() * 2.0 ** sw).to(tdt)
        B, R = torch.from_numpy(bias).cuda(), torch.from_numpy(resid).cuda()
        want_x = (A.double() @ W.double().T + B.double() + R.double()).float()
        ys = []
        for test in (0, 1, 3):
            what = f"{dtype_name} M {M} N {N} K {K} {variant} test {test}"
            x = R.clone(); y = torch.full((M, N), 9.0, dtype=tdt, device="cuda"); fb = ctypes.c_int(-1)
            binding.check(L.vitx_op_gemm_ln(dt, A.data_ptr(), W.data_ptr(), B.data_ptr(), x.data_ptr(), lw.data_ptr(), lb.data_ptr(), y.data_ptr(),
                                            M, N, K, X.LN_EPS, test, 50 if test else 200, fb, None), what)
            torch.cuda.synchronize()
            assert fb.value >= (1 if test else 0), what              # the forced modes really leave tiles to the fix-up launch
            _same(torch, x, want_x, what + " X")
            y2 = torch.empty_like(y)
            binding.check(L.vitx_op_layernorm(dt, x.data_ptr(), lw.data_ptr(), lb.data_ptr(), y2.data_ptr(), M, N, X.LN_EPS, None))
            torch.cuda.synchronize()
            _same(torch, y, y2, what + " Y against the stand-alone LayerNorm")
            ys.append(y)
        ln_check(torch, ys[0], want_x, lw, lb, ulp, f"{dtype_name} M {M} N {N} K {K} {variant}")
        _same(torch, ys[1], ys[0], "fix-up (test 1) against fused"); _same(torch, ys[2], ys[0], "fix-up (test 3) against fused")


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("M,N,K", [(256, 576, 192), (640, 768, 768), (256, 192, 768), (128, 1000, 192), (384, 2304, 768)])
def test_gemm_q4_exact(binding, torch_gpu, M, N, K, dtype_name):
    """vitx_op_gemm_q4 on q4_0 blocks whose scale is a power of two (the dequantised weight is an exact small integer times it)."""
    torch = torch_gpu
    dt, tdt, ulp = _types(binding, torch, dtype_name)
    n_pad, M_real = X.round_up(N, 128), M - 5
    a, _, bias, resid, _ = X.gemm_operands(M, N, K, 1, seed=M + 3 * N + 5 * K)
    L = binding.lib()
    for variant, (sa, sw) in X.VARIANTS.items():
        qs, ds, wq = X.q4_0_planes(N, n_pad, K, sw, seed=N + K)
        A = (torch.from_numpy(a).cuda() * 2.0 ** sa).to(tdt)
        dq, dd = torch.from_numpy(qs).cuda(), torch.from_numpy(ds.view(np.int16)).cuda()
        B = torch.zeros(n_pad, device="cuda"); B[:N] = torch.from_numpy(bias).cuda()
        R = torch.from_numpy(resid).cuda()
        v = A.double() @ torch.from_numpy(wq).cuda().double().T + B[:N].double()
        for epi in (0, 1, 2, 3):
            what = f"{dtype_name} M {M} N {N} K {K} {variant} epi {epi}"
            init = R.clone() if epi == 2 else torch.full((M, N), 7.0, dtype=tdt if epi < 2 else torch.float32, device="cuda")
            out = init.clone()
            binding.check(L.vitx_op_gemm_q4(dt, epi, A.data_ptr(), dq.data_ptr(), dd.data_ptr(), B.data_ptr(), out.data_ptr(), M, M_real, N, K, None), what)
            torch.cuda.synchronize()
            if epi == 1:
                want = _gelu64(torch, v[:M_real])
                tol = torch.maximum(want.abs(), v[:M_real].abs()) * 2 * ulp + 1e-6
                assert bool(((out[:M_real].double() - want).abs() <= tol).all()), what
                _same(torch, out[M_real:], init[M_real:], what + " rows past M_real")
                continue
            ref = init.clone()
            ref[:M_real] = (v.float().to(tdt) if epi == 0 else (v + R.double()).float() if epi == 2 else v.float())[:M_real]
            _same(torch, out, ref, what)


# ------------------------------------------------------------------------------------------------------------------
# 1c. patch embedding (patch_embed.hip) through a context's residual-stream trace
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("P,cin,S,n", X.PATCH_CASES)
def test_patch_embed_exact(pkg, binding, torch_gpu, tmp_path, P, cin, S, n, dtype_name):
    """A synthetic file whose patch kernel, bias, class token and position embedding are small integers, images of small integers: x[0] of the
    trace is the int64 patch embedding, every row of every image.  Patch 16 and 32 with 3 channels and patch 16 with 1 channel take the
    64-byte gather, patch 8 and 14 the per-element gather; the image counts leave a ragged last 128-row tile and put one image's patch 0 on
    the last row of a tile (the lanes that hold patch 0 also write the class row).  One stream, so that the tile rows are the batch's rows,
    and the default cut into two sub-batches."""
    dt, _, _ = _types(binding, torch_gpu, dtype_name)
    G, synth = pkg.ggml_file, pkg.synth
    D = 192                                                          # 1.5 column tiles of 128: the second one is ragged
    hp = G.HParams(D, 1, 3, 96 if cin == 1 else 10, P, S)
    t = synth.make_weights(hp, in_chans=cin)
    ints = X.patch_tensors(D, P, cin, hp.n_tokens, seed=P * 10 + cin)
    assert X.patch_bound(P, cin) < 2 ** 24
    t.update(ints)
    path = str(tmp_path / "ints.gguf")
    G.write_model(path, hp, t, ftype=1, id2label=dict(synth.VITSTR_LABELS) if cin == 1 else None)
    imgs = X.patch_images(n, S, cin, seed=S + n)
    want = X.patch_embed_ref(imgs, ints, P).astype(np.float32)
    last, on_edge = X.patch_edges(hp.n_tokens - 1, n)
    assert last != 0 and on_edge
    model = binding.Model(path)
    assert model.in_channels == cin
    for opts in ({"streams": 1}, {}):
        ctx = binding.Context(model, device=0, max_batch=n, dtype=dt, **opts)
        ctx.trace_enable(list(range(n)))
        ctx.forward(imgs)
        got = ctx.trace_read()[0]
        ctx.close()
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"patch {P} channels {cin} {dtype_name} {opts}: {len(bad)} of {want.size} values differ, first at image/token/column {bad[0]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    model.close()


# ------------------------------------------------------------------------------------------------------------------
# 1d. attention as exact routing
# ------------------------------------------------------------------------------------------------------------------
ATTN_KERNEL = {"single": 1, "flow": 3, "persist": 4, "stream": 5}


def attention_run(binding, torch, family, dtype_name, qkv32, n_img, N, H, hd):
    """Runs one attention family / entry point on f32 values (rounded to the operand type on upload); returns {name: output tensor}.
    `precise` (VITX_F16 only) runs both vitx_op_attention_f32 and vitx_op_attention_planes; `cls` returns [n_img][D]."""
    dt, tdt, _ = _types(binding, torch, dtype_name)
    L, D, rows = binding.lib(), H * hd, n_img * N
    x = torch.from_numpy(np.ascontiguousarray(qkv32)).cuda()
    xq = x.to(tdt)
    nan = lambda r: torch.full((r, D), float("nan"), dtype=tdt, device="cuda")
    outs = {}
    if family in ("auto", "generic"):
        outs[family] = nan(rows)
        binding.check(L.vitx_op_attention(dt, xq.data_ptr(), outs[family].data_ptr(), n_img, N, D, H, None), family)
    elif family in ATTN_KERNEL:
        outs[family] = nan(rows)
        binding.check(L.vitx_op_attention_ex(dt, ATTN_KERNEL[family], xq.data_ptr(), outs[family].data_ptr(), n_img, N, D, H, None), family)
    elif family == "cls":
        outs[family] = nan(n_img)
        binding.check(L.vitx_op_attention_cls(dt, xq.data_ptr(), 0, outs[family].data_ptr(), n_img, N, D, H, None), family)
    elif family == "precise":
        assert dtype_name == "f16"
        outs["f32"] = nan(rows)
        binding.check(L.vitx_op_attention_f32(x.data_ptr(), outs["f32"].data_ptr(), n_img, N, D, H, None), "vitx_op_attention_f32")
        hi = x.to(torch.float16); lo = ((x - hi.float()) * 2048.0).to(torch.float16)
        pad = 8
        buf = torch.full((2 * (rows + pad), 3 * D), float("nan"), dtype=torch.float16, device="cuda")       # NaN rows behind each plane: never read
        buf[:rows] = hi; buf[rows + pad:2 * rows + pad] = lo
        outs["planes"] = nan(rows)
        binding.check(L.vitx_op_attention_planes(buf.data_ptr(), (rows + pad) * 3 * D, outs["planes"].data_ptr(), n_img, N, D, H, None), "vitx_op_attention_planes")
    else:
        raise ValueError(family)
    torch.cuda.synchronize()
    return outs


ATTN_PARAMS = [(f, dn, c) for f in X.ATTN_CASES if f != "map" for dn in ("f16", "bf16") for c in X.ATTN_CASES[f] if not (f == "precise" and dn == "bf16")]


@pytest.mark.parametrize("family,dtype_name,case", ATTN_PARAMS, ids=lambda p: p if isinstance(p, str) else "n%d_N%d_H%d_hd%d" % p)
def test_attention_routes_exactly(binding, torch_gpu, family, dtype_name, case):
    """k_j = u_j (+-1), q_i = 32 u_{p(i)}: the score of key p(i) exceeds every other score of query i by a gap of at least 40 (asserted on the
    data), so every other probability is below e^-40 and cannot move an f32 sum that holds a 1 or a v: output row i is v[p(i)] bit for bit.
    A key in the wrong slot of a staged tile, a padded key that leaks, a head or an image mix-up all move some row to another v."""
    torch = torch_gpu
    n_img, N, H, hd = case
    rows0 = family == "cls"
    qkv, perm, gap = X.routing_qkv(n_img, N, H, hd, X.attn_seed(n_img, N, H, hd), rows0_only=rows0)
    assert gap >= X.MIN_GAP, gap
    _, tdt, _ = _types(binding, torch, dtype_name)
    want = torch.from_numpy(X.routed(qkv, perm, n_img, N, H, hd)).cuda().to(tdt)
    if rows0:
        want = want[::N].contiguous()
    for name, out in attention_run(binding, torch, family, dtype_name, qkv, n_img, N, H, hd).items():
        _same(torch, out, want, f"{name} {dtype_name} {case} (gap {gap:.0f})")


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("case", X.ATTN_CASES["map"], ids=lambda c: "n%d_N%d_H%d_hd%d" % c)
def test_attention_map_of_a_routed_class_token(binding, torch_gpu, case, dtype_name):
    """vitx_op_attention_map on the same inputs: the class-token map is exactly 1.0 at p(0).  Elsewhere it is expf(s - max) of an f32 softmax,
    which keeps values down to the f32 denormals (a gap of 40 leaves 4e-18, not 0): every other entry is at most e^-gap (times 1 + 1e-5 for
    the f32 exponential), far below anything that can move the 1."""
    torch = torch_gpu
    n_img, N, H, hd = case
    dt, tdt, _ = _types(binding, torch, dtype_name)
    qkv, perm, gap = X.routing_qkv(n_img, N, H, hd, X.attn_seed(n_img, N, H, hd), rows0_only=True)
    assert gap >= X.MIN_GAP
    xq = torch.from_numpy(qkv).cuda().to(tdt)
    cls = torch.full((n_img, H, N), float("nan"), device="cuda")
    binding.op_attention_map(dt, xq.data_ptr(), cls.data_ptr(), 0, n_img, N, H * hd, H)
    torch.cuda.synchronize()
    got = cls.cpu().numpy()
    hit = np.zeros((n_img, H, N), bool)
    np.put_along_axis(hit, perm[:, :, :1], True, axis=2)
    assert (got[hit] == 1.0).all(), (case, dtype_name, got[hit])
    assert (got[~hit] >= 0).all() and got[~hit].max(initial=0.0) <= np.exp(-gap) * (1 + 1e-5), (case, dtype_name, got[~hit].max(initial=0.0))
