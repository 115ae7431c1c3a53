"""The MXFP8 GEMM (gemm_mx8.hip), its GELU -> MX epilogue, fc1 -> fc2 on the device and LayerNorm -> MX, checked byte for byte on data that leaves
ONE correct result (tests/mx_data.py; its conditions and the mutants it tells apart: tests/test_cpu_mx_data.py).  No tolerance anywhere: whole
buffers, sentinel rows included, are compared with np.array_equal.

  a. EPI_BIAS (bf16) and EPI_BIAS_RESID (f32) on every case of mx_data.CASES: every M on a 16- / 64- / 128-row edge, ragged column tiles, N that is
     no multiple of 4 (unaligned vector stores in full tiles, the per-element path of epilogue16 in the last), one to five K steps, a wide scale
     range; three sentinel rows behind the output, two rows of NaN codes (0x7f elements, 0xff scales) behind A and its scales;
  b. EPI_BIAS_GELU on every non-wide case against the reference encoding of the one value gelu_tanh2 can return (v >= 8: v; v <= -16: -0.0);
  c. the buffers of (b), untouched, as the A operand of a second GEMM;
  d. a row's bits do not depend on M (random operands);
  e. LayerNorm -> MX is the reference encoder of vitx_op_layernorm_f32's output, every width;
  f. an epilogue the kernel does not have is refused and nothing is stored.

Reach for these when a change touches the lane map, the scale DMA, stage reuse or a producer of MX rows ("MXFP8 operand mode")."""
import numpy as np
import pytest

import exact_data as X
import mx_data as D

pytestmark = pytest.mark.gpu

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID = 0, 1, 2
VITX_ERR_ARG = 3
OUT_EXTRA, A_EXTRA = 3, 2                  # sentinel rows behind an output / NaN rows behind A
SENT16, SENT32, SENT8 = 0x5555, np.float32(-1234.5), 0x55
IDS = [D.case_id(c) for c in D.CASES]
GELU_IDS = [D.case_id(c) for c in D.GELU_CASES]


def _dev(torch, a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _same(got, want, what):
    """np.array_equal on bit patterns, with a message that names the first differing element."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    at = tuple(int(i) for i in bad[0])
    pytest.fail(f"{what}: {len(bad)} of {got.size} elements differ; first at {at}: got {got[at]!r}, want {want[at]!r}")


def _a_behind_nan_rows(torch, qa, sa):
    """A and its scales with A_EXTRA rows of NaN codes behind row M: the kernel clamps its reads to row M - 1, so they may change nothing."""
    M = qa.shape[0]
    a = np.full((M + A_EXTRA, qa.shape[1]), 0x7f, np.uint8); a[:M] = qa
    s = np.full((M + A_EXTRA, sa.shape[1]), 0xff, np.uint8); s[:M] = sa
    return _dev(torch, a), _dev(torch, s)


# ------------------------------------------------------------------------------------------------ a. bf16 and f32 outputs
@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_gemm_bias_and_residual_exact(binding, torch_gpu, case):
    torch = torch_gpu
    M, N, K, _ = case
    d = D.gemm_case(case)
    A, AS = _a_behind_nan_rows(torch, d["qa"], d["sa"])
    W, WS, B = _dev(torch, d["qw"]), _dev(torch, d["sw"]), _dev(torch, d["bias"])
    ptrs = [t.data_ptr() for t in (A, AS, W, WS, B)]
    # qkv: the float64 result rounded once, to nearest even
    want = np.full((M + OUT_EXTRA, N), SENT16, np.uint16); want[:M] = D.bf16_bits(d["ref"])
    out = torch.full((M + OUT_EXTRA, N), SENT16, dtype=torch.int16, device="cuda")
    binding.op_gemm_mxfp8(EPI_BIAS, *ptrs, out.data_ptr(), 0, M, N, K)
    torch.cuda.synchronize()
    _same(out.cpu().numpy().view(np.uint16), want, f"{D.case_id(case)} EPI_BIAS (bf16 bits)")
    # fc2: (acc + bias) + resid in f32, in place on the residual
    want = np.full((M + OUT_EXTRA, N), SENT32, np.float32); want[:M] = (d["ref"] + d["resid"].astype(np.float64)).astype(np.float32)
    init = np.full((M + OUT_EXTRA, N), SENT32, np.float32); init[:M] = d["resid"]
    out = _dev(torch, init)
    binding.op_gemm_mxfp8(EPI_BIAS_RESID, *ptrs, out.data_ptr(), 0, M, N, K)
    torch.cuda.synchronize()
    _same(out.cpu().numpy().view(np.uint32), want.view(np.uint32), f"{D.case_id(case)} EPI_BIAS_RESID (f32 bits)")


# ------------------------------------------------------------------------------------------------ b. GELU -> MX
def _run_fc1(binding, torch, case):
    """EPI_BIAS_GELU of a case into sentinel-filled buffers: (elements [M + 3][N_pad], scales [M + 3][N_pad / 32]) on the device."""
    M, N, K, _ = case
    d = D.gelu_case(case)
    A, AS = _a_behind_nan_rows(torch, d["qa"], d["sa"])
    W, WS, B = _dev(torch, d["qw"]), _dev(torch, d["sw"]), _dev(torch, d["bias"])
    npad = D.pad128(N)
    oq = torch.full((M + OUT_EXTRA, npad), SENT8, dtype=torch.uint8, device="cuda")
    os_ = torch.full((M + OUT_EXTRA, npad // 32), SENT8, dtype=torch.uint8, device="cuda")
    binding.op_gemm_mxfp8(EPI_BIAS_GELU, A.data_ptr(), AS.data_ptr(), W.data_ptr(), WS.data_ptr(), B.data_ptr(), oq.data_ptr(), os_.data_ptr(), M, N, K)
    torch.cuda.synchronize()
    return oq, os_


def _fc1_expected(case):
    M = case[0]
    d = D.gelu_case(case)
    q = np.full((M + OUT_EXTRA, d["q"].shape[1]), SENT8, np.uint8); q[:M] = d["q"]
    s = np.full((M + OUT_EXTRA, d["s"].shape[1]), SENT8, np.uint8); s[:M] = d["s"]
    return q, s


@pytest.mark.parametrize("case", D.GELU_CASES, ids=GELU_IDS)
def test_gelu_epilogue_exact(binding, torch_gpu, case):
    """Rows < M: the reference encoding, byte for byte (columns N .. N_pad zero, whole pad blocks 127, the block that holds N scaled by its
    real columns, an all-dead block 127 with elements 0x80); rows >= M keep the sentinel.  Scales first: a wrong block maximum or a scale byte
    at the wrong place shows there; then the elements."""
    oq, os_ = _run_fc1(binding, torch_gpu, case)
    q, s = _fc1_expected(case)
    _same(os_.cpu().numpy(), s, f"{D.case_id(case)} EPI_BIAS_GELU scales")
    _same(oq.cpu().numpy(), q, f"{D.case_id(case)} EPI_BIAS_GELU elements")


# ------------------------------------------------------------------------------------------------ c. fc1 -> fc2 without a host round trip
@pytest.mark.parametrize("case", D.FC2_CASES, ids=[D.case_id(c) for c in D.FC2_CASES])
def test_fc2_consumes_what_fc1_wrote(binding, torch_gpu, case):
    """The buffers fc1's epilogue wrote (elements [M + 3][N_pad], scales [M + 3][N_pad / 32], sentinel rows included) go straight into a second
    GEMM as its A operand with K = N.  Expected: the float64 product of the DECODED EXPECTED fc1 output with a fresh exact W2, which is exact
    in f32 on these cases (mx_data.fc2_operands; asserted in tests/test_cpu_mx_data.py).

    The cases are those that meet the exactness condition with the granule the e4m3 format guarantees (2^-9 times the row's smallest block
    scale): N <= 63.  With the granule the rows' actual elements have, 66 of the 76 GELU cases stay below 2^24, and on those an MI355X gave the
    float64 result on all but 5 (M15_N129_K128, M63_N200_K128, M64_N200_K384, M128_N129_K384, M128_N200_K384: 12 .. 55 elements each, e.g.
    M128_N129_K384 element (13, 0): 194773.625 for 194774.125, always below, at most 9.6e-6 of the value).  Those rows hold products 2^14 and
    more apart inside one 32-element block: the scaled MFMA does not add such a block like an f32 chain ("Lane map"), so exactness
    of every f32 partial sum is not enough there, and the test keeps to the cases the format's own granule covers."""
    torch = torch_gpu
    M, N, _, _ = case
    d = D.gelu_case(case)
    qw2, sw2, bias2, resid2, fig = d["fc2"]
    assert fig < 2.0 ** 24
    oq, os_ = _run_fc1(binding, torch, case)
    W2, WS2, B2 = _dev(torch, qw2), _dev(torch, sw2), _dev(torch, bias2)
    ref = D.gemm64(d["q"], d["s"], qw2, sw2, bias2, D.FC2_N, N, resid2)
    want = np.full((M + OUT_EXTRA, D.FC2_N), SENT32, np.float32); want[:M] = ref.astype(np.float32)
    assert np.array_equal(want[:M].astype(np.float64), ref)
    init = np.full((M + OUT_EXTRA, D.FC2_N), SENT32, np.float32); init[:M] = resid2
    out = _dev(torch, init)
    binding.op_gemm_mxfp8(EPI_BIAS_RESID, oq.data_ptr(), os_.data_ptr(), W2.data_ptr(), WS2.data_ptr(), B2.data_ptr(), out.data_ptr(), 0, M, D.FC2_N, N)
    torch.cuda.synchronize()
    _same(out.cpu().numpy().view(np.uint32), want.view(np.uint32), f"{D.case_id(case)} fc2 on fc1's buffers (f32 bits)")
    q, s = _fc1_expected(case)                                   # the second GEMM only read them
    _same(os_.cpu().numpy(), s, f"{D.case_id(case)} fc1 scales after fc2")
    _same(oq.cpu().numpy(), q, f"{D.case_id(case)} fc1 elements after fc2")


# ------------------------------------------------------------------------------------------------ d. a row's bits do not depend on M
def test_a_rows_bits_do_not_depend_on_m(binding, torch_gpu):
    """Random (non-exact) operands, M = 257: rows 0, 127, 128 and 256 run alone with M = 1 give the bits they have in the full run, in all three
    epilogues -- no row reads a neighbour's elements or scales, whichever 16-row tile, wave or workgroup it lands in."""
    torch = torch_gpu
    M, N, K = 257, 200, 384
    rng = np.random.default_rng(257)
    kp, npad = D.pad128(K), D.pad128(N)
    a = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-3, 4, (M, K // 32))).repeat(32, axis=1)).astype(np.float32)
    w = np.zeros((npad, K), np.float32); w[:N] = rng.standard_normal((N, K)) * 0.05
    (qa, sa), (qw, sw) = D.mxfp8.encode(a, kp), D.mxfp8.encode(w, kp)
    bias = rng.standard_normal(N).astype(np.float32)
    x0 = rng.standard_normal((M, N)).astype(np.float32)
    A, AS, W, WS, B = (_dev(torch, t) for t in (qa, sa, qw, sw, bias))

    def run(epi, r0, m):
        """rows r0 .. r0 + m of A: the output buffers as bit patterns"""
        pa, ps = A.data_ptr() + r0 * kp, AS.data_ptr() + r0 * (kp // 32)
        if epi == EPI_BIAS_GELU:
            oq = torch.full((m, npad), SENT8, dtype=torch.uint8, device="cuda"); os_ = torch.full((m, npad // 32), SENT8, dtype=torch.uint8, device="cuda")
            binding.op_gemm_mxfp8(epi, pa, ps, W.data_ptr(), WS.data_ptr(), B.data_ptr(), oq.data_ptr(), os_.data_ptr(), m, N, K)
            torch.cuda.synchronize()
            return [oq.cpu().numpy(), os_.cpu().numpy()]
        out = _dev(torch, x0[r0:r0 + m]) if epi == EPI_BIAS_RESID else torch.full((m, N), SENT16, dtype=torch.int16, device="cuda")
        binding.op_gemm_mxfp8(epi, pa, ps, W.data_ptr(), WS.data_ptr(), B.data_ptr(), out.data_ptr(), 0, m, N, K)
        torch.cuda.synchronize()
        return [out.cpu().numpy().view(np.uint32 if epi == EPI_BIAS_RESID else np.uint16)]

    for epi in (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID):
        full = run(epi, 0, M)
        for r in (0, 127, 128, 256):
            for got, whole in zip(run(epi, r, 1), full):
                _same(got, whole[r:r + 1], f"epilogue {epi} row {r} alone against the M = {M} run")


# ------------------------------------------------------------------------------------------------ e. LayerNorm -> MX
LN_HOSTILE_WIDTHS = (64, 192, 384, 768, 1024, 1280)              # tests/test_gpu_hostile.py test_layernorm_mx_hostile_rows


def _ln_inputs(D_):
    """(x, w, b, eps) sets: the rows of tests/test_gpu_mxfp8.py test_layernorm_mx_against_float64 and, for the widths tests/test_gpu_hostile.py
    covers, its hostile rows."""
    rng = np.random.default_rng(D_)
    x = (rng.standard_normal((203, D_)) * 3 + rng.standard_normal((203, 1))).astype(np.float32)
    w = (1 + 0.3 * rng.standard_normal(D_)).astype(np.float32); b = (0.2 * rng.standard_normal(D_)).astype(np.float32)
    sets = [("random", x[:m], w, b, 1e-6) for m in (1, 5, 203)]
    if D_ in LN_HOSTILE_WIDTHS:
        hx, _ = X.hostile_matrix(D_)
        hw, hb = X.ln_params(D_)
        sets.append(("hostile", hx, hw, hb, X.LN_EPS))
    return sets


@pytest.mark.parametrize("D_", X.LN_WIDTHS)
def test_layernorm_mx_is_the_encoder_of_the_f32_layernorm(binding, torch_gpu, D_):
    """layernorm_mx8_kernel is "the f32 value launch_layernorm rounds, encoded" and vitx_op_layernorm_f32 returns that value: the identity
    op_layernorm_mxfp8(x) == mxfp8.encode(op_layernorm_f32(x), mx_k_pad(D)), bytes and scales, at every width and M = 1, 5, 203 (and 640
    hostile rows).  The reference encoder pads with zero elements and scale 127; rows behind M keep their sentinel."""
    torch = torch_gpu
    kp = binding.mx_k_pad(D_)
    for name, x, w, b, eps in _ln_inputs(D_):
        M = x.shape[0]
        dx, dw, db = _dev(torch, x), _dev(torch, w), _dev(torch, b)
        y = torch.full((M, D_), float("nan"), dtype=torch.float32, device="cuda")
        binding.op_layernorm_f32(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), y.data_ptr(), M, D_, eps)
        dq = torch.full((M + A_EXTRA, kp), SENT8, dtype=torch.uint8, device="cuda"); ds = torch.full((M + A_EXTRA, kp // 32), SENT8, dtype=torch.uint8, device="cuda")
        binding.op_layernorm_mxfp8(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), dq.data_ptr(), ds.data_ptr(), M, D_, eps)
        torch.cuda.synchronize()
        y = y.cpu().numpy()
        assert np.isfinite(y).all(), (D_, name, M)
        q = np.full((M + A_EXTRA, kp), SENT8, np.uint8); s = np.full((M + A_EXTRA, kp // 32), SENT8, np.uint8)
        q[:M], s[:M] = D.mxfp8.encode(y, kp)
        assert not q[:M, D_:].any() and (s[:M, D_ // 32:] == 127).all()
        _same(ds.cpu().numpy(), s, f"D {D_} {name} M {M} scales")
        _same(dq.cpu().numpy(), q, f"D {D_} {name} M {M} elements")


# ------------------------------------------------------------------------------------------------ f. refusals
def test_unknown_epilogue_is_refused_and_stores_nothing(binding, torch_gpu):
    torch = torch_gpu
    case = (17, 129, 192, D.SPREAD)
    M, N, K, _ = case
    d = D.gemm_case(case)
    A, AS, W, WS, B = (_dev(torch, d[k]) for k in ("qa", "sa", "qw", "sw", "bias"))
    out = torch.full((M + OUT_EXTRA, N), float(SENT32), dtype=torch.float32, device="cuda")
    sc = torch.full((M + OUT_EXTRA, D.pad128(N) // 32), SENT8, dtype=torch.uint8, device="cuda")
    rc = binding.lib().vitx_op_gemm_mxfp8(3, A.data_ptr(), AS.data_ptr(), W.data_ptr(), WS.data_ptr(), B.data_ptr(), out.data_ptr(), sc.data_ptr(), M, N, K, None)
    torch.cuda.synchronize()
    assert rc == VITX_ERR_ARG, rc
    assert bool((out == float(SENT32)).all()) and bool((sc == SENT8).all())
