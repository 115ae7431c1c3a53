"""Every kernel that normalises a row, byte for byte: each case below runs one entry point on fixed inputs, and the sha1 of its raw output bytes is
the one recorded in tests/golden/ln_row_sha1.json.  The record is made by tests/golden/make_ln_golden.py, which imports CASES from here, on the
MI355X with a library built from a commit whose kernels are trusted -- the JSON names it -- and never from the code under test.

The row arithmetic F = ((x - mean) * rstd) * w + b has one definition (csrc/ln_row.h); the stand-alone LayerNorm, the f32 pre-norm, the
MX-encoding LayerNorm, the fix-up behind the LayerNorm-fusing GEMMs, the feature kernel and the attention-pooling kernel all take their row from
it.  A change to that definition, or to how a kernel stores the row, shows here as a changed hash.

Inputs come from numpy.random.default_rng(D): rows of standard_normal * U(0.2, 3) + U(-2, 2), then one constant row (variance 0) and one row with
a single 1e4 outlier; w = 1 + 0.2 N(0, 1), b = 0.3 N(0, 1).  The shapes are the smallest at which each thing can break: M = 7 rows are two
workgroups of the one-wave-per-row kernels, the second with three rows (the row >= M guard); the feature and pooling widths cover 1, 2 and 4
columns per lane, tiled and flat statistics, one and two rows per step.  Every output buffer carries rows of a sentinel behind its end, which
must stay as they are.

vitx_op_attention_pool has no operand-type argument and no 16-bit output (M and p are f32), so the rounded M (the value projection's operand) and
the pooled embedding's rounding are pinned through the forward of the attention-pooling fixture model, both operand types."""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import exact_data as X
import map_data as MD
import prefix_data as PD

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ln_row_sha1.json")
M_ROWS = 7
TAIL = 3                                   # sentinel rows behind every output
SENT = 9.0                                 # exact in f32, f16 and bf16
SENT_U8 = 0xA5
FEAT_WIDTHS = (64, 192, 256, 768, 1152, 2048)
POOL_WIDTHS = (64, 256, 768, 1152)
GEMM_LN_SHAPES = ((32768, 256, 128), (8192, 1024, 128))
DTYPES = {"f16": 0, "bf16": 1}


@functools.lru_cache(maxsize=None)
def ln_inputs(D, M=M_ROWS):
    """(x [M][D], w [D], b [D]) f32; rows M - 2 and M - 1 are the constant row and the outlier row."""
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((M, D)) * rng.uniform(0.2, 3.0, (M, 1)) + rng.uniform(-2.0, 2.0, (M, 1))).astype(np.float32)
    x[M - 2] = np.float32(3.25)
    x[M - 1, D // 3] = np.float32(1e4)
    w = (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    b = (0.3 * rng.standard_normal(D)).astype(np.float32)
    return x, w, b


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tdt(torch, dtype):
    return torch.float16 if dtype == 0 else torch.bfloat16


def _out(torch, rows, cols, tdt):
    """[rows + TAIL][cols] of the sentinel"""
    if tdt == torch.uint8:
        return torch.full((rows + TAIL, cols), SENT_U8, dtype=tdt, device="cuda")
    return torch.full((rows + TAIL, cols), SENT, dtype=tdt, device="cuda")


def _take(torch, t, rows):
    """The first `rows` rows of an output as bytes; the rows behind them must still hold the sentinel."""
    torch.cuda.synchronize()
    sent = SENT_U8 if t.dtype == torch.uint8 else SENT
    assert bool((t[rows:] == sent).all()), "rows behind the output were written"
    a = t[:rows].contiguous()
    return (a if a.dtype == torch.uint8 else a.view(torch.int16 if a.element_size() == 2 else torch.int32)).cpu().numpy().tobytes()


def _layernorm(D, dtype, eps):
    def run(pkg, binding, torch):
        x, w, b = (_dev(torch, a) for a in ln_inputs(D))
        y = _out(torch, M_ROWS, D, _tdt(torch, dtype))
        binding.check(binding.lib().vitx_op_layernorm(dtype, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M_ROWS, D, eps, None), "vitx_op_layernorm")
        return [_take(torch, y, M_ROWS)]
    return run


def _layernorm_f32(D, in_place):
    def run(pkg, binding, torch):
        x, w, b = (_dev(torch, a) for a in ln_inputs(D))
        y = _out(torch, M_ROWS, D, torch.float32)
        if in_place:
            y[:M_ROWS] = x
        binding.op_layernorm_f32(y.data_ptr() if in_place else x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M_ROWS, D, 1e-6)
        return [_take(torch, y, M_ROWS)]
    return run


def _layernorm_mx(D):
    def run(pkg, binding, torch):
        x, w, b = (_dev(torch, a) for a in ln_inputs(D))
        kp = binding.mx_k_pad(D)
        q, s = _out(torch, M_ROWS, kp, torch.uint8), _out(torch, M_ROWS, kp // 32, torch.uint8)
        binding.op_layernorm_mxfp8(x.data_ptr(), w.data_ptr(), b.data_ptr(), q.data_ptr(), s.data_ptr(), M_ROWS, D, 1e-6)
        return [_take(torch, q, M_ROWS), _take(torch, s, M_ROWS)]
    return run


N_IMG, N_TOK, POOL_HEADS = 2, 6, 2


def _features(D, first, l2, z_dtype=None):
    """cls + mean + tokens of 2 images of 6 rows (out_img_stride = the token block: cls and mean leave the rest of theirs to the sentinel), and
    with z_dtype the pooled head's operand."""
    def run(pkg, binding, torch):
        x, w, b = (_dev(torch, a) for a in ln_inputs(D, N_IMG * N_TOK))
        stride = (N_TOK - first) * D
        cls, mean, tok = (_out(torch, N_IMG, stride, torch.float32) for _ in range(3))
        z = _out(torch, N_IMG, 2 * D, _tdt(torch, z_dtype)) if z_dtype is not None else None
        binding.op_features_ex(x.data_ptr(), D, N_TOK * D, w.data_ptr(), b.data_ptr(), cls.data_ptr(), mean.data_ptr(), tok.data_ptr(), stride,
                               N_IMG, N_TOK, first, D, 1e-6, l2, z.data_ptr() if z is not None else 0, z_dtype or 0)
        return [_take(torch, t, N_IMG) for t in (cls, mean, tok)] + ([_take(torch, z, N_IMG)] if z is not None else [])
    return run


def _attention_pool(D):
    def run(pkg, binding, torch):
        x, w, b = (_dev(torch, a) for a in ln_inputs(D, N_IMG * N_TOK))
        u = _dev(torch, (np.random.default_rng(D + 1).standard_normal((POOL_HEADS, D)) * 2.0 / np.sqrt(D)).astype(np.float32))
        Mo, p = _out(torch, N_IMG, POOL_HEADS * D, torch.float32), _out(torch, N_IMG, POOL_HEADS * N_TOK, torch.float32)
        binding.op_attention_pool(x.data_ptr(), D, N_TOK * D, w.data_ptr(), b.data_ptr(), 1e-6, u.data_ptr(), Mo.data_ptr(), p.data_ptr(), N_IMG, N_TOK, D, POOL_HEADS)
        return [_take(torch, Mo, N_IMG), _take(torch, p, N_IMG)]
    return run


def _map_forward(dtype):
    """The forward of the attention-pooling fixture model: probabilities, logits and the pooled embedding of 3 images."""
    def run(pkg, binding, torch):
        model = binding.Model(MD.fixture_file(pkg))
        ctx = binding.Context(model, device=0, max_batch=3, dtype=dtype)
        ctx.feat_enable(cls=True)
        probs, logits = ctx.forward(PD.exact_images(3, 56, seed=1), want_logits=True)
        (feats,) = ctx.feat_read(3).values()                # the last layer's
        e = feats["cls"]
        ctx.close(); model.close()
        return [np.ascontiguousarray(a, np.float32).tobytes() for a in (probs, logits, e)]
    return run


@functools.lru_cache(maxsize=None)
def gemm_ln_inputs(M, N, K):
    """A [M][K], W [N][K], bias [N], residual rows [M][N] (ln_inputs' distribution), LayerNorm w, b: f32, drawn from default_rng(N)."""
    rng = np.random.default_rng(N)
    x = (rng.standard_normal((M, N), dtype=np.float32) * rng.uniform(0.2, 3.0, (M, 1)).astype(np.float32) + rng.uniform(-2.0, 2.0, (M, 1)).astype(np.float32))
    x[M - 2] = np.float32(3.25)
    x[M - 1, N // 3] = np.float32(1e4)
    w = (1.0 + 0.2 * rng.standard_normal(N)).astype(np.float32)
    b = (0.3 * rng.standard_normal(N)).astype(np.float32)
    a = (rng.standard_normal((M, K), dtype=np.float32) * np.float32(0.5))
    wt = (rng.standard_normal((N, K), dtype=np.float32) * np.float32(0.05))
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    return a, wt, bias, x, w, b


def _gemm_ln(M, N, K, dtype, test):
    """y only: how many tiles take the fix-up launch may vary, the bits may not."""
    def run(pkg, binding, torch):
        a, wt, bias, x, w, b = gemm_ln_inputs(M, N, K)
        tdt = _tdt(torch, dtype)
        A, W = _dev(torch, a).to(tdt), _dev(torch, wt).to(tdt)
        B, R, lw, lb = (_dev(torch, t) for t in (bias, x, w, b))
        y = _out(torch, M, N, tdt)
        fb = ctypes.c_int(-1)
        binding.check(binding.lib().vitx_op_gemm_ln(dtype, A.data_ptr(), W.data_ptr(), B.data_ptr(), R.data_ptr(), lw.data_ptr(), lb.data_ptr(), y.data_ptr(),
                                                    M, N, K, 1e-6, test, 50 if test else 200, fb, None), "vitx_op_gemm_ln")
        assert fb.value >= (1 if test else 0)
        return [_take(torch, y, M)]
    return run


CASES = {}
for _D in X.LN_WIDTHS:
    for _name, _dt in DTYPES.items():
        CASES[f"layernorm_{_name}_D{_D}"] = _layernorm(_D, _dt, 1e-6)
        if _D in (192, 768):
            CASES[f"layernorm_{_name}_D{_D}_eps1e-5"] = _layernorm(_D, _dt, 1e-5)
    CASES[f"layernorm_f32_D{_D}"] = _layernorm_f32(_D, False)
    if _D in (192, 768):
        CASES[f"layernorm_f32_D{_D}_in_place"] = _layernorm_f32(_D, True)
    CASES[f"layernorm_mxfp8_D{_D}"] = _layernorm_mx(_D)
for _D in FEAT_WIDTHS:
    for _first in (1, 2):
        for _l2 in (False, True):
            CASES[f"features_D{_D}_first{_first}_l2{int(_l2)}"] = _features(_D, _first, _l2)
    for _name, _dt in DTYPES.items():
        CASES[f"features_D{_D}_z_{_name}"] = _features(_D, 1, False, _dt)
for _D in POOL_WIDTHS:
    CASES[f"attention_pool_D{_D}"] = _attention_pool(_D)
for _name, _dt in DTYPES.items():
    CASES[f"map_forward_{_name}"] = _map_forward(_dt)
    for _shape in GEMM_LN_SHAPES:
        for _test in (0, 1):
            CASES["gemm_ln_{}_M{}_N{}_K{}_test{}".format(_name, *_shape, _test)] = _gemm_ln(*_shape, _dt, _test)


def sha1_of(pkg, binding, torch, name):
    h = hashlib.sha1()
    for part in CASES[name](pkg, binding, torch):
        h.update(len(part).to_bytes(8, "little"))
        h.update(part)
    return h.hexdigest()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_record_holds_exactly_these_cases(recorded):
    assert sorted(recorded["sha1"]) == sorted(CASES) and len(recorded["commit"]) == 40


@pytest.mark.parametrize("name", list(CASES))
def test_normalised_rows_keep_their_bytes(pkg, binding, torch_gpu, recorded, name):
    assert sha1_of(pkg, binding, torch_gpu, name) == recorded["sha1"][name]
