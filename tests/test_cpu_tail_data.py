"""Every condition test_gpu_tail.py relies on (tests/tail_data.py), checked without a GPU; the two entry points it calls and the argument checks
that return before any launch; and the order of vitx_topk on rows with ties, signed zeros, infinities and NaNs."""
import ctypes as C
import math

import numpy as np
import pytest

import tail_data as T

ERR_ARG = 3


# ------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------
def test_entries_exported_and_arguments_checked(binding):
    """vitx_op_topk and vitx_op_dequant_jobs exist; they and vitx_op_softmax_dt refuse what they cannot run with VITX_ERR_ARG, before any
    HIP call (no device is needed to get the refusal; the pointers only have to be non-null)."""
    L = binding.lib()
    for s in ("vitx_op_topk", "vitx_op_dequant_jobs"):
        assert s in binding.EXPORTS and hasattr(L, s), s
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    for args in ((None, 1, 4, 2, p), (p, 1, 4, 2, None), (p, 0, 4, 2, p), (p, -1, 4, 2, p), (p, 1, 0, 1, p), (p, 1, 4, 0, p), (p, 1, 4, -1, p), (p, 1, 4, 5, p)):
        assert L.vitx_op_topk(*args, None) == ERR_ARG, args
    assert b"vitx_op_topk" in L.vitx_last_error()
    for dt in (binding.F16, binding.BF16):
        for cols, ld in ((4, 3), (1000, 999), (1, 0), (4, -4)):
            assert L.vitx_op_softmax_dt(dt, p, p, 1, cols, ld, None) == ERR_ARG, (cols, ld)
    assert L.vitx_op_softmax(p, p, 1, 4, 3, None) == ERR_ARG
    assert L.vitx_op_softmax_dt(2, p, p, 1, 4, 4, None) == ERR_ARG

    vp4, i4 = C.c_void_p * 4, C.c_int * 4
    ptrs, N, n_pad, K = vp4(p, p, p, p), i4(2, 2, 2, 2), i4(2, 3, 2, 2), i4(32, 32, 64, 32)

    def jobs(dtype=0, qtype=3, njobs=4, blocks=ptrs, scales=ptrs, out=ptrs, N=N, n_pad=n_pad, K=K):
        return L.vitx_op_dequant_jobs(dtype, qtype, njobs, blocks, scales, out, N, n_pad, K, None)
    for bad in (dict(njobs=0), dict(njobs=5), dict(njobs=-1), dict(dtype=2), dict(blocks=None), dict(out=None), dict(N=None), dict(n_pad=None), dict(K=None),
                dict(blocks=vp4(p, None, p, p)), dict(out=vp4(p, p, None, p)), dict(N=i4(2, 2, 0, 2)), dict(n_pad=i4(2, 3, 2, 1)), dict(K=i4(32, 32, 48, 32)),
                dict(K=i4(32, 0, 64, 32)), dict(qtype=5), dict(qtype=2, scales=None), dict(qtype=2, scales=vp4(p, p, p, None))):
        assert jobs(**bad) == ERR_ARG, bad
    assert jobs(njobs=1, qtype=5, blocks=vp4(p, None, None, None), out=vp4(p, None, None, None), N=i4(2, 0, 0, 0), n_pad=i4(2, 0, 0, 0), K=i4(32, 0, 0, 0)) == ERR_ARG
    assert b"vitx_op_dequant_jobs" in L.vitx_last_error()


# ------------------------------------------------------------------------------------------------------------------
# the number formats
# ------------------------------------------------------------------------------------------------------------------
def test_rounding_helpers_agree():
    """round64_to (one rounding from float64) against numpy's own float64 -> float16, and to_bits (from f32) against it for both types on
    values that are f32 already: normal, subnormal, ties, both signs."""
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(20000) * np.exp2(rng.integers(-26, 15, 20000)), np.arange(-4096, 4096) * 2.0 ** -25,
                        (np.arange(2048, 4096) + 0.5) * 2.0 ** -5, [0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25]])
    x32 = x.astype(np.float32)
    assert np.array_equal(T.round64_to(x32.astype(np.float64), T.F16), x32.astype(np.float64).astype(np.float16).astype(np.float64))
    for dt in (T.F16, T.BF16):
        assert np.array_equal(T.round_to(x32, dt).astype(np.float64), T.round64_to(x32.astype(np.float64), dt))
        b = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
        fin = ~T.is_nan_bits(b, dt)
        assert np.array_equal(T.to_bits(T.from_bits(b[fin], dt), dt), b[fin])           # every value of the type survives the round trip
    assert T.to_bits(np.array([65520.0, 1e9, -1e9], np.float32), T.F16).tolist() == [0x7c00, 0x7c00, 0xfc00]      # f16 overflow gives inf
    assert T.is_nan_bits(T.to_bits(np.array([np.nan], np.float32), T.BF16), T.BF16).all()


# ------------------------------------------------------------------------------------------------------------------
# softmax
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n_all,n_omitted", [(T.F16, 19713, 268), (T.BF16, 16801, 4)])
def test_exp_arguments(dtype, n_all, n_omitted):
    allx = T.exp_arguments(dtype)
    assert allx.size == n_all and allx[0] == 0 and np.signbit(allx[0]) and allx[-1] == -20.0 and (np.diff(allx) < 0).all()
    assert np.array_equal(T.round_to(allx, dtype), allx)                                  # values of the type: rnd<T>(x - 0) is x
    x, e, omitted = T.safe_exp_arguments(dtype)
    assert omitted == n_omitted and x.size == n_all - omitted and omitted < 0.02 * n_all
    e64 = np.exp(x.astype(np.float64))
    assert (T.tie_distance_ulps(e64, dtype) > T.SAFE_ULPS).all()
    # e is the ONE value any expf within SAFE_ULPS - 1 ulps rounds to: the same from float64 in one rounding, and from the f32 values
    # SAFE_ULPS - 1 ulps either side
    assert np.array_equal(e.astype(np.float64), T.round64_to(e64, dtype))
    ulp = np.ldexp(1.0, np.frexp(e64)[1] - 1 - 23)
    for off in (-(T.SAFE_ULPS - 1), T.SAFE_ULPS - 1):
        assert np.array_equal(T.round_to((e64 + off * ulp).astype(np.float32), dtype), e)
    if dtype == T.F16:
        assert int((e == 0).sum()) == 171 and (x[e == 0] < -17.3).all()
        sub = (e > 0) & (e < 2.0 ** -14)
        assert int(sub.sum()) > 800                                                      # the f16 subnormal results are in (886 of the 891 there are)
    else:
        assert (e >= 2.0 ** -126).all()


@pytest.mark.parametrize("dtype", [T.F16, T.BF16])
def test_exp_case_layout_and_what_it_detects(dtype):
    cols, ld = 1000, 1024
    x, e, _ = T.safe_exp_arguments(dtype)
    plain, e64, p_ref = T.exp_case(dtype)
    moved, e64_m, p_ref_m = T.exp_case(dtype, perturbed=True)
    rows = plain.shape[0]
    assert plain.shape == (rows, ld) and e64.shape == p_ref.shape == (rows, cols) and rows == math.ceil(x.size / (cols - 1))
    assert np.array_equal(e64, e64_m) and np.array_equal(p_ref, p_ref_m)
    hot = T.routed_hot(rows, cols)
    for lg in (plain, moved):
        body = lg[:, :cols]
        assert (body[np.arange(rows), hot] == 0).all() and not np.signbit(body[np.arange(rows), hot]).any() and (body <= 0).all() and (body >= -20.01).all()
        assert (body.max(1) == 0).all()
        pad = lg[:, cols:]
        assert np.isnan(pad[:, 0::2]).all() and np.isposinf(pad[:, 1::2]).all()
        assert np.array_equal(T.round_to(body, dtype), plain[:, :cols])                   # rnd<T>(x - max) is the listed argument
    assert set(np.unique(plain[:, :cols]).tolist()) == set(np.unique(x).tolist()) | {0.0}   # every safe argument occurs
    off = moved[:, :cols] != plain[:, :cols]
    assert off.sum() >= 0.99 * (rows * (cols - 1)) and (T.round_to(moved[:, :cols], dtype) != moved[:, :cols])[off].all()
    assert np.array_equal(e64, T.round_to(np.exp(plain[:, :cols].astype(np.float64)).astype(np.float32), dtype).astype(np.float64))
    assert (p_ref[e64 > 0] > 2.0 ** -100).all() and np.allclose(p_ref.sum(1), 1.0, rtol=1e-12)

    # the definition passes on both; without the outer rounding it fails on both; without the inner one it fails where the arguments
    # are off the grid (on the grid the inner rounding is the identity by construction: that is what makes e known there)
    for lg in (plain, moved):
        assert T.softmax_gate_ratio(T.softmax_model(lg, cols, dtype), p_ref, cols) <= 1e-6
        assert T.softmax_gate_ratio(T.softmax_model(lg, cols, dtype, outer=False), p_ref, cols) > 100
    assert T.softmax_gate_ratio(T.softmax_model(moved, cols, dtype, inner=False), p_ref, cols) > 100
    assert T.softmax_gate_ratio(T.softmax_model(plain, cols, dtype, inner=False), p_ref, cols) <= 1e-6


def _kernel_sum_f32(e32: np.ndarray) -> np.ndarray:
    """softmax_kernel's arithmetic after the numerators, in numpy float32: per-thread strided sums, six butterfly steps, the four wave
    sums, one reciprocal, one product."""
    rows, cols = e32.shape
    n = math.ceil(cols / 256)
    pad = np.zeros((rows, n * 256), np.float32); pad[:, :cols] = e32
    t = np.zeros((rows, 256), np.float32)
    for j in range(n):
        t = t + pad[:, j * 256:(j + 1) * 256]
    w = t.reshape(rows, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ o]
    red = w[:, :, 0]
    inv = np.float32(1.0) / ((red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3]))
    return e32 * inv[:, None]


@pytest.mark.parametrize("dtype", [T.F16, T.BF16])
def test_softmax_gate_holds_for_the_kernels_arithmetic(dtype):
    """The gate is derived, not measured: (ceil(cols / 256) + 10) * 2^-24.  The kernel's own order of operations in f32 stays inside it, here
    and on adversarially rounded sums (10 000 random rows of the same numerators)."""
    cols = 1000
    assert T.softmax_gate(cols) == 14 * 2.0 ** -24 * 1.01 and T.softmax_gate(1) == 11 * 2.0 ** -24 * 1.01 and T.softmax_gate(257) == 12 * 2.0 ** -24 * 1.01
    _, e64, p_ref = T.exp_case(dtype)
    assert T.softmax_gate_ratio(_kernel_sum_f32(e64.astype(np.float32)), p_ref, cols) <= 1.0
    _, e, _ = T.safe_exp_arguments(dtype)
    rnd = e[np.random.default_rng(3).integers(0, e.size, (10000, cols))].astype(np.float64)
    rnd[:, 0] = 1.0
    r = T.softmax_gate_ratio(_kernel_sum_f32(rnd.astype(np.float32)), rnd / rnd.sum(1, keepdims=True), cols)
    assert r <= 1.0, r


def test_flat_routed_and_shift_data():
    shapes = T.sm_shapes()
    assert {s[1] for s in shapes} == set(T.SM_COLS) and {s[0] for s in shapes} == set(T.SM_ROWS)
    for cols in T.SM_COLS:
        lds = {s[2] for s in shapes if s[1] == cols}
        assert lds == {cols, cols + 1, T.round_up(cols, 256)} and min(lds) >= cols
        assert {s[0] for s in shapes if s[1] == cols} == ({1, 37} if cols == 21843 else set(T.SM_ROWS))
        # flat: the sum of `cols` ones is exact in f32 in any order, and 1 * (1 / cols) is the correctly rounded quotient
        assert cols < 2 ** 24 and np.float32(1) * (np.float32(1) / np.float32(cols)) == np.float32(1) / np.float32(cols)
    for dt in (T.F16, T.BF16):
        assert T.round_to(np.array([-200.0], np.float32), dt)[0] == -200.0            # routed: the cold logit is a value of both types,
    assert np.exp(np.float64(-200.0)) < 2.0 ** -150                                    # and its exponential is +0 in f32
    for lvl in T.SM_LEVELS:
        assert np.float32(lvl) == lvl
    hot = T.routed_hot(1025, 1000)
    assert set((hot % 256).tolist()) == set(range(256))                              # every thread of the block owns the maximum in some row
    assert set(T.routed_hot(37, 64).tolist()) >= set(range(3, 64, 7))
    x = T.shift_logits(37, 1000, 1)
    assert (x == np.rint(x)).all() and np.abs(x).max() == 20 and (x.max(1) == 20).all()
    for s in T.SHIFTS:
        y = x + np.float32(s)
        assert np.array_equal(y.astype(np.float64), x.astype(np.float64) + s)          # the shifted logits are exact in f32
        d = y - y.max(1, keepdims=True)
        assert np.array_equal(d, x - 20) and all(np.array_equal(T.round_to(d, dt), d) for dt in (T.F16, T.BF16))


# ------------------------------------------------------------------------------------------------------------------
# top-k
# ------------------------------------------------------------------------------------------------------------------
def host_topk(L, row: np.ndarray, k: int):
    """vitx_topk on one row: (value bits u32 [k], class i32 [k])."""
    row = np.ascontiguousarray(row, np.float32)
    idx = np.full(k, -7, np.int32); val = np.zeros(k, np.float32)
    rc = L.vitx_topk(row.ctypes.data_as(C.POINTER(C.c_float)), row.size, k, idx.ctypes.data_as(C.POINTER(C.c_int32)), val.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0
    return val.view(np.uint32), idx


def test_topk_sizes():
    assert T.tk_ks(1) == [1] and T.tk_ks(2) == [1, 2] and T.tk_ks(63) == [1, 2, 5, 63] and T.tk_ks(65) == [1, 2, 5, 65]
    assert T.tk_ks(127) == [1, 2, 5, 70, 127] and T.tk_ks(129) == [1, 2, 5, 70, 129] and T.tk_ks(1000) == [1, 2, 5, 70]
    assert {r % 4 for r in T.TK_ROWS} == {0, 1, 3} and max(T.TK_ROWS) > 8


@pytest.mark.parametrize("kind", T.TK_KINDS)
def test_topk_rows_and_the_host_order(binding, kind):
    """The rows are what their kind says; the order has every index once, not-NaN entries first, descending, ties by index; vitx_topk
    returns exactly that order, value bits included -- with NaNs in the row too, where `>` and `==` alone are no strict weak order."""
    L = binding.lib()
    for cols in T.TK_COLS:
        rows = T.topk_rows(kind, cols)
        assert rows.shape == (max(T.TK_ROWS), cols) and rows.dtype == np.float32
        nan = np.isnan(rows)
        if kind in ("levels", "equal", "ascending", "descending", "max_last", "zeros"):
            assert not nan.any() and rows.max() <= 1.0 < T.TK_GUARD and rows.min() >= 0.0
        if kind == "levels":
            assert cols < 64 or np.unique(rows).size == T.TK_LEVELS.size
        if kind == "equal":
            assert (rows == rows[:, :1]).all() and (rows[0] == 0).all()
        if kind == "ascending":
            assert (np.diff(rows, axis=1) > 0).all()
        if kind == "descending":
            assert (np.diff(rows, axis=1) < 0).all()
        if kind == "max_last":
            assert (rows.argmax(1) == cols - 1).all() and (cols == 1 or (rows[:, :-1].max(1) < rows[:, -1]).all())
        if kind == "zeros":
            assert (rows == 0).all() and (cols < 63 or (np.signbit(rows).any(1) & (~np.signbit(rows)).any(1)).all())
        if kind == "inf":
            assert not nan.any() and np.isinf(rows).any(1).all() and (cols < 63 or (np.isposinf(rows).any() and np.isneginf(rows).any()))
        if kind == "nan_one":
            assert (nan.sum(1) == 1).all()
        if kind == "nan_some":
            assert (nan.sum(1) == max(1, cols // 4)).all() and (cols < 63 or np.unique(rows.view(np.uint32)[nan]).size > 1)
        if kind == "nan_all":
            assert nan.all()
        if kind in T.TK_TIED:
            for k in T.tk_ks(cols):
                assert k == cols or T.straddles(rows[0], k), (cols, k)          # row 0 is in every case, whatever its row count
        for r in rows:
            o = T.topk_order(r)
            assert sorted(o.tolist()) == list(range(cols))
            n_ok = int((~np.isnan(r)).sum())
            assert not np.isnan(r[o[:n_ok]]).any() and np.isnan(r[o[n_ok:]]).all() and (np.diff(o[n_ok:]) > 0).all()
            v = r[o[:n_ok]]
            assert (v[:-1] >= v[1:]).all() and (np.diff(o[:n_ok])[v[:-1] == v[1:]] > 0).all()
        for k in T.tk_ks(cols):
            vals, idx = T.topk_expected(rows, k)
            for r in range(rows.shape[0]):
                hv, hi = host_topk(L, rows[r], k)
                assert np.array_equal(hi, idx[r]) and np.array_equal(hv, vals[r]), (kind, cols, k, r, hi[:8], idx[r][:8])


# ------------------------------------------------------------------------------------------------------------------
# dequant
# ------------------------------------------------------------------------------------------------------------------
def _codes_of(qtype, blocks):
    """The stored codes back from the bytes, with ggml's own shifts (dequant_f32 at d = 1, m = 0 undoes nothing but the offset)."""
    b = blocks.copy()
    b[:, 0:2] = np.array([0x3c00], np.uint16).view(np.uint8)
    if qtype in T.HAS_MIN:
        b[:, 2:4] = 0
    v = T.dequant_f32(qtype, b).astype(np.int64)
    return v + {T.Q4_0: 8, T.Q5_0: 16}.get(qtype, 0) if qtype != T.Q8_0 else v & 0xff


@pytest.mark.parametrize("qtype", T.QTYPES)
def test_dequant_blocks_and_reference(pkg, qtype):
    G = pkg.ggml_file
    n = T.N_CODES[qtype]
    assert G.BLOCK_BYTES[qtype] == T.BLOCK_BYTES[qtype]
    N, K = T.sweep_shape(qtype)
    assert N * (K // 32) == n
    for d_bits, m_bits in T.SWEEP_SCALES:
        blocks = T.sweep_blocks(qtype, d_bits, m_bits)
        assert blocks.shape == (n, T.BLOCK_BYTES[qtype])
        codes = _codes_of(qtype, blocks)
        for i in range(32):
            assert sorted(codes[:, i].tolist()) == list(range(n)), i            # every code at every position
        assert np.array_equal(codes, (np.arange(n)[:, None] + np.arange(32)[None, :]) % n)
        for dt in (T.F16, T.BF16):
            bits = T.to_bits(T.dequant_f32(qtype, blocks), dt)
            if (d_bits, m_bits) == T.SWEEP_SCALES[0] or qtype != T.Q8_0 or dt == T.F16:
                assert all(np.unique(bits[:, i]).size == n for i in range(32)), (dt, d_bits)   # and every code gives another output value
    # the reference is ggml's dequantize_row_* as the package's file reader states it (pinned to the reference elsewhere), on finite scales
    sc = T.hostile_scales()
    assert sc.size == 40 and set(T.FIXED_SCALES) <= set(sc.tolist()) and not T.is_nan_bits(sc, T.F16).any() and ((sc & 0x7c00) != 0x7c00).all()
    for (N, n_pad, K) in T.dq_shapes():
        blocks = T.scaled_blocks(qtype, N, K, N + K, sc)
        assert blocks.shape == (N * K // 32, T.BLOCK_BYTES[qtype])
        mine = T.dequant_f32(qtype, blocks)
        assert np.array_equal(mine.view(np.uint32).ravel(), G.dequantize(qtype, blocks.tobytes(), N * K).view(np.uint32))
        assert np.isfinite(mine).all()
        whole = T.dequant_bits(qtype, blocks, T.F16, N, n_pad, K)
        assert whole.shape == (n_pad, K) and not whole[N:].any()
    big = T.scaled_blocks(qtype, 200, 448, 648, sc)
    d_used = set(big[:, 0:2].copy().view(np.uint16).ravel().tolist())
    assert d_used == set(sc.tolist())                                           # 200 rows: every scale is some row's d
    if qtype in T.HAS_MIN:
        assert set(big[:, 2:4].copy().view(np.uint16).ravel().tolist()) == set(sc.tolist())
    f16 = T.to_bits(T.dequant_f32(qtype, big), T.F16)
    assert (f16 & 0x7fff == 0x7c00).any() and ((f16 & 0x7c00 == 0) & (f16 & 0x3ff != 0)).any()      # f16 overflow to inf and subnormal results occur
    n_bad, bad = T.nonfinite_blocks(qtype)
    out = T.dequant_f32(qtype, bad)
    assert bad.shape[0] == n_bad * 2 and np.isnan(out).any() and np.isinf(out).any() and np.isfinite(out).any()
    shapes = T.dq_shapes()
    assert {s[0] for s in shapes} == set(T.DQ_N) and {s[2] for s in shapes} == set(T.DQ_K)
    assert all({s[1] for s in shapes if s[0] == N} == {N, N + 3, T.round_up(N, 256)} for N in T.DQ_N)
    assert [T.job_n_pad(N, j) - N for j, (N, K) in enumerate(T.JOB_SHAPES)] == [5, 0, 13, 64] and T.JOB_SHAPES == ((192, 64), (64, 64), (256, 64), (64, 256))


def test_a_contracted_multiply_add_cannot_show():
    """The search the tests were meant to carry -- elements whose result differs between code * d rounded, then + m rounded, and one fused
    multiply-add -- finds nothing, and cannot: code * d (5 bits by 11) is exact in f32 for every code and every finite f16 d, so both
    evaluations round the same exact sum once.  Asserted over all 32 * 63 488 products."""
    n, inexact, differ = T.fused_search()
    assert n == 32 * 63488 and inexact == 0 and differ == 0


@pytest.mark.parametrize("dtype", [T.F16, T.BF16])
@pytest.mark.parametrize("qtype", T.HAS_MIN)
def test_double_rounding_elements(qtype, dtype):
    """What CAN hide behind the 16-bit rounding: rounding code * d + m to the operand type at once instead of to f32 first.  The generator
    keeps blocks whose every element tells the two apart."""
    blocks, found = T.double_rounding_blocks(qtype, dtype)
    assert found >= T.DOUBLE_ROUNDING_WANT[(qtype, dtype)] and blocks.shape[0] == found
    if not found:
        return
    d = blocks[:, 0:2].copy().view(np.float16).astype(np.float64); m = blocks[:, 2:4].copy().view(np.float16).astype(np.float64)
    c = _codes_of(qtype, blocks).astype(np.float64)
    assert (c == c[:, :1]).all()
    exact = c * d + m
    via_f32 = T.dequant_f32(qtype, blocks)
    assert np.array_equal(via_f32, exact.astype(np.float32))
    assert (T.round_to(via_f32, dtype).astype(np.float64) != T.round64_to(exact, dtype)).all()
