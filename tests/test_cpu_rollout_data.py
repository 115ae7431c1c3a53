"""The conditions the single-kernel rollout tests rely on (tests/rollout_data.py; tests/test_gpu_rollout.py), checked without a GPU: the exact
data is exact, the token counts reach every build and edge, every mutant of the definition is seen, and the bounds leave an f32 evaluation of
the definition below half of them."""
import numpy as np
import pytest

import rollout_data as R


def test_token_counts_reach_every_build_and_edge():
    assert {R.step_build(N) for N in R.STEP_N} == {1, 2, 4, 8, 16}
    for edge in (64, 128, 256, 512):                               # both sides of every build edge
        assert edge in R.STEP_N and edge + 1 in R.STEP_N and R.step_build(edge) < R.step_build(edge + 1)
    assert {N % 4 for N in R.STEP_N} == {0, 1, 2, 3}
    assert {N % 16 for N in R.STEP_N} >= {15, 0, 1, 2, 3}
    assert min(R.STEP_N) == 1 and max(R.STEP_N) == R.MAX_TOKENS
    assert all(R.n_images(N) == (3 if N <= 259 else 2) for N in R.STEP_N)
    assert {R.step_build(N) for N in R.STEP_ORDINARY_N} == {2, 4, 16} and {N % 4 for N in R.STEP_ORDINARY_N} == {0, 1, 2}
    assert {R.row_exact_h(N) for N in R.ROW_EXACT_N} == set(R.ROW_EXACT_H)
    assert {H for _, H in R.ROW_ORDINARY} == {3, 12} and all(N >= H + 2 for N, H in R.ROW_ORDINARY)


@pytest.mark.parametrize("N", R.STEP_N)
def test_step_exact_data_and_its_mutants(N):
    """step_exact asserts the 2^24 condition and the lossless cast itself; here: the ranges, that the images differ, that neither operand is
    symmetric, that a . r != r . a, and that every mutant defined at N changes an element of the expected buffer of EVERY seed the GPU test
    uses (0: the first launch, 1: the launch with the buffers' roles exchanged)."""
    for seed in (0, 1):
        a, r, exp = R.step_exact(N, seed)
        n = R.n_images(N)
        assert a.shape == r.shape == exp.shape == (n, N, N) and exp.dtype == np.float32
        p = a.astype(np.float64) * R.A_DEN
        assert np.array_equal(p, np.round(p)) and np.abs(p).max() <= R.A_MAX and np.abs(p).min() >= 1
        assert np.array_equal(r, np.round(r)) and np.abs(r).max() <= R.R_MAX and np.abs(r).min() >= 1
        for b in range(1, n):
            assert not np.array_equal(a[b], a[0]) and not np.array_equal(r[b], r[0]) and not np.array_equal(exp[b], exp[0])
        if N > 1:
            for b in range(n):
                assert not np.array_equal(a[b], a[b].T) and not np.array_equal(r[b], r[b].T)
        mut = R.step_mutants(a, r)
        want = {"last_64_column_group_unwritten", "image_0_r"}
        want |= {"k_tail_dropped", "no_zero_padding"} if N % 4 else set()
        want |= {"last_row_block_unwritten", "last_16_columns_unwritten"} if N % 16 else set()
        want |= {"r_transposed", "r_times_a"} if N > 1 else set()
        want |= {"in_place_hazard"} if N > 64 else set()
        assert set(mut) == want
        for name, m in mut.items():
            assert m.shape == exp.shape and (m != exp.astype(np.float64)).any(), (N, seed, name)
        # an in-place step whose r IS a (the overlap vitx_op_rollout_step refuses) is another product altogether
        if N > 1:
            assert not np.array_equal(a.astype(np.float64) @ a.astype(np.float64), exp.astype(np.float64))


def test_every_step_mutant_is_defined_somewhere():
    seen = set()
    for N in (3, 66):
        a, r, _ = R.step_exact(N)
        seen |= set(R.step_mutants(a, r))
    assert len(seen) == 9


@pytest.mark.parametrize("N", R.STEP_ORDINARY_N)
def test_step_ordinary_bound_holds_for_an_f32_emulation_and_sees_every_mutant(N):
    """The factors are non-negative and row-stochastic with peaked rows; an f32 evaluation of the definition (sequential, and numpy's blocked
    one) needs less than half of step_bound; every mutant exceeds it on at least one element.  Above 300 tokens: image 0 only (time)."""
    f, r0 = R.step_ordinary(N)
    a, r = f[0], r0
    assert a.dtype == r.dtype == np.float32 and (a >= 0).all() and (r >= 0).all()
    for x in (a, r):
        assert np.abs(x.astype(np.float64).sum(axis=-1) - 1.0).max() <= 1e-5
        off = x - 0.5 * np.eye(N, dtype=np.float32)
        assert np.median(off.max(axis=-1)) > 5.0 * 0.5 / N                   # peaked: a uniform row would have 0.5 / N
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(r[0], r[1])
    k = len(a) if N <= 300 else 1
    a64, r64 = a[:k].astype(np.float64), r[:k].astype(np.float64)
    ref = a64 @ r64
    bound = R.step_bound(N, ref)                                             # non-negative data: |a| . |r| is the product itself
    assert (bound > 0).all()
    for emu in (R.matmul_f32_sequential(a[:k], r[:k]), a[:k] @ r[:k]):
        ratio = float((np.abs(emu.astype(np.float64) - ref) / bound).max())
        assert ratio < 0.5, (N, ratio)
    full = R.step_mutants(a.astype(np.float64), r.astype(np.float64))
    for name, m in full.items():
        err = np.abs(m - a.astype(np.float64) @ r.astype(np.float64))
        assert (err > R.step_bound(N, a.astype(np.float64) @ r.astype(np.float64))).any(), (N, name)


def test_step_chain_bound_holds_for_an_f32_emulation():
    """Four steps in f32 against the float64 chain: within 4 * N * 2^-23 relative to the (non-negative) chain itself, with room to spare."""
    N = 197
    f, r0 = R.step_ordinary(N, steps=4)
    got, ref = r0[:1], r0[:1].astype(np.float64)
    for l in range(4):
        got = R.matmul_f32_sequential(f[l][:1], got)
        ref = f[l][:1].astype(np.float64) @ ref
    ratio = float((np.abs(got.astype(np.float64) - ref) / (4 * R.step_bound(N, ref))).max())
    assert ratio < 0.5, ratio


@pytest.mark.parametrize("N", R.ROW_EXACT_N)
def test_row_exact_data_and_its_mutants(N):
    cls, r, w, out = R.row_exact(N)
    n, H = R.n_images(N), R.row_exact_h(N)
    assert cls.shape == (n, H, N) and r.shape == (n, N, N) and w.shape == out.shape == (n, N)
    p = cls.astype(np.float64) * R.CLS_DEN
    assert np.array_equal(p, np.round(p)) and 1 <= np.abs(p).min() and np.abs(p).max() <= R.CLS_MAX
    assert float(np.float32(1.0) / np.float32(H)) * H == 1.0                 # inv_h is exact
    for b in range(1, n):
        assert not np.array_equal(cls[b], cls[0]) and not np.array_equal(out[b], out[0])
    want = {"one_head_missing"} | ({"half_on_column_1", "r_transposed"} if N > 1 else set())
    mut = R.row_mutants(cls, r)
    assert set(mut) == want
    for name, (mw, mo) in mut.items():
        assert (mo != out.astype(np.float64)).any(), (N, name)
    for name, (mw, mo) in R.row_mutants(cls, None).items():                  # r == NULL: the output is w
        assert (mo != w.astype(np.float64)).any(), (N, name)


@pytest.mark.parametrize("N,H", R.ROW_ORDINARY)
def test_row_ordinary_bounds_hold_for_an_f32_emulation_and_see_every_mutant(N, H):
    cls, r = R.row_ordinary(N, H)
    assert (cls >= 0).all() and (r >= 0).all() and np.abs(cls.astype(np.float64).sum(-1) - 1).max() <= 1e-5
    assert np.abs(r.astype(np.float64).sum(-1) - 1).max() <= 1e-5
    w64 = R.row_w64(cls)
    r64 = r.astype(np.float64)
    out64 = np.einsum("bj,bjk->bk", w64, r64)
    bw, bo = R.row_bounds(N, H, w64, out64)
    # f32 emulation of the kernel's definition: heads added in ascending order, times float(1 / H), halved, plus 0.5 [j == 0]; an fma chain
    s = np.zeros_like(cls[:, 0])
    for h in range(H):
        s = s + cls[:, h]
    w = np.float32(0.5) * (s * (np.float32(1.0) / np.float32(H)))
    w[:, 0] = w[:, 0] + np.float32(0.5)
    assert w.dtype == np.float32
    assert float((np.abs(w.astype(np.float64) - w64) / bw).max()) < 0.5
    acc = np.zeros((len(cls), N), np.float32)
    for j in range(N):
        acc = (acc.astype(np.float64) + w[:, j:j + 1].astype(np.float64) * r64[:, j, :]).astype(np.float32)      # fma: one rounding
    assert float((np.abs(acc.astype(np.float64) - out64) / bo).max()) < 0.5
    for name, (mw, mo) in R.row_mutants(cls, r).items():
        assert (np.abs(mo - out64) > bo).any(), (N, H, name)
    for name, (mw, mo) in R.row_mutants(cls, None).items():
        assert (np.abs(mw - w64) > bw).any(), (N, H, name)


def test_factor_of_mean_is_two_roundings_in_f32():
    rng = np.random.default_rng(5)
    m = rng.random((2, 17, 17)).astype(np.float32)
    f = R.factor_of_mean(m)
    m64 = m.astype(np.float64)
    want = ((0.5 * m64).astype(np.float32).astype(np.float64) + 0.5 * np.eye(17)).astype(np.float32)
    assert f.dtype == np.float32 and np.array_equal(f, want)
    # halving is exact, so the expression has ONE rounding: it is the correctly rounded 0.5 m + 0.5 [i == j], with or without contraction
    assert np.array_equal(f, (0.5 * m64 + 0.5 * np.eye(17)).astype(np.float32))
    assert (f != (0.5 * m64).astype(np.float32)).any() and np.array_equal(f[:, 0, 1], (0.5 * m64[:, 0, 1]).astype(np.float32))
    q = R.ordinary_qkv(2, 17, 64, 2)
    assert q.shape == (34, 192) and q.dtype == np.float32 and 1.5 < q.std() < 1.7
