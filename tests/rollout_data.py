"""Data generators, mutants and bounds of the single-kernel rollout tests (test_gpu_rollout.py): vitx_op_rollout_factor, vitx_op_rollout_step,
vitx_op_rollout_row (include/vitx.h; attention_map.hip).

Nothing here touches a GPU or libvitx.so: tests/test_cpu_rollout_data.py checks every condition the GPU tests rely on.

"Exact" data makes the one correct result unique: entries are small integers over a power of two, so every product and every partial sum in
ANY order is a multiple of one small unit far below 2^24 units, f32 arithmetic never rounds, and the expected buffer is the float64 product
cast to f32 without loss.  A test on it compares whole buffers bit for bit.
"Ordinary" data is what rollout multiplies: non-negative row-stochastic factors 0.5 softmax + 0.5 I with peaked rows.  Its bounds are the
classical componentwise ones for an f32 inner product in any order; no figure comes from the kernels.

The mutants restate the definition with one fault each -- the faults a tiled in-place product can have.  On every case where a mutant is
defined it changes at least one element of the exact expected buffer (and breaks the bound on the ordinary data): a kernel with that fault
cannot pass.
"""
from __future__ import annotations

import numpy as np

MAX_TOKENS = 1024                         # kAttnMeanMaxTokens (kernels.h)
# Both sides of every edge of the step kernel's builds (NT = 1, 2, 4, 8, 16: up to 64, 128, 256, 512, 1024 tokens), every N % 4, N % 16 in
# {15, 0, 1, 2, 3}, both ends of the supported range
STEP_N = (1, 3, 4, 15, 16, 17, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 258, 259, 511, 512, 513, 1023, 1024)
STEP_ORDINARY_N = (65, 122, 197, 226, 256, 577, 1024)
ROW_EXACT_N = (1, 4, 17, 255, 256, 257, 258, 1024)
ROW_EXACT_H = (1, 2, 4, 8)                # powers of two: s * (1 / H) is exact
ROW_ORDINARY = ((17, 12), (197, 3), (257, 12), (258, 3), (1024, 12))      # (N, H): H in {3, 12}; N >= H + 2 (row_bounds)
FACTOR_N = (1, 15, 16, 17, 63, 64, 65, 129, 257, 577, 1024)
FACTOR_HD = (64, 32, 80, 128)
FACTOR_MODES = ("bf16", "f16", "f16_planes")
A_DEN, A_MAX, R_MAX = 64, 8, 8            # step: a = p / 64 with integer |p| <= 8, r integer with |r| <= 8
CLS_DEN, CLS_MAX = 64, 8                  # row: cls = p / 64 with integer |p| <= 8
U = 2.0 ** -24                            # unit round-off of f32


def step_build(N: int) -> int:
    """NT of the step kernel's build that takes N tokens (launch_rollout_step)."""
    nt = (N + 63) // 64
    return next(b for b in (1, 2, 4, 8, 16) if nt <= b)


def n_images(N: int) -> int:
    return 3 if N <= 259 else 2


def _nonzero(rng, lim: int, shape):
    return rng.integers(1, lim + 1, shape) * rng.choice([-1, 1], shape)


# ------------------------------------------------------------------------------------------------------------------
# the step: a <- a . r
# ------------------------------------------------------------------------------------------------------------------
def step_exact(N: int, seed: int = 0):
    """(a, r, expected) f32 [n_images(N)][N][N]: a = p / 64, r integer, both non-zero everywhere, drawn per image; expected = a . r exactly."""
    n = n_images(N)
    rng = np.random.default_rng(7919 * N + seed)
    a = _nonzero(rng, A_MAX, (n, N, N)).astype(np.float64) / A_DEN
    r = _nonzero(rng, R_MAX, (n, N, N)).astype(np.float64)
    for b in range(n):                        # N = 1 leaves one entry per image: the images differ, r is not 1, the products differ
        a[b, 0, 0] = (b + 2.0) / A_DEN; r[b, 0, 0] = 2.0 * b + 3.0
    # every product is a multiple of 1 / 64; any partial sum of any subset stays below N * max|a| * max|r|: in units of 1 / 64 below 2^24
    assert N * np.abs(a).max() * np.abs(r).max() * A_DEN < 2 ** 24
    exp64 = a @ r
    exp = exp64.astype(np.float32)
    assert np.array_equal(exp.astype(np.float64), exp64)
    a32, r32 = a.astype(np.float32), r.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a) and np.array_equal(r32.astype(np.float64), r)
    return a32, r32, exp


def _flat_next(x: np.ndarray, extra: int) -> np.ndarray:
    """x [n][N][N] as one flat buffer followed by `extra` zeros (what lies behind the last image in the mutants that read on)."""
    return np.concatenate([x.reshape(-1), np.zeros(extra, x.dtype)])


def step_mutants(a: np.ndarray, r: np.ndarray) -> dict:
    """{name: what a step kernel with that fault leaves in the a buffer} for float64 a, r [n][N][N]; only the mutants defined at this N.
    `unwritten` cells keep a (the step is in place)."""
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    n, N, _ = a.shape
    good = a @ r
    out = {}
    k4, i16, j64 = N // 4 * 4, N // 16 * 16, (N - 1) // 64 * 64
    if N % 4:
        out["k_tail_dropped"] = a[:, :, :k4] @ r[:, :k4, :]
        # no zero padding: k in N .. kend - 1 goes on reading: a[i][k] is the next row's a[i + 1][k - N], r[k] the next image's row k - N
        kend = (N + 3) // 4 * 4
        af, rf = _flat_next(a, kend), _flat_next(r, kend * N)
        m = good.copy()
        for b in range(n):
            for k in range(N, kend):
                col = af[b * N * N + np.arange(N) * N + k]
                row = rf[b * N * N + k * N:b * N * N + k * N + N]
                m[b] += np.outer(col, row)
        out["no_zero_padding"] = m
    if N % 16:
        m = good.copy(); m[:, i16:, :] = a[:, i16:, :]
        out["last_row_block_unwritten"] = m
        m = good.copy(); m[:, :, i16:] = a[:, :, i16:]
        out["last_16_columns_unwritten"] = m
    m = good.copy(); m[:, :, j64:] = a[:, :, j64:]
    out["last_64_column_group_unwritten"] = m
    if N > 1:
        out["r_transposed"] = a @ r.transpose(0, 2, 1)
        out["r_times_a"] = r @ a
    out["image_0_r"] = a @ r[:1]
    if N > 64:
        # the in-place hazard: the first 64-column group is stored before the later groups read their rows of a
        stale = a.copy(); stale[:, :, :64] = good[:, :, :64]
        m = good.copy(); m[:, :, 64:] = (stale @ r)[:, :, 64:]
        out["in_place_hazard"] = m
    return out


def factor_matrices(n: int, N: int, seed: int, spread: float = 2.56) -> np.ndarray:
    """[n][N][N] f32: 0.5 softmax(randn * spread) + 0.5 I -- non-negative, rows sum to 1, peaked rows (the spread of
    test_op_attention_map_against_float64's scores: q, k of randn * 1.6)."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((n, N, N)) * spread
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return (0.5 * e / e.sum(axis=-1, keepdims=True) + 0.5 * np.eye(N)).astype(np.float32)


def step_ordinary(N: int, steps: int = 1):
    """(factors [steps][n][N][N], r0 [n][N][N]) f32: the chain is R_l = factors[l - 1] . R_(l - 1), R_0 = r0 (itself a factor: layer 0's)."""
    n = n_images(N)
    f = np.stack([factor_matrices(n, N, 100 * N + l + 1) for l in range(steps)])
    return f, factor_matrices(n, N, 100 * N)


def step_bound(N: int, absprod):
    """|got - ref64| <= N * 2^-23 * (|a| . |r|)_ij.  An f32 inner product of N terms in any order -- N rounded products, N - 1 rounded
    additions -- lies within gamma_N = N u / (1 - N u) of the exact one relative to sum |a_ik| |r_kj| (Higham, Accuracy and Stability of
    Numerical Algorithms, section 3.1), u = 2^-24.  The factor two covers 1 / (1 - N u) and an MFMA whose internal sums are only faithfully
    rounded (an error of up to one ulp, 2 u, per operation instead of u)."""
    return N * 2.0 ** -23 * absprod


def matmul_f32_sequential(a: np.ndarray, r: np.ndarray) -> np.ndarray:
    """f32 emulation of the definition: every product rounded to f32, added in ascending k, every sum rounded to f32."""
    a, r = np.asarray(a, np.float32), np.asarray(r, np.float32)
    c = np.zeros(a.shape[:-1] + r.shape[-1:], np.float32)
    for k in range(a.shape[-1]):
        c = c + a[..., :, k:k + 1] * r[..., k:k + 1, :]
    assert c.dtype == np.float32
    return c


# ------------------------------------------------------------------------------------------------------------------
# the last factor: out = w . r, w_j = 0.5 mean_h cls[h][j] + 0.5 [j == 0]
# ------------------------------------------------------------------------------------------------------------------
def row_exact_h(N: int) -> int:
    return ROW_EXACT_H[ROW_EXACT_N.index(N) % len(ROW_EXACT_H)]


def row_w64(cls: np.ndarray, half_col: int = 0, heads: int | None = None) -> np.ndarray:
    """float64 w [n][N] of cls [n][H][N]; the mutants: the identity's half on column `half_col`, only the first `heads` heads summed."""
    cls = np.asarray(cls, np.float64)
    H = cls.shape[1]
    w = 0.5 * (cls[:, :H if heads is None else heads].sum(axis=1) / H)
    if half_col < w.shape[1]:
        w[:, half_col] += 0.5
    return w


def row_exact(N: int, seed: int = 0):
    """(cls [n][H][N], r [n][N][N], w [n][N], out [n][N]) f32: cls = p / 64 and r integers, non-zero; w and out = w . r are exact."""
    n, H = n_images(N), row_exact_h(N)
    rng = np.random.default_rng(104729 * N + H + seed)
    cls = _nonzero(rng, CLS_MAX, (n, H, N)).astype(np.float64) / CLS_DEN
    r = _nonzero(rng, R_MAX, (n, N, N)).astype(np.float64)
    # the head sum: multiples of 1 / 64 up to H * 8 / 64; times 1 / H (a power of two), times 0.5, plus 0.5: w is a multiple of 2^-10
    unit = 1.0 / (CLS_DEN * 2 * max(ROW_EXACT_H))
    w = row_w64(cls)
    assert H in ROW_EXACT_H and np.array_equal(np.round(w / unit) * unit, w)
    # the fma chain s = fma(w_j, r_jk, s): every term and every partial sum a multiple of `unit`, below N * max|w| * max|r|
    assert N * np.abs(w).max() * np.abs(r).max() / unit < 2 ** 24
    out = np.einsum("bj,bjk->bk", w, r)
    cast = lambda x: x.astype(np.float32)
    for x in (cls, r, w, out):
        assert np.array_equal(cast(x).astype(np.float64), x)
    return cast(cls), cast(r), cast(w), cast(out)


def row_ordinary(N: int, H: int):
    """(cls [n][H][N], r [n][N][N]) f32: softmax rows with the factors' spread, r a product of two factors (rows sum to 1)."""
    n = n_images(N)
    rng = np.random.default_rng(31 * N + H)
    s = rng.standard_normal((n, H, N)) * 2.56
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    cls = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    f = factor_matrices(2 * n, N, 31 * N + H + 1).astype(np.float64)
    return cls, (f[:n] @ f[n:]).astype(np.float32)


def row_mutants(cls: np.ndarray, r: np.ndarray | None) -> dict:
    """{name: (w, out)} float64 of a row kernel with one fault; r None: out is w."""
    n, H, N = cls.shape
    r64 = None if r is None else np.asarray(r, np.float64)
    prod = lambda w, rr: w if rr is None else np.einsum("bj,bjk->bk", w, rr)
    out = {"one_head_missing": (row_w64(cls, heads=H - 1), r64)}
    if N > 1:
        out["half_on_column_1"] = (row_w64(cls, half_col=1), r64)
        if r64 is not None:
            out["r_transposed"] = (row_w64(cls), r64.transpose(0, 2, 1))
    return {k: (w, prod(w, rr)) for k, (w, rr) in out.items()}


def row_bounds(N: int, H: int, w64, w_absr64):
    """(bound on w, bound on out), non-negative cls:
      w:   H - 1 rounded additions, the product with float(1 / H) (itself rounded), the exact halving and the addition of 0.5 [j == 0]: at
           most H + 2 roundings of relative size u on a sum of non-negative terms -- |w - w64| <= (H + 2) * 2^-24 * w64_j to first order;
      out: an fma chain of N terms (one rounding each) on the rounded w: gamma_N + gamma_(H + 2) <= N * 2^-23 relative to (w . |r|)_k
           as long as H + 2 <= N, which ROW_ORDINARY keeps."""
    assert H + 2 <= N
    return (H + 2) * U * w64, N * 2.0 ** -23 * w_absr64


# ------------------------------------------------------------------------------------------------------------------
# the factor: 0.5 mean_h A_h + 0.5 I
# ------------------------------------------------------------------------------------------------------------------
def ordinary_qkv(n_img: int, N: int, D: int, H: int) -> np.ndarray:
    """[n_img * N][3 D] f32, drawn as test_gpu_attn_map.py::test_op_attention_map_against_float64 draws it (randn * 1.6: peaked rows)."""
    rng = np.random.default_rng(n_img * 7 + N * 13 + D + H)
    return (rng.standard_normal((n_img * N, 3 * D)) * 1.6).astype(np.float32)


def factor_of_mean(mean: np.ndarray) -> np.ndarray:
    """The factor the kernel defines, in numpy float32 from the head mean [n][N][N] f32: float32(0.5) * mean + float32(0.5) * [i == j], one
    rounded product and one rounded sum per entry, no contraction."""
    mean = np.asarray(mean)
    assert mean.dtype == np.float32
    half = np.float32(0.5)
    out = half * mean + half * np.eye(mean.shape[-1], dtype=np.float32)
    assert out.dtype == np.float32
    return out
