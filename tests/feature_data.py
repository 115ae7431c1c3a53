"""Inputs, references and bounds shared by tests/test_cpu_features.py and tests/test_gpu_features.py (vitx_feat_*, vitx_op_features).

Everything is seeded; the references are float64.  The bounds are the ones the feature contract states (include/vitx.h) and come from the
number formats, not from a measured result:
  f32 LayerNorm value   exact_data.ln_bound with ulp_out = 2^-23 (the output is f32)
  pooled mean           |d_i| <= 2^-24 * ((N - 1) * mean_t |F[t][i]| + 2 |mean_i|): an f32 sum of N - 1 terms in ANY fixed order is off by at
                        most (N - 2) 2^-24 sum|F| to first order, the division by N - 1 brings that to 2^-24 sum|F| = 2^-24 (N - 1) mean|F| and
                        adds one rounding of the quotient; the second |mean_i| covers the higher-order terms
  L2                    norm within 4 * 2^-24 * sqrt(D) of 1, elements within 8 * 2^-24 of v / ||v|| in float64"""
import numpy as np

import exact_data as X

U24 = 2.0 ** -24
OP_TOKENS = (2, 17, 65, 197, 577, 785)


def mixed_images(D: int, n_img: int, N: int, seed: int = 0) -> np.ndarray:
    """[n_img][N][D] f32: the rows of exact_data.hostile_matrix(D) dealt round-robin over the row kinds, so that every image with N >= 10
    holds all ten kinds (outlier channels and tokens, offset 1000, constant, zero, tiny variance, tile step, 1e15, 1e-20) and pooling mixes them."""
    hm, _kind = X.hostile_matrix(D, rows_per_kind=64, seed=seed)
    per = hm.reshape(len(X.ROW_KINDS), 64, D)
    rows = n_img * N
    idx = np.arange(rows)
    return per[idx % len(X.ROW_KINDS), (idx // len(X.ROW_KINDS)) % 64].reshape(n_img, N, D).copy()


def random_images(D: int, n_img: int, N: int, seed: int = 0) -> np.ndarray:
    """[n_img][N][D] f32 activations of an ordinary residual stream: unit-scale rows with a per-row offset and scale."""
    rng = np.random.default_rng(seed * 7919 + D * 31 + N)
    x = rng.standard_normal((n_img, N, D)) * rng.uniform(0.3, 3.0, (n_img, N, 1)) + rng.standard_normal((n_img, N, 1))
    return x.astype(np.float32)


def features64(x: np.ndarray, w: np.ndarray, b: np.ndarray, eps: float = X.LN_EPS):
    """float64 F of [n_img][N][D] rows: (F [n_img][N][D], bound [n_img][N][D] = exact_data.ln_bound for an f32 output)."""
    n_img, N, D = x.shape
    y, rstd, xmax = X.layernorm64(x.reshape(n_img * N, D), w, b, eps)
    return y.reshape(n_img, N, D), X.ln_bound(y, w, rstd, xmax, 2.0 ** -23).reshape(n_img, N, D)


def mean_bound(tokens: np.ndarray):
    """(float64 mean over the token axis of [n][N-1][D], its bound [n][D])."""
    t = np.asarray(tokens, np.float64)
    m = t.mean(axis=1)
    return m, U24 * (t.shape[1] * np.abs(t).mean(axis=1) + 2.0 * np.abs(m))


def pooled_f32(tokens: np.ndarray, waves: int = 16) -> np.ndarray:
    """An f32 restatement of one fixed-order pooled mean: wave w sums rows w, w + waves, ... in ascending order, the partial sums are added
    in wave order, one division.  Every operation rounds to f32."""
    t = np.asarray(tokens, np.float32)
    n, T, D = t.shape
    total = np.zeros((n, D), np.float32)
    for w in range(waves):
        acc = np.zeros((n, D), np.float32)
        for r in range(w, T, waves):
            acc = acc + t[:, r]
        total = acc if w == 0 else total + acc
    return total / np.float32(T)
