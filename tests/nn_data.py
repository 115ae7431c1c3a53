"""Numpy restatement of the nearest-neighbour selection and vote (include/vitx.h "nearest neighbours in a gallery"), shared by
tests/test_cpu_nn.py -- which pins it to the host's vitx_topk and checks its invariance under any cut of the columns -- and tests/test_gpu_nn.py.

    key(s, g) = (rank(s), ~g): rank grows with the value, 0 for a NaN (below -inf's), +0 and -0 share one; the k LARGEST keys, best first.
    A score is returned as its rank names it: either zero as +0, any NaN as the quiet NaN 0x7fc00000, every other value bit for bit.
    vote: w_j = exp((s_j - s_0) / T), vote[c] = sum_{j: label[idx_j] = c} w_j / sum_j w_j."""
import numpy as np

QNAN = np.uint32(0x7fc00000)


def rank(s):
    """The 32-bit rank of every f32 value (topk_rank of csrc/topk_rank.h)."""
    s = np.ascontiguousarray(s, np.float32)
    with np.errstate(invalid="ignore"):
        b = (s + np.float32(0.0)).view(np.uint32)              # -0 + 0 = +0
    r = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(s), np.uint32(0), r).astype(np.uint32)


def rank_value(r):
    """The f32 value a rank stands for, as bits."""
    r = np.asarray(r, np.uint32)
    b = np.where(r & np.uint32(0x80000000), r ^ np.uint32(0x80000000), ~r).astype(np.uint32)
    return np.where(r == 0, QNAN, b).astype(np.uint32)


def keys(scores, base_index=0):
    """64-bit keys rank << 32 | ~index of the last axis; a larger key is an earlier entry."""
    s = np.ascontiguousarray(scores, np.float32)
    g = (np.arange(s.shape[-1], dtype=np.uint64) + np.uint64(base_index)).astype(np.uint32)
    return (rank(s).astype(np.uint64) << np.uint64(32)) | (~g).astype(np.uint64)


def select(scores, k, base_index=0):
    """scores [n][G] f32 -> (idx [n][k] i32, score bits [n][k] u32), best first: a stable sort on the (rank, ~index) key, descending."""
    s = np.atleast_2d(np.ascontiguousarray(scores, np.float32))
    ky = keys(s, base_index)
    order = np.argsort(~ky, axis=-1, kind="stable")[:, :k]          # ~key ascending = key descending; keys of one row are distinct
    top = np.take_along_axis(ky, order, axis=-1)
    idx = (~(top & np.uint64(0xffffffff)).astype(np.uint32)).astype(np.int64).astype(np.int32)
    return idx, rank_value((top >> np.uint64(32)).astype(np.uint32))


def select_cut(scores, k, chunks, segs):
    """The same selection the way the device meets the columns: `chunks` = column counts fed one after another, every chunk cut into `segs` segments
    (segment s of every chunk goes to list s); each list keeps its k best, the lists are merged at the end.  Returns what select() returns."""
    s = np.atleast_2d(np.ascontiguousarray(scores, np.float32))
    ky = keys(s)
    n = s.shape[0]
    lists = [[np.zeros(0, np.uint64) for _ in range(segs)] for _ in range(n)]
    c0 = 0
    for cols in chunks:
        seg = ((cols + segs - 1) // segs + 3) // 4 * 4
        for i in range(n):
            for sg in range(segs):
                a, b = min(c0 + sg * seg, c0 + cols), min(c0 + (sg + 1) * seg, c0 + cols)
                lists[i][sg] = np.sort(np.concatenate([lists[i][sg], ky[i, a:b]]))[::-1][:k]
        c0 += cols
    assert c0 == s.shape[1]
    top = np.stack([np.sort(np.concatenate(lists[i]))[::-1][:k] for i in range(n)])
    idx = (~(top & np.uint64(0xffffffff)).astype(np.uint32)).astype(np.int64).astype(np.int32)
    return idx, rank_value((top >> np.uint64(32)).astype(np.uint32))


def vote64(score, idx, labels, n_labels, T):
    """score [n][k] f32 (the engine's own), idx [n][k], labels [G] -> vote [n][n_labels] float64."""
    s = np.asarray(score, np.float64)
    w = np.exp((s - s[:, :1]) / np.float64(np.float32(T)))
    lab = np.asarray(labels)[np.asarray(idx)]
    v = np.zeros((s.shape[0], n_labels), np.float64)
    for i in range(s.shape[0]):
        np.add.at(v[i], lab[i], w[i])
    return v / w.sum(1, keepdims=True)


# ------------------------------------------------------------------------------------------------ score rows for the selection kernel
HOSTILE = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.0, -1.0, 3.4028235e38, -3.4028235e38], np.float32)


def score_rows(kind, n, cols, seed=0):
    """[n][cols] f32 rows of one data kind of the selection tests."""
    rng = np.random.default_rng(seed)
    if kind == "distinct":
        return np.stack([rng.permutation(cols) for _ in range(n)]).astype(np.float32) / np.float32(8) - np.float32(cols / 16)
    if kind == "equal":
        return np.full((n, cols), 0.375, np.float32)
    if kind == "ties3":
        return rng.choice(np.array([-1.0, 0.0, 2.5], np.float32), (n, cols))
    if kind == "hostile":
        s = rng.choice(HOSTILE, (n, cols))
        s[0] = np.nan                                   # a row of nothing but NaN
        if n > 1:
            s[1] = rng.choice(np.array([0.0, -0.0], np.float32), cols)
        return s.astype(np.float32)
    if kind == "ascending":
        return np.tile(np.arange(cols, dtype=np.float32) * np.float32(0.5) - 7, (n, 1))
    if kind == "descending":
        return np.tile(-np.arange(cols, dtype=np.float32) * np.float32(0.5) + 7, (n, 1))
    raise ValueError(kind)


KINDS = ("distinct", "equal", "ties3", "hostile", "ascending", "descending")


# ------------------------------------------------------------------------------------------------ exact data for the op
def exact_case(n, G, seed):
    """The recipe of test_gpu_zeroshot.py's _exact_case: z = +-2^e (e per row), so ss = 64 4^e, nrm = 2^(e + 3), a = +-1/8; gallery entries j/8,
    |j| <= 8.  Every product is a multiple of 2^-6 and sum |a t| <= 8: any partial sum in any order is exact in f32.  Returns (z, t, a); the caller
    asserts the conditions (exact_conditions)."""
    rng = np.random.default_rng(seed)
    E = 64
    e = rng.integers(-12, 13, (n, 1))
    z = (rng.choice([-1.0, 1.0], (n, E)) * 2.0 ** e).astype(np.float32)
    t = (rng.integers(-8, 9, (G, E)) / 8.0).astype(np.float32)
    return z, t, (np.sign(z) / 8).astype(np.float32)


def exact_conditions(a, t):
    """(every product is an integer / 64, the largest sum of |products| * 64): the first must hold and the second stay below 2^24."""
    prod = np.abs(a[:, None, :].astype(np.float64) * t[None].astype(np.float64))
    return bool((prod * 64 == np.rint(prod * 64)).all()), float(prod.sum(-1).max() * 64)
