"""MXFP8 operands that leave ONE correct result, for the block-scaled GEMM of gemm_mx8.hip, its GELU -> MX epilogue and fc1 -> fc2 on the device
(tests/test_gpu_mx_exact.py; what that file leans on is checked without a GPU by tests/test_cpu_mx_data.py).  Independent of libvitx.so: the
reference encoder / decoder (vit.cpp_amd/mxfp8.py) and numpy only.

Elements are e4m3 codes of small integers (A from -4 .. 4, W from -2 .. 6: not mirror images), every 32-element block has its own E8M0 scale byte
    s[row][b] = 127 - spread + 3 level[row] + (b + row) % 3          (bytes 127 - spread .. 127 + spread)
so neighbouring K blocks of a row differ (the last term), neighbouring rows differ (their levels differ by a multiple of 3, their last terms
by 1 or 2) and a row's scales span a factor of 4 only, whatever `spread` is: the row's level cancels out of the exactness condition.  A's level
is drawn per row; W's level is one per 32-row group (its magnitude class; neighbouring groups differ), so output blocks of 32 columns get
different scales.  Columns K .. K_pad are zero elements with scale 127, rows N .. N_pad of W zero blocks with scale 127 (kernels.h).

Exactness (exactness()): with g[r][c] = 2^(min_b sa[r][b] + min_b sw[c][b] - 254), floored by the granule (lowest set bit) of bias[c] and of
resid[r][c], every term a w, the bias and the residual are multiples of g, and (sum_k |a w| + |bias| + |resid|) / g < 2^24: every partial sum, in
any order and grouping, is a multiple of g below 2^24 g, hence exact in f32, and the float64 product (gemm64) is the one correct result.

GELU (gelu_operands): the bias makes every v = acc + bias either >= 8 or <= -16.  gelu_tanh2 (device_common.h) is x * rcp(1 + exp2(x p)): for
x >= 8 the argument is <= -71, 1 + exp2(.) is 1 in f32 and the result is x; for x <= -16 it is >= 458, exp2 gives +inf, rcp 0, the result -0.0.
The expected bytes are the reference encoding of where(v >= 8, v, -0.0) (gelu_expected).

MUTANTS: faulty restatements, plain numpy.  The first six change the product (they return the float64 result), the last three the encoded GELU
output (they return elements, scales).  `applies` says which cases a mutant can change at all, and why not the others."""
import functools

import numpy as np

import _pkg

_pkg.load()
from vitcpp_amd import mxfp8  # noqa: E402

M_EDGES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
N_EDGES = (1, 3, 4, 31, 32, 33, 63, 65, 127, 128, 129, 200, 257)
K_EDGES = (32, 64, 128, 160, 192, 256, 384, 640)
SPREAD, SPREAD_WIDE = 4, 30
WIDE_CASE = (129, 200, 384, SPREAD_WIDE)


def _cases():
    out = [(M, N, K, SPREAD) for M in M_EDGES for N in (129, 200) for K in (128, 384)]
    out += [(M, N, 192, SPREAD) for M in (17, 129) for N in N_EDGES]
    out += [(65, 129, K, SPREAD) for K in K_EDGES]
    seen, uniq = set(), []
    for c in out + [WIDE_CASE]:
        if c not in seen:
            seen.add(c); uniq.append(c)
    return uniq


CASES = _cases()
GELU_CASES = [c for c in CASES if c[3] == SPREAD]              # every non-wide case


def case_id(c):
    return "M%d_N%d_K%d_s%d" % c


def case_seed(c):
    return c[0] * 7 + c[1] * 3 + c[2] + c[3]


def pad128(x):
    return (x + 127) // 128 * 128


# ------------------------------------------------------------------------------------------------ elements and scales
_E4M3 = mxfp8.e4m3_to_f32(np.arange(256, dtype=np.uint8))
_INT_CODE = np.zeros(33, np.uint8)                               # integers -16 .. 16 are all e4m3 values
for _v in range(-16, 17):
    _INT_CODE[_v + 16] = 0 if _v == 0 else int(np.flatnonzero(_E4M3 == float(_v))[0])


def int_codes(vals):
    """e4m3 codes of integers in -16 .. 16 (exact)."""
    vals = np.asarray(vals, np.int64)
    assert np.abs(vals).max(initial=0) <= 16
    return _INT_CODE[vals + 16]


def _levels(spread):
    return (2 * spread + 1) // 3                                 # levels 0 .. n - 1: bytes 127 - spread + 3 level + (0 .. 2) <= 127 + spread


def _scale_bytes(level, nb, nb_real, spread):
    rows = level.shape[0]
    s = 127 - spread + 3 * level[:, None] + (np.arange(nb)[None, :] + np.arange(rows)[:, None]) % 3
    s[:, nb_real:] = 127
    assert s.min() >= 127 - spread and s.max() <= 127 + spread
    return s.astype(np.uint8)


def _operand_pair(M, N, K, spread, rng):
    kp, npad = pad128(K), pad128(N)
    nb, nbr = kp // 32, (K + 31) // 32
    qa = np.zeros((M, kp), np.uint8); qa[:, :K] = int_codes(rng.integers(-4, 5, (M, K)))
    qw = np.zeros((npad, kp), np.uint8); qw[:N, :K] = int_codes(rng.integers(-2, 7, (N, K)))
    nl = _levels(spread)
    sa = _scale_bytes(rng.integers(0, nl, M), nb, nbr, spread)
    groups = npad // 32
    cls = np.zeros(groups, np.int64); cls[0] = rng.integers(0, nl)
    for j in range(1, groups):
        cls[j] = (cls[j - 1] + rng.integers(1, nl)) % nl         # neighbouring 32-row groups: different magnitude classes
    sw = _scale_bytes(np.repeat(cls, 32), nb, nbr, spread)
    sw[N:] = 127
    # the three properties of the scale bytes
    assert nbr < 2 or ((sa[:, 1:nbr] != sa[:, :nbr - 1]).all() and (sw[:N, 1:nbr] != sw[:N, :nbr - 1]).all())
    assert (sa[1:, :nbr] != sa[:-1, :nbr]).all() and (sw[1:N, :nbr] != sw[:N - 1, :nbr]).all()
    assert (cls[1:] != cls[:-1]).all()
    return qa, sa, qw, sw


def _row_exp(s, K):
    """min over the real blocks of a row's scale exponents."""
    return s[:, :(K + 31) // 32].astype(np.int64).min(axis=1) - 127


def operands(M, N, K, spread, seed):
    """qa [M][K_pad], sa [M][K_pad/32], qw [N_pad][K_pad], sw [N_pad][K_pad/32] uint8; bias [N], resid [M][N] f32.  The bias is an integer in
    -8 .. 8 times 2^(W row exponent + A's largest row exponent) (zero in the wide-range case: a single bias cannot be a small multiple of the
    granule of rows 2^58 apart), the residual an integer in -16 .. 16 times the element's own product granule."""
    rng = np.random.default_rng(seed)
    qa, sa, qw, sw = _operand_pair(M, N, K, spread, rng)
    ea, ew = _row_exp(sa, K), _row_exp(sw[:N], K)
    if spread <= 8:
        bias = rng.integers(-8, 9, N) * np.exp2(ew + ea.max())
    else:
        bias = np.zeros(N)
    resid = rng.integers(-16, 17, (M, N)) * np.exp2(ea[:, None] + ew[None, :])
    bias, resid = bias.astype(np.float32), resid.astype(np.float32)
    assert exactness(qa, sa, qw, sw, bias, resid, N, K) < 2.0 ** 24
    return qa, sa, qw, sw, bias, resid


def granule(x):
    """The largest power of two that divides x (float64; +inf for 0)."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    mant = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = mant & -mant
    with np.errstate(divide="ignore"):
        return np.where(x == 0, np.inf, np.exp2(e - 53.0) * low.astype(np.float64))


def exactness(qa, sa, qw, sw, bias, resid, N, K, a_granule=None):
    """max over (r, c) of (sum_k |a w| + |bias| + |resid|) / g -- the condition is that it stays below 2^24.  g = A's row granule times W's row
    granule (integer elements: 2^(the row's smallest scale exponent); a_granule overrides A's for operands that are not integers), floored by
    the granules of the bias and the residual."""
    M = qa.shape[0]
    a, w = np.abs(mxfp8.decode(qa, sa, K)), np.abs(mxfp8.decode(qw[:N], sw[:N], K))
    ga = np.exp2(_row_exp(sa, K).astype(np.float64)) if a_granule is None else a_granule
    g = ga[:, None] * np.exp2(_row_exp(sw[:N], K).astype(np.float64))[None, :]
    total = a @ w.T
    if bias is not None:
        b = np.broadcast_to(np.asarray(bias, np.float64)[None, :], (M, N))
        g = np.minimum(g, granule(b)); total = total + np.abs(b)
    if resid is not None:
        g = np.minimum(g, granule(resid)); total = total + np.abs(np.asarray(resid, np.float64))
    return float((total / g).max())


def gemm64(qa, sa, qw, sw, bias, N, K, resid=None):
    """The float64 restatement from decoded operands: A . W^T + bias (+ resid)."""
    v = mxfp8.decode(qa, sa, K) @ mxfp8.decode(qw[:N], sw[:N], K).T
    if bias is not None:
        v = v + np.asarray(bias, np.float64)[None, :]
    if resid is not None:
        v = v + np.asarray(resid, np.float64)
    return v


def bf16_bits(x64):
    """float64 (exact in f32) -> bf16 bit patterns, rounded once to nearest even."""
    x32 = np.asarray(x64).astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x64)
    u = np.ascontiguousarray(x32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ GELU
def _pow2ceil(x):
    x = np.asarray(x, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(x > 0, np.exp2(np.ceil(np.log2(np.maximum(x, 1e-300)))), 0.0)


def dead_columns(N):
    """bool [N]: scattered single columns (c % 11 == 5) and, from N = 33, every real column of block 1 (columns 32 .. 63)."""
    c = np.arange(N)
    return (c % 11 == 5) | ((c >= 32) & (c < 64))


def gelu_operands(M, N, K, spread, seed):
    """operands() with a bias that puts every v = acc + bias at >= 8 (pass-through) or <= -16 (dead): qa, sa, qw, sw, bias, dead [N].
    Pass-through column: bias = 2^ceil(log2(max_r |acc| + 8)); dead column: -(2^ceil(log2 max_r acc) + 16), from the column's OWN maximum (a
    global constant is not a small multiple of the small columns' granule).  Two columns are then set so that one block's maximum is exactly
    1.75 * 2^k and another's exactly a power of two (_boundaries).  The generator draws again (at most GELU_DRAWS times, deterministically)
    until the conditions of gelu_conditions hold: the draw is part of the data, the conditions are asserted on what comes out."""
    for draw in range(GELU_DRAWS):
        rng = np.random.default_rng([seed, draw, 1])
        qa, sa, qw, sw = _operand_pair(M, N, K, spread, rng)
        acc = gemm64(qa, sa, qw, sw, None, N, K)
        amax, pmax = np.abs(acc).max(axis=0), acc.max(axis=0)
        dead = dead_columns(N)
        bias = np.where(dead, -(_pow2ceil(np.maximum(pmax, 0.0)) + 16.0), _pow2ceil(amax + 8.0))
        if not _boundaries(acc, bias, dead, M, N):
            continue
        bias = bias.astype(np.float32)
        v = acc + bias
        if gelu_conditions_hold(v, M, N) and exactness(qa, sa, qw, sw, bias, None, N, K) < 2.0 ** 24:
            assert ((v <= -16) == dead[None, :]).all()
            return qa, sa, qw, sw, bias, dead
    raise AssertionError(f"no draw of M {M} N {N} K {K} meets the GELU conditions")


GELU_DRAWS = 16


def boundary_plan(M, N):
    """How a case gets its two boundary blocks: 'two_blocks' (N > 64: blocks 0 and 2, any M), 'two_rows' (one live block, two rows of it, 2 <= N
    <= 64 and M >= 2), or None: N = 1 has one bias for one column, and two rows' maxima cannot both be set."""
    if N > 64:
        return "two_blocks"
    return "two_rows" if N >= 2 and M >= 2 else None


def _boundaries(acc, bias, dead, M, N):
    plan = boundary_plan(M, N)
    live = np.flatnonzero(~dead)
    hi = np.abs(acc).max(axis=0) + np.abs(bias)                  # no v of the column exceeds it
    if plan is None:
        return True
    if plan == "two_blocks":
        # column c0 of the block, r = the row where it is smallest: v[r][c0] = t, the next f * 2^k at or above every other v of row r in the
        # block, is that row's maximum, and every other v of the column lies above it (so all are >= 8)
        for blk, f in ((0, 1.75), (2, 1.0)):
            cols = live[(live >= 32 * blk) & (live < 32 * blk + 32)]
            c0, rest = cols[0], cols[1:]
            r = int(acc[:, c0].argmin())
            t = f * _pow2ceil(max(float((acc[r, rest] + bias[rest]).max(initial=8.0)), 8.0) / f)
            bias[c0] = t - acc[r, c0]
        return True
    if plan == "two_rows":
        # columns c0, c1 of block 0: v[r1][c0] = 1.75 * 2^k is row r1's maximum, v[r2][c1] = 2^(k + 1) row r2's.  r2 / r1 = where column c1 is
        # largest / smallest, k from its range R (2^(k-2) <= R), so that v[r1][c1] = 2^(k+1) - R <= 1.75 * 2^k; c0 = a column whose step from
        # r1 to r2 is at most 2^(k-2), so that v[r2][c0] <= 2^(k+1)
        cols = live[live < 32]
        done = False
        for c1 in cols[np.argsort(-np.ptp(acc[:, cols], axis=0), kind="stable")]:      # the widest column first
            r2, r1 = int(acc[:, c1].argmax()), int(acc[:, c1].argmin())
            R = acc[r2, c1] - acc[r1, c1]
            if R <= 0:
                continue
            k = int(np.floor(np.log2(R))) + 2
            if 2.0 ** (k + 1) - R < 8 or 1.75 * 2.0 ** k < hi[cols[cols != c1]].max(initial=0):     # every v >= 8; no other column above the two maxima
                continue
            for c0 in cols:
                if c0 != c1 and acc[r2, c0] - acc[r1, c0] <= 2.0 ** (k - 2) and 1.75 * 2.0 ** k - acc[r1, c0] + acc[:, c0].min() >= 8:
                    bias[c0] = 1.75 * 2.0 ** k - acc[r1, c0]
                    bias[c1] = 2.0 ** (k + 1) - acc[r2, c1]
                    done = True
                    break
            if done:
                break
        return done


def gelu_values(v):
    """What gelu_tanh2 returns for v >= 8 (v itself) and v <= -16 (-0.0), f32."""
    assert ((v >= 8) | (v <= -16)).all()
    v32 = np.asarray(v).astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)
    return np.where(v >= 8, v32, np.float32(-0.0)).astype(np.float32)


def gelu_expected(v, N):
    """(elements [M][N_pad], scales [M][N_pad / 32]) the epilogue must write: columns N .. N_pad zero, whole pad blocks 127, the block that
    contains N scaled by its real columns only; an all-dead block is 32 bytes 0x80 (its pad columns 0) with scale 127."""
    return mxfp8.encode(gelu_values(v), pad128(N))


def block_maxima(y, N):
    """[M][N_pad / 32] maxima of |y| over the real columns of every block."""
    yp = np.zeros((y.shape[0], pad128(N))); yp[:, :N] = np.abs(y)
    return yp.reshape(y.shape[0], -1, 32).max(axis=2)


def gelu_conditions(v, N):
    """dict(b175, bpow2: number of blocks whose maximum is exactly 1.75 * 2^k / a power of two; neighbours: fraction of horizontally neighbouring
    real blocks with different scale bytes (None without a pair); distinct: number of different scale bytes)."""
    y = gelu_values(v)
    am = block_maxima(y, N)
    _, s = gelu_expected(v, N)
    real = (N + 31) // 32
    with np.errstate(divide="ignore"):
        m = np.where(am > 0, am / np.exp2(np.floor(np.log2(np.maximum(am, 1e-300)))), 0.0)
    sr = s[:, :real]
    return dict(b175=int((m == 1.75).sum()), bpow2=int((m == 1.0).sum()),
                neighbours=float((sr[:, 1:] != sr[:, :-1]).mean()) if real > 1 else None, distinct=int(np.unique(sr).size))


def gelu_conditions_hold(v, M, N):
    """Every v >= 8 or <= -16 and exact in f32; a block maximum of 1.75 * 2^k and one that is a power of two (where boundary_plan has a way);
    more than 0.9 of the neighbouring real blocks with different scales."""
    if not ((v >= 8) | (v <= -16)).all() or not np.array_equal(v.astype(np.float32).astype(np.float64), v):
        return False
    c = gelu_conditions(v, N)
    if boundary_plan(M, N) is not None and (c["b175"] < 1 or c["bpow2"] < 1):
        return False
    return c["neighbours"] is None or c["neighbours"] > 0.9


FC2_N = 100                                                      # columns of the second GEMM: a ragged tile, three whole blocks and a partial one
# The GELU cases whose second product meets the exactness condition as well (fc2_operands): those with N <= 63, the second GEMM's K.  fc1's outputs
# are e4m3 values, not integers: the granule of a row is 2^-9 (the smallest e4m3 step) times its smallest block scale, and a row whose blocks
# differ by 2^6 and more leaves no room below 2^24.  tests/test_cpu_mx_data.py asserts that these, and no other case, meet the condition.
FC2_CASES = [(M, N, 192, SPREAD) for M in (17, 129) for N in (1, 3, 4, 31, 32, 33, 63)]


def e4m3_row_granule(q, s):
    """[rows] the granule every element of an MX row is a multiple of, from the format alone: 2^-9, the smallest step of e4m3fn (its subnormals),
    times the smallest scale among the row's blocks that hold a non-zero element (1 for a row of zeros)."""
    nz = (q.reshape(q.shape[0], -1, 32) & 0x7f).any(axis=2)
    e = np.where(nz, s.astype(np.int64) - 127 - 9, 10 ** 6).min(axis=1)
    return np.where(e < 10 ** 5, np.exp2(np.minimum(e, 1000).astype(np.float64)), 1.0)


def fc2_operands(q1, s1, N, seed):
    """fc1's expected output (q1, s1: [M][N_pad], the second GEMM's A with K = N) -> qw2, sw2, bias2, resid2, figure.  W2 is operands()' W; the
    bias and the residual are integers times granules of THIS product (A's row granule: e4m3_row_granule).  figure = exactness() of the
    product with that granule: the case is usable where it is below 2^24."""
    M = q1.shape[0]
    rng = np.random.default_rng(seed)
    _, _, qw2, sw2 = _operand_pair(1, FC2_N, N, SPREAD, rng)
    ga = e4m3_row_granule(q1, s1)
    gw = np.exp2(_row_exp(sw2[:FC2_N], N).astype(np.float64))
    bias2 = (rng.integers(-8, 9, FC2_N) * gw * ga.max()).astype(np.float32)
    resid2 = (rng.integers(-16, 17, (M, FC2_N)) * ga[:, None] * gw[None, :]).astype(np.float32)
    return qw2, sw2, bias2, resid2, exactness(q1, s1, qw2, sw2, bias2, resid2, FC2_N, N, a_granule=ga)


# ------------------------------------------------------------------------------------------------ mutants
def _mut_k_halves(qa, sa, qw, sw, bias, N, K):
    """A lane's bytes 16 .. 31 taken from k = 32 + 16 g instead of 64 + 16 g: the MFMA multiplies A's elements 32 .. 95 of every 128-step at
    the positions 64 .. 127 (with those positions' scales and W elements)."""
    q = qa.copy().reshape(qa.shape[0], -1, 128)
    q[:, :, 64:128] = qa.reshape(qa.shape[0], -1, 128)[:, :, 32:96]
    return gemm64(q.reshape(qa.shape), sa, qw, sw, bias, N, pad128(K))


def _mut_a_scale_block(qa, sa, qw, sw, bias, N, K):
    """A's scale of block b of a step replaced by block (b + 1) mod 4 (a shift of the scale dword by 8 (g + 1))."""
    s = sa.reshape(sa.shape[0], -1, 4)[:, :, [1, 2, 3, 0]].reshape(sa.shape)
    return gemm64(qa, s, qw, sw, bias, N, pad128(K))


def _mut_w_scale_row(qa, sa, qw, sw, bias, N, K):
    """W's scale of row n taken from row n xor 16."""
    return gemm64(qa, sa, qw, sw[np.arange(sw.shape[0]) ^ 16], bias, N, pad128(K))


def _mut_stale_scales(qa, sa, qw, sw, bias, N, K):
    """Step kt uses the scale dwords of step kt - 2 (a stage's scales not refreshed), from the third step on."""
    def stale(s):
        t = s.copy(); t[:, 8:] = s[:, :-8]
        return t
    return gemm64(qa, stale(sa), qw, stale(sw), bias, N, pad128(K))


def _mut_drop_last_step(qa, sa, qw, sw, bias, N, K):
    q = qa.copy(); q[:, -128:] = 0
    return gemm64(q, sa, qw, sw, bias, N, pad128(K))


def _mut_row_clamp(qa, sa, qw, sw, bias, N, K):
    """The rows of the last, partial 64-row group all read row M - 1."""
    M = qa.shape[0]
    q, s = qa.copy(), sa.copy()
    q[64 * (M // 64):] = qa[M - 1]; s[64 * (M // 64):] = sa[M - 1]
    return gemm64(q, s, qw, sw, bias, N, pad128(K))


def _mut_halves_swapped(v, N):
    q, s = gelu_expected(v, N)
    return q.reshape(q.shape[0], -1, 2, 16)[:, :, ::-1].reshape(q.shape).copy(), s


def _mut_scale_neighbour(v, N):
    q, s = gelu_expected(v, N)
    return q, s[:, np.arange(s.shape[1]) ^ 1].copy()


def _mut_amax_own_lane(v, N):
    """No exchange between the four lanes of a block: lane g encodes its 8 columns (4 g .. 4 g + 3 and 16 + 4 g ..) with the exponent of their
    own maximum; the stored scale byte is lane 0's."""
    y = np.zeros((v.shape[0], pad128(N)), np.float32); y[:, :N] = gelu_values(v)
    lanes = y.reshape(y.shape[0], -1, 2, 4, 4)                                   # [row][block][half][g][e]
    e = mxfp8.block_exp(np.abs(lanes).max(axis=(2, 4)))                          # [row][block][g]
    scaled = (lanes.astype(np.float64) * np.exp2(-e.astype(np.float64))[:, :, None, :, None]).astype(np.float32)
    a = np.abs(scaled.astype(np.float64))
    # round to the nearest e4m3 value, ties to the even code (|scaled| <= 448 by the lane's own exponent)
    pos = _E4M3[:0x7f].astype(np.float64)
    hi_i = np.clip(np.searchsorted(pos, a), 1, 0x7e); lo_i = hi_i - 1
    dl, dh = a - pos[lo_i], pos[hi_i] - a
    code = np.where((dl < dh) | ((dl == dh) & (lo_i % 2 == 0)), lo_i, hi_i).astype(np.uint8)
    code = np.where(a == 0, 0, code).astype(np.uint8) | (np.signbit(scaled).astype(np.uint8) << 7)
    return code.reshape(y.shape), (e[:, :, 0] + 127).astype(np.uint8)


GEMM_MUTANTS = {"k_halves": _mut_k_halves, "a_scale_block": _mut_a_scale_block, "w_scale_row": _mut_w_scale_row, "stale_scales": _mut_stale_scales,
                "drop_last_step": _mut_drop_last_step, "row_clamp": _mut_row_clamp}
EPI_MUTANTS = {"halves_swapped": _mut_halves_swapped, "scale_neighbour": _mut_scale_neighbour, "amax_own_lane": _mut_amax_own_lane}
MUTANTS = {**GEMM_MUTANTS, **EPI_MUTANTS}


def applies(name, case):
    """(True, None) or (False, the structural reason the mutant cannot change this case)."""
    M, N, K, _ = case
    if name == "stale_scales" and pad128(K) < 384:
        return False, "K_pad < 384: no step has a step two before it"
    if name == "row_clamp" and M % 64 < 2:
        return False, "M % 64 < 2: the last 64-row group is empty or row M - 1 alone"
    if name == "k_halves" and K <= 64:
        return False, "K <= 64: bytes 16 .. 31 of every lane are padding under either map"
    if name == "amax_own_lane" and N <= 4:
        return False, "N <= 4: lane 0 holds every real column"
    return True, None


# ------------------------------------------------------------------------------------------------ the cases, generated once
@functools.lru_cache(maxsize=None)
def gemm_case(case):
    """dict(qa, sa, qw, sw, bias, resid, ref): operands() of a case and its float64 product + bias.  Shared: callers copy before they write."""
    M, N, K, spread = case
    qa, sa, qw, sw, bias, resid = operands(M, N, K, spread, case_seed(case))
    d = dict(qa=qa, sa=sa, qw=qw, sw=sw, bias=bias, resid=resid, ref=gemm64(qa, sa, qw, sw, bias, N, K))
    return d


@functools.lru_cache(maxsize=None)
def gelu_case(case):
    """dict(qa, sa, qw, sw, bias, dead, v, q, s, fc2): gelu_operands() of a case, v = acc + bias in float64, the expected elements and scales,
    and fc2 = fc2_operands() on them.  Shared: callers copy before they write."""
    M, N, K, spread = case
    qa, sa, qw, sw, bias, dead = gelu_operands(M, N, K, spread, case_seed(case))
    v = gemm64(qa, sa, qw, sw, bias, N, K)
    q, s = gelu_expected(v, N)
    d = dict(qa=qa, sa=sa, qw=qw, sw=sw, bias=bias, dead=dead, v=v, q=q, s=s)
    d["fc2"] = fc2_operands(q, s, N, case_seed(case) + 5)
    return d
