"""Data generators, references and CPU-side conditions of the class softmax, device top-k and block dequant tests (test_gpu_tail.py).

Nothing here touches a GPU or libvitx.so: tests/test_cpu_tail_data.py checks every condition the GPU tests rely on.

  * softmax: logits on which every numerator e_i = round_T(expf(round_T(x_i - max))) is known bit for bit, so the only freedom left to the
    kernel is the f32 summation, one reciprocal and one product -- which softmax_gate() bounds from the arithmetic;
  * top-k: rows with heavy ties, signed zeros, infinities and NaNs, and the order (topk_order) that vitx_topk and topk_kernel both follow;
  * dequant: blocks written byte by byte in the file layout (never by the quantiser), with every code at every position and with scales
    the quantiser never produces, and ggml's dequantize_row_* restated operation for operation in numpy float32.
"""
from __future__ import annotations

import functools
import math

import numpy as np

F16, BF16 = 0, 1
MANT = {F16: 10, BF16: 7}            # stored mantissa bits
EMIN = {F16: -14, BF16: -126}        # exponent of the smallest normal


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------------------------
# the two operand types in numpy: bits <-> f32, and round-to-nearest-even from f32 and from f64
# ------------------------------------------------------------------------------------------------------------------
def to_bits(x32: np.ndarray, dtype: int) -> np.ndarray:
    """f32 -> operand type, round to nearest even (overflow gives inf) -> its 16 bits."""
    x32 = np.ascontiguousarray(x32, np.float32)
    if dtype == F16:
        with np.errstate(over="ignore", invalid="ignore"):
            return x32.astype(np.float16).view(np.uint16)
    u = x32.view(np.uint32)
    r = ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(x32), ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def from_bits(b: np.ndarray, dtype: int) -> np.ndarray:
    b = np.ascontiguousarray(b, np.uint16)
    if dtype == F16:
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_to(x32: np.ndarray, dtype: int) -> np.ndarray:
    """The kernels' rnd<T>: f32 -> T -> f32."""
    return from_bits(to_bits(x32, dtype), dtype)


def grid_exponent(x64: np.ndarray, dtype: int) -> np.ndarray:
    """log2 of the spacing of the operand type's values at |x| (the subnormal spacing below the smallest normal)."""
    _, ex = np.frexp(np.asarray(x64, np.float64))
    return np.maximum(ex - 1, EMIN[dtype]) - MANT[dtype]


def round64_to(x64: np.ndarray, dtype: int) -> np.ndarray:
    """float64 -> T in ONE rounding (nearest even), as float64.  For finite values below the type's overflow threshold."""
    x64 = np.asarray(x64, np.float64)
    s = np.ldexp(1.0, grid_exponent(x64, dtype))
    return np.rint(x64 / s) * s              # x / s is exact (s is a power of two); rint rounds halves to even


def is_nan_bits(b: np.ndarray, dtype: int) -> np.ndarray:
    b = np.asarray(b, np.uint16)
    return ((b & 0x7c00) == 0x7c00) & ((b & 0x03ff) != 0) if dtype == F16 else ((b & 0x7f80) == 0x7f80) & ((b & 0x007f) != 0)


# ------------------------------------------------------------------------------------------------------------------
# class softmax
# ------------------------------------------------------------------------------------------------------------------
# softmax_kernel (softmax_topk.hip):  mx = max x;  e_i = rnd<T>(expf(rnd<T>(x_i - mx)));  p_i = e_i * (1 / sum e).
EXP_LOW_BITS = {F16: 0xCD00, BF16: 0xC1A0}       # -20 in either type
SAFE_ULPS = 64                                   # distance kept from every rounding tie of the type, in f32 ulps of exp(x)
SM_COLS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 1001, 21843)
SM_ROWS = (1, 37, 1025)
SM_LEVELS = (0.0, -30000.0, 30000.0)
SHIFTS = (-30000.0, 0.0, 30000.0)


def exp_arguments(dtype: int) -> np.ndarray:
    """Every value of the operand type in [-20, 0] with the sign bit set (-0 ... -20), as f32: 19 713 for f16, 16 801 for bf16."""
    return from_bits(np.arange(0x8000, EXP_LOW_BITS[dtype] + 1, dtype=np.uint32).astype(np.uint16), dtype)


def tie_distance_ulps(e64: np.ndarray, dtype: int) -> np.ndarray:
    """Distance of e to the nearest rounding tie of the operand type (a midpoint between two neighbouring values, the subnormal ones
    and the midpoint between 0 and the smallest subnormal included), in units of the f32 ulp of e."""
    e64 = np.asarray(e64, np.float64)
    s = np.ldexp(1.0, grid_exponent(e64, dtype))
    q = e64 / s
    dist = np.abs(q - np.floor(q) - 0.5) * s
    _, ex = np.frexp(e64)
    return dist / np.ldexp(1.0, ex - 1 - 23)


@functools.lru_cache(maxsize=None)
def safe_exp_arguments(dtype: int):
    """(x, e, omitted): the arguments whose float64 exp lies MORE than SAFE_ULPS f32 ulps from every tie, and e = round_T(exp(x)) -- which
    is then what ANY expf with an error below SAFE_ULPS - 1 ulps rounds to, so e is known without knowing the device's expf."""
    x = exp_arguments(dtype)
    e64 = np.exp(x.astype(np.float64))
    keep = tie_distance_ulps(e64, dtype) > SAFE_ULPS
    e = round_to(e64[keep].astype(np.float32), dtype)
    x, e = x[keep], e
    x.setflags(write=False); e.setflags(write=False)
    return x, e, int((~keep).sum())


def off_grid(x: np.ndarray, dtype: int, seed: int) -> np.ndarray:
    """x moved by an eighth of the type's spacing at x, up or down: f32 values that are NOT values of the type and that rnd<T> returns
    to x.  (The zero stays: it must remain the row's maximum.)  On these the kernel's INNER rounding is no identity."""
    rng = np.random.default_rng(seed)
    step = np.ldexp(1.0, grid_exponent(x.astype(np.float64), dtype) - 3)
    sign = rng.integers(0, 2, x.shape) * 2.0 - 1.0
    y = np.where(x == 0, x.astype(np.float64), x.astype(np.float64) + sign * step)
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y)
    return y32


def _pad_fill(logits: np.ndarray, cols: int) -> None:
    """Pad columns: NaN and +inf alternating.  A NaN read into the maximum is swallowed by fmaxf, +inf is not; either one read into the
    sum shows in every probability of the row."""
    ld = logits.shape[1]
    logits[:, cols:] = np.where((np.arange(cols, ld) & 1) == 0, np.float32(np.nan), np.float32(np.inf))


@functools.lru_cache(maxsize=None)
def exp_case(dtype: int, cols: int = 1000, ld: int = 1024, perturbed: bool = False):
    """Rows that between them hold every safe argument: the maximum, exactly 0, in column (row * 7 + 3) % cols, a seeded permutation of
    the arguments in the others (the last row wraps round).  Returns (logits [rows][ld] f32, e [rows][cols] f64, p_ref [rows][cols] f64)."""
    x, e, _ = safe_exp_arguments(dtype)
    rng = np.random.default_rng(1000 + dtype)
    per = cols - 1
    rows = -(-x.size // per)
    take = rng.permutation(x.size)[np.arange(rows * per) % x.size]
    xs = off_grid(x, dtype, 77 + dtype)[take] if perturbed else x[take]
    hot = (np.arange(rows) * 7 + 3) % cols
    mask = np.ones((rows, cols), bool); mask[np.arange(rows), hot] = False
    logits = np.empty((rows, ld), np.float32); _pad_fill(logits, cols)
    body = np.zeros((rows, cols), np.float32); body[mask] = xs
    logits[:, :cols] = body
    e64 = np.ones((rows, cols), np.float64); e64[mask] = e[take].astype(np.float64)
    p_ref = e64 / e64.sum(1, keepdims=True)
    for a in (logits, e64, p_ref):
        a.setflags(write=False)
    return logits, e64, p_ref


def softmax_gate(cols: int) -> float:
    """Relative bound on |p - p_ref| when every e_i is exact.  All terms are non-negative, so an f32 sum of them, however grouped, is off
    by at most (1 + u)^d - 1 relative, u = 2^-24, d = the number of additions on the longest path to the total: ceil(cols / 256)
    per-thread additions, six shuffle additions, two additions of the four wave sums.  The reciprocal and the product p_i = e_i * inv
    are correctly rounded, one u each; a subnormal p_i does not occur (e >= 2^-24, the sum < 2^10).  Together
    (ceil(cols / 256) + 10) u, plus one percent for the second-order terms ((1 + u)^d - 1 - d u < d^2 u^2, far below 1 % of d u)."""
    return (math.ceil(cols / 256) + 10) * 2.0 ** -24 * 1.01


def softmax_model(logits: np.ndarray, cols: int, dtype: int, inner: bool = True, outer: bool = True) -> np.ndarray:
    """The kernel's definition in float64, with either rounding point optional (what a kernel that had lost it would compute)."""
    x = logits[:, :cols].astype(np.float64)
    d = (x - x.max(1, keepdims=True)).astype(np.float32)
    if inner:
        d = round_to(d, dtype)
    e = np.exp(d.astype(np.float64))
    if outer:
        e = round_to(e.astype(np.float32), dtype).astype(np.float64)
    return e / e.sum(1, keepdims=True)


def softmax_gate_ratio(p: np.ndarray, p_ref: np.ndarray, cols: int) -> float:
    """max |p - p_ref| / (p_ref * gate) over the entries with p_ref > 0 (the others must be +0 bit for bit: checked apart)."""
    pos = p_ref > 0
    return float((np.abs(p.astype(np.float64)[pos] - p_ref[pos]) / (p_ref[pos] * softmax_gate(cols))).max())


def sm_lds(cols: int):
    return sorted({cols, cols + 1, round_up(cols, 256)})


def sm_shapes():
    """(rows, cols, ld) of the flat and the routed rows; the one large column count takes only the small row counts."""
    return [(rows, cols, ld) for cols in SM_COLS for ld in sm_lds(cols) for rows in SM_ROWS if not (cols > 1001 and rows > 37)]


def logits_buffer(rows: int, cols: int, ld: int, body: np.ndarray) -> np.ndarray:
    out = np.empty((rows, ld), np.float32); _pad_fill(out, cols)
    out[:, :cols] = body
    return out


def routed_hot(rows: int, cols: int) -> np.ndarray:
    return (np.arange(rows) * 7 + 3) % cols


def shift_logits(rows: int, cols: int, seed: int) -> np.ndarray:
    """Integer logits in [-20, 20]; every row holds a 20, so x - max is an integer in [-40, 0]: exact in f32, a value of either type."""
    x = np.random.default_rng(seed).integers(-20, 21, (rows, cols)).astype(np.float32)
    x[np.arange(rows), routed_hot(rows, cols)] = 20.0
    return x


# ------------------------------------------------------------------------------------------------------------------
# top-k
# ------------------------------------------------------------------------------------------------------------------
TK_COLS = (1, 2, 63, 64, 65, 127, 128, 129, 1000, 1001)
TK_ROWS = (1, 3, 4, 5, 9)
TK_KINDS = ("levels", "equal", "ascending", "descending", "max_last", "zeros", "inf", "nan_one", "nan_some", "nan_all")
TK_TIED = ("levels", "equal", "zeros")            # kinds whose row 0 must have a tie across every position k < cols
TK_LEVELS = np.array([0.0, 2.0 ** -20, 0.001, 0.01, 0.125, 0.25, 0.5, 1.0], np.float32)
TK_GUARD = 2.0                                    # input guard rows: above every probability, so a read outside the row is selected
NAN_BITS = np.array([0x7fc00000, 0xffc00000, 0x7fc00123, 0x7f800001, 0xffffffff], np.uint32)


def tk_ks(cols: int):
    ks = {1, 2, 5, min(cols, 70)}
    if cols <= 129:
        ks.add(cols)
    return sorted(k for k in ks if k <= cols)


def topk_order(row: np.ndarray) -> np.ndarray:
    """The whole row in the order of vitx_topk / topk_kernel: not-NaN first, by value descending then index ascending (+0 and -0 tie);
    NaN last, by index ascending.  A stable sort on (is NaN, -value), restated with the index as an explicit last key."""
    nan = np.isnan(row)
    key = np.where(nan, np.float32(0), row) + np.float32(0)            # -0 + 0 = +0
    return np.lexsort((np.arange(row.size), -key, nan))


def straddles(row: np.ndarray, k: int) -> bool:
    """A tie across position k: the k-th and the (k + 1)-th entry of the order compare equal (so only the index decides which is returned)."""
    o = topk_order(row)
    return k < row.size and bool(row[o[k - 1]] == row[o[k]])


def _levels_row(rng, cols: int) -> np.ndarray:
    return TK_LEVELS[rng.integers(0, TK_LEVELS.size, cols)]


@functools.lru_cache(maxsize=None)
def topk_rows(kind: str, cols: int) -> np.ndarray:
    """max(TK_ROWS) rows of one kind at one width (f32).  A case with fewer rows uses the first ones."""
    R = max(TK_ROWS)
    rng = np.random.default_rng(TK_KINDS.index(kind) * 10007 + cols)
    out = np.empty((R, cols), np.float32)
    for r in range(R):
        if kind in ("levels", "inf", "nan_one", "nan_some"):
            row = _levels_row(rng, cols)
            if kind == "levels" and r == 0:
                for _ in range(10000):
                    if all(straddles(row, k) for k in tk_ks(cols) if k < cols):
                        break
                    row = _levels_row(rng, cols)
            n_special = {"inf": max(1, cols // 8), "nan_one": 1, "nan_some": max(1, cols // 4)}.get(kind, 0)
            at = rng.permutation(cols)[:min(n_special, cols)]
            if kind == "inf":
                row[at] = np.where(rng.integers(0, 2, at.size) == 0, np.float32(np.inf), np.float32(-np.inf))
            elif n_special:
                row[at] = NAN_BITS[rng.integers(0, NAN_BITS.size, at.size)].view(np.float32)
        elif kind == "equal":
            row = np.full(cols, TK_LEVELS[r % TK_LEVELS.size], np.float32)
        elif kind in ("ascending", "descending"):
            row = (np.arange(1, cols + 1, dtype=np.float64) / (cols + 1) * 2.0 ** -r).astype(np.float32)
            row = row[::-1].copy() if kind == "descending" else row
        elif kind == "max_last":
            row = (rng.permutation(cols).astype(np.float64) / (2 * cols)).astype(np.float32)
            row[-1] = 0.95
        elif kind == "zeros":
            row = np.where(rng.integers(0, 2, cols) == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
            if r == 0 and cols > 1:
                row[0], row[1] = -0.0, 0.0                      # were +0 ranked above -0, class 1 would come before class 0
        else:
            assert kind == "nan_all"
            row = NAN_BITS[rng.integers(0, NAN_BITS.size, cols)].view(np.float32).copy()
        out[r] = row
    out.setflags(write=False)
    return out


def topk_expected(rows: np.ndarray, k: int):
    """(value bits u32 [rows][k], class i32 [rows][k]) of the first k entries of the order of every row."""
    order = np.stack([topk_order(r)[:k] for r in rows])
    vals = np.take_along_axis(rows.view(np.uint32), order, 1)
    return vals, order.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------
# block dequant
# ------------------------------------------------------------------------------------------------------------------
Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 = 2, 3, 6, 7, 8
QTYPES = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0)
BLOCK_BYTES = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34}
N_CODES = {Q4_0: 16, Q4_1: 16, Q5_0: 32, Q5_1: 32, Q8_0: 256}
HAS_MIN = (Q4_1, Q5_1)
# f16 bit patterns no quantiser writes: +-0, smallest and largest subnormal (both signs), smallest normal, +-1, +-65504
FIXED_SCALES = (0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0400, 0x3c00, 0xbc00, 0x7bff, 0xfbff)
NONFINITE_SCALES = (0x7c00, 0xfc00, 0x7e00, 0xfe00, 0x7c01, 0x3c00)      # +-inf, quiet and signalling NaN, and 1 for the other field
DQ_N = (1, 5, 200)
DQ_K = (32, 64, 448)
JOB_SHAPES = ((192, 64), (64, 64), (256, 64), (64, 256))                   # (N, K) of qkv, proj, fc1, fc2 at D = 64


def dq_n_pads(N: int):
    return sorted({N, N + 3, round_up(N, 256)})


@functools.lru_cache(maxsize=None)
def hostile_scales() -> np.ndarray:
    """The fixed patterns followed by seeded random FINITE patterns: 40 in all."""
    r = np.random.default_rng(5).integers(0, 0x10000, 400).astype(np.uint16)
    r = r[(r & 0x7c00) != 0x7c00][:40 - len(FIXED_SCALES)]
    out = np.concatenate([np.array(FIXED_SCALES, np.uint16), r])
    assert out.size == 40
    out.setflags(write=False)
    return out


def pack_blocks(qtype: int, codes: np.ndarray, d_bits: np.ndarray, m_bits: np.ndarray | None = None) -> np.ndarray:
    """codes [nb][32] (0 .. N_CODES - 1; the stored code: q4_0 means code - 8, q5_0 code - 16, q8_0 the int8 with these bits), f16 bit
    patterns d (and m) [nb] -> blocks [nb][BLOCK_BYTES] u8 in the file layout: d, (m), (qh: bit j = bit 4 of element j's code),
    qs (q4 / q5: byte j = low four bits of element j | low four bits of element j + 16 << 4; q8: byte j = element j)."""
    codes = np.asarray(codes, np.uint8); nb = codes.shape[0]
    assert codes.shape == (nb, 32) and int(codes.max(initial=0)) < N_CODES[qtype]
    out = np.zeros((nb, BLOCK_BYTES[qtype]), np.uint8)
    out[:, 0:2] = np.asarray(d_bits, np.uint16).reshape(nb, 1).view(np.uint8)
    at = 2
    if qtype in HAS_MIN:
        out[:, 2:4] = np.asarray(m_bits, np.uint16).reshape(nb, 1).view(np.uint8); at = 4
    if qtype in (Q5_0, Q5_1):
        qh = np.zeros(nb, np.uint32)
        for j in range(32):
            qh |= ((codes[:, j].astype(np.uint32) >> np.uint32(4)) & np.uint32(1)) << np.uint32(j)
        out[:, at:at + 4] = qh.reshape(nb, 1).view(np.uint8); at += 4
    if qtype == Q8_0:
        out[:, at:] = codes
    else:
        out[:, at:] = (codes[:, :16] & 15) | ((codes[:, 16:] & 15) << 4)
    return out


def dequant_f32(qtype: int, blocks: np.ndarray, fused: bool = False) -> np.ndarray:
    """ggml's dequantize_row_* operation for operation in float32: blocks [nb][BLOCK_BYTES] u8 -> [nb][32] f32.  The product is rounded
    to f32, then the sum (the library is built with contraction off); fused = the sum of the EXACT product rounded once, what a
    contracted multiply-add would give."""
    b = np.asarray(blocks, np.uint8); nb = b.shape[0]
    d = b[:, 0:2].copy().view(np.float16).astype(np.float32)                 # [nb][1]
    at = 2
    m = None
    if qtype in HAS_MIN:
        m = b[:, 2:4].copy().view(np.float16).astype(np.float32); at = 4
    x = np.empty((nb, 32), np.int32)
    if qtype == Q8_0:
        x[:] = b[:, at:].view(np.int8)
    else:
        if qtype in (Q5_0, Q5_1):
            qh = b[:, at:at + 4].copy().view(np.uint32); at += 4           # [nb][1]
            j = np.arange(16, dtype=np.uint32)
            h0 = ((qh >> j) << np.uint32(4)) & np.uint32(0x10)
            h1 = (qh >> (j + np.uint32(12))) & np.uint32(0x10)
        else:
            h0 = h1 = np.uint32(0)
        qs = b[:, at:].astype(np.uint32)
        x[:, :16] = (qs & 15) | h0
        x[:, 16:] = (qs >> 4) | h1
        x -= {Q4_0: 8, Q5_0: 16}.get(qtype, 0)
    xf = x.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if m is None:
            return xf * d
        if fused:
            return (xf.astype(np.float64) * d.astype(np.float64) + m.astype(np.float64)).astype(np.float32)   # the f64 product and sum are exact here: see fused_search
        return xf * d + m


def dequant_bits(qtype: int, blocks: np.ndarray, dtype: int, N: int, n_pad: int, K: int) -> np.ndarray:
    """The whole destination [n_pad][K] as 16-bit patterns: the f32 values rounded once to the operand type, +0 in the pad rows."""
    out = np.zeros((n_pad, K), np.uint16)
    out[:N] = to_bits(dequant_f32(qtype, blocks), dtype).reshape(N, K)
    return out


def split_q4_0(blocks: np.ndarray):
    """File layout (18-byte blocks) -> the device layout of q4_0: nibble plane [nb][16] u8 and f16 scale plane [nb] u16."""
    return np.ascontiguousarray(blocks[:, 2:]), np.ascontiguousarray(blocks[:, 0:2]).view(np.uint16).reshape(-1)


def sweep_shape(qtype: int):
    """(N, K) that holds the N_CODES blocks of the code sweep, eight blocks to a row."""
    return N_CODES[qtype] // 8, 256


def sweep_blocks(qtype: int, d_bits: int, m_bits: int) -> np.ndarray:
    """Block b holds code (b + i) % n_codes at position i, b in range(n_codes): every code at every position."""
    n = N_CODES[qtype]
    codes = (np.arange(n)[:, None] + np.arange(32)[None, :]) % n
    return pack_blocks(qtype, codes, np.full(n, d_bits, np.uint16), np.full(n, m_bits, np.uint16))


SWEEP_SCALES = ((0x3c00, 0x0000), (0x28c1, 0xbd7b))        # (d, m): 1 and 0 -- the codes themselves --, then 0.0371.. and -1.37..


def scaled_blocks(qtype: int, N: int, K: int, seed: int, scales: np.ndarray) -> np.ndarray:
    """N rows of K / 32 blocks with seeded random codes; row r takes d = scales[(r + seed) % n] and, from the same list at another
    stride, m = scales[(3 r + r // n + 7 seed + 1) % n]."""
    rng = np.random.default_rng(seed * 31 + qtype)
    nbk = K // 32; n = len(scales)
    codes = rng.integers(0, N_CODES[qtype], (N * nbk, 32))
    r = np.repeat(np.arange(N), nbk)
    sc = np.asarray(scales, np.uint16)
    return pack_blocks(qtype, codes, sc[(r + seed) % n], sc[(3 * r + r // n + 7 * seed + 1) % n])


def nonfinite_blocks(qtype: int, K: int = 64):
    """One row for every pair (d, m) from NONFINITE_SCALES (36 rows, seeded random codes): (N, blocks)."""
    n = len(NONFINITE_SCALES); nbk = K // 32
    codes = np.random.default_rng(qtype).integers(0, N_CODES[qtype], (n * n * nbk, 32))
    r = np.repeat(np.arange(n * n), nbk)
    sc = np.array(NONFINITE_SCALES, np.uint16)
    return n * n, pack_blocks(qtype, codes, sc[r // n], sc[r % n])


def dq_shapes():
    return [(N, n_pad, K) for N in DQ_N for n_pad in dq_n_pads(N) for K in DQ_K]


def job_n_pad(N: int, j: int) -> int:
    """A ragged pad for every job: 5, 0, 13 and 64 rows."""
    return N + (5, 0, 13, 64)[j]


@functools.lru_cache(maxsize=None)
def fused_search():
    """Would a contracted multiply-add show?  It cannot.  A code has at most 5 significant bits and an f16 scale at most 11, so code * d
    has at most 16 and is EXACT in f32 for every code and every finite f16 d; round(code * d + m) is then the same single rounding of
    the same exact sum whether the product was rounded first or not.  Returns (products checked, inexact products, elements whose
    f32 value differs between dequant_f32(fused=False) and (fused=True)) over every code and every finite scale with seeded m."""
    d_bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    d_bits = d_bits[(d_bits & 0x7c00) != 0x7c00]
    d = d_bits.view(np.float16).astype(np.float32)
    codes = np.arange(32, dtype=np.float32)
    prod32 = codes[None, :] * d[:, None]
    prod64 = codes[None, :].astype(np.float64) * d[:, None].astype(np.float64)
    inexact = int((prod32.astype(np.float64) != prod64).sum())
    rng = np.random.default_rng(11)
    m_bits = rng.choice(d_bits, d_bits.size)
    blocks = pack_blocks(Q5_1, np.tile(np.arange(32), (d_bits.size, 1)), d_bits, m_bits)
    a, b = dequant_f32(Q5_1, blocks), dequant_f32(Q5_1, blocks, fused=True)
    return prod32.size, inexact, int((a.view(np.uint32) != b.view(np.uint32)).sum())


# elements the seeded search below must find (they are rare: the exact sum has to lie within half an f32 ulp of a tie of the type without
# sitting on it; with the 4-bit codes of q4_1 and an 11-bit d none exists for f16 in the range searched)
DOUBLE_ROUNDING_WANT = {(Q4_1, F16): 0, (Q4_1, BF16): 8, (Q5_1, F16): 32, (Q5_1, BF16): 8}


@functools.lru_cache(maxsize=None)
def double_rounding_blocks(qtype: int, dtype: int):
    """What the 11-bit (8-bit) rounding CAN hide is where the value is rounded: the kernel must round code * d + m to f32 and then once to
    the operand type; an evaluation that goes to the operand type directly (a packed 16-bit multiply-add, a mixed-precision fma with a
    16-bit destination) rounds the exact sum once and differs where the f32 rounding carries the sum onto or across a tie of the type.
    Seeded search for (code, d, m) whose two results differ; one block each, the code at all 32 positions.
    Returns (blocks [found][BLOCK_BYTES], found)."""
    assert qtype in HAS_MIN
    rng = np.random.default_rng(900 + qtype * 2 + dtype)
    n = 1 << 22
    c = rng.integers(1, N_CODES[qtype], n)
    d_bits = (rng.integers(0x0001, 0x1000, n) | (rng.integers(0, 2, n) << 15)).astype(np.uint16)      # |d| in [2^-24, 2^-12)
    m_bits = (rng.integers(0x3c00, 0x4c00, n) | (rng.integers(0, 2, n) << 15)).astype(np.uint16)      # |m| in [1, 16)
    d = d_bits.view(np.float16).astype(np.float64); m = m_bits.view(np.float16).astype(np.float64)
    exact = c * d + m                                     # 16 bits at 2^-24 or above + 11 bits below 2^4: exact in float64
    once = round64_to(exact, dtype)
    twice = round_to(exact.astype(np.float32), dtype).astype(np.float64)
    hit = np.flatnonzero(once != twice)
    blocks = pack_blocks(qtype, np.repeat(c[hit][:, None], 32, 1), d_bits[hit], m_bits[hit])
    return blocks, int(hit.size)
