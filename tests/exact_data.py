"""Data generators and CPU-side conditions of the exact and hostile-data kernel tests (test_gpu_exact.py, test_gpu_hostile.py,
test_gpu_attention.py).

Nothing here touches a GPU or libvitx.so: tests/test_cpu_exact_data.py checks every condition the GPU tests rely on.

"Exact" data makes a kernel's correct result unique, so a test needs no tolerance and can compare every element of an output buffer:
  * GEMM operands are small integers (times a power of two): every product and every partial sum is an integer (times that power of two)
    far below 2^24, so f32 accumulation is exact IN ANY ORDER;
  * attention operands route every query to one key by a score gap so large that every other probability vanishes in f32, or make every
    key of an item the same vector, so that every numerator is exactly 1 and the sums are integers ("flat": every key weighs 1 / N).
"Hostile" data keeps a float64 reference and a tolerance, but has the shape of a trained model's residual stream instead of randn.
"Spread" / "peaked" attention data is randn; its gates are derived from the float64 reference and an emulation of the definition.
"""
from __future__ import annotations

import numpy as np

# ------------------------------------------------------------------------------------------------------------------
# GEMM with integer operands
# ------------------------------------------------------------------------------------------------------------------
A_MAX, W_MAX, BIAS_MAX = 4, 4, 32          # |A|, |W| <= 4, |bias| <= 32 (integers)
RESID_MAX = 2 ** 15                        # |residual|, |pos| <= 2^15 (integers below 2^16)
# (A scale, W scale) as powers of two: plain integers, and A * 2^-3, W * 2^-5 so that not every exponent is a small integer's
VARIANTS = {"int": (0, 0), "scaled": (-3, -5)}
M_REAL_VALUES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513)
N_VALUES = (4, 60, 64, 192, 252, 256, 260, 768, 1000, 2304)
K_VALUES = (64, 128, 192, 768, 3072)
KERNELS = (0, 1, 2, 945, 445, 245, 122)    # vitx_op_gemm_ex kernel ids
EPILOGUES = (0, 1, 2, 3, 4, 5)


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def gemm_small_cases():
    """(M, M_real, N, K): every listed M_real, N and K occurs; M is M_real rounded up to 128 and, as a second case, to 256."""
    trip = [(1, 4, 64), (63, 60, 128), (64, 64, 192), (65, 192, 768), (127, 252, 3072), (128, 256, 64), (129, 260, 128), (255, 768, 192),
            (256, 1000, 768), (257, 2304, 3072), (511, 60, 3072), (513, 1000, 64), (1, 2304, 128), (127, 4, 768)]
    out = []
    for m_real, n, k in trip:
        for m in sorted({round_up(m_real, 128), round_up(m_real, 256)}):
            out.append((m, m_real, n, k))
    return out


def gemm_wide_cases():
    """Tile counts around the is_wide threshold (128 tiles of 256 x 256) and around whole rounds of 256 CUs: N = 256 with 127, 128, 256, 257
    row tiles, N = 768 with 85, 86, 113 (339 tiles) and 171 row tiles, each with M_real = M and M_real = M - 100.  K = 128 takes the
    ping-pong kernel, K = 192 (not a multiple of 128) the wide ring kernels."""
    out = []
    for n, ntm, k in ((256, 127, 128), (256, 128, 192), (256, 256, 128), (256, 257, 128), (768, 85, 128), (768, 86, 192), (768, 113, 128), (768, 171, 128)):
        for cut in (0, 100):
            out.append((ntm * 256, ntm * 256 - cut, n, k))
    return out


def is_wide(M: int, N: int, K: int) -> bool:
    """Restatement of the dispatcher's is_wide() (gemm.hip) for vitx_op_gemm_ex, whose W holds N rounded up to 256 rows."""
    return M % 256 == 0 and (M // 256) * (round_up(N, 256) // 256) >= 128


def tail_split_rows(M: int, N: int, n_cu: int) -> int:
    """Rows the forced tail split (kernel 2) leaves to its first launch, 0 when it does not split (launch_gemm, gemm.hip)."""
    ntm, ntn = M // 256, round_up(N, 256) // 256
    tiles = ntm * ntn
    rounds, rem = tiles // n_cu, tiles % n_cu
    if not (rounds >= 1 and 0 < rem <= n_cu * 6 // 10):
        return 0
    m_main = rounds * n_cu // ntn
    return m_main * 256 if (m_main >= 1 and m_main * 256 < M) else 0


def gemm_bound(K: int, variant: str) -> float:
    """Largest magnitude, in units of the smallest bit any value of the case can carry, of any partial or final sum of a case:
    it must stay below 2^24 for f32 arithmetic to be exact in any order."""
    sa, sw = VARIANTS[variant]
    unit = 2.0 ** (sa + sw)                                     # every product is a multiple of this
    return (K * A_MAX * W_MAX * unit + BIAS_MAX + RESID_MAX) / unit


def gemm_operands(M: int, N: int, K: int, tpi: int, seed: int):
    """Integer A [M][K] (pad rows included: a kernel that stores them is caught), W [N][K], bias [N], residual [M][N], pos [tpi + 1][N]."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-A_MAX, A_MAX + 1, (M, K)).astype(np.float32)
    w = rng.integers(-W_MAX, W_MAX + 1, (N, K)).astype(np.float32)
    bias = rng.integers(-BIAS_MAX, BIAS_MAX + 1, N).astype(np.float32)
    resid = rng.integers(-RESID_MAX, RESID_MAX + 1, (M, N)).astype(np.float32)
    pos = rng.integers(-RESID_MAX, RESID_MAX + 1, (tpi + 1, N)).astype(np.float32)
    return a, w, bias, resid, pos


def hilo_values(variant: str):
    """Every value acc + bias can take in a variant (|acc| <= 3072 * 16 in units of the variant's bit)."""
    sa, sw = VARIANTS[variant]
    unit = 2.0 ** (sa + sw)
    lim = int((3072 * A_MAX * W_MAX * unit + BIAS_MAX) / unit)
    return (np.arange(-lim, lim + 1, dtype=np.float64) * unit).astype(np.float32)


def gelu64(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(0.79788456080286535588 * x * (1.0 + 0.044715 * x * x)))


def q4_0_planes(N: int, n_pad: int, K: int, scale_exp: int, seed: int):
    """q4_0 blocks whose f16 scale is 2^scale_exp: nibble plane [n_pad][K/32][16], scale plane [n_pad][K/32] (f16 bits) as vitx_op_gemm_q4
    takes them, and the dequantised weights [N][K] = (nibble - 8) * 2^scale_exp with nibble - 8 in [-4, 4] (exact in f16 and bf16)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-W_MAX, W_MAX + 1, (N, K))
    nib = (w + 8).astype(np.uint8).reshape(N, K // 32, 32)
    qs = np.zeros((n_pad, K // 32, 16), np.uint8)
    qs[:N] = nib[:, :, :16] | (nib[:, :, 16:] << 4)              # low nibbles = the first 16 elements of a block, high = the last 16
    ds = np.zeros((n_pad, K // 32), np.uint16)
    ds[:N] = np.float16(2.0 ** scale_exp).view(np.uint16)
    return qs, ds, (w * 2.0 ** scale_exp).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------
# Patch embedding with integer tensors
# ------------------------------------------------------------------------------------------------------------------
# (patch, channels, image size, images): tokens per image tpi = (img / patch)^2 is odd, so that some image's patch 0 falls on the last row of
# a 128-row tile (image b with b * tpi % 128 == 127), and images * tpi is not a multiple of 128 (ragged last tile).  One channel = a
# ViTSTR file, whose head reads 25 tokens: tpi >= 25.
PATCH_CASES = ((16, 3, 48, 75), (32, 3, 96, 75), (16, 1, 80, 90), (8, 3, 24, 75), (14, 3, 42, 75))


def patch_edges(tpi: int, n_img: int):
    """(rows in the last 128-row tile, images whose patch 0 is the last row of a tile).  The tests trace EVERY image, so both sides of every
    tile edge are compared."""
    return (n_img * tpi) % 128, [b for b in range(n_img) if (b * tpi) % 128 == 127]


def patch_tensors(D: int, P: int, cin: int, n_tok: int, seed: int):
    """Integer patch kernel [D][cin][P][P] in [-2, 2], bias [D] in [-32, 32], cls_token [1][1][D] and pos_embed [1][n_tok][D] below 2^12."""
    rng = np.random.default_rng(seed)
    return {"patch_embed.proj.weight": rng.integers(-2, 3, (D, cin, P, P)).astype(np.float32),
            "patch_embed.proj.bias": rng.integers(-32, 33, D).astype(np.float32),
            "cls_token": rng.integers(-4096, 4097, (1, 1, D)).astype(np.float32),
            "pos_embed": rng.integers(-4096, 4097, (1, n_tok, D)).astype(np.float32)}


def patch_images(n: int, S: int, cin: int, seed: int) -> np.ndarray:
    """[n][S][S][cin] (or [n][S][S] for one channel) floats that are integers in [-8, 8]."""
    x = np.random.default_rng(seed).integers(-8, 9, (n, S, S, cin)).astype(np.float32)
    return x if cin == 3 else x[..., 0]


def patch_embed_ref(imgs: np.ndarray, t: dict, P: int) -> np.ndarray:
    """int64 patch embedding: [n][tpi + 1][D]; token 0 = cls_token + pos_embed[0], token 1 + p = patch p . kernel + bias + pos_embed[1 + p]."""
    x = np.asarray(imgs, np.int64)
    if x.ndim == 3:
        x = x[..., None]
    n, S, _, cin = x.shape
    g = S // P
    w = t["patch_embed.proj.weight"].astype(np.int64)           # [D][cin][P][P]
    D = w.shape[0]
    patches = x.reshape(n, g, P, g, P, cin).transpose(0, 1, 3, 5, 2, 4).reshape(n, g * g, cin * P * P)      # [n][patch][c][ky][kx]
    pos = t["pos_embed"].astype(np.int64)[0]
    out = np.empty((n, g * g + 1, D), np.int64)
    out[:, 1:] = patches @ w.reshape(D, -1).T + t["patch_embed.proj.bias"].astype(np.int64) + pos[1:]
    out[:, 0] = t["cls_token"].astype(np.int64)[0, 0] + pos[0]
    return out


def patch_bound(P: int, cin: int) -> int:
    return cin * P * P * 2 * 8 + 32 + 4096


# ------------------------------------------------------------------------------------------------------------------
# Attention as exact routing
# ------------------------------------------------------------------------------------------------------------------
Q_SCALE = 32.0
MIN_GAP = 40.0


def routing_qkv(n_img: int, N: int, H: int, hd: int, seed: int, rows0_only: bool = False):
    """qkv [n_img * N][3 * H * hd] f32 (exact in f16 and bf16), the permutation p [n_img][H][N] with out[i] = v[p[i]], and the smallest score
    gap in float64.  k_j = u_j (random +-1), q_i = 32 u_{p(i)}, v = +-{1, 1.5, .. 3.5} * 2^{-2..1} (three significant bits, never zero).
    Every (image, head) has its own u, p and v.  rows0_only: the gap of query 0 only (vitx_op_attention_cls, the class-token map)."""
    rng = np.random.default_rng(seed)
    D = H * hd
    qkv = np.zeros((n_img, N, 3, H, hd), np.float32)
    perm = np.empty((n_img, H, N), np.int64)
    gap = np.inf
    for b in range(n_img):
        for h in range(H):
            u = rng.integers(0, 2, (N, hd)).astype(np.float64) * 2 - 1
            p = rng.permutation(N)
            v = rng.choice([-1.0, 1.0], (N, hd)) * rng.integers(2, 8, (N, hd)) * 0.5 * np.exp2(rng.integers(-2, 2, (N, hd)))
            qkv[b, :, 0, h] = Q_SCALE * u[p]; qkv[b, :, 1, h] = u; qkv[b, :, 2, h] = v
            perm[b, h] = p
            qs = (Q_SCALE * u[p[:1]] if rows0_only else Q_SCALE * u[p])
            s = qs @ u.T / np.sqrt(hd)                             # float64 scores, scaled as the kernels scale them
            idx = np.arange(s.shape[0])
            hit = s[idx, p[:s.shape[0]]].copy()
            s[idx, p[:s.shape[0]]] = -np.inf
            if N > 1:
                gap = min(gap, float((hit - s.max(axis=1)).min()))
    return qkv.reshape(n_img * N, 3 * D), perm, gap


def routed(qkv: np.ndarray, perm: np.ndarray, n_img: int, N: int, H: int, hd: int) -> np.ndarray:
    """The one correct attention output [n_img * N][H * hd]: row i of (image, head) is v[p(i)]."""
    v = qkv.reshape(n_img, N, 3, H, hd)[:, :, 2]                  # [n_img][N][H][hd]
    out = np.empty_like(v)
    for b in range(n_img):
        for h in range(H):
            out[b, :, h] = v[b, perm[b, h], h]
    return out.reshape(n_img * N, H * hd)


# family -> [(n_img, N, H, head_dim)], at the token counts the existing tests of each family use (tests/test_gpu_kernels.py, test_gpu_parity_r02.py,
# _r04.py, test_gpu_r05.py, test_gpu_head_dims.py, test_gpu_cls_tail.py), N lowered for the small head dimensions until the gap holds
ATTN_CASES = {
    "auto": [(2, 197, 3, 64), (3, 17, 2, 64), (1, 257, 2, 64), (1, 577, 2, 64), (2, 50, 1, 64), (1, 785, 2, 64)],
    "single": [(2, 197, 3, 64), (3, 17, 2, 64), (1, 257, 2, 64), (1, 577, 2, 64), (2, 224, 1, 64), (1, 608, 1, 64)],
    "flow": [(2, 197, 3, 64), (1, 577, 2, 64), (2, 300, 1, 64), (1, 785, 2, 64), (3, 17, 2, 64), (1, 4097, 1, 64)],
    "persist": [(45, 197, 12, 64), (3, 208, 2, 64), (2, 224, 3, 64), (2, 193, 3, 64), (2, 215, 3, 64)],
    "stream": [(1, 577, 2, 64), (2, 197, 3, 64), (1, 785, 2, 64), (2, 300, 1, 64), (3, 225, 2, 64), (1, 1025, 1, 64), (2, 129, 2, 64), (9, 65, 1, 64),
               (2, 64, 3, 64), (1, 1, 1, 64), (4, 33, 2, 64), (1, 31, 1, 64), (1, 4097, 1, 64)],
    "precise": [(2, 197, 3, 64), (1, 577, 2, 64), (3, 17, 2, 64), (1, 1, 1, 64), (2, 65, 2, 64), (1, 128, 1, 64), (1, 129, 3, 64), (1, 257, 2, 64),
                (1, 785, 1, 64), (1, 1025, 1, 64), (23, 208, 12, 64)],
    "generic": [(3, 17, 2, 32), (2, 50, 2, 32), (2, 197, 2, 80), (1, 257, 3, 80), (1, 50, 4, 96), (2, 65, 1, 128), (1, 300, 2, 128)],
    "cls": [(7, 197, 12, 64), (3, 577, 16, 64), (5, 50, 3, 64), (4, 65, 8, 32), (2, 197, 2, 128), (3, 7, 4, 16), (9, 1, 2, 64), (2, 785, 1, 64)],
    "map": [(2, 197, 3, 64), (1, 577, 2, 64), (3, 17, 2, 32), (2, 65, 1, 128), (1, 50, 4, 96), (2, 197, 2, 80)],
}


def attn_seed(n_img: int, N: int, H: int, hd: int) -> int:
    return N if (n_img, H, hd) == (1, 1, 64) else N + 1000 * n_img + 100000 * H + 7 * hd


def dominant_qkv(n_img: int, N: int, H: int, hd: int, seed: int) -> np.ndarray:
    """randn * 0.8 q, k, v with one key row and one query row per image scaled by 30: scores in the hundreds, both signs."""
    rng = np.random.default_rng(seed)
    D = H * hd
    x = (rng.standard_normal((n_img, N, 3 * D)) * 0.8).astype(np.float32)
    for b in range(n_img):
        x[b, rng.integers(0, N), D:2 * D] *= 30.0
        x[b, rng.integers(0, N), :D] *= 30.0
    return x.reshape(n_img * N, 3 * D)


def attention64(qkv: np.ndarray, n_img: int, N: int, H: int, hd: int) -> np.ndarray:
    """Plain float64 softmax attention of the values given."""
    x = np.asarray(qkv, np.float64).reshape(n_img, N, 3, H, hd)
    q, k, v = (x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))             # [n_img][H][N][hd]
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(hd)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    return (p @ v).transpose(0, 2, 1, 3).reshape(n_img * N, H * hd)


# ------------------------------------------------------------------------------------------------------------------
# Attention with a flat softmax: every key carries the same weight, and the output is still exact
# ------------------------------------------------------------------------------------------------------------------
FLAT_SIGNS = (-1, 0, 1)


def flat_gain(hd: int) -> int:
    return int(round(48.0 / np.sqrt(hd)))


def flat_qkv(n_img: int, N: int, H: int, hd: int, sign: int, seed: int):
    """qkv [n_img * N][3 * H * hd] f32 (exact in f16 and bf16) and c [n_img][H][hd]: the one correct output is c in every row.
    Per (image, head): every key is the same +-1 vector kappa; q_i = sign * g * kappa on a random half of the columns (another half for
    every query), g = flat_gain(hd), so every raw score of the item is the integer sign * g * hd / 2 (about sign * 24 after the scale)
    whatever the summation order, s - max = 0 and every numerator is 1; v_j = c + z_j with integer c in 1..3 per column and integer
    16 <= |z_j| <= 64 whose column sums vanish (pairs +a, -a; an odd N holds one triple a, b, -(a + b) with a, b <= 32), rows shuffled
    per column.  All partial sums of numerators and of numerator * v are integers below 2^24: sum p v = N c and sum p = N exactly.
    N = 1 leaves z = 0 (the only sum-free choice)."""
    rng = np.random.default_rng(seed)
    g = flat_gain(hd)
    qkv = np.zeros((n_img, N, 3, H, hd), np.float32)
    c = np.empty((n_img, H, hd), np.float32)
    for b in range(n_img):
        for h in range(H):
            kappa = rng.integers(0, 2, hd) * 2.0 - 1.0
            half = np.argsort(rng.random((N, hd)), axis=1) < hd // 2          # hd / 2 columns of every query
            cc = ((np.arange(hd) + rng.integers(0, 3)) % 3 + 1.0)[rng.permutation(hd)]
            z = np.zeros((N, hd))
            n_pair, odd = (N - 3) // 2 if N % 2 and N >= 3 else N // 2, N % 2 and N >= 3
            a = rng.integers(16, 65, (n_pair, hd))
            parts = [a, -a]
            if odd:
                t = rng.integers(16, 33, (2, hd)) * rng.choice([-1, 1], (1, hd))
                parts.append(np.concatenate([t, -t.sum(axis=0, keepdims=True)]))
            if N >= 2:
                z = rng.permuted(np.concatenate(parts), axis=0)
            qkv[b, :, 0, h] = sign * g * kappa * half; qkv[b, :, 1, h] = kappa; qkv[b, :, 2, h] = cc + z
            c[b, h] = cc
    return qkv.reshape(n_img * N, 3 * H * hd), c


def flat_expected(c: np.ndarray, N: int) -> np.ndarray:
    """[n_img * N][H * hd]: c of the row's image in every row."""
    n_img, H, hd = c.shape
    return np.repeat(c.reshape(n_img, 1, H * hd), N, axis=1).reshape(n_img * N, H * hd)


# family -> [(n_img, N, H, head_dim)] of the flat, spread and peaked cases: flat data needs no score gap, so every token count runs.  Each
# family meets N % 16 in {15, 0, 1} and N % 64 in {63, 0, 1} inside its own range with three images (first, middle, last) and two heads:
#   single   instantiated for ceil(N / 32) in {1 .. 7, 9, 19}: 1 .. 224, 257 .. 288, 577 .. 608 tokens (kAttnNkt, attention_single.hip);
#   persist  193 .. 224 tokens, 13 sixteen-key tiles up to 208 and 14 above; 215 = a partly filled fourteenth tile, odd head count;
#   flow / stream / precise  any count, 64-key chunks (precise: the persistent build for 193 .. 224, the two-pass build elsewhere);
#   auto     both sides of 192 | 193 (single -> persistent), 208 | 209 (13 -> 14 tiles), 224 | 225 (persistent -> pipelined),
#            256 | 257 (pipelined -> single), 288 | 289 (single -> pipelined);
#   generic  head dims 8 .. 128 other than 64, 16-key tiles, 32-key steps, 64-query workgroups;  cls / map  any count.
def _three(ns, H=2, hd=64):
    return [(3, n, H, hd) for n in ns]


_CHUNK_EDGES = (15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)
FLAT_CASES = {
    "auto": _three((192, 193, 208, 209, 224, 225, 256, 257, 288, 289, 577)) + [(2, 1, 2, 64)],
    "single": _three((15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 223, 224, 257, 271, 272, 273, 287, 288, 577, 591, 592, 593, 607, 608)),
    "flow": _three(_CHUNK_EDGES + (575, 576, 577, 1023, 1024, 1025)) + [(2, 4097, 2, 64)],
    "persist": _three((193, 197, 207, 208, 209, 223, 224)) + [(2, 215, 3, 64)],
    "stream": _three((1,) + _CHUNK_EDGES + (577, 1023, 1024, 1025)) + [(2, 4097, 2, 64)],
    "precise": _three((1,) + _CHUNK_EDGES + (197, 207, 208, 209, 223, 224, 225, 577, 1023, 1024, 1025)) + [(2, 215, 3, 64), (2, 4097, 2, 64)],
    "generic": _three((15, 16, 17, 197), hd=32) + _three((63, 64, 65, 257), hd=80) + _three((127, 128, 129), hd=96) + _three((31, 32, 33, 193), hd=128)
               + [(3, 50, 2, 16), (3, 49, 3, 8), (2, 1, 2, 32)],
    "cls": _three((1, 15, 16, 17, 255, 256, 257, 1025)) + _three((63, 64, 65), 4, 32) + _three((127, 128, 129), hd=128) + [(3, 197, 12, 64), (3, 577, 2, 16), (2, 4097, 2, 64)],
    "map": _three((15, 16, 63, 257)) + [(3, 17, 2, 32), (3, 64, 2, 128), (3, 65, 2, 80), (3, 197, 3, 64), (2, 577, 2, 64), (2, 1, 2, 64), (2, 1024, 2, 64)],
}
# Spread and peaked data run the same lists without the counts below 15 tokens: with one key the softmax is the constant 1, no scale can
# move it, and condition (c) of test_cpu_exact_data.py (a 2 % scale fault must break a gate) has nothing to act on.  The flat cases keep N = 1.
SPREAD_MIN_N = 15
SPREAD_CASES = {f: [c for c in cs if c[1] >= SPREAD_MIN_N] for f, cs in FLAT_CASES.items() if f != "map"}
SPREAD_MAX_N = 1025            # above it only "peaked" runs: see spread_kinds
CPU_FULL_MAX_N = 1025          # test_cpu_exact_data.py: above it the float64 conditions take the first 512 query rows of every item (minutes otherwise)


def spread_kinds(N: int):
    """The data kinds of a token count.  One key of 4097 carries 2.4e-4 of a spread row's weight, a sixteenth of bf16's unit round-off:
    no gate that lets the bf16 definition's own rounding through can see it leak (measured on the float64 reference: 0.26 of the bound,
    3.0 times the emulation's mean), so above 1025 tokens the data is sharpened instead of the condition being dropped."""
    return ("spread", "peaked") if N <= SPREAD_MAX_N else ("peaked",)


def spread_qkv(n_img: int, N: int, H: int, hd: int, seed: int, kind: str = "spread") -> np.ndarray:
    """randn * 0.8 q, k, v (a softmax over hundreds of keys); "peaked": q times 3 (an effective support of ten or so keys)."""
    D = H * hd
    x = (np.random.default_rng(seed).standard_normal((n_img * N, 3 * D)) * 0.8).astype(np.float32)
    if kind == "peaked":
        x[:, :D] *= 3.0
    elif kind != "spread":
        raise ValueError(kind)
    return x


# The gates of the spread / peaked tests (test_gpu_attention.py) and everything they are made of.  torch, on whatever device the operands
# are on: the GPU tests compute reference, bound and emulation in float64 / f32 on the device, the CPU conditions run the same code.
ATTN_K = 1                     # the k of the bound: smallest of 1, 2, 4 that leaves the emulation below half of the bound on every case
ATTN_MEAN_FACTOR = 3.0         # head-room of the mean gate over the emulation's own mean error: summation order, MFMA accumulation
ATTN_UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}       # unit round-off of the type numerators and exponent arguments are rounded to
ATTN_ULP = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7}        # one ulp of the output type, relative
LOG2E = 1.44269504088896340736


def heads_of(t, n_img: int, N: int, H: int, hd: int):
    """[n_img * N][3 * H * hd] -> q, k, v [n_img * H][N][hd]"""
    x = t.reshape(n_img, N, 3, H, hd).permute(2, 0, 3, 1, 4).reshape(3, n_img * H, N, hd)
    return x[0], x[1], x[2]


def rows_of(o, n_img: int, N: int, H: int, hd: int):
    """[n_img * H][N][hd] -> [n_img * N][H * hd]"""
    return o.reshape(n_img, H, N, hd).permute(0, 2, 1, 3).reshape(n_img * N, H * hd)


def attention_ref(q, k, v, scale: float, want_bound: bool = False):
    """float64 softmax attention of q [B][Nq][hd] against k, v [B][Nk][hd]; with want_bound also
    cond[b][i][d] = sum_j w_ij (2 + |s_ij - max_i|) |v_jd - out_id|: the first-order effect on out of a relative error on every weight and
    an absolute error proportional to |s - max| on every exponent argument (a constant v costs nothing: only its spread is charged)."""
    import torch
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.transpose(1, 2) * scale
    d = s - s.amax(dim=2, keepdim=True)
    w = torch.exp(d)
    w = w / w.sum(dim=2, keepdim=True)
    out = w @ v
    if not want_bound:
        return out
    a = w * (2.0 + d.abs())
    del s, d, w
    B, Nq, hd = out.shape
    cond = torch.empty_like(out)
    step = max(1, (1 << 25) // (B * k.shape[1] * hd))
    for i in range(0, Nq, step):
        cond[:, i:i + step] = (a[:, i:i + step, :, None] * (v[:, None, :, :] - out[:, i:i + step, None, :]).abs()).sum(dim=2)
    return out, cond


def attention_bound(ref, cond, dtype_name: str, k: int = ATTN_K):
    """|got - ref64| <= |ref64| * ulp_out + k * u * cond + 1e-7"""
    return ref.abs() * ATTN_ULP[dtype_name] + k * ATTN_UNIT[dtype_name] * cond + 1e-7


def attention_emu(q, k, v, scale: float, dtype_name: str, schedule: str = "single"):
    """f32 emulation of a family's DEFINITION (device_common.h AttnExp / AttnExpRt, the kernels' headers), not of a kernel's output:
    operands rounded to the type ("precise": the f32 values as they are -- two fp16 planes carry 22 bits of them), f32 raw scores,
      f16 / precise:  e = round16(exp2(round16(fma(s, scale, -(scale * max))) * log2 e)),
      bf16:           e = round_bf16(exp2(fma(s, kk, -(kk * max)))), kk = scale * log2 e,
    f32 row sum of the ROUNDED numerators, f32 P.V of the unnormalised numerators, (P.V) * (1 / sum) rounded once to the output type.
    schedule "online" (the bf16 pipelined kernel): keys in tiles of 32, queries in waves of 32 rows (rows past N repeat the last one);
    the subtracted constant is a RUNNING maximum that a wave moves, for all its rows at once, only when some row's tile maximum exceeds
    it by more than 8 / kk; sum and accumulators are then multiplied by exp2 of each row's own shift; numerators are rounded at the
    scale they have when formed.  What no emulation models: the order of the f32 sums and the MFMA's internal accumulation."""
    import torch
    f32 = torch.float32
    tdt = torch.float16 if dtype_name == "f16" else torch.bfloat16
    rnd = lambda x: x.to(tdt).to(f32)
    fma = lambda s, kk, nmx: (s.double() * kk + nmx.double()).to(f32)          # exact product and sum, one rounding
    if schedule == "precise":
        assert dtype_name == "f16"
        q, k, v = q.to(f32), k.to(f32), v.to(f32)
    else:
        q, k, v = rnd(q.to(f32)), rnd(k.to(f32)), rnd(v.to(f32))
    if dtype_name == "f16":
        kk = float(np.float32(scale))
        numer = lambda s, nmx: rnd(torch.exp2(rnd(fma(s, kk, nmx)) * float(np.float32(1.44269504))))
    else:
        kk = float(np.float32(scale) * np.float32(LOG2E))
        numer = lambda s, nmx: rnd(torch.exp2(fma(s, kk, nmx)))
    kk32 = torch.tensor(kk, dtype=f32, device=q.device)
    if schedule != "online":
        s = q @ k.transpose(1, 2)
        e = numer(s, -(kk32 * s.amax(dim=2, keepdim=True)))
        return rnd((e @ v) * (1.0 / e.sum(dim=2, keepdim=True)))
    assert dtype_name == "bf16"
    B, Nq, hd = q.shape
    nb = (Nq + 31) // 32
    qp = q[:, torch.arange(nb * 32, device=q.device).clamp(max=Nq - 1)].reshape(B, nb, 32, hd)
    mxs = torch.full((B, nb, 32, 1), -float("inf"), dtype=f32, device=q.device)
    nmx = torch.zeros_like(mxs); tot = torch.zeros_like(mxs)
    o = torch.zeros((B, nb, 32, hd), dtype=f32, device=q.device)
    tau = float(np.float32(8.0) / np.float32(kk))
    for t0 in range(0, k.shape[1], 32):
        kt, vt = k[:, None, t0:t0 + 32], v[:, None, t0:t0 + 32]
        s = qp @ kt.transpose(2, 3)
        tm = s.amax(dim=3, keepdim=True)
        move = (tm > mxs + tau).flatten(2).any(dim=2)[:, :, None, None]
        mnew = torch.maximum(mxs, tm)
        sc = torch.where(move, torch.exp2((mxs - mnew) * kk32), torch.ones_like(mxs))
        mxs = torch.where(move, mnew, mxs)
        nmx = -(kk32 * mxs)
        tot = tot * sc; o = o * sc
        e = numer(s, nmx)
        tot = tot + e.sum(dim=3, keepdim=True); o = o + e @ vt
    return rnd(o * (1.0 / tot)).reshape(B, nb * 32, hd)[:, :Nq]


def attention_schedule(family: str, dtype_name: str, N: int) -> str:
    """Which definition a family follows at a token count: the bf16 pipelined kernel (forced, or the automatic choice outside the
    single-pass and persistent ranges) keeps a running maximum; `precise` multiplies f32 values; everything else is single-pass."""
    if family == "precise":
        return "precise"
    single = (N + 31) // 32 in (1, 2, 3, 4, 5, 6, 7, 9, 19)
    if dtype_name == "bf16" and (family == "flow" or (family == "auto" and not (192 < N <= 224) and not (single and N <= 288))):
        return "online"
    return "single"


def attention_faults(q, k, v, scale: float, n_img: int, H: int):
    """The three faults the gates must see, applied to the float64 reference: {name: out64}.  leak: one more key, token 0 of the next
    image's same head (a zero key and value behind the last image: what a buffer load returns past the end); drop: the last key is
    missing; scale: the softmax scale 2 % too large."""
    import torch
    B, N, hd = k.shape
    nxt = lambda t: torch.cat([t.reshape(n_img, H, N, hd)[1:, :, :1], torch.zeros((1, H, 1, hd), dtype=t.dtype, device=t.device)]).reshape(B, 1, hd)
    return {"leak": attention_ref(q, torch.cat([k, nxt(k)], dim=1), torch.cat([v, nxt(v)], dim=1), scale),
            "drop": attention_ref(q, k[:, :-1], v[:, :-1], scale),
            "scale": attention_ref(q, k, v, scale * 1.02)}


def attention_gate_ratios(got, ref, bound, emu):
    """(worst |got - ref| / bound, mean|got - ref| / mean|emu - ref|): the test passes with the first <= 1 and the second <= ATTN_MEAN_FACTOR"""
    err = (got.double() - ref).abs()
    return float((err / bound).max()), float(err.mean() / (emu.double() - ref).abs().mean())


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm on hostile rows
# ------------------------------------------------------------------------------------------------------------------
ROW_KINDS = ("gauss", "outlier_ch", "outlier_tok", "offset", "const", "tinyvar", "zero", "tile_step", "huge", "small")
LN_WIDTHS = (64, 128, 192, 256, 384, 512, 768, 1024, 1280, 1536, 320, 448, 576, 640, 896, 1152, 1408, 1664, 2048)     # VITX_LN_WIDTHS (kernels.h)
LN_EPS = 1e-6


def hostile_rows(kind: str, M: int, D: int, seed: int = 0) -> np.ndarray:
    """M rows of one kind, f32.  Inputs beyond 1e18 are out of scope: the f32 square of a deviation overflows."""
    rng = np.random.default_rng(seed + 1000 * ROW_KINDS.index(kind) + D)
    g = rng.standard_normal((M, D)) * 0.7 + 0.1
    if kind == "gauss":
        x = g
    elif kind == "outlier_ch":
        x = g.copy(); x[:, [D // 3, D - 5]] *= 400.0              # two channels hundreds of times larger than the rest
    elif kind == "outlier_tok":
        x = g.copy(); x[::3] *= 200.0                             # every third token
    elif kind == "offset":
        x = g + 1000.0
    elif kind == "const":
        x = np.full((M, D), 3.25)                                 # padding rows
    elif kind == "tinyvar":
        x = 10.0 + 1e-4 * rng.standard_normal((M, D))
    elif kind == "zero":
        x = np.zeros((M, D))
    elif kind == "tile_step":
        x = g.copy(); x[:, :256] += 50.0                          # the first 256-column tile sits 50 above the others
    elif kind == "huge":
        x = g * 1e15
    elif kind == "small":
        x = g * 1e-20
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def hostile_matrix(D: int, rows_per_kind: int = 64, seed: int = 0):
    """All row kinds stacked: ([len(ROW_KINDS) * rows_per_kind][D] f32, the kind of every row)."""
    x = np.concatenate([hostile_rows(k, rows_per_kind, D, seed) for k in ROW_KINDS])
    return x, np.repeat(np.arange(len(ROW_KINDS)), rows_per_kind)


def ln_params(D: int, seed: int = 0):
    rng = np.random.default_rng(seed + D)
    return (1 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)


def layernorm64(x, w, b, eps: float = LN_EPS):
    """float64 LayerNorm and the statistics the bound needs: (y, rstd [M][1], max|x| per row [M][1])."""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    return (x - mean) * rstd * np.asarray(w, np.float64) + np.asarray(b, np.float64), rstd, np.abs(x).max(axis=1, keepdims=True)


def ln_cond(w, rstd, xmax):
    """The conditioning term of the bound: an f32 mean carries an error of a few 2^-24 max|x|, which rstd magnifies."""
    return np.abs(np.asarray(w, np.float64)) * rstd * xmax * 2.0 ** -21


def ln_bound(y64, w, rstd, xmax, ulp_out: float):
    """|y - y64| <= |y64| * ulp_out + |w| * rstd64 * max|x_row| * 2^-21 + 1e-6"""
    return np.abs(y64) * ulp_out + ln_cond(w, rstd, xmax) + 1e-6


def ln_tiled_f32(x: np.ndarray, w: np.ndarray, b: np.ndarray, eps: float = LN_EPS) -> np.ndarray:
    """f32 emulation of the tiled two-pass LayerNorm definition (ln_row.h): per 256-column tile a fixed tree for the sum and, around the
    tile's own mean, for the squared deviations; tiles merged in index order (equal counts).  Every operation rounds to f32."""
    f = np.float32
    x = np.asarray(x, f)
    M, D = x.shape
    assert D % 256 == 0 and 1 <= D // 256 <= 4
    NT = D // 256

    def tree(a):                                                   # a [M][NT][4 w][2 j][8 k]: piece values -> tile totals [M][NT]
        s = a[..., 0, :] + a[..., 1, :]                            # s(w, k)
        p = ((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])) + ((s[..., 4] + s[..., 5]) + (s[..., 6] + s[..., 7]))     # P(w)
        return ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]

    xt = x.reshape(M, NT, 4, 2, 8, 4)                              # piece 16 w + 8 j + k = 4 consecutive columns
    mc = tree((xt[..., 0] + xt[..., 1]) + (xt[..., 2] + xt[..., 3])) * f(1.0 / 256.0)
    d = xt - mc[:, :, None, None, None, None]
    d = d * d
    m2 = tree((d[..., 0] + d[..., 1]) + (d[..., 2] + d[..., 3]))
    sm, q = mc[:, 0].copy(), m2[:, 0].copy()
    for c in range(1, NT):
        sm = sm + mc[:, c]; q = q + m2[:, c]
    mean = sm / f(NT)
    dv = mc[:, 0] - mean
    ww = dv * dv
    for c in range(1, NT):
        dv = mc[:, c] - mean; ww = ww + dv * dv
    rstd = f(1.0) / np.sqrt((q + f(256.0) * ww) / f(D) + f(eps))
    y = ((x - mean[:, None]) * rstd[:, None]) * np.asarray(w, f) + np.asarray(b, f)
    assert y.dtype == np.float32
    return y


# ------------------------------------------------------------------------------------------------------------------
# GELU over its whole domain
# ------------------------------------------------------------------------------------------------------------------
def gelu_sweep(bf16_range: bool) -> np.ndarray:
    """+-0, +-2^-24 .. +-60000 on a geometric grid (8 points per octave), 4096 points in [-6, 6] and, for bf16, up to +-1e30; f32, padded with
    zeros to a multiple of 256 values."""
    top = np.log2(60000.0)
    mag = np.exp2(np.arange(-24 * 8, int(top * 8) + 1) / 8.0)
    mag = np.append(mag, 60000.0)
    if bf16_range:
        mag = np.append(mag, np.exp2(np.arange(16 * 8, int(np.log2(1e30) * 8) + 1) / 8.0))
    v = np.concatenate([[0.0, -0.0], mag, -mag, np.linspace(-6.0, 6.0, 4096)]).astype(np.float32)
    return np.concatenate([v, np.zeros(round_up(v.size, 256) - v.size, np.float32)])
