"""The dense head's label map restated in numpy (include/vitx.h "dense prediction"), shared by tests/test_cpu_dense.py -- which pins it to the host
function vitx_dense_labels_host and to torch's F.interpolate -- and tests/test_gpu_dense.py.

labels(...) is the header's arithmetic written independently of csrc/dense_resample.h: per axis, in f32 (numpy rounds every f32 operation on its own),
    scale = f32(g) / f32(out);  s = (f32(o) + 0.5) * scale - 0.5, clamped below at 0;  i0 = int(s);  i1 = i0 + (i0 < g - 1);  l = s - f32(i0);  h = 1 - l
    top = hx a + lx b;  bot = hx c + lx d;  v = hy top + ly bot
and the winner in vitx_topk's order: value descending, class ascending, +0 and -0 tie, NaN last (a pixel of NaNs only: class 0).  A NaN score is
returned as the quiet NaN 0x7fc00000.

MUTANTS are the mistakes the tests must be able to see; labels(..., mutant=name) makes one of them:
    pad_leak       column K of the logit rows (the first pad column) takes part in the comparison
    last_dropped   class K - 1 never takes part
    tie_high       among equal values the HIGHER class index wins
    clamp_g2       the first source index is clamped at g - 2 (the last cell is reached through i1 only)
    xy_swapped     the x weights are applied along y and the y weights along x (the indices stay)

hostile(...) builds logit rows [n gh gw][ld] with, where the shape has room: two equal planes on top of a region (exact ties after resampling too), a
cell of alternating -0 / +0, a NaN plane in image 0 (class 0, K >= 2), a cell of NaNs only in the last image, +inf and -inf entries (0 * inf = NaN at
the pixels whose weight is exactly 0), one cell in the far corner that only the LAST class wins, and pad columns K .. ld filled with +inf and NaN.
"""
import numpy as np

MUTANTS = ("pad_leak", "last_dropped", "tie_high", "clamp_g2", "xy_swapped")
F = np.float32

# (gh, gw) -> (out_h, out_w), K, images: every grid at scale 1 and x 16, the non-integer ratios, the widths around the 4-pixel pack and the 64-pixel
# tile, every K on one shape.  (16, 37) x 16 is several tiles wide and high; K = 150 and 256 at scale 1 on (14, 14) stage the window in class chunks.
GRIDS = ((1, 1), (1, 5), (2, 3), (14, 14), (16, 37))
KS = (1, 2, 21, 128, 129, 150, 256)
WIDTHS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65)


def cases():
    out = []
    for i, (gh, gw) in enumerate(GRIDS):
        out.append((gh, gw, gh, gw, KS[i % len(KS)], 3))                       # scale 1
        out.append((gh, gw, 16 * gh, 16 * gw, KS[(i + 3) % len(KS)], 1 if gh * gw > 100 else 3))     # x 16
    out.append((14, 14, 37, 37, 21, 3))
    out.append((3, 5, 224, 17, 150, 1))
    out.append((14, 14, 14, 14, 150, 1))                                       # 15 x 15 cells x 152 floats: more than one class chunk
    out.append((16, 37, 16, 37, 256, 3))                                       # scale 1, a window of 17 x 38 cells, 256 classes
    for j, w in enumerate(WIDTHS):
        out.append((1, 1, 2, w, KS[j % len(KS)], 3))
        if w >= 3:
            out.append((2, 3, 5, w, KS[(j + 2) % len(KS)], 1 + 2 * (j & 1)))
    for K in KS:
        out.append((2, 3, 32, 48, K, 3))
    return out


def pad_to(K):
    """K_pad of the engine: K rounded up to 128."""
    return (K + 127) // 128 * 128


def rank(v):
    """topk_rank.h: 0 for a NaN, else the value's bits made monotone (-0 + 0 = +0 first)."""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        b = (v + F(0.0)).view(np.uint32)
    r = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return np.where(np.isnan(v), np.uint32(0), r).astype(np.uint32)


def axis(g, out, mutant=None):
    o = np.arange(out, dtype=F)
    scale = F(g) / F(out)
    s = np.maximum((o + F(0.5)) * scale - F(0.5), F(0.0))
    i0 = s.astype(np.int32)
    if mutant == "clamp_g2" and g >= 2:
        i0 = np.minimum(i0, g - 2)
    i1 = i0 + (i0 < g - 1)
    l = (s - i0.astype(F)).astype(F)
    h = (F(1.0) - l).astype(F)
    return i0, i1, l, h


def values(logits, n, gh, gw, K, out_h, out_w, mutant=None):
    """v [n][out_h][out_w][K] f32: the K planes resampled."""
    P = np.asarray(logits, F).reshape(n, gh, gw, -1)[..., :K]
    y0, y1, ly, hy = axis(gh, out_h, mutant)
    x0, x1, lx, hx = axis(gw, out_w, mutant)
    wy_h, wy_l, wx_h, wx_l = hy[None, :, None, None], ly[None, :, None, None], hx[None, None, :, None], lx[None, None, :, None]
    if mutant == "xy_swapped":
        wy_h, wx_h, wy_l, wx_l = wx_h, wy_h, wx_l, wy_l
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = P[:, y0][:, :, x0], P[:, y0][:, :, x1]
        c, d = P[:, y1][:, :, x0], P[:, y1][:, :, x1]
        top = (wx_h * a).astype(F) + (wx_l * b).astype(F)
        bot = (wx_h * c).astype(F) + (wx_l * d).astype(F)
        return ((wy_h * top).astype(F) + (wy_l * bot).astype(F)).astype(F)


def labels(logits, n, gh, gw, K, out_h, out_w, mutant=None):
    """(labels [n][out_h][out_w] u8, score bits [n][out_h][out_w] u32)"""
    Ke = K + 1 if mutant == "pad_leak" else K
    v = values(logits, n, gh, gw, Ke, out_h, out_w, mutant)
    r = rank(v)
    if mutant == "last_dropped" and K > 1:
        r = r[..., :K - 1]
    if mutant == "tie_high":
        win = r.shape[-1] - 1 - np.argmax(r[..., ::-1], axis=-1)
    else:
        win = np.argmax(r, axis=-1)                    # the first of equal ranks: the lowest class; all ranks 0 (NaNs only): class 0
    sc = np.take_along_axis(v, win[..., None], axis=-1)[..., 0]
    bits = np.where(np.isnan(sc), np.uint32(0x7fc00000), sc.view(np.uint32))
    return win.astype(np.uint8), bits.astype(np.uint32)


def hostile(n, gh, gw, K, ld, seed=0):
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((n, gh, gw, ld)).astype(F)
    if K >= 3:                                          # two equal planes on top of the left part: class 1 must win there, not class K - 1
        w = gw // 2 + 1
        P[:, :, :w, 1] += F(3.0)
        P[:, :, :w, K - 1] = P[:, :, :w, 1]
    if K >= 2:
        P[:, 0, 0, :K] = np.where(np.arange(K) % 2 == 0, F(-0.0), F(0.0))      # a cell of zeros of both signs
        P[0, :, :, 0] = np.nan                          # a NaN plane: class 0 of image 0 never wins against a number
        P[:, gh // 2, gw // 2, K // 2] = np.inf
        P[:, gh // 2, gw - 1, (K // 2 + 1) % K] = -np.inf
    if gh * gw > 1:
        P[n - 1, gh - 1, 0, :K] = np.nan                # a cell of NaNs only: the pixels that see nothing else get class 0
        P[:, gh - 1, gw - 1, :K] -= F(8.0)
        P[:, gh - 1, gw - 1, K - 1] = F(9.0)            # the far corner belongs to the last class alone
    P[..., K:] = np.where(np.arange(ld - K) % 2 == 0, F(np.inf), F(np.nan))   # the pad columns
    return P.reshape(n * gh * gw, ld)


def normal(n, gh, gw, K, ld, seed=0):
    P = np.random.default_rng(seed).standard_normal((n, gh, gw, ld)).astype(F)
    P[..., K:] = np.nan
    return P.reshape(n * gh * gw, ld)


# ---- the linear head on exact data (the GEMM in front of the label kernel) -------------------------------------------------------------
def exact_head(rows, K, Dc, seed=0):
    """(a [rows][Dc], w [K][Dc], bias [K]) f32 of small integers / 8: exact in fp16 and bf16, every product a multiple of 1/64 and every partial sum
    below 2^24 / 64 -- the f32 accumulation is exact in any order, so numpy's float64 product rounded to f32 is the GEMM's result bit for bit."""
    rng = np.random.default_rng(seed)
    a = (rng.integers(-8, 9, (rows, Dc)) / 8.0).astype(F)
    w = (rng.integers(-8, 9, (K, Dc)) / 8.0).astype(F)
    bias = (rng.integers(-16, 17, K) / 8.0).astype(F)
    assert Dc * 64 + 128 < 2 ** 24
    return a, w, bias


def patch_logits64(a, w, bias):
    return a.astype(np.float64) @ w.astype(np.float64).T + bias.astype(np.float64)
