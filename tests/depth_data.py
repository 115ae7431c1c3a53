"""The depth head's tail restated in numpy (include/vitx.h "depth estimation"), shared by tests/test_cpu_depth.py -- which pins it to the host
function vitx_depth_host and to torch in mmseg's own order -- and tests/test_gpu_depth.py.

depth(...) is the header's arithmetic written independently of csrc/depth_bins.h, in f32 (numpy rounds every f32 operation on its own): the taps
c[cell][k] + o[img][k], the K planes resampled x u with dense_data.values (the axis arithmetic of "dense prediction"), then for k ascending
    r = v_k < 0 ? 0 : v_k;  p = r + 0.1;  S = S + p;  q = p * bins[k];  Tm = Tm + q;      fine = Tm / S
the fine plane resampled to out_h x out_w with the same arithmetic, and the clamp.  A NaN is returned as the quiet NaN 0x7fc00000, in both planes.

MUTANTS are the mistakes the tests must be able to see; depth(..., mutant=name) makes one of them:
    pad_leak          column K of the logit rows (the first pad column) is summed as one more bin
    last_dropped      bin K - 1 never takes part
    relu_after_eps    p = max(v + 0.1, 0): the clipping after the shift
    upsample_skipped  the bins are reduced on the coarse grid and one resize takes the result to the output
    clamp_missing     the depth map is not clamped
    xy_swapped        the x weights are applied along y and the y weights along x (the indices stay), in the fine plane
    offset_image0     every image takes image 0's offsets

hostile(...) builds logit rows [n gh gw][ld], offsets [n][ld] (a different row per image) and bins [K] with, where the shape has room: a NaN logit,
+inf (S and Tm both inf: a NaN depth), -inf (clipped to 0 -- but 0 * -inf = NaN where a weight is exactly 0), a cell where every v_k < 0 (the depth
there is the mean of the bins), a cell of values straddling +-0, cells whose depth lands below min_depth and above max_depth, and pad columns
K .. ld of +inf and NaN in the logits and in the offsets.
"""
import numpy as np

import dense_data as DD

MUTANTS = ("pad_leak", "last_dropped", "relu_after_eps", "upsample_skipped", "clamp_missing", "xy_swapped", "offset_image0")
F = np.float32
QNAN = np.uint32(0x7fc00000)
LO, HI = F(2.0), F(6.0)                        # the clamp of the hostile cases, inside the bins' range 0.5 .. 10

GRIDS = ((1, 1), (1, 5), (2, 3), (3, 5), (14, 14))
US = (1, 2, 4)
KS = (1, 2, 3, 4, 5, 64, 255, 256)


def widths(fw):
    """The output widths of a fine plane fw wide: around the 4-pixel pack and the 64-pixel tile, and a non-integer scale."""
    return sorted({w for w in (fw, fw + 1, fw + 3, 63, 64, 65, 3 * fw + 1) if w >= fw})


def cases():
    """(gh, gw, u, K, out_h, out_w, n): every grid with every u, the Ks and the widths cycling over them; every K and every width on one shape each;
    (14, 14) at u = 1 and K = 256 stages its window in more than one chunk of bins."""
    out = []
    i = 0
    for gh, gw in GRIDS:
        for u in US:
            fh, fw = u * gh, u * gw
            ws = widths(fw)
            out.append((gh, gw, u, KS[i % len(KS)], max(fh, 16 + (i & 1)), ws[i % len(ws)], 1 if gh * gw > 100 else 3))
            i += 1
    out.append((14, 14, 1, 256, 17, 14, 2))                                   # 14 x 14 cells x 256 bins: four chunks
    out.append((14, 14, 2, 256, 28, 65, 1))                                   # two chunks
    out.append((14, 14, 4, 256, 56, 56, 1))                                   # the published shape at 196 patches: one chunk, output = fine plane
    for K in KS:
        out.append((2, 3, 4, K, 17, 37, 3))
    for w in widths(12):
        out.append((2, 3, 4, 5, 16, w, 3))
        out.append((3, 5, 2, 64, 17, max(w, 10), 2))
    return out


def pad_to(K):
    """K_pad of the engine: K rounded up to 128."""
    return (K + 127) // 128 * 128


def bins_ud(K, lo=0.5, hi=10.0):
    return np.linspace(np.float64(lo), np.float64(hi), K).astype(F)


def _quiet(a):
    b = np.ascontiguousarray(a, F).view(np.uint32)
    return np.where(np.isnan(a), QNAN, b).astype(np.uint32)


def _reduce(v, bins, K, mutant=None):
    """[...][Ke] resampled logits -> Tm / S over the bins in ascending order."""
    S = np.zeros(v.shape[:-1], F); T = np.zeros(v.shape[:-1], F)
    last = K - 1 if (mutant == "last_dropped" and K > 1) else K
    ks = list(range(last)) + ([K] if mutant == "pad_leak" else [])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in ks:
            vk = v[..., k]
            if mutant == "relu_after_eps":
                p = np.where(vk + F(0.1) < 0, F(0.0), vk + F(0.1)).astype(F)
            else:
                r = np.where(vk < 0, F(0.0), vk).astype(F)                    # a NaN compares false: it stays
                p = (r + F(0.1)).astype(F)
            S = (S + p).astype(F)
            q = (p * F(bins[min(k, K - 1)])).astype(F)
            T = (T + q).astype(F)
        return (T / S).astype(F)


def depth(logits, offsets, bins, n, gh, gw, K, u, out_h, out_w, lo, hi, mutant=None):
    """(depth bits [n][out_h][out_w] u32, fine bits [n][u gh][u gw] u32)"""
    Ke = K + 1 if mutant == "pad_leak" else K
    P = np.asarray(logits, F).reshape(n, gh * gw, -1)[..., :Ke]
    with np.errstate(invalid="ignore", over="ignore"):
        if offsets is not None:
            o = np.asarray(offsets, F)[:, :Ke]
            if mutant == "offset_image0":
                o = np.broadcast_to(o[:1], o.shape)
            P = (P + o[:, None, :]).astype(F)
        P = np.ascontiguousarray(P).reshape(n * gh * gw, Ke)
        if mutant == "upsample_skipped":
            fh, fw = gh, gw
            fine = _reduce(P.reshape(n, gh, gw, Ke), bins, K, mutant)
        else:
            fh, fw = u * gh, u * gw
            fine = _reduce(DD.values(P, n, gh, gw, Ke, fh, fw, "xy_swapped" if mutant == "xy_swapped" else None), bins, K, mutant)
        fine = _quiet(fine).view(F)
        d = DD.values(fine.reshape(n * fh * fw, 1), n, fh, fw, 1, out_h, out_w)[..., 0]
        if mutant != "clamp_missing":
            d = np.where(d < F(lo), F(lo), np.where(d > F(hi), F(hi), d)).astype(F)
    return _quiet(d), _quiet(fine)


def hostile(n, gh, gw, K, ld, seed=0):
    """(logits [n gh gw][ld], offsets [n][ld], bins [K])"""
    rng = np.random.default_rng(seed)
    P = (rng.standard_normal((n, gh, gw, ld)) * 1.5).astype(F)
    off = (rng.standard_normal((n, ld)) * 0.25).astype(F)
    off[:, ::3] = F(0.0)                                                      # some exact zeros: a -0 tap stays -0 there
    cy, cx = gh // 2, gw // 2
    P[:, cy, cx, K // 2] = np.inf                                             # S and Tm both inf: NaN
    P[:, cy, gw - 1, (K // 2 + 1) % K] = -np.inf                              # clipped to 0; NaN where its weight is exactly 0
    if gh * gw > 1:
        P[:, gh - 1, 0, :K] = -np.abs(P[:, gh - 1, 0, :K]) - F(2.0)           # every v_k < 0 at the pixels that see this cell alone: the mean of the bins
        P[:, 0, gw - 1, :K] = np.array([-0.0, 0.0, -1e-30, 1e-30], F)[np.arange(K) % 4]      # straddling +-0
    if gh * gw > 2:
        P[:, 0, 0, :K] = F(-3.0); P[:, 0, 0, 0] = F(60.0)                     # the first bin alone: a depth below min_depth
        P[:, gh - 1, gw - 1, :K] = F(-3.0); P[:, gh - 1, gw - 1, K - 1] = F(60.0)     # the last bin alone: above max_depth
    if gh * gw > 4:
        P[0, 0, 1, 0] = np.nan                                                # a NaN logit
    P[..., K:] = np.where(np.arange(ld - K) % 2 == 0, F(np.inf), F(np.nan))   # the pad columns
    off[:, K:] = np.where(np.arange(ld - K) % 2 == 0, F(np.nan), F(np.inf))
    return P.reshape(n * gh * gw, ld), off, bins_ud(K)


def normal(n, gh, gw, K, ld, seed=0):
    """Ordinary data: |logit + offset| <= 4 (the condition of the bound in test_cpu_depth.py), NaN pad columns."""
    rng = np.random.default_rng(seed)
    P = np.clip(rng.standard_normal((n, gh, gw, ld)) * 1.2, -3.0, 3.0).astype(F)
    off = np.clip(rng.standard_normal((n, ld)) * 0.4, -1.0, 1.0).astype(F)
    P[..., K:] = np.nan; off[:, K:] = np.nan
    return P.reshape(n * gh * gw, ld), off, bins_ud(K)


# ---- the linear head on exact data (the GEMMs in front of the kernels) -----------------------------------------------------------------
def exact_head(rows, n, K, Dc, seed=0):
    """(a [rows][Dc], a_cls [n][Dc], wp [K][Dc], wc [K][Dc], bias [K]) f32 of small integers / 8 (dense_data.exact_head's rule: exact in fp16 and bf16,
    the f32 accumulation exact in any order)."""
    rng = np.random.default_rng(seed)
    g = lambda *s: (rng.integers(-8, 9, s) / 8.0).astype(F)
    assert Dc * 64 + 128 < 2 ** 24
    return g(rows, Dc), g(n, Dc), g(K, Dc), g(K, Dc), (rng.integers(-16, 17, K) / 8.0).astype(F)
