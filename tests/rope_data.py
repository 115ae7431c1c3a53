"""Files with rotary position embeddings (include/vitx.h "rotary position embeddings"), shared by tests/test_cpu_rope.py -- which pins the
restatement of such a file to transformers' DINOv3ViTModel -- and tests/test_gpu_rope.py.

What the family owns of the float64 restatement tests/ref64.py: the rotation of q and k of the patch rows in every layer (table64, rotate64), the
operation order of rope.hip in numpy f32, and the micro fixture.  With T = 1 + registers, patch p = (y, x) of a gh x gw grid, hd the head dim, theta
the file's rope[1]:
    cy = 2 (y + 0.5) / gh - 1, cx = 2 (x + 0.5) / gw - 1, inv_j = theta^(-4 j / hd) for j < hd / 4
    angle[p][j] = 2 pi cy inv_j, angle[p][hd / 4 + j] = 2 pi cx inv_j                                  (hd / 2 columns)
    a = q[.., j], b = q[.., hd / 2 + j]:  a' = a cos - b sin,  b' = b cos + a sin                        (k alike; rows 0 .. T - 1 untouched)
The position table of such a file is all zero; the restatement adds it like any other.

MUTANTS are the mistakes the tests must be able to see; ref64.forward64(..., mutant=name) makes one of them:
    no_rope         nothing is rotated
    xy_swapped      the first quarter of the columns takes cx, the second cy
    sin_negated     the rotation runs the other way
    rope_on_prefix  the prefix rows are rotated too (prefix row t with the table row of patch t)
    wrong_grid      the coordinates of a (gh + 1) x (gw + 1) grid (its first gh rows and gw columns)

The micro fixture (fixture_tensors; D 128, 2 layers, 2 heads of 64, patch 14, image 56, 4 registers: N = 21; erf-GELU, eps 1e-5; zero pos_embed):
pkg.synth.make_weights with the q and k rows of every attn.qkv.weight and attn.qkv.bias multiplied by QK_SCALE.  make_weights draws every matrix at
0.02: q . k / sqrt(hd) then stays within a few hundredths, every softmax is nearly uniform and position information of any kind moves the stream by
less than the operand rounding does.  The factor makes the scores of unit size.  It is chosen so that BOTH of these hold, computed by
tests/test_cpu_rope.py::test_fixture_separates_the_mutants_from_operand_rounding and not assumed (the gates are tests/ref64.py's; the chosen
value and the measured distances stand at QK_SCALE below):
    the operand-rounded restatement lies inside HALF a gate of the unrounded one, and every mutant more than TWICE a gate away."""
import numpy as np

import arch_data as AD

MUTANTS = ("no_rope", "xy_swapped", "sin_negated", "rope_on_prefix", "wrong_grid")
MICRO = AD.MICRO
REGISTERS = 4
THETA = 100.0
# Chosen and measured by test_fixture_separates_the_mutants_from_operand_rounding on the 17 images of the GPU tests, per stage (layer 1, layer 2) as
# (max|d| / rms, rms(d) / rms); the gates are fp16 (2.5e-2, 2e-3), bf16 rms 2.5e-2, probabilities 1e-3 / 2e-2:
#   rounded against unrounded   fp16 (2.9e-4, 4e-5) (5.9e-4, 6e-5), max|dprob| 2.4e-4;  bf16 (7.8e-3, 1.6e-3) (8.0e-3, 1.7e-3), max|dprob| 3.4e-3
#   no_rope          (0.33, 0.050) (0.52, 0.073), max|dprob| 0.28        xy_swapped  (0.38, 0.051) (0.47, 0.076), max|dprob| 0.36
#   sin_negated      (0.34, 0.054) (0.54, 0.079), max|dprob| 0.38        wrong_grid  (0.28, 0.033) (0.37, 0.051), max|dprob| 0.35
#   rope_on_prefix   (0.39, 0.040) (0.51, 0.059), max|dprob| 0.38        (the mutants' figures are the same in both operand types to two digits)
# At 6 the mutants are half as far (wrong_grid: rms 0.013 / 0.019, inside twice the bf16 stage gate; max|dprob| 0.13); rounding q and k to bf16
# around the rotation, which the restatement does not model, costs rms 3.5e-4 / 6.5e-4 at 12: a fortieth of the gate.
QK_SCALE = 12.0


def table64(theta, hd, gh, gw, mutant=None):
    """(cos, sin), float64 [gh * gw][hd / 2], row-major over (y, x)."""
    if mutant == "wrong_grid":
        c, s = table64(theta, hd, gh + 1, gw + 1)
        keep = (np.arange(gh)[:, None] * (gw + 1) + np.arange(gw)[None, :]).reshape(-1)
        return c[keep], s[keep]
    q = hd // 4
    inv = np.float64(theta) ** (-4.0 * np.arange(q) / hd)
    cy = 2.0 * (np.arange(gh) + 0.5) / gh - 1.0
    cx = 2.0 * (np.arange(gw) + 0.5) / gw - 1.0
    ay = np.repeat(cy, gw)[:, None] * inv[None, :]
    ax = np.tile(cx, gh)[:, None] * inv[None, :]
    ang = 2.0 * np.pi * (np.concatenate([ax, ay], 1) if mutant == "xy_swapped" else np.concatenate([ay, ax], 1))
    return np.cos(ang), (-np.sin(ang) if mutant == "sin_negated" else np.sin(ang))


def rotate64(x, cos, sin, T, mutant=None):
    """x [n][H][N][hd] float64 -> the same with rows T .. rotated by cos / sin [N - T][hd / 2]."""
    if mutant == "no_rope":
        return x
    half = x.shape[-1] // 2
    out = x.copy()

    def rot(rows, c, s):
        a, b = x[:, :, rows, :half], x[:, :, rows, half:]
        out[:, :, rows, :half] = a * c - b * s
        out[:, :, rows, half:] = b * c + a * s

    rot(slice(T, None), cos, sin)
    if mutant == "rope_on_prefix":
        rot(slice(0, T), cos[:T], sin[:T])
    return out


def rope_of(t):
    """theta of a file's `rope` tensor (kind 1), or None."""
    if "rope" not in t:
        return None
    r = np.asarray(t["rope"], np.float32).reshape(-1)
    assert r[0] == 1 and r[2] == 0 and r[3] == 0
    return float(r[1])


# ------------------------------------------------------------------------------------------------ the operation order of rope.hip in numpy f32
def rope_f32(a, b, c, s):
    """a' = a c - b s, b' = b c + a s with every product and each sum rounded to f32 (numpy f32 arithmetic never fuses)."""
    a, b, c, s = (np.asarray(v, np.float32) for v in (a, b, c, s))
    return (a * c).astype(np.float32) - (b * s).astype(np.float32), (b * c).astype(np.float32) + (a * s).astype(np.float32)


def to_bits16(x, dtype):
    """f32 -> the operand type's bits (uint16), round to nearest even: 0 fp16, 1 bf16."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == 0:
        return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def from_bits16(b, dtype):
    b = np.ascontiguousarray(b, np.uint16)
    if dtype == 0:
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def split_hilo(v):
    """f32 -> (hi, lo) fp16 bits as the qkv GEMM's two-plane epilogue splits: hi = RNE(v), lo = RNE((v - hi) 2048)."""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)).astype(np.float32) * np.float32(2048.0)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def rope_bits(qkv, cos, sin, n_img, N, prefix, D, H, dtype, lo=None):
    """What vitx_op_rope must leave in qkv [rows >= n_img * N][3 D] (uint16 bits of `dtype`; lo: the parity mode's second plane, fp16) for the
    f32 tables cos / sin [N - prefix][hd / 2]: the numpy-f32 restatement, bit for bit.  Returns the new plane(s)."""
    hd = D // H; half = hd // 2
    out = qkv.copy(); out_lo = None if lo is None else lo.copy()
    view = lambda a: a[:n_img * N].reshape(n_img, N, 3, H, hd)[:, prefix:, :2]      # [n][P][q|k][H][hd]
    x = from_bits16(view(qkv), dtype)
    if lo is not None:
        x = (x + (from_bits16(view(lo), 0) * np.float32(1.0 / 2048.0)).astype(np.float32)).astype(np.float32)
    c = np.asarray(cos, np.float32)[None, :, None, None, :]; s = np.asarray(sin, np.float32)[None, :, None, None, :]
    ra, rb = rope_f32(x[..., :half], x[..., half:], c, s)
    r = np.concatenate([ra, rb], -1)
    if lo is None:
        view(out)[...] = to_bits16(r, dtype)
        return out
    hi_b, lo_b = split_hilo(r)
    view(out)[...] = hi_b; view(out_lo)[...] = lo_b
    return out, out_lo


# ------------------------------------------------------------------------------------------------ the micro fixture
def fixture_tensors(pkg, name=MICRO, qk_scale=QK_SCALE, rope=True):
    """make_weights with 4 registers + `arch` {erf, 1e-5} + `rope` {1, 100} in the converter's order, a zero pos_embed, q and k rows times qk_scale.
    rope=False: the same file without the `rope` tensor (tools/rope_cost.py measures one against the other)."""
    hp = pkg.synth.hparams_for(name)
    w = pkg.synth.make_weights(hp, head_scale=4.0, registers=REGISTERS)
    D = hp.hidden_size
    out = {"arch": np.array([AD.ACT_ERF, 1e-5, 0, 0], np.float32)}
    if rope:
        out["rope"] = np.array([1, THETA, 0, 0], np.float32)
    for k, v in w.items():
        out[k] = v
    out["pos_embed"] = np.zeros_like(out["pos_embed"])
    f = np.float32(qk_scale)
    for i in range(hp.num_hidden_layers):
        for nm in (f"blocks.{i}.attn.qkv.weight", f"blocks.{i}.attn.qkv.bias"):
            a = out[nm].copy(); a[:2 * D] *= f; out[nm] = a
    return hp, out


def fixture_file(pkg, ftype=1, name=MICRO, rope=True):
    from ref64 import cached_file
    return cached_file(f"rope-{name}-s{QK_SCALE:g}-r{int(rope)}-ft{ftype}",
                       lambda tmp: pkg.ggml_file.write_model(tmp, *fixture_tensors(pkg, name, rope=rope), ftype=ftype))
