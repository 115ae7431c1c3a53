"""Rectangular images (include/vitx.h "rectangular contexts"), shared by tests/test_cpu_rect.py -- which pins the restatement to transformers' ViTModel,
Dinov2Model and DINOv3ViTModel on non-square inputs -- and tests/test_gpu_rect.py.

What the family owns of the float64 restatement tests/ref64.py: the patch rows of an [n][H][W][3] batch (patchify64), the position table of a
gh x gw grid (pos_table), the exact images, the fixtures and the shapes of the GPU tests:
    patch p = (py, px) = (p // gw, p % gw), raster order, x fastest; its pixels are rows py P .. py P + P - 1, columns px P .. px P + P - 1
    the position table is binding.pos_embed_resample (host) of the file's table at (gh, gw) whenever (gh, gw) != (g_in, g_in)
    the rope table is table64(theta, hd, gh, gw)

MUTANTS are the mistakes the tests must be able to see; ref64.forward64(..., mutant=name) makes one of them:
    grid_transposed  tokens laid out as gw x gh: token p holds the patch (p % gh, p // gh)
    square_pitch     the image row pitch is img_h instead of img_w pixels (read from the batch's memory, wrapping at its end)
    pos_transposed   the table is resampled to (gw, gh) and added in its own row order
    pos_square       the file's table is used without resampling: its class row and its first gh gw patch rows
    rope_transposed  (files with `rope`) the rotation table of a (gw, gh) grid in its own row order

The fixtures (fixture_tensors): pkg.synth.make_weights at head scale 4 of
    p16      vit_micro_patch16_64: P * Cin = 48, the patch embedding's 16-float gather
    p14r4    vit_micro_patch14_56 with 4 registers: P * Cin = 42, the per-element gather
    p14rope  rope_data.fixture_tensors (4 registers, zero pos_embed, `rope`, its own QK_SCALE)
make_weights draws pos_embed and every matrix at 0.02: position information then moves the stream by less than the operand rounding does (the note
at rope_data.QK_SCALE).  p16 and p14r4 therefore multiply pos_embed by POS_SCALE and the q and k rows of every attn.qkv.weight / bias by QK_SCALE.
Both factors are chosen so that, on the GPU tests' own images and shapes (CASES), the operand-rounded restatement lies inside HALF a gate of
tests/ref64.py of the unrounded one and every mutant more than TWICE a gate away: computed by
tests/test_cpu_rect.py::test_fixture_separates_the_mutants_from_operand_rounding, not assumed."""
import numpy as np

import rope_data as RD

MUTANTS = ("grid_transposed", "square_pitch", "pos_transposed", "pos_square")
ROPE_MUTANTS = ("grid_transposed", "square_pitch", "rope_transposed")
REGISTERS = 4
FIXTURES = {"p16": ("vit_micro_patch16_64", 0), "p14r4": ("vit_micro_patch14_56", REGISTERS), "p14rope": ("vit_micro_patch14_56", REGISTERS)}
HEADS = 2
# fixture, (img_h, img_w): the shapes of the GPU forward tests
CASES = (("p14r4", (28, 70)), ("p14r4", (70, 28)), ("p14rope", (28, 70)), ("p14rope", (70, 28)), ("p16", (48, 80)))
# Chosen and measured by test_fixture_separates_the_mutants_from_operand_rounding on the 17 images of the GPU tests (images(17, h, w)), worst case
# over CASES, per stage (layer 1, layer 2) as (max|d| / rms, rms(d) / rms); the gates are fp16 (2.5e-2, 2e-3), bf16 rms 2.5e-2, probabilities
# 1e-3 / 2e-2.  The measured figures stand in MEASURED below, written by hand from that test's output.
POS_SCALE = 25.0
QK_SCALE = 12.0
MEASURED = """
rounded against unrounded, worst over CASES:  fp16 (4.2e-4, 4e-5) (1.4e-3, 8e-5), max|dprob| 3.5e-4;  bf16 (9.8e-3, 1.7e-3) (1.2e-2, 1.9e-3), max|dprob| 3.2e-3
nearest mutant per kind (the same in both operand types to two digits), fixtures p14r4 / p16:
    grid_transposed  (5.6, 1.2) (5.7, 1.2)         square_pitch  (6.3, 1.3) (6.3, 1.3)
    pos_transposed   (1.5, 0.37) (1.6, 0.37)       pos_square    (1.6, 0.45) (1.7, 0.45)       max|dprob| 0.023 .. 0.064
fixture p14rope:
    grid_transposed  (6.6, 1.3) (6.6, 1.3)         square_pitch  (7.6, 1.4) (7.4, 1.4)
    rope_transposed  (0.29, 0.049) (0.43, 0.074)   max|dprob| 0.19 .. 0.40
At QK_SCALE 6 the probabilities of the mutants move by 0.010 .. 0.045 only (the traces stay as far); at POS_SCALE 50 the pos mutants are 1.7 times as far
and the others a seventh nearer: 25 and 12 keep every figure an order of magnitude from its gate.
"""


def mutants_of(t):
    return ROPE_MUTANTS if "rope" in t else MUTANTS


def _binding():
    import _pkg
    _pkg.load()
    from vitcpp_amd import binding
    return binding


def images(n, h, w, seed=1):
    """[n][h][w][3] f32 images whose pixels are multiples of 1/16 in [-4, 4) (prefix_data.exact_images on a rectangle): exact in bf16 and fp16."""
    return (np.random.default_rng(seed + 1000 * h + w).integers(-64, 64, (n, h, w, 3)) / 16.0).astype(np.float32)


def patchify64(px, P, mutant=None):
    """px [n][H][W][3] float64 -> [n][gh gw][3 P P] patch rows in raster order, each in the file kernel's order [c][ky][kx]."""
    n, Hh, Ww, _ = px.shape
    gh, gw = Hh // P, Ww // P
    if mutant == "square_pitch":
        flat = px.reshape(-1)
        b, y, x, c = np.meshgrid(np.arange(n), np.arange(Hh), np.arange(Ww), np.arange(3), indexing="ij")
        px = flat[((b * Hh * Ww + y * Hh + x) * 3 + c) % flat.size]
    pt = px.reshape(n, gh, P, gw, P, 3).transpose(0, 1, 3, 5, 2, 4).reshape(n, gh, gw, 3 * P * P)
    if mutant == "grid_transposed":
        return pt.transpose(0, 2, 1, 3).reshape(n, gh * gw, -1)      # token p = (p // gh, p % gh) read as (x, y)
    return pt.reshape(n, gh * gw, -1)


def pos_table(t, gh, gw, mutant=None, binding=None, interp=0):
    """The [1 + gh gw][D] f32 table of a rect context: the file's resampled on the host (binding.pos_embed_resample), or a mutant's."""
    pos = np.ascontiguousarray(t["pos_embed"][0], np.float32)
    g_in = int(round((pos.shape[0] - 1) ** 0.5))
    assert pos.shape[0] == 1 + g_in * g_in
    if mutant == "pos_square":
        assert gh * gw <= g_in * g_in
        return pos[:1 + gh * gw]
    if mutant == "pos_transposed":
        gh, gw = gw, gh
    if (gh, gw) == (g_in, g_in):
        return pos
    return (binding or _binding()).pos_embed_resample(pos, (gh, gw), interp, grid_in=(g_in, g_in))


# ------------------------------------------------------------------------------------------------ the fixtures
def fixture_tensors(pkg, kind, pos_scale=POS_SCALE, qk_scale=QK_SCALE):
    name, registers = FIXTURES[kind]
    if kind == "p14rope":
        return RD.fixture_tensors(pkg, name)
    hp = pkg.synth.hparams_for(name)
    out = dict(pkg.synth.make_weights(hp, head_scale=4.0, registers=registers))
    D = hp.hidden_size
    out["pos_embed"] = (out["pos_embed"] * np.float32(pos_scale)).astype(np.float32)
    for i in range(hp.num_hidden_layers):
        for nm in (f"blocks.{i}.attn.qkv.weight", f"blocks.{i}.attn.qkv.bias"):
            a = out[nm].copy(); a[:2 * D] *= np.float32(qk_scale); out[nm] = a
    return hp, out


def fixture_file(pkg, kind, ftype=1):
    """Path of the (cached) model file of a fixture."""
    from ref64 import cached_file
    return cached_file(f"rect-{kind}-p{POS_SCALE:g}-q{QK_SCALE:g}-ft{ftype}", lambda tmp: pkg.ggml_file.write_model(tmp, *fixture_tensors(pkg, kind), ftype=ftype))
