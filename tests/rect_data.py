"""Float64 restatement of the forward on a rectangular image (include/vitx.h "rectangular contexts"), shared by tests/test_cpu_rect.py -- which pins
it to transformers' ViTModel, Dinov2Model and DINOv3ViTModel on non-square inputs -- and tests/test_gpu_rect.py.

It is tests/arch_data.py::forward64 (class token + register tokens, the file's activation and epsilon, the `around` / `wround` / `uround` rounding
points) and, for a file with `rope`, tests/rope_data.py's rotation (qk64, table64), on a gh x gw grid of an [n][H][W][3] batch:
    patch p = (py, px) = (p // gw, p % gw), raster order, x fastest; its pixels are rows py P .. py P + P - 1, columns px P .. px P + P - 1
    the position table is binding.pos_embed_resample (host) of the file's table at (gh, gw) whenever (gh, gw) != (g_in, g_in)
    the rope table is table64(theta, hd, gh, gw)

MUTANTS are the mistakes the tests must be able to see; forward64(..., mutant=name) makes one of them:
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
tests/test_gpu_arch.py of the unrounded one and every mutant more than TWICE a gate away: computed by
tests/test_cpu_rect.py::test_fixture_separates_the_mutants_from_operand_rounding, not assumed."""
import os

import numpy as np

import arch_data as AD
import prefix_data as PD
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


def forward64(t, imgs, heads=HEADS, mutant=None, around=None, wround=None, uround=None, binding=None, interp=0):
    """t: {name: f32 array, torch shapes} (prefix_data.file_tensors); imgs [n][H][W][3] f32, H and W multiples of the patch size.
    Returns dict(trace [L + 1][n][N][D], final [n][N][D], mean [n][D], q / k [L][n][H][N][hd] (after the rotation of a `rope` file), logits
    [n][C], probs [n][C]), N = gh gw + 1 + registers."""
    f8 = lambda a: np.asarray(a, np.float64)
    W = (lambda a: f8(wround(a))) if wround else f8
    U = (lambda a: f8(uround(a))) if uround else f8
    activation, eps, pre_norm = AD.arch_of(t)
    eps = float(np.float32(eps))
    theta = RD.rope_of(t)
    D = t["cls_token"].shape[-1]
    R = t["reg_token"].shape[1] if "reg_token" in t else 0
    T = 1 + R
    L = 1 + max(int(k.split(".")[1]) for k in t if k.startswith("blocks."))
    P = t["patch_embed.proj.weight"].shape[-1]
    n, Hh, Ww = imgs.shape[:3]
    assert Hh % P == 0 and Ww % P == 0
    gh, gw = Hh // P, Ww // P
    hd = D // heads
    pos = f8(pos_table(t, gh, gw, mutant, binding, interp))
    assert pos.shape == (1 + gh * gw, D)
    if theta is not None:
        cos, sin = RD.table64(theta, hd, gw, gh) if mutant == "rope_transposed" else RD.table64(theta, hd, gh, gw)
    else:
        cos, sin = np.ones((gh * gw, hd // 2)), np.zeros((gh * gw, hd // 2))      # the identity: qk64 then is the plain projection
    patches = patchify64(f8(around(imgs) if around else imgs), P, mutant)
    emb = patches @ W(t["patch_embed.proj.weight"]).reshape(D, -1).T + f8(t["patch_embed.proj.bias"]).reshape(-1)
    x = np.empty((n, gh * gw + T, D))
    x[:, 0] = f8(t["cls_token"]).reshape(D) + pos[0]
    if R:
        x[:, 1:T] = f8(t["reg_token"][0])
    x[:, T:] = emb + pos[1:]
    if pre_norm:
        x = AD.layernorm64(x, f8(t["pre_norm.weight"]), f8(t["pre_norm.bias"]), eps)
    trace, qs, ks = [x.copy()], [], []
    for i in range(L):
        p = f"blocks.{i}."
        v = lambda name: f8(t[p + name])
        q, k, vv = RD.qk64(t, x, i, heads, cos, sin, None, wround, uround)
        s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(hd)
        a = np.exp(s - s.max(-1, keepdims=True)); a /= a.sum(-1, keepdims=True)
        o = U((a @ vv).transpose(0, 2, 1, 3).reshape(n, -1, D))
        x = x + o @ W(t[p + "attn.proj.weight"]).T + v("attn.proj.bias")
        h = U(AD.act64(U(AD.layernorm64(x, v("norm2.weight"), v("norm2.bias"), eps)) @ W(t[p + "mlp.fc1.weight"]).T + v("mlp.fc1.bias"), activation))
        x = x + h @ W(t[p + "mlp.fc2.weight"]).T + v("mlp.fc2.bias")
        trace.append(x.copy()); qs.append(q); ks.append(k)
    F = AD.layernorm64(x, f8(t["norm.weight"]), f8(t["norm.bias"]), eps)
    mean = PD.pooled64(F, T)
    hw = W(t["head.weight"])
    z = U(F[:, 0] if hw.shape[1] == D else np.concatenate([F[:, 0], mean], 1))
    logits = z @ hw.T + f8(t["head.bias"])
    e = np.exp(logits - logits.max(1, keepdims=True))
    return dict(trace=np.stack(trace), final=F, mean=mean, q=np.stack(qs), k=np.stack(ks), logits=logits, probs=e / e.sum(1, keepdims=True))


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
    cache_dir = os.environ.get("VITX_CACHE", "/tmp/vitx_cache")
    os.makedirs(cache_dir, exist_ok=True)
    path = os.path.join(cache_dir, f"rect-{kind}-p{POS_SCALE:g}-q{QK_SCALE:g}-ft{ftype}.gguf")
    if not os.path.exists(path):
        hp, t = fixture_tensors(pkg, kind)
        tmp = path + f".tmp{os.getpid()}"
        pkg.ggml_file.write_model(tmp, hp, t, ftype=ftype)
        os.replace(tmp, path)
    return path
