"""The float64 restatement of the forward, once, for every model family (include/vitx.h), with the gates the end-to-end GPU tests hold their results
to and the writer of the cached fixture files.  The CPU tests pin it to transformers family by family (tests/test_cpu_arch.py, _registers, _rope,
_swiglu, _rect, _map_head, _text); the GPU tests decide pass or fail against it.

What a file is gets read from its tensors:
    arch            activation and the epsilon of every LayerNorm (arch_data.arch_of; absent: tanh-GELU, 1e-6)
    pre_norm.*      a LayerNorm of every token row in front of layer 0
    cls_token       a class row in front of the patches, or none; reg_token: R register rows behind it (no position embedding)
    rope            q and k of the patch rows are rotated in every layer (rope_data.table64, rotate64)
    glu             the gated MLP (swiglu_data.swiglu64); the `arch` activation is then not applied
    attn_pool.*     the attention-pooling head (map_data.head64) in place of the class / cls + mean head

Token layout of an image, T = class row + R, N = gh gw + T:
    row 0 (a class-token file)   cls_token + pos[0]
    the R rows behind it         reg_token[r]
    rows T .. N - 1              patch p + its position row, raster order
Rounding points, where the engine has them: `around` on the pixels, `wround` on every matrix, `uround` on the activations that enter a GEMM
(LayerNorm outputs, attention output, MLP activation output, the stored fc1 output of a gated MLP, the head operand).  All None: none anywhere.
The text tower also rounds the stored qkv (blocks64 round_qkv); the image towers do not.

`mutant=` makes one of the mistakes the tests must be able to see.  The names, their meaning and their measured distances stand with the family
that lists them (prefix_data.MUTANTS, rope_data.MUTANTS, swiglu_data.MUTANTS, rect_data.MUTANTS / ROPE_MUTANTS); a name that is unknown or that
cannot apply to the file raises ValueError."""
import os

import numpy as np

import arch_data as AD
import map_data as MD
import prefix_data as PD
import rect_data as XD
import rope_data as RD
import swiglu_data as SD
from arch_data import layernorm64  # noqa: F401  (the one definition; ref64.layernorm64 for callers)

# ------------------------------------------------------------------------------------------------ the gates of the end-to-end GPU tests
PROB_TOL = {0: 1e-3, 1: 2e-2}                      # max|dprob| by operand type (0 fp16, 1 bf16)
F16_STAGE = (2.5e-2, 2e-3)                         # max|d| / rms and rms(d) / rms of a trace stage
BF16_STAGE_RMS = 2.5e-2                            # bf16: rms(d) / rms alone (the bound against a reference without bf16 rounding points)


def stage_errors(x, ref):
    """[(max|d| / rms, rms(d) / rms)] of stages 1 .. of x, ref [L + 1][n][N][D]."""
    out = []
    for il in range(1, x.shape[0]):
        rms = float(np.sqrt((ref[il] ** 2).mean()))
        out.append((float(np.abs(x[il] - ref[il]).max()) / rms, float(np.sqrt(((x[il] - ref[il]) ** 2).mean())) / rms))
    return out


def stage_ok(e_max, e_rms, dtype, scale=1.0):
    """F16 e_max <= 2.5e-2 and e_rms <= 2e-3; BF16 e_rms <= 2.5e-2."""
    return (e_max <= scale * F16_STAGE[0] and e_rms <= scale * F16_STAGE[1]) if dtype == 0 else e_rms <= scale * BF16_STAGE_RMS


# ------------------------------------------------------------------------------------------------ the cached fixture files
def cached_file(stem, write):
    """Path of `stem`.gguf in the VITX_CACHE directory; a missing file is made by write(temporary path) and moved into place."""
    cache_dir = os.environ.get("VITX_CACHE", "/tmp/vitx_cache")
    os.makedirs(cache_dir, exist_ok=True)
    path = os.path.join(cache_dir, stem + ".gguf")
    if not os.path.exists(path):
        tmp = path + f".tmp{os.getpid()}"
        write(tmp)
        os.replace(tmp, path)
    return path


# ------------------------------------------------------------------------------------------------ the arithmetic
PREFIX_MUTANTS = PD.MUTANTS + ("pos_transposed", "pos_square")           # need a class token (and the table the class row leads)
ROPE_MUTANTS = RD.MUTANTS + ("rope_transposed",)                         # need `rope`
GLU_MUTANTS = SD.MUTANTS                                                 # need `glu`
GRID_MUTANTS = ("grid_transposed", "square_pitch")                       # any image tower


def check_mutant(t, mutant):
    """ValueError for a mutant name that is unknown or cannot apply to the file of tensors t."""
    for names, tensor in ((PREFIX_MUTANTS, "cls_token"), (ROPE_MUTANTS, "rope"), (GLU_MUTANTS, "glu")):
        if mutant in names:
            if tensor not in t:
                raise ValueError(f"mutant {mutant!r} needs a file with `{tensor}`")
            return
    if mutant is not None and mutant not in GRID_MUTANTS:
        raise ValueError(f"unknown mutant {mutant!r}")


def _rounders(wround, uround):
    f8 = lambda a: np.asarray(a, np.float64)
    return f8, (lambda a: f8(wround(a))) if wround else f8, (lambda a: f8(uround(a))) if uround else f8


def _pos_table(t, gh, gw, mutant, binding, interp):
    """rect_data.pos_table; the table of a file without a class token goes through it behind a class row of zeros."""
    if "cls_token" in t:
        return XD.pos_table(t, gh, gw, mutant, binding, interp)
    pos = np.asarray(t["pos_embed"][0], np.float32)
    return XD.pos_table({"pos_embed": np.concatenate([np.zeros_like(pos[:1]), pos])[None]}, gh, gw, None, binding, interp)[1:]


def qk64(t, x, i, heads, cos=None, sin=None, mutant=None, wround=None, uround=None, eps=None, round_qkv=False):
    """q, k and v, each [n][H][N][hd], of layer i from the residual stream x [n][N][D] that enters it; q and k rotated by cos / sin
    [N - T][hd / 2] when given (rope_data.table64).  eps None: the file's."""
    f8, W, U = _rounders(wround, uround)
    eps = float(np.float32(AD.arch_of(t)[1] if eps is None else eps))
    p = f"blocks.{i}."
    n, N, D = x.shape
    qkv = U(layernorm64(f8(x), f8(t[p + "norm1.weight"]), f8(t[p + "norm1.bias"]), eps)) @ W(t[p + "attn.qkv.weight"]).T + f8(t[p + "attn.qkv.bias"])
    if round_qkv:
        qkv = U(qkv)
    q, k, v = (qkv[..., j * D:(j + 1) * D].reshape(n, -1, heads, D // heads).transpose(0, 2, 1, 3) for j in range(3))
    if cos is None:
        return q, k, v
    T = N - cos.shape[0]
    return RD.rotate64(q, cos, sin, T, mutant), RD.rotate64(k, cos, sin, T, mutant), v


def blocks64(t, x, heads, activation, eps, glu=None, cos=None, sin=None, mask=None, mutant=None, wround=None, uround=None, round_qkv=False):
    """The layer stack on a residual stream x [n][N][D] float64.  Per layer: norm1, qkv, the rotation (cos / sin given), softmax(q k^T / sqrt(hd)
    + mask) v, proj, norm2, the MLP by `activation` or, glu = F, the gate.  round_qkv: the stored qkv is rounded with `uround` (the text tower).
    Returns (x after the last layer, trace [L + 1][n][N][D] of the stream entering each layer and leaving the last, q, k [L][n][H][N][hd])."""
    f8, W, U = _rounders(wround, uround)
    n, _, D = x.shape
    L = 1 + max(int(k.split(".")[1]) for k in t if k.startswith("blocks."))
    hd = D // heads
    trace, qs, ks = [x.copy()], [], []
    for i in range(L):
        p = f"blocks.{i}."
        v = lambda name: f8(t[p + name])
        q, k, vv = qk64(t, x, i, heads, cos, sin, mutant, wround, uround, eps, round_qkv)
        s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(hd)
        if mask is not None:
            s = s + mask
        a = np.exp(s - s.max(-1, keepdims=True)); a /= a.sum(-1, keepdims=True)
        o = U((a @ vv).transpose(0, 2, 1, 3).reshape(n, -1, D))
        x = x + o @ W(t[p + "attn.proj.weight"]).T + v("attn.proj.bias")
        y = U(layernorm64(x, v("norm2.weight"), v("norm2.bias"), eps))
        if glu is None:
            h = U(AD.act64(y @ W(t[p + "mlp.fc1.weight"]).T + v("mlp.fc1.bias"), activation))
        else:
            b1 = v("mlp.fc1.bias").copy()
            assert b1.shape == (2 * glu,) and t[p + "mlp.fc2.weight"].shape == (D, glu)
            if mutant == "up_bias_dropped":
                b1[glu:] = 0.0
            h = U(SD.swiglu64(U(y @ W(t[p + "mlp.fc1.weight"]).T + b1), glu, mutant))
        x = x + h @ W(t[p + "mlp.fc2.weight"]).T + v("mlp.fc2.bias")
        trace.append(x.copy()); qs.append(q); ks.append(k)
    return x, np.stack(trace), np.stack(qs), np.stack(ks)


def forward64(t, imgs, heads, pos=None, mutant=None, activation=None, eps=None, pre_norm=None, around=None, wround=None, uround=None,
              binding=None, interp=0, folded=True, flat=False):
    """t: {name: f32 array, torch shapes} (prefix_data.file_tensors); imgs [n][H][W][3] f32, H and W multiples of the patch size.
    pos: another position table than rect_data.pos_table's (the file's own at the file's grid, resampled by `binding` / `interp` elsewhere).
    activation / eps / pre_norm: None = the file's own; an attention-pooling file applies them to its head too, in the form `folded` / `flat`
    select (map_data.head64).  Returns dict(embed [n][N][D] (the rows in front of the pre-norm), trace [L + 1][n][N][D] (stage 0 enters layer
    0), final [n][N][D], mean [n][D], q / k [L][n][H][N][hd] after the rotation, logits [n][C], probs [n][C]) + e, M, p of map_data.head64."""
    f8, W, U = _rounders(wround, uround)
    check_mutant(t, mutant)
    pooling = "attn_pool.latent" in t
    if (flat or not folded) and not pooling:
        raise ValueError("flat / folded select the form of an attention-pooling head: the file has none")
    if pos is not None and mutant in ("pos_transposed", "pos_square"):
        raise ValueError(f"mutant {mutant!r} is a mistake in making the table: it cannot apply to a given one")
    f_act, f_eps, f_pre = AD.arch_of(t)
    activation = f_act if activation is None else activation
    eps = float(np.float32(f_eps if eps is None else eps))
    pre_norm = f_pre if pre_norm is None else pre_norm
    theta, glu = RD.rope_of(t), SD.glu_of(t)
    D = t["pos_embed"].shape[-1]
    c = int("cls_token" in t)
    R = t["reg_token"].shape[1] if "reg_token" in t else 0
    T = c + R
    P = t["patch_embed.proj.weight"].shape[-1]
    n, Hh, Ww = imgs.shape[:3]
    assert Hh % P == 0 and Ww % P == 0
    gh, gw = Hh // P, Ww // P
    G = gh * gw
    pos = f8(_pos_table(t, gh, gw, mutant, binding, interp) if pos is None else pos)
    assert pos.shape == (c + G, D)
    cos = sin = None
    if theta is not None:
        cos, sin = RD.table64(theta, D // heads, gw, gh) if mutant == "rope_transposed" else RD.table64(theta, D // heads, gh, gw, mutant)
    patches = XD.patchify64(f8(around(imgs) if around else imgs), P, mutant)
    emb = patches @ W(t["patch_embed.proj.weight"]).reshape(D, -1).T + f8(t["patch_embed.proj.bias"]).reshape(-1)
    x = np.empty((n, G + T, D))
    if c:
        x[:, 0] = f8(t["cls_token"]).reshape(D) + pos[0]
    if R:
        x[:, c:T] = f8(t["reg_token"][0]) + (pos[1:T] if mutant == "pos_on_registers" else 0.0)
    x[:, T:] = emb + (pos[c:] if mutant != "patch_pos_shifted" else pos[(T + np.arange(G)) % (1 + G)])
    embed = x.copy()
    if pre_norm:
        x = layernorm64(x, f8(t["pre_norm.weight"]), f8(t["pre_norm.bias"]), eps)
    x, trace, q, k = blocks64(t, x, heads, activation, eps, glu, cos, sin, None, mutant, wround, uround)
    F = layernorm64(x, f8(t["norm.weight"]), f8(t["norm.bias"]), eps)
    mean = PD.pooled64(F, T, mutant)
    hw = W(t["head.weight"])
    out = dict(embed=embed, trace=trace, final=F, mean=mean, q=q, k=k)
    if pooling:
        hd = MD.head64(t, F, heads, folded=folded, flat=flat, activation=activation, eps=eps, wround=wround, uround=uround)
        out.update(e=hd["e"], M=hd["M"], p=hd["p"])
        z = U(hd["e"])
    else:
        z = U(F[:, 0] if hw.shape[1] == D else np.concatenate([F[:, 0], mean], 1))
    logits = z @ hw.T + f8(t["head.bias"])
    e = np.exp(logits - logits.max(1, keepdims=True))
    out.update(logits=logits, probs=e / e.sum(1, keepdims=True))
    return out
