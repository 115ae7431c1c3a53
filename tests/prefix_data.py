"""Float64 restatement of the forward with prefix tokens (class token + R register tokens), shared by tests/test_cpu_registers.py and
tests/test_gpu_registers.py (include/vitx.h "register tokens and the pooled head").

Token layout of an image, T = 1 + R, N = g^2 + T:
    row 0          cls_token + pos_embed[0]
    rows 1 .. R    reg_token[r]                    (no position embedding)
    rows T .. N-1  patch p + pos_embed[1 + p]      (raster order)
Pre-norm blocks, fused qkv with biases, softmax(q k^T / sqrt(hd)) v, tanh-GELU MLP, LayerNorm eps 1e-6 (LayerScale is already folded into
attn.proj / mlp.fc2 of a file).  Head: logits = W . F[0] + b (head.weight [C][D]) or W . concat(F[0], mean of F[T .. N-1]) + b ([C][2 D]),
F = the final norm of the last residual stream.  Everything is float64 on the f32 values it is given; `around` / `wround` / `uround` place
the operand type's rounding where the engine places it -- on the patch pixels, on every matrix, and on the activations that enter a GEMM
(LayerNorm outputs, attention output, GELU output, the head operand).  All None: no rounding anywhere.

MUTANTS are the mistakes the GPU tests must be able to see; forward64(..., mutant=name) makes one of them."""
import numpy as np

EPS = 1e-6
MUTANTS = ("pos_on_registers", "patch_pos_shifted", "registers_in_mean", "mean_over_n_minus_1")


def f16_round(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def bf16_round(x):
    """f32 -> bf16 -> f32, round to nearest even (finite values)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def file_tensors(pkg, path):
    """{name: f32 array in torch shape} of a model file, block types dequantised (ggml_file.py; no native library needed)."""
    mf = pkg.ggml_file.read_model(path)
    return {t.name: pkg.ggml_file.dequantize(t.ttype, t.raw, int(np.prod(t.ne))).reshape(tuple(reversed(t.ne))) for t in mf.tensors}


def layernorm64(x, w, b):
    mu = x.mean(-1, keepdims=True); var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + EPS) * w + b


def gelu64(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * x * (1.0 + 0.044715 * x * x)))


def pooled64(F, T, mutant=None):
    """Mean of the final-norm patch rows F[:, T:] ([n][N][D] -> [n][D])."""
    if mutant == "registers_in_mean":
        return F[:, 1:].mean(1)
    if mutant == "mean_over_n_minus_1":
        return F[:, T:].sum(1) / (F.shape[1] - 1)
    return F[:, T:].mean(1)


def qk64(t, x, i, heads, wround=None, uround=None):
    """q, k, v [n][H][N][hd] of layer i from the residual stream x [n][N][D] that enters it."""
    f8 = lambda a: np.asarray(a, np.float64)
    W = (lambda a: f8(wround(a))) if wround else f8
    U = (lambda a: f8(uround(a))) if uround else f8
    p = f"blocks.{i}."
    n, _, D = x.shape
    qkv = U(layernorm64(f8(x), f8(t[p + "norm1.weight"]), f8(t[p + "norm1.bias"]))) @ W(t[p + "attn.qkv.weight"]).T + f8(t[p + "attn.qkv.bias"])
    return tuple(qkv[..., j * D:(j + 1) * D].reshape(n, -1, heads, D // heads).transpose(0, 2, 1, 3) for j in range(3))


def forward64(t, imgs, heads, pos=None, mutant=None, around=None, wround=None, uround=None):
    """t: {name: f32 array, torch shapes} (file_tensors); imgs [n][S][S][3] f32; pos: another [1 + g^2][D] table than the file's.
    Returns dict(trace [L + 1][n][N][D], final [n][N][D], mean [n][D], q / k [L][n][H][N][hd], logits [n][C], probs [n][C])."""
    f8 = lambda a: np.asarray(a, np.float64)
    W = (lambda a: f8(wround(a))) if wround else f8
    U = (lambda a: f8(uround(a))) if uround else f8
    D = t["cls_token"].shape[-1]
    R = t["reg_token"].shape[1] if "reg_token" in t else 0
    T = 1 + R
    L = 1 + max(int(k.split(".")[1]) for k in t if k.startswith("blocks."))
    P = t["patch_embed.proj.weight"].shape[-1]
    n, S = imgs.shape[0], imgs.shape[1]
    g = S // P
    pos = f8(t["pos_embed"][0] if pos is None else pos)
    assert pos.shape == (1 + g * g, D)
    px = f8(around(imgs) if around else imgs)
    patches = px.reshape(n, g, P, g, P, 3).transpose(0, 1, 3, 5, 2, 4).reshape(n, g * g, 3 * P * P)      # [c][ky][kx], the kernel's order
    emb = patches @ W(t["patch_embed.proj.weight"]).reshape(D, -1).T + f8(t["patch_embed.proj.bias"]).reshape(-1)
    ppos = pos[1:] if mutant != "patch_pos_shifted" else pos[(1 + R + np.arange(g * g)) % (1 + g * g)]
    x = np.empty((n, g * g + T, D))
    x[:, 0] = f8(t["cls_token"]).reshape(D) + pos[0]
    if R:
        x[:, 1:T] = f8(t["reg_token"][0]) + (pos[1:T] if mutant == "pos_on_registers" else 0.0)
    x[:, T:] = emb + ppos
    trace, qs, ks = [x.copy()], [], []
    hd = D // heads
    for i in range(L):
        p = f"blocks.{i}."
        v = lambda name: f8(t[p + name])
        q, k, vv = qk64(t, x, i, heads, wround, uround)
        s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(hd)
        a = np.exp(s - s.max(-1, keepdims=True)); a /= a.sum(-1, keepdims=True)
        o = U((a @ vv).transpose(0, 2, 1, 3).reshape(n, -1, D))
        x = x + o @ W(t[p + "attn.proj.weight"]).T + v("attn.proj.bias")
        h = U(gelu64(U(layernorm64(x, v("norm2.weight"), v("norm2.bias"))) @ W(t[p + "mlp.fc1.weight"]).T + v("mlp.fc1.bias")))
        x = x + h @ W(t[p + "mlp.fc2.weight"]).T + v("mlp.fc2.bias")
        trace.append(x.copy()); qs.append(q); ks.append(k)
    F = layernorm64(x, f8(t["norm.weight"]), f8(t["norm.bias"]))
    mean = pooled64(F, T, mutant)
    hw = W(t["head.weight"])
    z = U(F[:, 0] if hw.shape[1] == D else np.concatenate([F[:, 0], mean], 1))
    logits = z @ hw.T + f8(t["head.bias"])
    e = np.exp(logits - logits.max(1, keepdims=True))
    return dict(trace=np.stack(trace), final=F, mean=mean, q=np.stack(qs), k=np.stack(ks), logits=logits, probs=e / e.sum(1, keepdims=True))


def cls_maps64(q, k):
    """Class-token attention rows [n][H][N] of one layer's q, k [n][H][N][hd]."""
    s = np.einsum("nhd,nhjd->nhj", q[:, :, 0], k) / np.sqrt(q.shape[-1])
    a = np.exp(s - s.max(-1, keepdims=True))
    return a / a.sum(-1, keepdims=True)


def exact_images(n, S, seed=0):
    """[n][S][S][3] f32 images whose pixels are multiples of 1/16 in [-4, 4): exact in bf16 and fp16, so the patch-embedding products carry no
    operand rounding of the pixels in either type."""
    return (np.random.default_rng(seed).integers(-64, 64, (n, S, S, 3)) / 16.0).astype(np.float32)
