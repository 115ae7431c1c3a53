"""Float64 restatement of the forward parametrised by MLP activation, LayerNorm epsilon and pre-norm (include/vitx.h "activation, epsilon and
pre-norm"), shared by tests/test_cpu_arch.py -- which pins it to transformers' ViT, DINOv2 and CLIP -- and tests/test_gpu_arch.py.

It is tests/prefix_data.py::forward64 (same token layout, same rounding points: `around` on the pixels, `wround` on every matrix, `uround` on
the activations that enter a GEMM) with three things read from the file's tensors instead of being fixed:
    activation   t["arch"][0]: 0 tanh-GELU, 1 erf-GELU x Phi(x), 2 QuickGELU x sigmoid(1.702 x)      (absent: 0)
    eps          t["arch"][1], the epsilon of EVERY LayerNorm                                          (absent: 1e-6)
    pre-norm     t["pre_norm.weight"], t["pre_norm.bias"]: a LayerNorm of every token row after the patch embedding and before layer 0; trace
                 stage 0 is the stream AFTER it (what enters layer 0), `embed` the rows in front of it
`activation=`, `eps=` and `pre_norm=False` override the file: the mutants the GPU tests must be able to tell from the real thing."""
import os

import numpy as np

import prefix_data as PD

ACT_TANH, ACT_ERF, ACT_QUICK = 0, 1, 2
ACT_NAMES = {ACT_TANH: "tanh", ACT_ERF: "erf", ACT_QUICK: "quick"}
EPI = {ACT_TANH: 1, ACT_ERF: 6, ACT_QUICK: 7}          # the fc1 epilogue of each activation (vitx_op_gemm)
MICRO = "vit_micro_patch14_56"                         # D 128, 2 layers, 2 heads, patch 14, image 56: the shape of tests/test_cpu_registers.py


def act64(x, activation):
    """The activation in float64."""
    x = np.asarray(x, np.float64)
    if activation == ACT_TANH:
        return PD.gelu64(x)
    if activation == ACT_ERF:
        # x Phi(x) with Phi through erfc on the negative side: 0.5 (1 + erf) would cancel there in any precision
        z = np.abs(x) / np.sqrt(2.0)
        q = 0.5 * _erfc64(z)
        return np.where(x < 0, x * q, x * (1.0 - q))
    if activation == ACT_QUICK:
        return x / (1.0 + np.exp(-1.702 * x))
    raise ValueError(activation)


def _erfc64(z):
    z = np.asarray(z, np.float64)
    try:
        from scipy.special import erfc
        return erfc(z)
    except ImportError:
        import torch
        return torch.erfc(torch.from_numpy(np.ascontiguousarray(z))).numpy()


def ulp_T(want, dtype):
    """One unit in the last place of the output type (0 fp16, 1 bf16) at |want|; fp16's subnormal spacing is 2^-24."""
    a = np.abs(np.asarray(want, np.float64))
    _, ex = np.frexp(np.where(a > 0, a, 1.0))           # a = m 2^ex, m in [0.5, 1): floor(log2 a) = ex - 1
    e = np.where(a > 0, ex - 1, -1000)
    if dtype == 0:
        return np.ldexp(1.0, np.maximum(e, -14) - 10)
    return np.ldexp(1.0, np.maximum(e, -126) - 7)


def act_tol(want, dtype):
    """The bound of the epilogue's exact test: one ulp of the output type at the float64 value + the absolute floor of the tanh epilogue's
    existing assertion (tests/test_gpu_parity_r02.py:91)."""
    return ulp_T(want, dtype) + 1e-6


def grid():
    """x = k / 64, k in [-512, 512): every fc1 value of the exact test without the +1/128 of its odd rows."""
    return np.arange(-512, 512) / 64.0


def separated(act_a, act_b, dtype, x=None):
    """Points of the grid where the float64 activation `act_b` lies more than two tolerances (of act_a's value) from act_a: where a kernel that
    evaluated the wrong one could not pass the exact test."""
    x = grid() if x is None else x
    wa, wb = act64(x, act_a), act64(x, act_b)
    return np.abs(wa - wb) > 2 * act_tol(wa, dtype)


def arch_of(t):
    """(activation, eps, has_pre_norm) a file's tensors state."""
    a = np.asarray(t["arch"], np.float32).reshape(-1) if "arch" in t else None
    return (int(a[0]) if a is not None else ACT_TANH, float(a[1]) if a is not None else 1e-6, "pre_norm.weight" in t)


def layernorm64(x, w, b, eps):
    mu = x.mean(-1, keepdims=True); var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def forward64(t, imgs, heads, pos=None, activation=None, eps=None, pre_norm=None, around=None, wround=None, uround=None):
    """t: {name: f32 array, torch shapes} (prefix_data.file_tensors); imgs [n][S][S][3] f32; pos: another [1 + g^2][D] table than the file's.
    activation / eps / pre_norm: None = the file's own (arch_of).  Returns dict(embed [n][N][D] (the rows in front of the pre-norm), trace
    [L + 1][n][N][D], final [n][N][D], mean [n][D], logits [n][C], probs [n][C])."""
    f8 = lambda a: np.asarray(a, np.float64)
    W = (lambda a: f8(wround(a))) if wround else f8
    U = (lambda a: f8(uround(a))) if uround else f8
    f_act, f_eps, f_pre = arch_of(t)
    activation = f_act if activation is None else activation
    eps = float(np.float32(f_eps if eps is None else eps))
    pre_norm = f_pre if pre_norm is None else pre_norm
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
    x = np.empty((n, g * g + T, D))
    x[:, 0] = f8(t["cls_token"]).reshape(D) + pos[0]
    if R:
        x[:, 1:T] = f8(t["reg_token"][0])
    x[:, T:] = emb + pos[1:]
    embed = x.copy()
    if pre_norm:
        x = layernorm64(x, f8(t["pre_norm.weight"]), f8(t["pre_norm.bias"]), eps)
    trace = [x.copy()]
    hd = D // heads
    for i in range(L):
        p = f"blocks.{i}."
        v = lambda name: f8(t[p + name])
        qkv = U(layernorm64(x, v("norm1.weight"), v("norm1.bias"), eps)) @ W(t[p + "attn.qkv.weight"]).T + v("attn.qkv.bias")
        q, k, vv = (qkv[..., j * D:(j + 1) * D].reshape(n, -1, heads, hd).transpose(0, 2, 1, 3) for j in range(3))
        s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(hd)
        a = np.exp(s - s.max(-1, keepdims=True)); a /= a.sum(-1, keepdims=True)
        o = U((a @ vv).transpose(0, 2, 1, 3).reshape(n, -1, D))
        x = x + o @ W(t[p + "attn.proj.weight"]).T + v("attn.proj.bias")
        h = U(act64(U(layernorm64(x, v("norm2.weight"), v("norm2.bias"), eps)) @ W(t[p + "mlp.fc1.weight"]).T + v("mlp.fc1.bias"), activation))
        x = x + h @ W(t[p + "mlp.fc2.weight"]).T + v("mlp.fc2.bias")
        trace.append(x.copy())
    F = layernorm64(x, f8(t["norm.weight"]), f8(t["norm.bias"]), eps)
    mean = PD.pooled64(F, T)
    hw = W(t["head.weight"])
    z = U(F[:, 0] if hw.shape[1] == D else np.concatenate([F[:, 0], mean], 1))
    logits = z @ hw.T + f8(t["head.bias"])
    e = np.exp(logits - logits.max(1, keepdims=True))
    return dict(embed=embed, trace=np.stack(trace), final=F, mean=mean, logits=logits, probs=e / e.sum(1, keepdims=True))


# ------------------------------------------------------------------------------------------------ synthetic files of the three model classes
# name: (activation, eps, pre-norm, head_pool, CLIP-style zero biases and MLP scale)
FIXTURES = {
    "vit_erf": (ACT_ERF, 1e-12, False, 0, False),        # HuggingFace ViT's defaults
    "dinov2_erf": (ACT_ERF, 1e-6, False, 1, False),      # DINOv2: erf, cls + mean head
    "clip": (ACT_QUICK, 1e-5, True, 0, True),            # CLIP: QuickGELU, 1e-5, pre_layrnorm, bias-free patch convolution and projection
    "eps_1e-2": (ACT_TANH, 1e-2, False, 0, False),       # nothing but a large epsilon: the eps mutant's fixture
    "tanh_pre": (ACT_TANH, 1e-5, True, 0, False),        # tanh with eps and a pre-norm: what a VITX_MXFP8 context still takes
    "vitstr_erf": (ACT_ERF, 1e-6, False, 0, False),      # refused at context creation when written with one input channel
    "vitstr_pre": (ACT_TANH, 1e-6, True, 0, False),
}
# make_weights draws every matrix at 0.02: the fc1 outputs then stay inside |x| < 0.5, where the three activations nearly coincide, and the MLP
# branch is a few per cent of the stream.  The CLIP fixture scales mlp.fc1.weight and mlp.fc2.weight so that the activation sees arguments of
# unit scale and its output carries the stream: only then does "the wrong activation" move the trace by more than the F16 gates (measured on the
# restatement: 7.8e-3 / 9.4e-3 rms per layer against the gate's 2e-3; at scale 1 it is 7e-4 and no end-to-end test could tell them apart).
CLIP_MLP_SCALE = (8.0, 4.0)


def fixture_tensors(pkg, kind, name=MICRO, in_chans=3):
    """Synthetic weights of pkg.synth.make_weights (head scale 4, as the other micro fixtures) + the extensions of `kind`, in the converter's order:
    `arch` first, `pre_norm.*` directly after pos_embed."""
    act, eps, pre, pool, clip = FIXTURES[kind]
    hp = pkg.synth.hparams_for(name)
    w = pkg.synth.make_weights(hp, head_scale=4.0, in_chans=in_chans, head_pool=pool)
    D = hp.hidden_size
    rng = np.random.default_rng(77)
    out = {}
    if (act, np.float32(eps)) != (ACT_TANH, np.float32(1e-6)):
        out["arch"] = np.array([act, eps, 0, 0], np.float32)
    for k, v in w.items():
        out[k] = v
        if k == "pos_embed" and pre:
            out["pre_norm.weight"] = (1.0 + rng.standard_normal(D) * 0.1).astype(np.float32)
            out["pre_norm.bias"] = (rng.standard_normal(D) * 0.1).astype(np.float32)
    if clip:
        out["patch_embed.proj.bias"] = np.zeros_like(out["patch_embed.proj.bias"])
        out["head.bias"] = np.zeros_like(out["head.bias"])
        for i in range(hp.num_hidden_layers):
            out[f"blocks.{i}.mlp.fc1.weight"] = out[f"blocks.{i}.mlp.fc1.weight"] * np.float32(CLIP_MLP_SCALE[0])
            out[f"blocks.{i}.mlp.fc2.weight"] = out[f"blocks.{i}.mlp.fc2.weight"] * np.float32(CLIP_MLP_SCALE[1])
    return hp, out


def fixture_file(pkg, kind, ftype=1, name=MICRO, in_chans=3):
    """Path of the (cached) model file of a fixture."""
    cache_dir = os.environ.get("VITX_CACHE", "/tmp/vitx_cache")
    os.makedirs(cache_dir, exist_ok=True)
    path = os.path.join(cache_dir, f"arch-{name}-c{in_chans}-{kind}-ft{ftype}.gguf")
    if not os.path.exists(path):
        hp, t = fixture_tensors(pkg, kind, name, in_chans)
        tmp = path + f".tmp{os.getpid()}"
        pkg.ggml_file.write_model(tmp, hp, t, ftype=ftype, id2label=dict(pkg.synth.VITSTR_LABELS) if in_chans == 1 else None)
        os.replace(tmp, path)
    return path
