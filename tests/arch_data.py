"""What the activation / epsilon / pre-norm family (include/vitx.h "activation, epsilon and pre-norm") owns of the float64 restatement
tests/ref64.py: the three activations and the LayerNorm in float64, what a file's `arch` tensor states, the bound and the grid of the exact epilogue
test, and the synthetic files of the three model classes.  Shared by tests/test_cpu_arch.py -- which pins the restatement to transformers' ViT,
DINOv2 and CLIP -- and tests/test_gpu_arch.py.
    activation   t["arch"][0]: 0 tanh-GELU, 1 erf-GELU x Phi(x), 2 QuickGELU x sigmoid(1.702 x)      (absent: 0)
    eps          t["arch"][1], the epsilon of EVERY LayerNorm                                          (absent: 1e-6)
    pre-norm     t["pre_norm.weight"], t["pre_norm.bias"]: a LayerNorm of every token row after the patch embedding and before layer 0; trace
                 stage 0 is the stream AFTER it (what enters layer 0), `embed` the rows in front of it
ref64.forward64's `activation=`, `eps=` and `pre_norm=False` override the file: the mutants the GPU tests must be able to tell from the real thing."""
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
    from ref64 import cached_file
    labels = dict(pkg.synth.VITSTR_LABELS) if in_chans == 1 else None
    return cached_file(f"arch-{name}-c{in_chans}-{kind}-ft{ftype}",
                       lambda tmp: pkg.ggml_file.write_model(tmp, *fixture_tensors(pkg, kind, name, in_chans), ftype=ftype, id2label=labels))
