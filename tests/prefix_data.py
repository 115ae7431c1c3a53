"""What the prefix-token family (class token + R register tokens, the cls + mean head; include/vitx.h "register tokens and the pooled head") owns
of the float64 restatement tests/ref64.py, and the helpers every family shares: the operand roundings, file_tensors, tanh-GELU, the pooled
mean, the class-token attention rows and the exact images.  Shared by tests/test_cpu_registers.py and tests/test_gpu_registers.py.

MUTANTS are the layout mistakes the GPU tests must be able to see; ref64.forward64(..., mutant=name) makes one of them:
    pos_on_registers     the register rows take pos_embed[1 .. R]
    patch_pos_shifted    patch p takes the position row of patch p + R (wrapping)
    registers_in_mean    the pooled mean runs over the register rows too
    mean_over_n_minus_1  the pooled sum is divided by N - 1"""
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


def gelu64(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * x * (1.0 + 0.044715 * x * x)))


def pooled64(F, T, mutant=None):
    """Mean of the final-norm patch rows F[:, T:] ([n][N][D] -> [n][D])."""
    if mutant == "registers_in_mean":
        return F[:, 1:].mean(1)
    if mutant == "mean_over_n_minus_1":
        return F[:, T:].sum(1) / (F.shape[1] - 1)
    return F[:, T:].mean(1)


def cls_maps64(q, k):
    """Class-token attention rows [n][H][N] of one layer's q, k [n][H][N][hd]."""
    s = np.einsum("nhd,nhjd->nhj", q[:, :, 0], k) / np.sqrt(q.shape[-1])
    a = np.exp(s - s.max(-1, keepdims=True))
    return a / a.sum(-1, keepdims=True)


def exact_images(n, S, seed=0):
    """[n][S][S][3] f32 images whose pixels are multiples of 1/16 in [-4, 4): exact in bf16 and fp16, so the patch-embedding products carry no
    operand rounding of the pixels in either type."""
    return (np.random.default_rng(seed).integers(-64, 64, (n, S, S, 3)) / 16.0).astype(np.float32)
