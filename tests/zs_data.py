"""Float64 restatement of zero-shot classification (include/vitx.h "zero-shot classification"), shared by tests/test_cpu_zeroshot.py -- which pins
it to transformers' CLIPModel and SiglipModel -- and tests/test_gpu_zeroshot.py.

    a = z / |z| (an all-zero z stays zero);  c_k = a . t_k;  l_k = c_k * scale + bias;
    softmax: p_k = exp(l_k - max l) / sum_j exp(l_j - max l);   sigmoid: p_k = 1 / (1 + exp(-l_k))

restate() takes the operands AS THE DEVICE MULTIPLIES THEM -- a and t already rounded to the operand type -- so what is left between it and the
device is the f32 accumulation order of the products and expf.  device_operand() is the device's own arithmetic for a, operation for operation in
f32 (zs_embed_kernel: lane l of a wave owns the 16-byte pieces l, l + 64, ... of the row and adds its squares in column order; the 64 partial sums
meet in a butterfly; IEEE square root and division; RNE to the operand type)."""
import numpy as np

import arch_data as AD
import map_data as MD
import prefix_data as PD
import ref64 as R64

SOFTMAX, SIGMOID = 0, 1
ROUND = {0: PD.f16_round, 1: PD.bf16_round}
# the issue's bound on a pre-scale cosine by operand type (0 fp16, 1 bf16): both operands rounded once (unit vectors: every element's rounding error
# is at most 2^-12 / 2^-9 of itself, so each operand moves the product by at most that), plus f32 accumulation of E products
COS_BOUND = {0: lambda E: 2 * 2.0 ** -12 + E * 2.0 ** -24, 1: lambda E: 2 * 2.0 ** -9 + E * 2.0 ** -24}


def normalise64(z):
    z = np.asarray(z, np.float64)
    n = np.sqrt((z * z).sum(-1, keepdims=True))
    return np.divide(z, n, out=np.zeros_like(z), where=n > 0)


def unit_rows(x):
    """f32 rows of unit length (normalised in float64, rounded once)."""
    return normalise64(x).astype(np.float32)


def device_sumsq(z):
    """sum z^2 per row of z [n][E] f32 in zs_embed_kernel's order, in f32."""
    z = np.ascontiguousarray(z, np.float32)
    n, E = z.shape
    assert E % 64 == 0
    nv = E // 4
    ss = np.zeros((n, 64), np.float32)
    for v0 in range(0, nv, 64):                      # step s of every lane: piece v0 + lane
        lanes = min(64, nv - v0)
        piece = z[:, 4 * v0:4 * (v0 + lanes)].reshape(n, lanes, 4)
        for e in range(4):
            ss[:, :lanes] = ss[:, :lanes] + piece[:, :, e] * piece[:, :, e]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        ss = ss + ss[:, idx ^ o]
    assert (ss == ss[:, :1]).all()
    return ss[:, 0]


def device_operand(z, dtype):
    """a [n][E] f32 values of the operand rows the device writes for z [n][E] f32."""
    z = np.ascontiguousarray(z, np.float32)
    nrm = np.sqrt(device_sumsq(z))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(nrm > 0, z / nrm, z).astype(np.float32)
    return ROUND[dtype](a)


def restate(a, t, kind, scale, bias):
    """a [n][E], t [K][E]: the operands as multiplied.  Returns dict(cos, logits, probs), float64."""
    cos = np.asarray(a, np.float64) @ np.asarray(t, np.float64).T
    logits = cos * np.float64(np.float32(scale)) + np.float64(np.float32(bias))
    return dict(cos=cos, logits=logits, probs=probs64(logits, kind))


def probs64(logits, kind):
    l = np.asarray(logits, np.float64)
    if kind == SIGMOID:
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-l))
    e = np.exp(l - l.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def logit_tol(a, t, scale, bias):
    """What f32 may put between the device's logits and restate()'s on the same operands: E products accumulated in f32 in some order (at most
    E * 2^-24 of sum |a_i t_i|), then one multiply and one add, each rounded once."""
    a = np.abs(np.asarray(a, np.float64)); t = np.abs(np.asarray(t, np.float64))
    E = a.shape[-1]
    mag = a @ t.T
    return (E + 2) * 2.0 ** -24 * (mag * abs(float(scale)) + abs(float(bias))) + 1e-38


def margins(logits):
    """top-1 class and top-1 minus top-2 logit per row."""
    l = np.asarray(logits, np.float64)
    order = np.argsort(-l, axis=-1, kind="stable")
    rows = np.arange(l.shape[0])
    return order[:, 0], l[rows, order[:, 0]] - l[rows, order[:, 1]]


# ------------------------------------------------------------------------------------------------ the two micro model files
CLIP_E = 64            # projection width of the CLIP-class micro file below (arch_data's own has 10 "classes": not a multiple of 64)
N_IMAGES, BANK_K = 17, 24
CLIP_SCALE, SIGLIP_SCALE, SIGLIP_BIAS = 100.0, 112.0, -12.5      # of the order of the released models' exp(logit_scale) and logit_bias


def clip_tensors(pkg, name=AD.MICRO):
    """arch_data's CLIP-class fixture with a [64][D] bias-free projection as its head: E = 64."""
    hp, t = AD.fixture_tensors(pkg, "clip", name)
    D = hp.hidden_size
    rng = np.random.default_rng(2718)
    hp.num_classes = CLIP_E
    t["head.weight"] = np.clip(rng.standard_normal((CLIP_E, D), dtype=np.float32) * np.float32(0.08), -0.16, 0.16).astype(np.float32)
    t["head.bias"] = np.zeros(CLIP_E, np.float32)
    return hp, t


def clip_file(pkg, ftype=1, name=AD.MICRO):
    return R64.cached_file(f"zs-clip-{name}-e{CLIP_E}-ft{ftype}", lambda tmp: pkg.ggml_file.write_model(tmp, *clip_tensors(pkg, name), ftype=ftype))


def model_file(pkg, family):
    return clip_file(pkg) if family == "clip" else MD.fixture_file(pkg)


def images():
    return PD.exact_images(N_IMAGES, 56, seed=1)


def embedding64(pkg, family):
    """The float64 embedding of the 17 images under the file's restatement: the logits row (CLIP-class) or the pooled embedding e (SigLIP-class)."""
    t = PD.file_tensors(pkg, model_file(pkg, family))
    return R64.forward64(t, images(), 2)["logits" if family == "clip" else "e"]


def bank(family, emb):
    """(t [K][E] f32 unit rows, kind, scale, bias) of a family's end-to-end tests, from `emb` = embedding64(pkg, family) [17][E].  The first 17 classes
    point along what tells image k from the mean image (plus a quarter of a random direction), the rest are random.  The SigLIP-class micro model
    spreads its images (mutual cosines down to 0.17): every image has its own top-1 class, top-2 margins of 16 logits and more.  The CLIP-class one
    maps all 17 to nearly one embedding (mutual cosines >= 0.9997: a class token under 0.02-scale weights), so they share ONE top-1 class; seed 42
    puts its top-2 margin at 3.1 .. 4.7 logits, 4 to 6 times the bf16 logit bound's double (tests/test_cpu_zeroshot.py recomputes both)."""
    emb = np.asarray(emb, np.float64)
    E = emb.shape[1]
    rng = np.random.default_rng(42 if family == "clip" else 32)
    d = normalise64(emb - emb.mean(0))
    t = normalise64(rng.standard_normal((BANK_K, E)))
    t[:N_IMAGES] = normalise64(d + 0.25 * t[:N_IMAGES])
    if family == "clip":
        return unit_rows(t), SOFTMAX, CLIP_SCALE, 0.0
    return unit_rows(t), SIGMOID, SIGLIP_SCALE, SIGLIP_BIAS
