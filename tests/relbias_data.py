"""The relative position bias (include/vitx.h) in float64: index rule, the op's cases, the synthetic files and their forward.  For test_{cpu,gpu}_relbias.py."""
import functools

import numpy as np

import prefix_data as PD
import ref64 as R64

NAME, HEADS, LAYERS, GRID = "vit_micro_patch16_64", 2, 2, 4      # D 128, patch 16, image 64
# N = 2; rectangular; across a 16-query tile; across the 64-key chunk and query block; ViT-B; BEiT-L/512: more than 48 KiB of dynamic LDS
OP_GRIDS = [(1, 1), (2, 3), (4, 4), (5, 13), (14, 14), (32, 32)]
OP_H, OP_IMG = 3, 2
# max |out - float64| <= GATE * max |float64|: what test_gpu_attention_wide.py::test_wide_against_float64 holds vitx_op_attention_generic to
GATE = 0.05


def index(gh, gw, g=None, swap=False):
    """timm's gen_relative_position_index, [N][N], class token first; g: the table's own grid side (offsets around its centre), None: the grid's own table.
    swap: the mistake of taking dx for dy (clipped into the table)."""
    sh, sw = (gh, gw) if g is None else (g, g)
    num = (2 * sh - 1) * (2 * sw - 1) + 3
    y, x = np.divmod(np.arange(gh * gw), gw)
    dy, dx = y[:, None] - y[None, :], x[:, None] - x[None, :]
    if swap:
        dy, dx = np.clip(dx, 1 - sh, sh - 1), np.clip(dy, 1 - sw, sw - 1)
    idx = np.empty((gh * gw + 1,) * 2, np.int64)
    idx[1:, 1:] = (dy + sh - 1) * (2 * sw - 1) + dx + sw - 1
    idx[0, 1:], idx[1:, 0], idx[0, 0] = num - 3, num - 2, num - 1
    return idx


@functools.lru_cache(maxsize=None)
def op_case(dtype_name, gh, gw):
    """(qkv [OP_IMG * N][3 * 64 OP_H] f32 already rounded to the type, table [OP_H][num] f32 in +-4: a different one per head)."""
    rng = np.random.default_rng(1000 * gh + gw)
    qkv = (PD.f16_round if dtype_name == "f16" else PD.bf16_round)(rng.standard_normal((OP_IMG * (gh * gw + 1), 3 * 64 * OP_H)) * 0.8)
    return qkv, rng.uniform(-4, 4, (OP_H, (2 * gh - 1) * (2 * gw - 1) + 3)).astype(np.float32)


def attention64(qkv, B, n_img, H):
    """softmax(q k^T / sqrt(hd) + B) v in float64: qkv [n_img * N][3 D], B [H][N][N] -> [n_img * N][D]."""
    D = qkv.shape[1] // 3
    q, k, v = (np.asarray(qkv, np.float64).reshape(n_img, -1, 3, H, D // H)[:, :, j].transpose(0, 2, 1, 3) for j in range(3))
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(D // H) + B
    a = np.exp(s - s.max(-1, keepdims=True))
    return ((a / a.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(-1, D)


def tensors(pkg, shared, pool):
    """The micro model with `rel_bias` in +-2 ([1] or [L] tables) and a zero position table, as BEiT has it; pool: the `pool` order-1 head."""
    hp = pkg.synth.hparams_for(NAME, ftype=1)
    t = pkg.synth.make_weights(hp, head_scale=4.0, head_pool=4 if pool else 0)
    t["pos_embed"] = np.zeros_like(t["pos_embed"])
    rb = np.random.default_rng(7).uniform(-2, 2, (1 if shared else LAYERS, HEADS, (2 * GRID - 1) ** 2 + 3)).astype(np.float32)
    return hp, {"rel_bias": rb, **t}


def fixture_file(pkg, shared, pool):
    return R64.cached_file(f"relbias-{NAME}-shared{int(shared)}-pool{int(pool)}", lambda p: pkg.ggml_file.write_model(p, *tensors(pkg, shared, pool)))


def forward64(t, imgs, wround=None, uround=None):
    """probs [n][C] of a `rel_bias` file: ref64's embedding, then ref64.blocks64 layer by layer with that layer's B as the additive mask; the class-token head
    or (`pool`, order 1) the norm of the mean of the raw patch rows."""
    f8, W, U = R64._rounders(wround, uround)
    x = R64.forward64({k: v for k, v in t.items() if k not in ("rel_bias", "pool")}, imgs, HEADS, wround=wround, uround=uround)["embed"]
    B = f8(t["rel_bias"])[..., index(GRID, GRID)]
    for i in range(LAYERS):
        one = {k.replace(f"blocks.{i}.", "blocks.0."): v for k, v in t.items() if k.startswith(f"blocks.{i}.")}
        x = R64.blocks64(one, x, HEADS, 0, PD.EPS, mask=B[i % len(B)], wround=wround, uround=uround)[0]
    z = x[:, 1:].mean(1) if "pool" in t else x[:, 0]
    logits = U(R64.layernorm64(z, f8(t["norm.weight"]), f8(t["norm.bias"]), PD.EPS)) @ W(t["head.weight"]).T + f8(t["head.bias"])
    e = np.exp(logits - logits.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)
