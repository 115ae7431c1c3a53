"""Windowed attention with a decomposed relative position term (include/vitx.h) in float64, and the op's cases.  For test_{cpu,gpu}_window.py."""
import functools

import numpy as np

import prefix_data as PD
import ref64 as R64
from relbias_data import GATE      # max |out - float64| <= GATE * max |float64|: what test_gpu_relbias.py holds attention_bias to

D, H, DH = 128, 2, 64
# zero tables, one global window: the generic kernel's bits.  72 keys cross a chunk, 65 keys leave one key in the second; 64 x 64 fills the 64 KiB of LDS
GLOBAL = [(1, 1), (3, 5), (8, 8), (9, 8), (13, 5), (64, 64)]
# (grid, window): edge windows of 2 real + 12 pad positions per axis; pads on both axes of a rectangle; a chunk edge; one column; a window that is the grid;
# the Segment-Anything grid: 25 windows, the last of a row or column with 8 real and 6 pad positions, and a global window as wide (a Bw panel of 64 rows)
F64_CASES = [((16, 16), (14, 14)), ((5, 7), (3, 3)), ((9, 8), (9, 8)), ((17, 1), (17, 1)), ((15, 15), (15, 15)), ((64, 64), (14, 14)), ((24, 64), (24, 64))]
# name -> (grid, window, case() arguments): data on which one mistake moves the result by far more than the gate -- pad keys read as zeros or dropped
# (a bias of 6 dominates every pad key); swapped axes (one table zero, a non-square window); an index off by one (only the last table row is non-zero);
# the term added to the scaled score or without its sqrt(dh) (|q| 4, tables 1: the term is several units of the exponent)
SHARP = {
    "pad keys are the bias": ((5, 7), (3, 3), dict(tables=0.0, bias=6.0)),
    "rows only": ((6, 10), (6, 10), dict(tables=(1.0, 0.0))),
    "columns only": ((6, 10), (6, 10), dict(tables=(0.0, 1.0))),
    "last table row": ((7, 6), (7, 6), dict(tables=1.0, only_last=True)),
    "unscaled query": ((5, 5), (5, 5), dict(tables=1.0, q=4.0)),
}


def _round(dtype_name):
    return PD.f16_round if dtype_name == "f16" else PD.bf16_round


@functools.lru_cache(maxsize=None)
def case(dtype_name, grid, win, n_img=2, tables=0.5, bias=0.5, q=0.8, only_last=False):
    """(qkv [n_img * gh gw][3 D], Rh [2 wh - 1][64], Rw [2 ww - 1][64], qkv bias [3 D]): f32 values the type holds exactly; tables: a magnitude or (Rh's, Rw's)."""
    rng, rnd = np.random.default_rng(100 * grid[0] + grid[1]), _round(dtype_name)
    th, tw = tables if isinstance(tables, tuple) else (tables, tables)
    qkv = rng.standard_normal((n_img * grid[0] * grid[1], 3 * D)) * 0.8
    qkv[:, :D] *= q / 0.8
    Rh, Rw = (rng.uniform(-t, t, (2 * w - 1, DH)) for t, w in ((th, win[0]), (tw, win[1])))
    if only_last:
        Rh[:-1], Rw[:-1] = 0, 0
    return rnd(qkv), rnd(Rh), rnd(Rw), rnd(rng.uniform(-bias, bias, 3 * D))


def attention64(qkv, Rh, Rw, bias, n_img, grid, win):
    """float64: the grid padded to whole windows with tokens whose q, k, v are `bias`, softmax(q k^T / 8 + q . Rh[qy - ky + wh - 1] + q . Rw[qx - kx + ww - 1]) v
    per window and head, pads dropped -> [n_img * gh gw][D]."""
    (gh, gw), (wh, ww) = grid, win
    ny, nx = -(-gh // wh), -(-gw // ww)
    x = np.tile(np.asarray(bias, np.float64), (n_img, ny * wh, nx * ww, 1))
    x[:, :gh, :gw] = np.asarray(qkv, np.float64).reshape(n_img, gh, gw, -1)
    q, k, v = x.reshape(n_img, ny, wh, nx, ww, 3, H, DH).transpose(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, n_img, ny, nx, H, wh * ww, DH)
    y, c = np.divmod(np.arange(wh * ww), ww)
    dy, dx = y[:, None] - y[None, :], c[:, None] - c[None, :]
    ar = np.arange(wh * ww)[:, None]
    pos = (q @ np.asarray(Rh, np.float64).T)[..., ar, dy + wh - 1] + (q @ np.asarray(Rw, np.float64).T)[..., ar, dx + ww - 1]
    s = q @ k.swapaxes(-1, -2) / 8 + pos
    a = np.exp(s - s.max(-1, keepdims=True))
    o = (a / a.sum(-1, keepdims=True)) @ v
    return o.reshape(n_img, ny, nx, H, wh, ww, DH).transpose(0, 1, 4, 2, 5, 3, 6).reshape(n_img, ny * wh, nx * ww, D)[:, :gh, :gw].reshape(-1, D)


def window_rows(n_img, grid, ws):
    """Token rows [n_img * windows][ws^2] of a grid that is a multiple of ws: each window gathered as an image."""
    gh, gw = grid
    t = np.arange(n_img * gh * gw).reshape(n_img, gh // ws, ws, gw // ws, ws)
    return t.transpose(0, 1, 3, 2, 4).reshape(-1, ws * ws)


# ---- the synthetic file: D 128, two heads, three layers (layer 1 global), a 5 x 5 grid of 8-pixel patches, windows of 3, the final norm an identity
LAYERS, GRID, WS, IMG = 3, 5, 3, 40


def tensors(pkg, identity_norm=True, heads=H):
    hp = pkg.synth.HParams(D, LAYERS, heads, 10, IMG // GRID, IMG, ftype=1)
    return hp, pkg.synth.make_window_weights(hp, WS, global_layers=(1,), identity_norm=identity_norm, head_scale=4.0)


def fixture_file(pkg):
    return R64.cached_file("window-micro-5x5-ws3", lambda p: pkg.ggml_file.write_model(p, *tensors(pkg)))


def forward64(t, imgs, wround=None, uround=None):
    """(tokens [n][G][D], probs [n][C]) of a `window` file in float64: ref64's embedding, then per layer attention64 on the rounded qkv rows with
    that layer's window and tables and the plain block around it; the final norm as the file's flag says, the mean of the rows, the head."""
    f8, W, U = R64._rounders(wround, uround)
    act, eps, _ = R64.AD.arch_of(t)
    eps = float(np.float32(eps))
    x = R64.forward64({k: v for k, v in t.items() if k not in ("window", "pool")}, imgs, H, wround=wround, uround=uround)["embed"]
    n = len(x)
    for i in range(LAYERS):
        v = lambda name: f8(t[f"blocks.{i}.{name}"])
        w = WS if t["window"][2 + i] else GRID
        qkv = U(U(R64.layernorm64(x, v("norm1.weight"), v("norm1.bias"), eps)) @ W(t[f"blocks.{i}.attn.qkv.weight"]).T + v("attn.qkv.bias"))
        o = U(attention64(qkv.reshape(-1, 3 * D), W(t[f"blocks.{i}.attn.rel_pos_h"]), W(t[f"blocks.{i}.attn.rel_pos_w"]), U(v("attn.qkv.bias")), n, (GRID, GRID), (w, w)))
        x = x + o.reshape(n, -1, D) @ W(t[f"blocks.{i}.attn.proj.weight"]).T + v("attn.proj.bias")
        y = U(R64.layernorm64(x, v("norm2.weight"), v("norm2.bias"), eps))
        x = x + U(R64.AD.act64(y @ W(t[f"blocks.{i}.mlp.fc1.weight"]).T + v("mlp.fc1.bias"), act)) @ W(t[f"blocks.{i}.mlp.fc2.weight"]).T + v("mlp.fc2.bias")
    F = x if t["window"][1] else R64.layernorm64(x, f8(t["norm.weight"]), f8(t["norm.bias"]), eps)
    logits = U(F.mean(1)) @ W(t["head.weight"]).T + f8(t["head.bias"])
    e = np.exp(logits - logits.max(1, keepdims=True))
    return F, e / e.sum(1, keepdims=True)
