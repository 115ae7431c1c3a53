"""Reference encoder and decoder of the MXFP8 operand type (include/vitx.h, VITX_MXFP8), independent of libvitx.so.

A block is 32 consecutive K elements of one row.  a = max|x_i| = m * 2^E (m in [1, 2), from the bits, f32 subnormals included);
e = E - 8 if m <= 1.75 else E - 7, clamped to >= -127; scale byte s = e + 127; q_i = RNE_e4m3fn(x_i * 2^-e); a == 0: s = 127, q = 0.
Rows are padded to k_pad (zero elements; whole padding blocks get s = 127).  torch.float8_e4m3fn does the element rounding: the rule
never hands it a value above 448 (torch turns those into NaN).
"""
from __future__ import annotations

import numpy as np
import torch


def k_pad_of(K: int) -> int:
    return (K + 127) // 128 * 128


def block_exp(amax: np.ndarray) -> np.ndarray:
    """Block exponent e for f32 block maxima (>= 0)."""
    a = np.asarray(amax, np.float32)
    bits = a.view(np.uint32) & np.uint32(0x7fffffff)
    ef = (bits >> 23).astype(np.int64)
    man = (bits & np.uint32(0x7fffff)).astype(np.int64)
    E = ef - 127
    sub = (ef == 0) & (man != 0)
    if sub.any():                                     # subnormal: normalise the fraction
        ms = man[sub]
        lead = np.floor(np.log2(ms.astype(np.float64))).astype(np.int64)      # exact for integers < 2^23
        E[sub] = lead - 149
        man[sub] = (ms << (23 - lead)) & 0x7fffff
    e = np.where(man <= 0x600000, E - 8, E - 7)
    e = np.maximum(e, -127)
    return np.where(bits == 0, 0, e).astype(np.int64)


def encode(x: np.ndarray, k_pad: int | None = None):
    """f32 [rows, K] -> (q uint8 [rows, k_pad], scales uint8 [rows, k_pad // 32])."""
    x = np.atleast_2d(np.asarray(x, np.float32))
    rows, K = x.shape
    k_pad = k_pad_of(K) if k_pad is None else k_pad
    xp = np.zeros((rows, k_pad), np.float32); xp[:, :K] = x
    blocks = xp.reshape(rows, k_pad // 32, 32)
    e = block_exp(np.abs(blocks).max(axis=2))
    scaled = blocks.astype(np.float64) * np.exp2(-e.astype(np.float64))[..., None]     # exact: a power-of-two scaling of an f32
    q = torch.from_numpy(scaled.astype(np.float32).reshape(rows, k_pad)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return q.copy(), (e + 127).astype(np.uint8)


def e4m3_to_f32(q: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(q, np.uint8)).view(torch.float8_e4m3fn).to(torch.float32).numpy()


def decode(q: np.ndarray, scales: np.ndarray, K: int | None = None) -> np.ndarray:
    """(q, scales) -> f64 [rows, K] (exact)."""
    q = np.atleast_2d(q); rows, kp = q.shape
    v = e4m3_to_f32(q).astype(np.float64) * np.repeat(np.exp2(scales.astype(np.float64) - 127.0), 32, axis=1)[:, :kp]
    return v[:, :K] if K is not None else v
