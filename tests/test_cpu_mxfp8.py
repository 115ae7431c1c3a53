"""MXFP8 operand type (include/vitx.h, VITX_MXFP8), host side: the C++ encoder against the independent reference (vit.cpp_amd/mxfp8.py)
on adversarial blocks, the decode error bound, the header and exports, argument errors and the CLI choice."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 3


def adversarial_rows():
    """Rows of 192 values (K not a multiple of 128: 64 padding columns), one kind of block per 32 columns."""
    rng = np.random.default_rng(7)
    rows = []
    rows.append(np.zeros(192, np.float32))                                                   # all zeros
    r = np.zeros(192, np.float32); r[3] = 1.0; r[40] = -3.5e-3; r[100] = 2.0 ** -140; rows.append(r)   # single nonzero elements
    for k in (-130, -20, 0, 7, 100):                                                        # maxima at, just under, just over 1.75 * 2^k
        r = (rng.standard_normal(192) * 2.0 ** (k - 2)).astype(np.float32)
        at = np.float32(1.75 * 2.0 ** k) if k > -126 else np.float32(1.75) * np.float32(2.0 ** k)
        r[0] = at; r[32] = np.nextafter(at, np.float32(0)); r[64] = -np.nextafter(at, np.float32(np.inf))
        r[96] = np.float32(2.0 ** k); r[128] = np.nextafter(np.float32(2.0 ** (k + 1)), np.float32(0)); r[160] = -np.float32(1.5 * 2.0 ** k)
        rows.append(r)
    sub = np.array([1e-45, 3e-44, 1.1754942e-38, 5.877e-39, 1e-40], np.float32)               # f32 subnormals
    r = np.resize(sub, 192).astype(np.float32) * np.resize([1, -1, 1], 192).astype(np.float32); rows.append(r)
    r = np.full(192, 3.3e38, np.float32); r[1::3] = -np.float32(3.4028235e38); r[2::5] = 1.0; rows.append(r)   # near FLT_MAX
    # RNE ties in e4m3: with the block maximum 256 (e = 0), e4m3 steps are 2^-9 .. 32; put values exactly halfway between codes
    r = np.zeros(192, np.float32)
    r[0::32] = 256.0
    ties = np.array([1.0625, 1.1875, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 0.0029296875, 232.0, 240.0 + 8.0, -1.0625, -17.0], np.float32)
    for b in range(6):
        r[b * 32 + 1: b * 32 + 1 + len(ties)] = ties
    rows.append(r)
    rows.append((rng.standard_normal(192) * np.exp2(rng.integers(-30, 30, 192))).astype(np.float32))   # mixed signs and magnitudes
    return np.stack(rows)


def test_host_encoder_matches_reference_bit_for_bit(pkg, binding):
    from vitcpp_amd import mxfp8
    x = adversarial_rows()
    for k_pad in (256, 384):
        q, s = binding.mxfp8_quantize(x, k_pad)
        qr, sr = mxfp8.encode(x, k_pad)
        assert q.shape == (x.shape[0], k_pad) and s.shape == (x.shape[0], k_pad // 32)
        np.testing.assert_array_equal(s, sr)
        np.testing.assert_array_equal(q, qr)
        assert (q[:, 192:] == 0).all() and (s[:, 6:] == 127).all()          # padding: zero elements, scale 127
    assert (s[0] == 127).all() and (q[0] == 0).all()                        # an all-zero block
    # the boundary rule: m <= 1.75 -> e = E - 8 (1.75 * 2^k encodes as 448 = 0x7e), just over -> e = E - 7
    q, s = binding.mxfp8_quantize(np.array([[1.75 * 4.0] + [0.0] * 31, [np.nextafter(np.float32(7.0), np.float32(8.0))] + [0.0] * 31], np.float32))
    assert s[0, 0] == 127 + 2 - 8 and q[0, 0] == 0x7e
    assert s[1, 0] == 127 + 2 - 7 and q[1, 0] == 0x76                      # 7.0000005 * 2^5 = 224.00002 -> 224 = 1.75 * 2^7 = 0x76


def test_decode_error_is_within_half_an_e4m3_ulp(pkg, binding):
    from vitcpp_amd import mxfp8
    rng = np.random.default_rng(3)
    x = np.concatenate([adversarial_rows()[:, :192], (rng.standard_normal((32, 192)) * np.exp2(rng.integers(-60, 60, (32, 1)))).astype(np.float32)])
    q, s = binding.mxfp8_quantize(x)
    dec = mxfp8.decode(q, s, 192)
    e = np.repeat(s[:, :6].astype(np.float64) - 127.0, 32, axis=1)
    y = np.abs(x.astype(np.float64)) * np.exp2(-e)                          # the scaled magnitude that was rounded
    assert y.max() <= 448.0
    ulp = np.where(y < 2.0 ** -6, 2.0 ** -9, np.exp2(np.floor(np.log2(np.maximum(y, 2.0 ** -6))) - 3))
    err = np.abs(dec - x.astype(np.float64)) * np.exp2(-e)
    assert (err <= 0.5 * ulp).all(), float((err / ulp).max())


def test_header_declares_mxfp8_and_symbols_are_exported(pkg, binding):
    h = open(os.path.join(ROOT, "include", "vitx.h")).read()
    assert re.search(r"VITX_MXFP8\s*=\s*2", h)
    for sym in ("vitx_mxfp8_quantize", "vitx_op_quantize_mxfp8", "vitx_op_layernorm_mxfp8", "vitx_op_gemm_mxfp8"):
        assert sym in binding.EXPORTS and re.search(r"\b%s\s*\(" % sym, h), sym
        assert hasattr(binding.lib(), sym), sym
    assert binding.MXFP8 == 2


def test_null_and_bad_arguments_give_err_arg(pkg, binding):
    L = binding.lib()
    assert L.vitx_mxfp8_quantize(None, 1, 32, 128, None, None) == ERR_ARG
    x = np.zeros((2, 64), np.float32); q = np.zeros(256, np.uint8); s = np.zeros(8, np.uint8)
    import ctypes as C
    xp, qp, sp = x.ctypes.data_as(C.POINTER(C.c_float)), q.ctypes.data_as(C.POINTER(C.c_uint8)), s.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.vitx_mxfp8_quantize(xp, 2, 64, 48, qp, sp) == ERR_ARG          # k_pad not a multiple of 32
    assert L.vitx_mxfp8_quantize(xp, 2, 64, 32, qp, sp) == ERR_ARG          # k_pad < K
    assert L.vitx_mxfp8_quantize(xp, 2, 64, 128, qp, sp) == 0
    assert L.vitx_op_quantize_mxfp8(None, 1, 32, 128, None, None, None) == ERR_ARG
    assert L.vitx_op_layernorm_mxfp8(None, None, None, None, None, 4, 768, 1e-6, None) == ERR_ARG
    assert L.vitx_op_gemm_mxfp8(0, None, None, None, None, None, None, None, 128, 768, 768, None) == ERR_ARG


def test_cli_accepts_dtype_mxfp8(pkg, tmp_path):
    from vitcpp_amd import cli
    # argparse accepts the choice (an unknown one exits with status 2); the missing model then fails the load with status 1
    assert cli.main(["-m", str(tmp_path / "missing.gguf"), "--dtype", "mxfp8"]) == 1
    with pytest.raises(SystemExit) as e:
        cli.main(["-m", str(tmp_path / "missing.gguf"), "--dtype", "fp8"])
    assert e.value.code == 2
