"""Image embeddings and token features on the host side (no GPU): the C ABI symbols and flags, the argument checks that come before any
device call, the CLI's options, and the two conditions the GPU tests' bounds rest on (tests/feature_data.py):
  - the f32 restatement of the kernels' LayerNorm definition stays within half of exact_data.ln_bound (f32 output) on the inputs the GPU test uses;
  - a fixed-order f32 pooled mean stays within the bound the contract states for it."""
import os
import re

import numpy as np
import pytest

import exact_data as X
import feature_data as FD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = 3, 5
FUNCS = ("vitx_feat_enable", "vitx_feat_floats", "vitx_feat_images", "vitx_feat_read", "vitx_feat_device", "vitx_op_features")


def test_header_declares_the_feature_functions_and_flags(binding):
    hdr = open(os.path.join(ROOT, "include", "vitx.h")).read()
    for s in FUNCS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in binding.EXPORTS and hasattr(binding.lib(), s), s
    for name, val in (("VITX_FEAT_CLS", 1), ("VITX_FEAT_MEAN", 2), ("VITX_FEAT_TOKENS", 4), ("VITX_FEAT_L2", 8)):
        assert f"#define {name} {val}" in hdr
    assert (binding.FEAT_CLS, binding.FEAT_MEAN, binding.FEAT_TOKENS, binding.FEAT_L2) == (1, 2, 4, 8)
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH]).decode()
    for s in FUNCS:
        assert re.search(r" T %s$" % s, out, re.M), s
    assert "vit_embed_batch" in subprocess.check_output(["nm", "-DC", binding.LIB_PATH]).decode()


def test_feature_calls_without_a_context_are_argument_errors(binding):
    L = binding.lib()
    assert L.vitx_feat_enable(None, 1, 0) == ERR_ARG
    assert L.vitx_feat_floats(None) == 0 and L.vitx_feat_images(None) == 0 and L.vitx_feat_device(None) is None
    assert L.vitx_feat_read(None, None, 0) == ERR_ARG


def test_op_features_argument_checks_come_before_any_device_call(binding):
    """NULL pointers, N == 1 with a mean or token output, misaligned pointers, odd strides: VITX_ERR_ARG; a hidden size without an
    instantiation: VITX_ERR_UNSUPPORTED.  The pointers are never dereferenced on the host: any aligned non-zero value serves."""
    L = binding.lib()
    p, q = 0x10000, 0x20000
    args = lambda **kw: [kw.get(k, d) for k, d in (("x", p), ("rs", 768), ("is_", 197 * 768), ("w", p), ("b", p), ("cls", q), ("mean", None), ("tok", None),
                                                     ("os", 768), ("n", 2), ("N", 197), ("D", 768), ("eps", 1e-6), ("l2", 0), ("st", None))]
    for bad in (dict(x=None), dict(w=None), dict(b=None), dict(cls=None), dict(n=0), dict(N=0), dict(D=0),
                dict(N=1, mean=q), dict(N=1, tok=q), dict(N=1, cls=None, mean=q),
                dict(x=p + 4), dict(cls=q + 8), dict(mean=q + 4), dict(rs=770), dict(is_=197 * 768 + 2), dict(os=769)):
        assert L.vitx_op_features(*args(**bad)) == ERR_ARG, bad
    for D in (100, 96, 4096, 832):
        assert L.vitx_op_features(*args(D=D, rs=D, is_=197 * D, os=D)) == ERR_UNSUPPORTED, D
    assert b"hidden size" in L.vitx_last_error()


def test_cli_accepts_and_rejects_the_embed_options(pkg, tmp_path, capsys):
    from vitcpp_amd import cli
    none = str(tmp_path / "none.gguf")
    out = str(tmp_path / "e.npy")
    # accepted: parsing succeeds and the run ends at the missing model file (exit code 1, as the reference's main does)
    for extra in (["--embed", out], ["--embed", out, "--embed-kind", "mean", "--embed-l2"], ["--embed", out, "--embed-kind", "tokens"],
                  ["--dir", str(tmp_path), "--embed", out, "--embed-kind", "cls", "--embed-l2"]):
        assert cli.main(["-m", none] + extra) == 1, extra
    capsys.readouterr()
    for extra, word in ((["--embed-kind", "mean"], "--embed"), (["--embed-l2"], "--embed"), (["--embed", out, "--embed-kind", "pooled"], "--embed-kind"),
                        (["--embed", out, "--embed-kind", "tokens", "--embed-l2"], "--embed-l2"), (["--embed"], "--embed")):
        with pytest.raises(SystemExit) as e:
            cli.main(["-m", none] + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
    assert not os.path.exists(out)


@pytest.mark.parametrize("D", [256, 512, 768, 1024])
def test_f32_restatement_of_the_layernorm_stays_within_half_the_bound_on_the_gpu_tests_inputs(D):
    """exact_data.ln_tiled_f32 (the kernels' definition, every operation rounded to f32, NOT rounded to an operand type) against float64 on the
    images tests/test_gpu_features.py feeds the kernel: at most 0.5 x exact_data.ln_bound with ulp_out = 2^-23.  The GPU test asserts 1.0."""
    w, b = X.ln_params(D)
    worst = 0.0
    for N in FD.OP_TOKENS:
        n_img = 8 if N <= 65 else 3
        for x in (FD.mixed_images(D, n_img, N, seed=N), FD.random_images(D, n_img, N, seed=N)):
            y = X.ln_tiled_f32(x.reshape(n_img * N, D), w, b).reshape(x.shape)
            y64, bound = FD.features64(x, w, b)
            assert np.isfinite(y).all()
            worst = max(worst, float((np.abs(y - y64) / bound).max()))
    print(f"D {D}: f32 restatement / bound = {worst:.3f}")
    assert worst <= 0.5, worst


def test_mixed_images_hold_every_row_kind_in_every_image():
    x = FD.mixed_images(768, 3, 17)
    hm, _ = X.hostile_matrix(768)
    per = hm.reshape(len(X.ROW_KINDS), 64, 768)
    for img in x:
        kinds = {k for r in img for k in range(len(X.ROW_KINDS)) if (per[k] == r).all(axis=1).any()}
        assert kinds == set(range(len(X.ROW_KINDS)))


@pytest.mark.parametrize("D", [256, 512, 768, 1024])
def test_fixed_order_f32_pooled_mean_stays_within_its_bound(D):
    """|d_i| <= 2^-24 ((N - 1) mean_t |F[t][i]| + 2 |mean_i|) for fixed-order f32 sums of the f32 features of hostile and random images: one
    sequential sum (waves = 1), and the 8- and 16-wave orders of the kernel."""
    w, b = X.ln_params(D)
    for N in (2, 17, 65, 197):
        for x in (FD.mixed_images(D, 4, N, seed=N), FD.random_images(D, 4, N, seed=N)):
            tok = X.ln_tiled_f32(x.reshape(4 * N, D), w, b).reshape(4, N, D)[:, 1:]
            m64, mb = FD.mean_bound(tok)
            for waves in (1, 8, 16):
                assert (np.abs(FD.pooled_f32(tok, waves) - m64) <= mb).all(), (N, waves)
