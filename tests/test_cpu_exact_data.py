"""The conditions the exact and hostile-data GPU tests rely on (tests/exact_data.py), checked without a GPU: the data, not a tolerance,
is what makes those tests exact, so the data is tested."""
import numpy as np
import pytest
import torch

import exact_data as X
import test_gpu_exact as TE


def test_gemm_sums_are_exact_in_f32_for_every_case():
    for M, M_real, N, K in X.gemm_small_cases() + X.gemm_wide_cases():
        assert K <= 3072 and M % 128 == 0 and 0 < M_real <= M and N % 4 == 0 and K % 64 == 0
        for variant in X.VARIANTS:
            assert X.gemm_bound(K, variant) < 2 ** 24, (M, N, K, variant)
    for P, cin, S, n in X.PATCH_CASES:
        assert X.patch_bound(P, cin) < 2 ** 24
    # the generators keep to the ranges the bound assumes, and are exact in both operand types
    a, w, bias, resid, pos = X.gemm_operands(128, 60, 192, 50, 1)
    assert np.abs(a).max() <= X.A_MAX and np.abs(w).max() <= X.W_MAX and np.abs(bias).max() <= X.BIAS_MAX
    assert max(np.abs(resid).max(), np.abs(pos).max()) <= X.RESID_MAX < 2 ** 16
    for arr in (a, w):
        for sc in (1.0, 2.0 ** -3, 2.0 ** -5):
            t = torch.from_numpy(arr * np.float32(sc))
            assert torch.equal(t.to(torch.float16).float(), t) and torch.equal(t.to(torch.bfloat16).float(), t)


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("variant", list(X.VARIANTS))
def test_hi_lo_planes_hold_every_possible_value_exactly(variant, tdt):
    """Epilogue 5: hi = round(v), lo = round((v - hi) * 2048); on every value acc + bias can take, hi + lo / 2048 == v."""
    v = torch.from_numpy(X.hilo_values(variant))
    hi = v.to(tdt)
    assert torch.isfinite(hi.float()).all()
    lo = ((v - hi.float()) * 2048.0).to(tdt)
    assert torch.equal(hi.float() + lo.float() / 2048.0, v)
    assert (hi.float() != v).any()                       # the hi plane alone does round: the lo plane is needed


def test_shape_list_covers_every_axis_value_and_dispatcher_edge():
    small, wide = X.gemm_small_cases(), X.gemm_wide_cases()
    assert {c[1] for c in small} == set(X.M_REAL_VALUES)
    assert {c[2] for c in small} == set(X.N_VALUES)
    assert {c[3] for c in small} == set(X.K_VALUES)
    for M, M_real, N, K in small:
        assert M in (X.round_up(M_real, 128), X.round_up(M_real, 256))
    for m_real in X.M_REAL_VALUES:                       # both roundings of every M_real
        assert {X.round_up(m_real, 128), X.round_up(m_real, 256)} == {c[0] for c in small if c[1] == m_real}
    # a forced 256-row family must refuse the odd multiples of 128, and some shape must be refused for K
    assert any(M % 256 for M, _, _, _ in small) and any(K < 128 for _, _, _, K in small) and any(K % 128 for _, _, _, K in small)
    # wide shapes: N = 256 with 127 / 128 / 256 / 257 row tiles, N = 768 with 85 / 86 / 113 / 171, full and ragged
    for n, tiles in ((256, (127, 128, 256, 257)), (768, (85, 86, 113, 171))):
        for t in tiles:
            assert (t * 256, t * 256, n) in {c[:3] for c in wide} and (t * 256, t * 256 - 100, n) in {c[:3] for c in wide}
    assert not X.is_wide(127 * 256, 256, 128) and X.is_wide(128 * 256, 256, 128)
    assert all(X.is_wide(c[0], c[2], c[3]) for c in wide if c[0] != 127 * 256)
    # kernel 2 takes its two-launch path on a 256-CU device for the VERDICT's 339 tiles and for 257 tiles
    assert X.tail_split_rows(113 * 256, 768, 256) == 85 * 256
    assert X.tail_split_rows(257 * 256, 256, 256) == 256 * 256
    assert X.tail_split_rows(256 * 256, 256, 256) == 0
    # every (family, epilogue, type) runs every shape its family takes: each family must take a ragged-row and a ragged-column shape
    for kernel in X.KERNELS:
        took = [c for c in small + wide if TE.family_takes(kernel, c[0], c[3])]
        assert any(c[1] % 256 for c in took) and any(c[2] % 256 for c in took), kernel
        assert any(c[1] % 256 and c[2] % 256 for c in took), kernel
        if TE.FAMILY_RULES.get(kernel, (0,))[0] == 256:       # ... and refuse the odd multiples of 128
            assert any(not TE.family_takes(kernel, c[0], c[3]) for c in small), kernel


def test_q4_0_blocks_decode_to_the_integers():
    import _pkg
    G = _pkg.load().ggml_file
    for exp in (0, -5):
        qs, ds, w = X.q4_0_planes(40, 128, 192, exp, 3)
        raw = np.concatenate([ds[:40, :, None].view(np.uint8).reshape(40, 6, 2), qs[:40]], axis=2).tobytes()        # the file's 18-byte blocks
        assert np.array_equal(G.dequantize(2, raw, 40 * 192).reshape(40, 192), w)
        assert not qs[40:].any() and not ds[40:].any() and np.abs(w).max() <= 4 * 2.0 ** exp


def test_patch_cases_have_the_edges():
    for P, cin, S, n in X.PATCH_CASES:
        tpi = (S // P) ** 2
        last, on_edge = X.patch_edges(tpi, n)
        assert S % P == 0 and last != 0 and on_edge and max(on_edge) < n - 1, (P, cin, S, n)
        assert cin == 3 or tpi + 1 >= 25
    assert {(P * cin) % 16 == 0 for P, cin, _, _ in X.PATCH_CASES} == {True, False}          # the 64-byte gather and the per-element gather
    assert {(16, 3), (32, 3), (16, 1), (8, 3), (14, 3)} == {(P, cin) for P, cin, _, _ in X.PATCH_CASES}
    t = X.patch_tensors(8, 4, 3, 5, 0)
    img = X.patch_images(2, 8, 3, 1)
    ref = X.patch_embed_ref(img, t, 4)
    w = t["patch_embed.proj.weight"]
    want = (img[1, 4:8, 0:4].transpose(2, 0, 1) * w[5]).sum() + t["patch_embed.proj.bias"][5] + t["pos_embed"][0, 3, 5]      # image 1, patch (1, 0)
    assert ref.shape == (2, 5, 8) and ref[1, 3, 5] == want


@pytest.mark.parametrize("family", list(X.ATTN_CASES))
def test_attention_routing_gap(family):
    """gap >= 40: every other probability is below e^-40 = 4.2e-18, and 4097 of them times |v| <= 7 stay below half an f32 ulp of the
    smallest |v| = 0.25 (1.2e-13 against 1.5e-8) and of the 1 in the denominator."""
    for n_img, N, H, hd in X.ATTN_CASES[family]:
        qkv, perm, gap = X.routing_qkv(n_img, N, H, hd, X.attn_seed(n_img, N, H, hd), rows0_only=family in ("cls", "map"))
        assert gap >= X.MIN_GAP, (family, n_img, N, H, hd, gap)
        assert N <= 4097
        t = torch.from_numpy(qkv)
        assert torch.equal(t.to(torch.float16).float(), t) and torch.equal(t.to(torch.bfloat16).float(), t)
        v = qkv.reshape(n_img * N, 3, -1)[:, 2]
        assert 0.25 <= np.abs(v).min() and np.abs(v).max() <= 7.0
        assert 4097 * np.exp(-X.MIN_GAP) * 7.0 < 0.25 * 2.0 ** -25
        if N <= 1025 and n_img * H <= 6:                       # the float64 softmax agrees that the output is the routed row
            assert np.abs(X.attention64(qkv, n_img, N, H, hd) - X.routed(qkv, perm, n_img, N, H, hd))[::(1 if family not in ("cls", "map") else N)].max() < 1e-12


def test_issue_gaps_at_head_dim_64():
    for N, want in ((197, 136), (577, 112), (1025, 112), (4097, 96)):
        assert X.routing_qkv(1, N, 1, 64, X.attn_seed(1, N, 1, 64))[2] == want


@pytest.mark.parametrize("D", [256, 512, 768, 1024])
def test_layernorm_bound_is_pinned_by_an_f32_emulation(D):
    """The tolerance of the hostile-row LayerNorm tests is set by the problem's conditioning, not by the kernels: an f32 emulation of the
    tiled two-pass definition stays below half of it on every row kind."""
    x, kind = X.hostile_matrix(D)
    w, b = X.ln_params(D)
    y64, rstd, xmax = X.layernorm64(x, w, b)
    y32 = X.ln_tiled_f32(x, w, b)
    assert np.isfinite(y32).all()
    cond = X.ln_cond(w, rstd, xmax) + 1e-6
    ratio = np.abs(y32 - y64) / cond
    for i, name in enumerate(X.ROW_KINDS):
        r = float(ratio[kind == i].max())
        print(f"D {D} {name}: f32 emulation uses {r:.3f} of the bound")
        assert r < 0.5, (name, r)
    assert len(set(X.LN_WIDTHS)) == 19


def test_hostile_rows_are_what_they_say():
    D = 768
    for k in X.ROW_KINDS:
        x = X.hostile_rows(k, 64, D)
        assert x.shape == (64, D) and x.dtype == np.float32 and np.isfinite(x).all() and np.abs(x).max() < 1e18
    assert (X.hostile_rows("const", 64, D) == 3.25).all() and not X.hostile_rows("zero", 64, D).any()
    assert np.abs(X.hostile_rows("outlier_ch", 64, D)).max() > 100 and X.hostile_rows("offset", 64, D).min() > 990
    t = X.hostile_rows("tile_step", 64, D)
    assert t[:, :256].mean() - t[:, 256:].mean() > 49


def test_gelu_sweep_covers_the_domain():
    for bf in (False, True):
        v = X.gelu_sweep(bf)
        assert v.size % 256 == 0 and np.isfinite(v).all()
        assert np.abs(v).max() == (60000.0 if not bf else np.abs(v).max()) and (np.abs(v).max() > 9e29) == bf
        nz = np.abs(v[v != 0])
        assert nz.min() <= 2.0 ** -24 and ((v > -0.76) & (v < -0.74)).sum() >= 4
        assert np.signbit(v[v == 0]).any() and (~np.signbit(v[v == 0])).any()
        assert ((v >= -6) & (v <= 6)).sum() >= 4096
    assert abs(X.gelu64(-0.7517916) + 0.17004) < 1e-4 and X.gelu64(-40.0) == 0.0
