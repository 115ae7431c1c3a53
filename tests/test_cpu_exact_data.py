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


FLAT_N = (1, 2, 3, 17, 64, 65, 193, 197, 208, 224, 225, 289, 577, 785, 1025, 4097)


def _flat_moved(q, k, v, c, hd, dn, schedule):
    """per query row: does the emulated output differ from c somewhere?"""
    out = X.attention_emu(q, k, v, 1.0 / np.sqrt(hd), dn, schedule)
    return ~(out == c).all(dim=2)


@pytest.mark.parametrize("hd", [32, 64, 128])
def test_flat_softmax_data_is_exact_and_sees_a_dropped_or_padded_key(hd):
    """flat_qkv: every value representable in both operand types, z sums to zero per column and is never zero, every raw score of an item
    is one integer; the f32 / operand-type emulation of every definition gives c bit for bit; and the sensitivity the GPU test relies on:
    a dropped key moves every output row at every N >= 2 in both types; a zero pad key (k = 0, v = 0) counted in the row sum moves every
    row for sign = -1 at every N, for sign = 0 only while c N / (N + 1) does not round back to c (bf16: up to 289 tokens, not from 577;
    f16: up to 1025, not at 4097), never for sign = +1: hence all three signs, and sign = -1 as the pad detector."""
    for N in FLAT_N:
        if N == 4097 and hd != 64:
            continue
        for sign in X.FLAT_SIGNS:
            qkv, c = X.flat_qkv(2, N, 1, hd, sign, X.attn_seed(2, N, 1, hd) + 17 * sign)
            t = torch.from_numpy(qkv)
            assert torch.equal(t.to(torch.float16).float(), t) and torch.equal(t.to(torch.bfloat16).float(), t)
            q, k, v = X.heads_of(t, 2, N, 1, hd)
            cc = torch.from_numpy(c).reshape(2, 1, hd)
            z = v - cc
            assert (z.sum(dim=1) == 0).all() and ((z != 0).all() if N > 1 else not z.any()) and z.abs().max() <= 64 and (N == 1 or z.abs().min() >= 16)
            assert cc.min() >= 1 and cc.max() <= 3 and not torch.equal(cc[0], cc[1])
            raw = q.double() @ k.double().transpose(1, 2)
            assert (raw == sign * X.flat_gain(hd) * (hd // 2)).all() and abs(abs(raw[0, 0, 0].item()) / np.sqrt(hd) - 24 * abs(sign)) < 2.5
            assert (v.abs().sum(dim=1) < 2 ** 24).all()
            assert np.array_equal(X.rows_of(cc.expand(2, N, hd).contiguous(), 2, N, 1, hd).numpy(), X.flat_expected(c, N))
            zero = torch.zeros((2, 1, hd))
            for dn, schedule in (("f16", "single"), ("bf16", "single"), ("bf16", "online"), ("f16", "precise")):
                if schedule != "single" and hd != 64:
                    continue
                what = (N, hd, sign, dn, schedule)
                assert not _flat_moved(q, k, v, cc, hd, dn, schedule).any(), what
                if N >= 2:
                    assert _flat_moved(q, k[:, :-1], v[:, :-1], cc, hd, dn, schedule).all(), what
                pad = _flat_moved(q, torch.cat([k, zero], 1), torch.cat([v, zero], 1), cc, hd, dn, schedule)
                if sign == -1:
                    assert pad.all(), what
                elif sign == 1:
                    assert not pad.any(), what
                elif N <= 289 or (dn == "f16" and N <= 1025):
                    assert pad.all(), what
                elif N >= (577 if dn == "bf16" else 4097):
                    assert not pad.any(), what


def test_attention_case_lists_meet_every_edge():
    """Every family: at least two images and two heads everywhere, three images at every edge; N % 16 in {15, 0, 1} and N % 64 in {63, 0, 1}
    inside its range; the automatic choice on both sides of each of its thresholds; a partly filled fourteenth tile with an odd head count."""
    for f, cases in X.FLAT_CASES.items():
        assert all(n_img >= 2 and H >= 2 for n_img, N, H, hd in cases), f
        ns = {N for n_img, N, H, hd in cases if n_img >= 3}
        assert {n % 16 for n in ns} >= {15, 0, 1} and {n % 64 for n in ns} >= {63, 0, 1} or f in ("auto", "persist"), f
    assert {N for _, N, _, _ in X.FLAT_CASES["auto"]} >= {192, 193, 208, 209, 224, 225, 256, 257, 288, 289}
    assert {n % 16 for _, n, _, _ in X.FLAT_CASES["persist"]} >= {15, 0, 1} and all(192 < n <= 224 for _, n, _, _ in X.FLAT_CASES["persist"])
    assert any(208 < N < 224 and H % 2 for fam in (X.FLAT_CASES, X.ATTN_CASES) for _, N, H, _ in fam["persist"])
    assert all((N + 31) // 32 in (1, 2, 3, 4, 5, 6, 7, 9, 19) for _, N, _, _ in X.FLAT_CASES["single"])
    assert all(hd != 64 for _, _, _, hd in X.FLAT_CASES["generic"]) and {hd for _, _, _, hd in X.FLAT_CASES["generic"]} >= {32, 80, 96, 128}
    for f, cases in X.SPREAD_CASES.items():
        assert cases == [c for c in X.FLAT_CASES[f] if c[1] >= X.SPREAD_MIN_N] and len(cases) >= len(X.FLAT_CASES[f]) - 1
    # what the emulation's schedule follows: the dispatcher's ranges (launch_attention, attention.hip)
    S = X.attention_schedule
    assert [S("auto", "bf16", n) for n in (192, 193, 224, 225, 256, 257, 288, 289, 577)] == ["single", "single", "single", "online", "online", "single", "single", "online", "online"]
    assert S("auto", "f16", 4097) == "single" and S("flow", "bf16", 197) == "online" and S("precise", "f16", 197) == "precise" and S("stream", "bf16", 577) == "single"


SPREAD_DISTINCT = sorted({(c[1], c[2], c[3]) for cs in X.SPREAD_CASES.values() for c in cs})


@pytest.mark.parametrize("N,H,hd", SPREAD_DISTINCT, ids=lambda v: str(v))
def test_attention_gates_see_a_leaked_key_a_dropped_key_and_a_wrong_scale(N, H, hd):
    """For every spread / peaked case (the gates do not depend on the family: one per distinct N, H, head dim, operand type and
    schedule; two images, which is what the leak needs): with the gates of test_gpu_attention.py computed from the float64 reference and
    the emulation,
      * the emulation of the definition needs at most half of the per-element bound with k = ATTN_K = 1, the smallest candidate;
      * one leaked key (token 0 of the next image; a zero key behind the last image), the dropped last key and a scale 2 % too large,
        each applied to the float64 reference, break the per-element gate or the mean gate.
    Above CPU_FULL_MAX_N tokens the first 512 query rows of every item stand for the buffer (rows are independent; the whole float64
    problem takes minutes here); test_gpu_attention.py asserts the same on the whole buffer of those cases."""
    scale = 1.0 / np.sqrt(hd)
    for kind in X.spread_kinds(N):
        x = torch.from_numpy(X.spread_qkv(2, N, H, hd, X.attn_seed(2, N, H, hd), kind))
        for dn, schedules in (("f16", ("single",)), ("bf16", ("single", "online")), ("f16", ("precise",))):
            if schedules != ("single",) and hd != 64:
                continue
            q, k, v = X.heads_of(x if schedules == ("precise",) else x.to(torch.float16 if dn == "f16" else torch.bfloat16).float(), 2, N, H, hd)
            if N > X.CPU_FULL_MAX_N:
                q = q[:, :512]
            ref, cond = X.attention_ref(q, k, v, scale, want_bound=True)
            bound = X.attention_bound(ref, cond, dn)
            faults = X.attention_faults(q, k, v, scale, 2, H)
            for schedule in schedules:
                emu = X.attention_emu(q, k, v, scale, dn, schedule)
                need, _ = X.attention_gate_ratios(emu, ref, bound, emu)
                line = f"N {N} H {H} hd {hd} {kind} {dn} {schedule}: emulation {need:.3f} of the bound;"
                assert need <= 0.5, line
                for name, out in faults.items():
                    worst, mean = X.attention_gate_ratios(out, ref, bound, emu)
                    line += f" {name} {worst:.2f} of the bound, {mean:.2f} of the emulation's mean;"
                    assert worst > 1.0 or mean > X.ATTN_MEAN_FACTOR, line
                print(line)


def test_attention_emulation_restates_the_oracle():
    """exact_data.attention_emu (single-pass) against oracle.attention in the modes that restate the engine's rounding points: same
    definition, another summation order and another exp (expf / the fp16 table against exp2), the oracle's output not rounded to the
    operand type: the two agree within one output ulp plus what two exps one f32 ulp apart do to a numerator of the operand type."""
    from oracle import oracle as O
    O.build()
    n_img, N, H, hd = 2, 197, 2, 64
    x32 = X.spread_qkv(n_img, N, H, hd, 3)
    for dn, mode, tdt in (("f16", O.GPU_F16, torch.float16), ("bf16", O.GPU_BF16, torch.bfloat16)):
        xr = torch.from_numpy(x32).to(tdt).float()
        q, k, v = X.heads_of(xr, n_img, N, H, hd)
        emu = X.rows_of(X.attention_emu(q, k, v, 0.125, dn), n_img, N, H, hd).numpy()
        ora = O.attention(xr.numpy(), n_img, N, H * hd, H, mode)
        err = np.abs(emu - ora)
        assert err.max() <= np.abs(ora).max() * X.ATTN_ULP[dn] and err.mean() <= 0.5 * np.abs(ora).mean() * X.ATTN_ULP[dn], (dn, err.max(), err.mean())


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
