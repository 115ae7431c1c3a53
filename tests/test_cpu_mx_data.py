"""What tests/test_gpu_mx_exact.py leans on, checked without a GPU (tests/mx_data.py): on every case the operands satisfy the exactness condition
(so the float64 product is the one result an f32 accumulation in any order can give), the GELU data meets its conditions, every applicable
mutant changes the expected output -- so a device result equal to the expectation is none of them -- and the host encoder agrees with the
reference encoder on the expected GELU outputs, negative zeros included."""
import numpy as np
import pytest

import mx_data as D

IDS = [D.case_id(c) for c in D.CASES]
GELU_IDS = [D.case_id(c) for c in D.GELU_CASES]


def test_case_lists_are_the_tile_edges():
    assert D.M_EDGES == (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
    assert D.N_EDGES == (1, 3, 4, 31, 32, 33, 63, 65, 127, 128, 129, 200, 257)
    assert D.K_EDGES == (32, 64, 128, 160, 192, 256, 384, 640)
    want = {(M, N, K, 4) for M in D.M_EDGES for N in (129, 200) for K in (128, 384)} | {(M, N, 192, 4) for M in (17, 129) for N in D.N_EDGES} | \
           {(65, 129, K, 4) for K in D.K_EDGES} | {(129, 200, 384, 30)}
    assert set(D.CASES) == want and len(D.CASES) == len(want)
    assert set(D.GELU_CASES) == want - {(129, 200, 384, 30)}
    assert {D.pad128(c[2]) for c in D.CASES} >= {128, 256, 384, 640}           # one K step (the prologue alone), two, three, five
    assert any(c[1] % 4 for c in D.CASES) and any(c[1] % 4 == 0 and c[1] % 128 for c in D.CASES)


def test_granule_and_bf16_rounding():
    assert list(D.granule([0.0, 1.0, 6.0, -0.75, 2.0 ** 40, 3 * 2.0 ** -30])) == [np.inf, 1.0, 2.0, 0.25, 2.0 ** 40, 2.0 ** -30]
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -20), 0.0])
    assert list(D.bf16_bits(x)) == [0x3f80, 0x3f80, 0x3f82, 0xbf81, 0]          # ties go to the even code
    assert list(D.int_codes([0, 1, -1, 6, -4, 16])) == [0x00, 0x38, 0xb8, 0x4c, 0xc8, 0x58]


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_operands_leave_one_result_and_every_gemm_mutant_changes_it(case):
    M, N, K, spread = case
    d = D.gemm_case(case)
    qa, sa, qw, sw, bias, resid, ref = (d[k] for k in ("qa", "sa", "qw", "sw", "bias", "resid", "ref"))
    kp, npad, nbr = D.pad128(K), D.pad128(N), (K + 31) // 32
    assert qa.shape == (M, kp) and sa.shape == (M, kp // 32) and qw.shape == (npad, kp) and sw.shape == (npad, kp // 32)
    # padding: columns K .. K_pad zero with scale 127, rows N .. N_pad of W zero blocks with scale 127
    assert not qa[:, K:].any() and not qw[:, K:].any() and not qw[N:].any()
    assert (sa[:, nbr:] == 127).all() and (sw[:, nbr:] == 127).all() and (sw[N:] == 127).all()
    # the scale bytes: inside 127 +- spread and using that range, neighbours differ along K and across rows, W's class changes per 32-row group
    real_a, real_w = sa[:, :nbr].astype(int), sw[:N, :nbr].astype(int)
    assert real_a.min() >= 127 - spread and real_a.max() <= 127 + spread and real_w.min() >= 127 - spread and real_w.max() <= 127 + spread
    if nbr > 1:
        assert (real_a[:, 1:] != real_a[:, :-1]).all() and (real_w[:, 1:] != real_w[:, :-1]).all()
    assert (real_a[1:] != real_a[:-1]).all() and (real_w[1:] != real_w[:-1]).all()
    cls = [int(real_w[g:g + 32].min()) for g in range(0, N, 32) if g + 3 <= N]       # (a group of fewer than 3 rows need not show all three phases)
    assert all(a != b for a, b in zip(cls, cls[1:]))
    if spread == D.SPREAD_WIDE and M > 64:
        assert real_a.max() - real_a.min() > 40 and real_w.max() - real_w.min() > 40
    # W is not A's pattern: other element range
    ea, ew = D.mxfp8.e4m3_to_f32(qa[:, :K]), D.mxfp8.e4m3_to_f32(qw[:N, :K])
    assert ea.min() >= -4 and ea.max() <= 4 and ew.min() >= -2 and ew.max() <= 6 and (ea == np.round(ea)).all() and (ew == np.round(ew)).all()
    # the exactness condition, restated
    fig = D.exactness(qa, sa, qw, sw, bias, resid, N, K)
    assert fig < 2.0 ** 24, fig
    out32 = ref + resid.astype(np.float64)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and np.array_equal(out32.astype(np.float32).astype(np.float64), out32)
    for name, mutant in D.GEMM_MUTANTS.items():
        ok, why = D.applies(name, case)
        mu = mutant(qa, sa, qw, sw, bias, N, K)
        d16 = not np.array_equal(D.bf16_bits(mu.astype(np.float32).astype(np.float64)), D.bf16_bits(ref))
        d32 = not np.array_equal((mu + resid).astype(np.float32), out32.astype(np.float32))
        if ok:
            assert d16 and d32, f"mutant {name} leaves the expected output of {case} unchanged (bf16 differs: {d16}, f32 differs: {d32})"
        else:
            assert why and not d16 and not d32, f"mutant {name} is declared inapplicable to {case} ({why}) but changes it"


@pytest.mark.parametrize("case", D.GELU_CASES, ids=GELU_IDS)
def test_gelu_data_meets_its_conditions_and_every_epilogue_mutant_changes_it(binding, case):
    M, N, K, spread = case
    d = D.gelu_case(case)
    v, q, s, dead, bias = d["v"], d["q"], d["s"], d["dead"], d["bias"]
    assert D.exactness(d["qa"], d["sa"], d["qw"], d["sw"], bias, None, N, K) < 2.0 ** 24
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    assert ((v >= 8) | (v <= -16)).all() and ((v <= -16) == dead[None, :]).all()
    # dead columns: scattered single ones (from N = 6) and every real column of block 1 (from N = 33); the others pass through
    assert N < 6 or (dead[5] and not dead[4] and (N < 7 or not dead[6]))
    assert N <= 32 or dead[32:min(N, 64)].all()
    assert not dead.all()
    npad, real = D.pad128(N), (N + 31) // 32
    y = D.gelu_values(v)
    assert np.array_equal(np.signbit(y), np.broadcast_to(dead[None, :], y.shape))          # dead: -0.0, not +0.0
    # the expected buffers: pad columns zero, whole pad blocks 127, an all-dead block scale 127 with elements 0x80
    assert q.shape == (M, npad) and s.shape == (M, npad // 32) and not q[:, N:].any() and (s[:, real:] == 127).all()
    assert (q[:, :N][:, dead] == 0x80).all()
    if N > 32:
        assert (s[:, 1] == 127).all()
    c = D.gelu_conditions(v, N)
    print(f"{D.case_id(case)}: {c}, fc2 figure 2^{np.log2(d['fc2'][4]):.1f}")
    if D.boundary_plan(M, N) is None:
        assert N == 1                                              # one column, one bias: two rows' maxima cannot both be set
    else:
        assert c["b175"] >= 1 and c["bpow2"] >= 1
    assert c["neighbours"] is None or c["neighbours"] > 0.9
    assert (c["neighbours"] is None) == (N <= 32)
    # the host encoder agrees with the reference encoder on these values, negative zeros included
    qh, sh = binding.mxfp8_quantize(y, npad)
    assert np.array_equal(qh, q) and np.array_equal(sh, s)
    for name, mutant in D.EPI_MUTANTS.items():
        ok, why = D.applies(name, case)
        qm, sm = mutant(v, N)
        changed = not (np.array_equal(qm, q) and np.array_equal(sm, s))
        if ok:
            assert changed, f"mutant {name} leaves the expected output of {case} unchanged"
        else:
            assert why and not changed, f"mutant {name} is declared inapplicable to {case} ({why}) but changes it"


def test_own_lane_mutant_rounds_like_the_reference_encoder():
    """amax_own_lane carries its own e4m3 rounding: where all four lanes of a block arrive at the block's exponent it must reproduce the
    reference encoder byte for byte (so what it changes elsewhere is the exponent, not the rounding)."""
    case = (129, 200, 192, D.SPREAD)
    d = D.gelu_case(case)
    qm, sm = D.MUTANTS["amax_own_lane"](d["v"], case[1])
    y = np.zeros(d["q"].shape, np.float32); y[:, :case[1]] = D.gelu_values(d["v"])
    e_lane = D.mxfp8.block_exp(np.abs(y.reshape(y.shape[0], -1, 2, 4, 4)).max(axis=(2, 4)))
    same = (e_lane == (d["s"].astype(np.int64) - 127)[:, :, None]).all(axis=2)
    assert same.sum() > 100 and (~same).sum() > 100
    qb, qr = qm.reshape(y.shape[0], -1, 32), d["q"].reshape(y.shape[0], -1, 32)
    assert np.array_equal(qb[same], qr[same]) and np.array_equal(sm[same], d["s"][same])


def test_every_mutant_applies_to_at_least_three_cases_and_fc2_keeps_four():
    for name in D.GEMM_MUTANTS:
        assert sum(D.applies(name, c)[0] for c in D.CASES) >= 3, name
    for name in D.EPI_MUTANTS:
        assert sum(D.applies(name, c)[0] for c in D.GELU_CASES) >= 3, name
    assert set(D.MUTANTS) == {"k_halves", "a_scale_block", "w_scale_row", "stale_scales", "drop_last_step", "row_clamp", "halves_swapped", "scale_neighbour",
                              "amax_own_lane"}
    usable = [c for c in D.GELU_CASES if D.gelu_case(c)["fc2"][4] < 2.0 ** 24]
    print(f"fc1 -> fc2: {len(usable)} of {len(D.GELU_CASES)} cases keep the second product exact")
    assert len(usable) >= 4
    # the cases the GPU test runs are exactly those: a ragged second row tile (M = 129), K = N from 1 to 63, a second block that is all dead
    assert len(set(D.FC2_CASES)) == len(D.FC2_CASES) and set(D.FC2_CASES) == set(usable)
    assert any(c[0] > 128 for c in D.FC2_CASES) and any(c[1] > 32 for c in D.FC2_CASES)
    for c in D.FC2_CASES:
        d = D.gelu_case(c)
        qw2, sw2, bias2, resid2, _ = d["fc2"]
        units = D.mxfp8.decode(d["q"], d["s"]) / D.e4m3_row_granule(d["q"], d["s"])[:, None]
        assert np.array_equal(units, np.round(units))             # the row granule divides every element of the row
        ref = D.gemm64(d["q"], d["s"], qw2, sw2, bias2, D.FC2_N, c[1], resid2)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and np.abs(ref).max() > 0
