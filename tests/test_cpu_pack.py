"""Packed batches, the host side (include/vitx.h "packed batches"): every refusal vitx_pack_check makes, row0 of a mixed list with and without
register tokens, the distinct-grid count a forward compares with max_grids, pack_images against rect_shape, and the 4-head fixture variants.
For tests/test_gpu_pack_scale.py: the dispatcher's rule restated (pack_data.gemm_family), the ladder of row counts and its packs, the half-gate
precondition and the mutants' distances on the probes, and the call sequences that restart the rotary arena and evict."""
import numpy as np
import pytest

import pack_data as KD
import prefix_data as PD
import preproc_data as PPD
import rect_data as XD
import text_data as TD
import wide_data as WD


def _model(pkg, binding, kind):
    return binding.Model(XD.fixture_file(pkg, kind))


def _refused(binding, model, shapes, max_tokens, max_images):
    with pytest.raises(binding.VitxError) as ei:
        binding.pack_check(model, shapes, max_tokens, max_images)
    return ei.value.code


@pytest.mark.parametrize("kind,registers", [("p16", 0), ("p14r4", 4)])
def test_row0_of_a_mixed_list(pkg, binding, kind, registers):
    model = _model(pkg, binding, kind)
    P = model.hparams.patch_size
    shapes = KD.mixed_shapes(P)
    want = KD.row0_of(shapes, P, registers)
    assert want[-1] == sum(g + 1 + registers for g in (1, 7, 10, 16, 10, 16, 1))
    got = binding.pack_check(model, shapes, int(want[-1]), len(shapes))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(binding.pack_check(model, shapes[::-1], 10 ** 6, 64), KD.row0_of(shapes[::-1], P, registers))
    assert np.array_equal(binding.pack_check(model, shapes[:1], 10 ** 6, 1), [0, 2 + registers])
    model.close()


def test_every_refusal_of_a_forward_call(pkg, binding):
    model = _model(pkg, binding, "p14r4")
    P = 14
    shapes = KD.mixed_shapes(P)
    rows = int(KD.row0_of(shapes, P, 4)[-1])
    ARG = binding.ERR_ARG
    for bad in ((P + 1, P), (P, P - 1), (0, P), (P, 0), (-P, P), (P, -P), (16, 16)):      # not a positive multiple of the patch size (16: the other fixture's)
        assert _refused(binding, model, shapes[:3] + [bad] + shapes[3:], 10 ** 6, 64) == ARG, bad
        assert "patch size" in str(binding.lib().vitx_last_error())
    assert _refused(binding, model, shapes, 10 ** 6, len(shapes) - 1) == ARG              # n above max_images
    assert _refused(binding, model, shapes, rows - 1, 64) == ARG                          # one token above max_tokens
    assert "max_tokens" in str(binding.lib().vitx_last_error())
    assert binding.pack_check(model, shapes, rows, len(shapes))[-1] == rows               # both bounds are inclusive
    L = binding.lib()
    import ctypes as C
    s = np.ascontiguousarray(shapes, np.int32)
    i32p = C.POINTER(C.c_int32)
    assert L.vitx_pack_check(model._h, s.ctypes.data_as(i32p), 0, 10 ** 6, 64, None) == ARG       # n = 0
    assert L.vitx_pack_check(model._h, s.ctypes.data_as(i32p), -1, 10 ** 6, 64, None) == ARG
    assert L.vitx_pack_check(model._h, None, 1, 10 ** 6, 64, None) == ARG
    assert L.vitx_pack_check(None, s.ctypes.data_as(i32p), 1, 10 ** 6, 64, None) == ARG
    assert L.vitx_pack_check(model._h, s.ctypes.data_as(i32p), len(shapes), 10 ** 6, 64, None) == 0      # row0 may be NULL
    model.close()
    text = binding.Model(TD.text_file(pkg, "clip"))
    assert _refused(binding, text, [(16, 16)], 10 ** 6, 4) == ARG                         # a text model
    assert "text" in str(binding.lib().vitx_last_error())
    text.close()


def test_distinct_grids_against_max_grids(pkg, binding):
    """What a forward compares with its context's max_grids: the mixed pack names five grids, twins and transposes counted as they are."""
    model = _model(pkg, binding, "p16")
    P = 16
    assert binding.pack_distinct_grids(model, KD.mixed_shapes(P)) == 5
    assert binding.pack_distinct_grids(model, [(P, 2 * P), (2 * P, P)]) == 2              # a grid and its transpose are two
    assert binding.pack_distinct_grids(model, [(3 * P, 2 * P)] * 9) == 1
    assert binding.pack_distinct_grids(model, [(P, k * P) for k in range(1, 41)]) == 40   # above the default cache of 32: such a call is refused
    model.close()


def test_pack_images_shapes_are_rect_shape(pkg, binding):
    pp = binding.Preproc.make(resize_a=16, resize_b=16, filter=binding.PP_PIL_BICUBIC, mean255=(127.5,) * 3, std255=(127.5,) * 3)
    srcs = [PPD.image("random", nx, ny, seed=nx) for nx, ny in ((50, 37), (37, 50), (40, 40), (90, 31))]
    for P, short in ((16, 32), (14, 28)):
        pixels, shapes = binding.pack_images(srcs, pp, short, patch=P)
        assert shapes.dtype == np.int32 and shapes.shape == (4, 2)
        at = 0
        for img, (h, w) in zip(srcs, shapes):
            assert (w, h) == binding.rect_shape(img.shape[1], img.shape[0], P, short) and min(h, w) == short and h % P == 0 and w % P == 0
            one = binding.preprocess_rect(img, pp, w, h)
            assert np.array_equal(pixels[at:at + one.size].view(np.uint32), one.ravel().view(np.uint32))
            at += one.size
        assert at == pixels.size
    capped = binding.pack_images(srcs[3:], pp, 32, 48, patch=16)[1]
    assert tuple(capped[0]) == binding.rect_shape(90, 31, 16, 32, 48)[::-1] and max(capped[0]) == 48


@pytest.mark.parametrize("kind", KD.VARIANTS)
def test_the_four_head_variants_load(pkg, binding, kind):
    """The variants are the two-head fixtures' tensors under a header with 4 heads: head dim 32, everything else as filed."""
    model = binding.Model(KD.variant_file(pkg, kind))
    hp = model.hparams
    assert (hp.hidden_size, hp.num_hidden_layers, hp.num_attention_heads) == (128, 2, KD.HEADS4)
    assert model.head_pool == binding.POOL_CLS and model.in_channels == 3
    assert (model.glu is not None) == (kind == "gluh4") and bool(model.has_pre_norm) == (kind == "preerfh4")
    assert (model.rope is not None) == (kind in ("p14ropeh4", "gluh4"))
    model.close()


# ------------------------------------------------------------------------------------------------ large packs (tests/test_gpu_pack_scale.py leans on these)
ORDER = {122: 0, 245: 1, "pp": 2}


def test_gemm_family_restates_the_dispatcher():
    """What gemm.hip states in words: a column count that is no multiple of 256 stays on the 64 x 128 tiles at any row count (the D = 128 micro
    fixtures: 384, 128, 128, and 512 = fc1); at D = 512 every GEMM climbs 122 -> 245 -> pp, never back, 245 from 128 tiles of 128 x 256, pp from 128
    tiles of 256 x 256; a K that is no multiple of 128 never takes the ping-pong kernel."""
    for N, K in ((384, 128), (128, 128), (128, 512)):
        assert {KD.gemm_family(M, N, K) for M in range(256, 1 << 17, 256)} == {122}, (N, K)
    assert KD.gemm_family(256, 512, 128) == 122 and KD.gemm_family(1 << 16, 512, 128) == "pp"      # D = 128's fc1 is not pinned
    for key in KD.SCALE_KEYS:
        for nm, (N, K) in KD.layer_gemms(key).items():
            fam = [KD.gemm_family(M, N, K) for M in range(256, 1 << 15, 256)]
            assert [ORDER[f] for f in fam] == sorted(ORDER[f] for f in fam) and set(fam) == set(ORDER), (key, nm)
            first = {f: 256 * (1 + fam.index(f)) for f in (245, "pp")}
            assert first[245] // 128 * (N // 256) >= 128 > (first[245] - 256) // 128 * (N // 256), (key, nm, first)
            assert first["pp"] // 256 * (N // 256) >= 128 > (first["pp"] - 256) // 256 * (N // 256), (key, nm, first)
    assert KD.gemm_family(1 << 15, 512, WD.F_ODD) in (445, 945)                                      # glu_odd's fc2: wide, but K % 128 != 0
    assert KD.layer_gemms("glu_hplus")["fc1"] == (2816, 512) and KD.layer_gemms("glu_hplus")["fc2"] == (512, 1408)


@pytest.mark.parametrize("key", KD.SCALE_KEYS)
def test_ladder_walks_every_family_combination(key):
    lad, th = KD.ladder(key), KD.thresholds(key)
    combos = lambda rows: tuple(KD.families(key, rows).values())
    every = {combos(M) for M in range(256, th[-1] + 257, 256)}
    assert lad == sorted(lad) and len(every) == len(th) + 1
    assert combos(lad[0]) == (122,) * 4 and combos(lad[-1]) == ("pp",) * 4
    if key == "vit_erf":
        assert len(every) == 7 and {combos(r) for r in lad} == every
        padded = {KD.round_up(r, 256) for r in lad}
        assert all(t - 256 in padded and t in padded for t in th), (th, sorted(padded))          # the last block below and the first at every switch
    else:
        assert len(lad) == 3 and combos(lad[1]) not in ((122,) * 4, ("pp",) * 4)
    assert {0, 1, 255} <= {r % 256 for r in lad}
    assert lad[-1] * WD.P * WD.P * 3 * 4 < 52 << 20                                               # the pixels of the top rung


@pytest.mark.parametrize("key", KD.SCALE_KEYS)
def test_packs_of_the_ladder(key):
    """Every rung's pack: exactly the rung's rows; every probe once, one first and one last; no image next to a copy of itself; runs of one shape
    and single images both occur; the 14 x 14 probe's segment has a multiple of 256 strictly inside; the reference calls are one row block each."""
    Tp = KD.prefix_rows(key)
    assert len(set(KD.PROBE_GRIDS)) == 6 and len(KD.FILLER_GRIDS) <= 8 and len(set(KD.FILLER_GRIDS)) <= 4
    imgs = KD.distinct_images()
    assert all(not np.array_equal(imgs[i], imgs[j]) for i in range(KD.N_DISTINCT) for j in range(i) if KD.GRIDS[i] == KD.GRIDS[j])
    for rows in KD.ladder(key):
        ids = KD.pack_ids(rows, Tp)
        assert KD.rows_of(ids, Tp) == rows and len(ids) <= KD.max_images(key)
        assert ids[0] < KD.N_PROBES and ids[-1] < KD.N_PROBES and sorted(i for i in ids if i < KD.N_PROBES) == list(range(KD.N_PROBES))
        assert all(a != b for a, b in zip(ids, ids[1:]))
        shapes = KD.shapes_of(ids)
        same = [a == b for a, b in zip(shapes, shapes[1:])]
        assert any(same) and not all(same) and 1 < KD.pe_runs(shapes) < len(ids)
        r0 = KD.row0_of_ids(ids, Tp)
        k = ids.index(1)
        assert r0[k] // 256 < (r0[k + 1] - 1) // 256 and r0[k] % 256 != 0, (rows, r0[k], r0[k + 1])
        assert (r0[-1] - 1) // 256 == (rows - 1) // 256                                           # the last probe ends on the last (ragged) block
        assert len(set(r0[1:-1] // 256)) > 1 and KD.poisoned(ids) and all(ids[k] >= KD.N_PROBES for k in KD.poisoned(ids))
    calls = KD.reference_calls(Tp)
    assert sorted(i for c in calls for i in c) == list(range(KD.N_DISTINCT))
    for c in calls:
        assert KD.rows_of(c, Tp) <= 256 and set(KD.families(key, KD.rows_of(c, Tp)).values()) == {122}
    small = KD.small_pack_ids(Tp)
    n, rows = len(small), KD.rows_of(small, Tp)
    assert 256 < n <= 1300 and KD.round_up(n, 256) > 256 and 9 <= int(np.ceil(np.log2(n + 1))) <= 11
    assert all(KD.GRIDS[i] == (1, 1) for i in small) and len(set(small)) == 3 and all(a != b for a, b in zip(small, small[1:]))
    assert 245 in KD.families(key, rows).values() and rows <= KD.ladder(key)[-1]


def _scale_tensors(pkg, key):
    return PD.file_tensors(pkg, WD.fixture_file(pkg, key))


@pytest.mark.parametrize("key", KD.SCALE_KEYS)
def test_scale_probe_preconditions(pkg, binding, key):
    """Computed, not assumed: on every probe that has a restatement, operand rounding (both types) moves the restatement by half a gate at most;
    the mutants of rect_data asserted on the GPU (pack_data.SCALE_MUTANTS) are two gates or more from the rounded restatement on at least one
    probe, in both types, and no other mutant is."""
    t = _scale_tensors(pkg, key)
    assert ("rope" in t) == (key != "vit_erf") and (t["reg_token"].shape[1] if "reg_token" in t else 0) == KD.prefix_rows(key) - 1
    exact = {i: KD.probe_ref(key, t, i, binding=binding) for i in KD.parity_probes(key)}
    ref = {}
    for dtype in (0, 1):
        for i in KD.parity_probes(key):
            ref[dtype, i] = KD.probe_ref(key, t, i, dtype, binding=binding)
            d = KD.probe_distance(ref[dtype, i][0], ref[dtype, i][1], exact[i])
            print(f"{key} probe {KD.GRIDS[i]} {'F16' if dtype == 0 else 'BF16'}: rounded against unrounded {d[0]:.3e} {d[1]:.3e} = {KD.gates(d):.3f} gates")
            assert KD.gates(d) <= 0.5, (key, i, dtype, d)
    if key == "glu_hplus":
        return
    assert set(KD.SCALE_MUTANTS[key]) | set(KD.SCALE_MUTANTS_NEAR[key]) == set(XD.mutants_of(t))
    for mut in XD.mutants_of(t):
        far = []
        for dtype in (0, 1):
            ds = [KD.gates(KD.probe_distance(*KD.probe_ref(key, t, i, dtype, mut, binding), ref[dtype, i])) for i in KD.parity_probes(key) if KD.mutant_applies(mut, KD.GRIDS[i])]
            print(f"{key} {mut} {'F16' if dtype == 0 else 'BF16'}: {' '.join(f'{x:.2f}' for x in ds)} gates")
            far.append(max(ds) >= 2.0)
            if mut in KD.SCALE_MUTANTS_NEAR[key]:
                assert abs(max(ds) - KD.SCALE_MUTANTS_NEAR[key][mut]) < 0.01, (key, mut, dtype, max(ds))       # the listed distance is the computed one
        assert far == [mut in KD.SCALE_MUTANTS[key]] * 2, (key, mut, far)


def test_cache_sequences_restart_and_evict(pkg, binding):
    """The call sequences of the table-cache tests, by pack_data.cache_trace: with max_grids 32 at least two restarts, one of them in a call that
    names a cached and a missing grid, and no eviction; with max_grids 2 restarts and evictions interleave; the roomy arena never restarts;
    rope_off after a restart differs from the roomy context's for a grid both hold.  The back-to-back sequence: B evicts b and builds c, C restarts."""
    model = _model(pkg, binding, KD.CACHE_KIND)
    hp = model.hparams
    assert (hp.patch_size, hp.hidden_size // hp.num_attention_heads // 2, 1 + model.num_registers) == (14, KD.CACHE_HALF, KD.CACHE_PREFIX)
    assert hp.img_size // hp.patch_size == KD.CACHE_FILE_GRID[0] and model.rope is not None
    model.close()
    calls = KD.CACHE_CALLS
    assert max(KD.call_rows(c) for c in calls) <= KD.CACHE_MAX_TOKENS
    tr = KD.cache_trace(calls, KD.CACHE_MAX_TOKENS, KD.CACHE_HALF, 32)
    restarts = [k for k, s in enumerate(tr) if s["restarted"]]
    assert len(restarts) >= 2 and not any(s["evicted"] for s in tr)
    mixed = [k for k in restarts if any(g in tr[k - 1]["held"] for g in calls[k]) and any(g not in tr[k - 1]["held"] for g in calls[k])]
    assert mixed, restarts
    for k in restarts:
        assert tr[k]["held"] == list(dict.fromkeys(calls[k])) and tr[k]["rope_off"][calls[k][0]] == 0
    roomy = KD.cache_trace(calls, KD.CACHE_ROOMY_TOKENS, KD.CACHE_HALF, 32)
    assert not any(s["restarted"] or s["evicted"] for s in roomy)
    assert any(tr[k]["rope_off"][g] != roomy[k]["rope_off"][g] for k in mixed for g in calls[k])        # a stale rope_off would point elsewhere
    assert any(tr[k]["rope_off"][g] != tr[k - 1]["rope_off"].get(g, -1) for k in mixed for g in calls[k] if g in tr[k - 1]["held"])
    two = KD.cache_trace(calls, KD.CACHE_MAX_TOKENS, KD.CACHE_HALF, 2)
    kinds = ["r" if s["restarted"] else "e" if s["evicted"] else "-" for s in two]
    assert kinds.count("r") >= 2 and kinds.count("e") >= 2 and "er" in "".join(kinds) and "re" in "".join(kinds), kinds
    assert all(len(s["held"]) <= 2 for s in two)
    assert not any(s["restarted"] or s["evicted"] for s in KD.cache_trace(calls, 10 ** 6, 0, 32))       # no rope: no arena
    a, b, c = KD.B2B_CALLS
    assert max(KD.call_rows(x) for x in KD.B2B_CALLS) <= KD.B2B_MAX_TOKENS
    bb = KD.cache_trace(KD.B2B_CALLS, KD.B2B_MAX_TOKENS, KD.CACHE_HALF, 2)
    assert bb[1]["evicted"] == [a[1]] and not bb[1]["restarted"] and bb[1]["held"] == [a[0], b[0]] and b[1] == a[0]
    assert bb[2]["restarted"] and bb[2]["held"] == list(c) and not set(c) & set(a + b)


def test_pack_launches_counts_pack_forward():
    """The derivation on the mixed pack of tests/test_gpu_pack.py: seven images, no two neighbours of one shape, two layers."""
    shapes = KD.mixed_shapes(16)
    assert KD.pack_launches(shapes, 2, new_grids=4) == (4 + 7 + 2 * 7 + 3, 7)
    assert KD.pack_launches(shapes[:1] * 3, 3, 0, rope=True, glu=True, pre=True, feat=True) == (1 + 1 + 3 * 9 + 3 + 1, 1)
