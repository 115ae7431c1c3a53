"""What tests/test_gpu_wide_families.py leans on, checked without a GPU (tests/wide_data.py): every wide fixture is a file its family's parser and
restatement take, batch_for() really makes two different wide sub-batches with ragged last row blocks, the launch counts restate forward.cpp
consistently, and on the boundary images of that batch every listed mutant lies at least TWICE a gate from the restatement, in both operand
roundings -- so a GPU result inside the gates of the restatement is outside those of every mutant, whatever it is."""
import numpy as np
import pytest

import arch_data as AD
import prefix_data as PD
import rope_data as RD
import swiglu_data as SD
import wide_data as WD

KEYS = list(WD.FIXTURES)
_T = {}


def _tensors(pkg, key):
    if key not in _T:
        _T[key] = PD.file_tensors(pkg, WD.fixture_file(pkg, key))
    return _T[key]


def _boundary(key):
    N = WD.FIXTURES[key].tokens
    n, s1 = WD.batch_for(N)
    ids = WD.boundary_ids(n, s1)
    return ids, WD.images(N)[ids]


def test_the_wide_configuration_is_the_smallest_with_a_peer(pkg):
    hp = pkg.synth.hparams_for(WD.NAME)
    assert (hp.hidden_size, hp.num_hidden_layers, hp.num_attention_heads, hp.num_classes, hp.patch_size, hp.img_size) == (WD.D, WD.L, WD.H, 10, WD.P, WD.S)
    assert WD.D // 256 == 2 and WD.D // WD.H == 64 and WD.L == 3
    assert WD.rows_needed(512) == 16384 and WD.rows_needed(256) == 32768 and WD.rows_needed(768) == 43 * 256 and WD.rows_needed(1024) == 8192
    assert sorted({f.tokens for f in WD.FIXTURES.values()}) == [4, 5, 9]


@pytest.mark.parametrize("key", KEYS)
def test_every_fixture_loads_and_is_what_the_table_says(pkg, key):
    fx = WD.FIXTURES[key]
    t = _tensors(pkg, key)
    assert t["blocks.2.attn.qkv.weight"].shape == (3 * WD.D, WD.D) and "blocks.3.norm1.weight" not in t
    assert ("cls_token" in t) == (not fx.map) and ("attn_pool.latent" in t) == fx.map
    assert (t["reg_token"].shape[1] if "reg_token" in t else 0) == max(fx.prefix - 1, 0)
    assert t["pos_embed"].shape == (1, WD.G2 + (0 if fx.map else 1), WD.D)
    assert t["head.weight"].shape == (10, 2 * WD.D if fx.pool else WD.D)
    assert ("pre_norm.weight" in t) == fx.pre
    assert (SD.glu_of(t) or 0) == fx.glu
    assert t["blocks.0.mlp.fc1.weight"].shape == ((2 * fx.glu, WD.D) if fx.glu else (4 * WD.D, WD.D))
    assert t["blocks.0.mlp.fc2.weight"].shape == ((WD.D, fx.glu) if fx.glu else (WD.D, 4 * WD.D))
    act, eps, pre = AD.arch_of(t)
    want = {"vit_erf": (AD.ACT_ERF, 1e-12), "clip": (AD.ACT_QUICK, 1e-5), "dinov2_reg": (AD.ACT_TANH, 1e-6), "siglip_map": (AD.ACT_TANH, 1e-6),
            "dinov3_rope": (AD.ACT_ERF, 1e-5), "glu_g": (AD.ACT_ERF, 1e-6), "glu_hplus": (AD.ACT_TANH, 1e-5), "glu_odd": (AD.ACT_ERF, 1e-6)}[key]
    assert (act, np.float32(eps)) == (want[0], np.float32(want[1]))
    assert (RD.rope_of(t) is not None) == (key in ("dinov3_rope", "glu_hplus"))
    # the widths of the table: fc2's K is a whole number of the ping-pong kernel's K-tile pairs (128) but not of 256 -- or, glu_odd, of neither
    assert WD.fusable(key) == fx.fusable
    if fx.glu:
        assert fx.glu % 64 == 0 and fx.glu % 256 != 0 and (fx.glu % 128 == 0) == fx.fusable and 2 * fx.glu > 4 * WD.D
    assert fx.cls_tail == (key in ("vit_erf", "clip", "dinov3_rope", "glu_hplus"))


@pytest.mark.parametrize("tokens", [4, 5, 9])
def test_batch_for_makes_two_different_wide_ragged_sub_batches(tokens):
    n, s1 = WD.batch_for(tokens)
    s2 = n - s1
    need = WD.rows_needed(WD.D)
    for s in (s1, s2):
        M = WD.padded_rows(s, tokens)
        assert M >= need and (M // 256) * (WD.D // 256) >= 128            # is_wide (gemm.hip; tests/exact_data.py is_wide)
        assert s * tokens % 256 != 0 and M - s * tokens < 256             # a ragged last row block: its pad rows are stored by the fusing GEMMs
    assert s1 != s2 and WD.padded_rows(s1, tokens) != WD.padded_rows(s2, tokens)
    assert n >= 16                                                        # forward.cpp: two sub-batches from 8 images per slice on
    ids = WD.boundary_ids(n, s1)
    assert len(ids) == 6 and {s1 - 1, s1, 0, n - 1} <= set(ids)
    print(f"N {tokens}: batch {n} = {s1} + {s2} images, {s1 * tokens} + {s2 * tokens} rows in {WD.padded_rows(s1, tokens) // 256} + {WD.padded_rows(s2, tokens) // 256} row blocks")


@pytest.mark.parametrize("key", KEYS)
def test_launch_counts_restate_the_forward(key):
    fx = WD.FIXTURES[key]
    c, ct = WD.launches(key), WD.launches(key, traced=True)
    assert c["cls_tail"] == fx.cls_tail and not ct["cls_tail"]
    assert c["standalone"] == ct["standalone"] == c["fused"] + c["layernorm"]
    if not fx.fusable:
        assert c["fused"] == 0 and c["layernorm"] == c["standalone"] and WD.forced_tiles(key, fx.tokens) == 0
        return
    # per sub-batch a fusing context keeps: the pre-norm, norm1 of layer 0, norm2 of a class-rows-only last layer, the final norm
    assert c["layernorm"] == 2 * (int(fx.pre) + 1 + int(fx.cls_tail) + (0 if fx.pool else 1))
    assert c["fused"] == 2 * (4 if fx.cls_tail else 5) and ct["fused"] == 10
    # 64 + 65 row blocks of two column tiles: 25 + 26 tiles of every fusing launch are forced
    assert WD.forced_tiles(key, fx.tokens) == c["fused"] // 2 * 51


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("key", KEYS)
def test_every_mutant_is_two_gates_from_the_restatement(pkg, key, dtype):
    """The restatement with the operand type's rounding, on the boundary images of the GPU test's batch, against every listed mutant (rounded alike):
    the largest figure / gate must be at least 2.  The rounded restatement's own distance from the unrounded one, the noise floor a gate has to
    clear, is printed and must stay under three quarters of a gate (wide_data.QK_WIDE, HEAD_WIDE and HEAD_WIDE_MAP see to it)."""
    fx = WD.FIXTURES[key]
    t = _tensors(pkg, key)
    ids, imgs = _boundary(key)
    ref = WD.forward64(key, t, imgs, dtype)
    exact = WD.forward64(key, t, imgs)
    assert ref["trace"].shape == (WD.L + 1, len(ids), fx.tokens, WD.D) and np.isfinite(ref["probs"]).all()
    _, parts = WD.distance(key, ref, exact, dtype)
    parts.pop("stage0", None)                  # (rounded against unrounded patch weights: not a figure any test gates)
    print(f"{key} dtype {dtype}: rounded restatement against the unrounded one: worst figure / gate {max(parts.values()):.3f}  " + " ".join(f"{k} {v:.3f}" for k, v in parts.items()))
    assert max(parts.values()) <= 0.75, "operand rounding alone must stay well inside the gates, or they say nothing about a kernel"
    print(f"{key} dtype {dtype}: top-1 probabilities {np.round(ref['probs'].max(1), 4)}")
    for name, kw in fx.mutants(dtype).items():
        far, parts = WD.distance(key, ref, WD.forward64(key, t, imgs, dtype, **kw), dtype)
        print(f"{key} dtype {dtype}: mutant {name}: worst figure / gate {far:.2f}  " + " ".join(f"{k} {v:.2f}" for k, v in parts.items()))
        assert far >= 2.0, (key, dtype, name, parts)
