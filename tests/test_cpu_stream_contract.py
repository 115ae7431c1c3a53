"""The stream contract of include/vitx.h, on the CPU: every prototype with a `void *stream` parameter takes a side in tests/stream_data.py --
ENQUEUE_ONLY (tests/test_gpu_stream_order.py stalls it) or HOST_WAITS (with the header's own words for the wait) -- so a new entry point cannot
ship without one; and the decoy and sentinel generators of the stall harness give finite, in-range data that differs from the real input in every
element a consumer reads."""
import os

import numpy as np

import stream_data as S
import test_gpu_stream_order as G

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vitx.h")


def test_every_stream_prototype_stands_in_exactly_one_table():
    names = S.stream_prototypes(HEADER)
    assert len(names) == len(set(names)) == 59, (len(names), sorted(n for n in names if names.count(n) > 1))
    for tricky in ("vitx_op_gemm_ex", "vitx_op_features_ex", "vitx_op_depth", "vitx_op_nn", "vitx_op_gemm_mxfp8", "vitx_preprocess_rect_device"):      # prototypes that span lines
        assert tricky in names
    assert "vitx_op_patch_embed_rect" not in names and "vitx_forward" not in names          # (null stream; host pointers)
    both = set(S.ENQUEUE_ONLY) & set(S.HOST_WAITS)
    assert not both, f"in both tables: {sorted(both)}"
    missing = [n for n in names if n not in S.ENQUEUE_ONLY and n not in S.HOST_WAITS]
    assert not missing, f"include/vitx.h has stream entry points that stand in no table of tests/stream_data.py: {missing}"
    stale = sorted((set(S.ENQUEUE_ONLY) | set(S.HOST_WAITS)) - set(names))
    assert not stale, f"tables name entry points the header does not have: {stale}"


def test_the_quoted_waits_are_the_headers_own_words():
    text = S.header_text(HEADER)
    quotes = dict(S.HOST_WAITS)
    quotes.update({k: v for k, v in S.ENQUEUE_ONLY.items() if v})
    assert all(S.HOST_WAITS.values())
    for name, words in quotes.items():
        assert words in text, f"{name}: include/vitx.h does not say {words!r}"
    assert text.count("only enqueue") >= 20


def test_the_gpu_file_covers_every_enqueue_only_entry():
    for name in S.ENQUEUE_ONLY:
        assert name in G.COVERED, f"{name} is listed as enqueue-only and tests/test_gpu_stream_order.py does not stall it"
        assert callable(getattr(G, G.COVERED[name], None)), (name, G.COVERED[name])
    assert not set(G.COVERED) - set(S.ENQUEUE_ONLY), sorted(set(G.COVERED) - set(S.ENQUEUE_ONLY))
    assert not {entry for entry, _ in G.OPS.values()} & set(S.HOST_WAITS)


def test_float_decoys_are_finite_in_range_and_differ_everywhere():
    for shape, scale, seed in (((5, 128), 1.0, 1), ((34, 384), 0.8, 3), ((3, 56, 56, 3), 1.0, 2), ((2, 17, 17), 0.1, 1)):
        real = S.real_f32(shape, seed, scale)
        assert real.dtype == np.float32 and np.isfinite(real).all() and np.abs(real).max() <= 4 * scale
        for positive in (False, True):
            r = np.abs(real) if positive else real
            for given in (scale, None):
                d = S.decoy_f32(r, seed, given, positive=positive)
                assert d.shape == r.shape and d.dtype == np.float32 and np.isfinite(d).all() and np.abs(d).max() <= 4.75 * scale
                assert not positive or (d >= 0).all()
                gap = np.abs(d.astype(np.float64) - r)
                assert gap.min() >= 0.9 * (np.abs(r).max() / 4 if given is None else scale) / 8, gap.min()
                # the difference survives both 16-bit roundings: an fp16 / bf16 ulp at 4.75 scale is below scale / 8
                assert (d.astype(np.float16) != r.astype(np.float16)).all()
                bf = lambda a: (np.ascontiguousarray(a, np.float32).view(np.uint32) + 0x8000) >> 16
                assert (np.abs(bf(d).astype(np.int64) - bf(r).astype(np.int64)) >= 1).all()


def test_byte_and_index_decoys_are_valid_and_differ_everywhere():
    u = S.real_u8((2, 17, 23, 3), 1)
    d = S.decoy_u8(u, 1)
    assert d.dtype == np.uint8 and d.shape == u.shape and (d != u).all()
    for bound in (2, 16, 96):
        ids = np.random.default_rng(bound).integers(0, bound, (4, 24)).astype(np.int32)
        x = S.decoy_index(ids, bound, 7)
        assert x.dtype == np.int32 and (x >= 0).all() and (x < bound).all() and (x != ids).all()


def test_prompt_decoys_keep_every_row_valid():
    import text_data as TD
    for family, eos in (("clip", TD.CLIP_CFG["eos_token_id"]), ("siglip", -1)):
        V = (TD.CLIP_CFG if family == "clip" else TD.SIGLIP_CFG)["vocab_size"]
        for seed in (40, 41):
            ids = TD.prompts(family, 4, seed=seed)
            d = S.decoy_prompts(ids, V, eos, seed)
            assert d.dtype == np.int32 and d.shape == ids.shape and (d >= 0).all() and (d < V).all()
            if eos < 0:
                assert (d != ids).all()
            else:                                                  # EOS stays where it was (the pooled position is the row's own), everything else differs
                assert ((d == eos) == (ids == eos)).all() and (d[ids != eos] != ids[ids != eos]).all()
                assert (TD.pooled_positions(d, eos) == TD.pooled_positions(ids, eos)).all()


def test_sentinels_are_finite_values_of_their_types():
    assert set(S.SENTINELS) == {"float32", "float16", "bfloat16", "uint8", "int32"}
    assert np.isfinite(np.float32(S.sentinel("float32"))) and np.float32(S.sentinel("float32")) < -1e38
    assert np.isfinite(np.float16(S.sentinel("float16"))) and np.float16(S.sentinel("float16")) == -np.finfo(np.float16).max
    assert abs(S.sentinel("bfloat16")) < 3.38e38                    # the largest finite bf16 is 3.3895e38
    assert S.sentinel("uint8") == 255 and -2 ** 31 <= S.sentinel("int32") < 0
    assert np.isfinite(np.array([S.sentinel("int32")], np.int32).view(np.float32)[0])      # a pair buffer {f32, i32} filled with it holds no NaN either

