"""Attention maps on packed contexts, the host side (include/vitx.h "packed batches"): the tables of a call (vitx_pack_attn_check) against a numpy
restatement, every refusal with its code and the image it names, the exported symbols, and the CLI's parser."""
import os
import re

import numpy as np
import pytest

import pack_attn_data as AD
import pack_data as KD
import rect_data as XD

NEW = ("vitx_pack_attn_enable", "vitx_pack_attn_floats", "vitx_pack_attn_read", "vitx_pack_attn_device", "vitx_pack_attn_check",
       "vitx_op_attention_map_packed", "vitx_op_rollout_step_packed", "vitx_op_rollout_row_packed")


def _model(pkg, binding, kind):
    return binding.Model(XD.fixture_file(pkg, kind))


@pytest.mark.parametrize("kind,registers", [("p16", 0), ("p14r4", 4)])
@pytest.mark.parametrize("rollout", [False, True])
def test_tables_of_the_mixed_pack(pkg, binding, kind, registers, rollout):
    """rblk0 and sq0 of pack_data.mixed_shapes, without and with register tokens, are the running counts of ceil(N_i / 16) and of N_i^2 over the rows
    vitx_pack_check gives; with rollout the call passes exactly from the arena size sum N_i^2 on."""
    m = _model(pkg, binding, kind)
    P = m.hparams.patch_size
    shapes = KD.mixed_shapes(P)
    row0 = KD.row0_of(shapes, P, registers)
    assert np.array_equal(binding.pack_check(m, shapes, 10 ** 6, len(shapes)), row0)
    rblk0, sq0 = AD.tables(row0)
    got = binding.pack_attn_check(m, shapes, rollout=rollout, max_sq_tokens=int(sq0[-1]) if rollout else 0)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], rblk0) and np.array_equal(got[1], sq0)
    assert rblk0[-1] == sum(-(-int(n) // 16) for n in np.diff(row0)) and sq0[-1] == sum(int(n) ** 2 for n in np.diff(row0))
    m.close()


def test_every_refusal_names_its_cause(pkg, binding):
    m = _model(pkg, binding, "p16")
    P, L = m.hparams.patch_size, m.hparams.num_hidden_layers
    shapes = KD.mixed_shapes(P)
    sq = int(AD.tables(KD.row0_of(shapes, P, 0))[1][-1])

    def refused(code, *words, shapes=shapes, **kw):
        with pytest.raises(binding.VitxError) as e:
            binding.pack_attn_check(m, shapes, **kw)
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)

    ARG, UNS = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    # the enable's arguments
    refused(ARG, "layer mask", layer_mask=1 << L, flags=0)
    refused(ARG, "layer mask", layer_mask=(1 << 63) | 1, flags=0)
    refused(ARG, "unknown flags", layer_mask=1, flags=2)
    refused(ARG, "unknown flags", layer_mask=0, flags=binding.ATTN_ROLLOUT | 4, max_sq_tokens=sq)
    for bad in (0, -1, 2 ** 31):
        refused(ARG, "max_sq_tokens", rollout=True, max_sq_tokens=bad)
    # per call, rollout on: the matrices against the arenas (one float short), and the token bound, which names the image
    refused(ARG, "max_sq_tokens", str(sq), rollout=True, max_sq_tokens=sq - 1)
    big = list(shapes)
    big[2] = (32 * P, 32 * P)                          # 1 + 1024 tokens
    refused(UNS, "image 2", "1024", "1025", shapes=big, rollout=True, max_sq_tokens=2 ** 31 - 1)
    big[5] = (40 * P, 40 * P)
    refused(UNS, "image 2", shapes=big, rollout=True, max_sq_tokens=2 ** 31 - 1)        # the first one
    # ... which class maps alone do not have
    assert binding.pack_attn_check(m, big, layers=[L - 1])[0][-1] > 0
    # exactly 1024 tokens passes (31 x 33 patches and the class token)
    edge = [(31 * P, 33 * P), (P, P)]
    r, s = binding.pack_attn_check(m, edge, rollout=True, max_sq_tokens=1024 * 1024 + 4)
    assert list(r) == [0, 64, 65] and list(s) == [0, 1024 * 1024, 1024 * 1024 + 4]
    # the shapes' own refusals are vitx_pack_check's
    refused(ARG, "patch size", shapes=[(P + 1, P)], rollout=False)
    m.close()


def test_symbols_are_exported_and_listed(pkg, binding):
    header = open(_header_path()).read()
    for name in NEW:
        assert name in binding.EXPORTS, name
        assert hasattr(binding.lib(), name), name
        assert re.search(r"\b" + name + r"\(", header), name
    # none of them takes a stream: the three kernel entry points are synchronous (the header says so)
    for name in NEW:
        proto = re.search(r"\n(?:int|const void \*)\s*" + name + r"\(([^;]*)\);", header).group(1)
        assert "stream" not in proto, (name, proto)


def _header_path():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vitx.h")


def test_launch_count_formula():
    """pack_attn_data.map_launches on the cases the GPU test measures (L = 2) and on a deeper model."""
    assert AD.map_launches(2, [1], False) == 1 and AD.map_launches(2, [0, 1], False) == 2
    assert AD.map_launches(2, [], True) == 1 + 0 + 1 + 1 and AD.map_launches(2, [1], True) == 1 + 1 + 0 + 1
    assert AD.map_launches(12, [], True) == 11 + 10 + 1 + 1 and AD.map_launches(12, range(12), True) == 12 + 11 + 10 + 1
    assert AD.map_launches(1, [0], True) == 1 + 0 + 0 + 1


def test_cli_parser_takes_pack_attn_map_and_keeps_the_pinned_words(pkg, capsys, tmp_path):
    from vitcpp_amd import cli
    a = cli.make_parser().parse_args(["-m", "m.gguf", "-i", "a.jpg,b.jpg", "--pack", "--img-fit", "32", "--attn-map", "out", "--attn-kind", "last"])
    assert a.pack and a.attn_map == "out" and a.attn_kind == "last" and a.img_fit == 32
    # accepted by main's own checks: it gets as far as the model file, which does not exist (exit status 1, no parser error)
    assert cli.main(["-m", str(tmp_path / "none.gguf"), "-i", "a.jpg,b.jpg", "--pack", "--img-fit", "32", "--attn-map", str(tmp_path / "out")]) == 1
    assert "vit: error:" not in capsys.readouterr().err
    for extra in ([], ["--attn-map", "out"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["-m", "none.gguf", "-i", "a.jpg,b.jpg", "--pack"] + extra)
        assert e.value.code == 2
        assert "--pack takes --img-fit" in capsys.readouterr().err
