"""Attention maps on the host side: the C ABI symbols, the binding's helpers and the CLI's PGM writer (no GPU)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attention_map_symbols_are_exported(binding):
    L = binding.lib()
    for s in ("vitx_attn_enable", "vitx_attn_floats", "vitx_attn_images", "vitx_attn_read", "vitx_op_attention_map", "vitx_ctx_graph_launches"):
        assert s in binding.EXPORTS and hasattr(L, s)
    hdr = open(os.path.join(ROOT, "include", "vitx.h")).read()
    assert "#define VITX_ATTN_ROLLOUT 1" in hdr and binding.ATTN_ROLLOUT == 1


def test_attention_map_calls_without_a_context_are_argument_errors(binding):
    L = binding.lib()
    assert L.vitx_attn_enable(None, 1, 0) == 3
    assert L.vitx_attn_floats(None) == 0 and L.vitx_attn_images(None) == 0 and L.vitx_ctx_graph_launches(None) == -1
    assert L.vitx_attn_read(None, None, 0) == 3
    assert L.vitx_op_attention_map(0, None, 0, None, None, 1, 197, 768, 12, None) == 3


def test_rollout_entry_points_refuse_bad_arguments_before_any_device_call(binding):
    """The refusals need no device: they come first (pointers that are never dereferenced)."""
    L = binding.lib()
    for s in ("vitx_op_rollout_factor", "vitx_op_rollout_step", "vitx_op_rollout_row"):
        assert s in binding.EXPORTS and hasattr(L, s)
    a, r = 0x100000, 0x200000
    assert L.vitx_op_rollout_factor(0, None, 0, a, 1, 197, 768, 12, None) == 3 and L.vitx_op_rollout_factor(0, a, 0, None, 1, 197, 768, 12, None) == 3
    assert L.vitx_op_rollout_factor(0, a, 0, r, 1, 1025, 768, 12, None) == 5 and L.vitx_op_rollout_factor(0, a, 0, r, 1, 197, 800, 32, None) == 5
    assert L.vitx_op_rollout_step(None, r, 1, 8, None) == 3 and L.vitx_op_rollout_step(a, None, 1, 8, None) == 3
    assert L.vitx_op_rollout_step(a, r, 0, 8, None) == 3 and L.vitx_op_rollout_step(a, r, 1, 0, None) == 3 and L.vitx_op_rollout_step(a, r, 1, 1025, None) == 5
    for aa, rr in ((a, a), (a, a + 4 * 63), (a + 4 * 63, a)):               # one image of 8 x 8 floats: 256 bytes
        assert L.vitx_op_rollout_step(aa, rr, 1, 8, None) == 3
        assert b"overlap" in L.vitx_last_error()
    assert L.vitx_op_rollout_row(None, 16, None, a, 8, 1, 8, 2, None) == 3 and L.vitx_op_rollout_row(a, 16, None, None, 8, 1, 8, 2, None) == 3
    assert L.vitx_op_rollout_row(a, 15, None, r, 8, 1, 8, 2, None) == 3 and L.vitx_op_rollout_row(a, 16, None, r, 7, 1, 8, 2, None) == 3
    assert L.vitx_op_rollout_row(a, 16, None, r, 8, 1, 8, 0, None) == 3 and L.vitx_op_rollout_row(a, 2050, None, r, 1025, 1, 1025, 2, None) == 5


def test_attn_pgm_upsamples_by_nearest_neighbour_and_scales_to_255(pkg):
    from vitcpp_amd import cli
    grid = np.arange(16, dtype=np.float32).reshape(4, 4)[::-1].copy()
    data = cli.attn_pgm(grid, 64)
    head = b"P5\n64 64\n255\n"
    assert data.startswith(head) and len(data) == len(head) + 64 * 64
    pic = np.frombuffer(data[len(head):], np.uint8).reshape(64, 64)
    assert pic[:16, :16].min() == pic[:16, :16].max() == 204      # grid[0, 0] = 12 of 0..15: 12 / 15 * 255
    assert pic.max() == 255 and pic.min() == 0
    i, j = np.unravel_index(int(np.argmax(grid)), grid.shape)
    assert (pic[i * 16:(i + 1) * 16, j * 16:(j + 1) * 16] == 255).all()
    assert np.array_equal(pic[::16, ::16], np.rint(grid / 15 * 255).astype(np.uint8))
    flat = cli.attn_pgm(np.full((2, 2), 0.25, np.float32), 6)
    assert flat.endswith(bytes(36))


def test_cli_refuses_attn_map_in_directory_mode(pkg, tmp_path, capsys):
    import pytest
    from vitcpp_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["-m", str(tmp_path / "none.gguf"), "--dir", str(tmp_path), "--attn-map", str(tmp_path / "m.pgm")])
    assert e.value.code == 2 and "--attn-map" in capsys.readouterr().err
    assert not (tmp_path / "m.pgm").exists()
