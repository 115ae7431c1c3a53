"""vitx_pack_pool_chunks (include/vitx.h "packed batches", pool_head) against its definition, and its refusals.  Host only."""
import ctypes as C

import numpy as np
import pytest

@pytest.mark.parametrize("rows", [[1], [128], [129], [1, 127, 128, 129, 261], [4000] + [196] * 5, [2 ** 31 - 1]])
def test_chunks_against_the_definition(binding, rows):
    R, chunk0 = binding.pack_pool_chunks(rows)
    assert R == binding.lib().vitx_pack_pool_chunk_rows() and R >= 16
    assert chunk0.tolist() == [sum(-(-r // R) for r in rows[:i]) for i in range(len(rows) + 1)]
    assert binding.lib().vitx_pack_pool_chunks((C.c_int * len(rows))(*rows), len(rows), None) == 0      # the table is optional

@pytest.mark.parametrize("rows", [[], [0], [5, -1], [2 ** 31 - 1] * 200])
def test_chunks_refusals(binding, rows):
    with pytest.raises(binding.VitxError) as ei:
        binding.pack_pool_chunks(rows)
    assert ei.value.code == binding.ERR_ARG
    assert binding.lib().vitx_pack_pool_chunks(None, 3, None) == binding.ERR_ARG
