"""Host refusals of the staged packed attention's entry points: each gives its code before any device call (no GPU here)."""
import pytest

import pack_data as KD
import rect_data as XD


def test_op_attention_packed_ex_refusals(binding):
    B, p = binding, 4096
    G, S = B.PACK_ATTN_GENERIC, B.PACK_ATTN_STAGED
    arg = [(0, S, 0, p, p, 1, 192, 3), (0, S, p, 0, p, 1, 192, 3), (0, S, p, p, 0, 1, 192, 3), (0, S, p, p, p, 0, 192, 3), (2, S, p, p, p, 1, 192, 3),
           (0, 3, p, p, p, 1, 192, 3), (0, -1, p, p, p, 1, 192, 3), (0, G, p, p, p, 1, 0, 3)]
    uns = [(0, S, p, p, p, 1, 128, 4), (1, S, p, p, p, 1, 384, 3), (0, G, p, p, p, 1, 136 * 2, 2), (0, B.PACK_ATTN_AUTO, p, p, p, 1, 12, 3)]
    for code, calls in ((B.ERR_ARG, arg), (B.ERR_UNSUPPORTED, uns)):
        for a in calls:
            with pytest.raises(B.VitxError) as ei:
                B.op_attention_packed_ex(*a)
            assert ei.value.code == code, a
    assert B.lib().vitx_pack_attn_kernel(None) == 0


@pytest.mark.parametrize("kind,kernel,code", [("p16", 3, "ERR_ARG"), ("p16", -1, "ERR_ARG"), ("p16h4", 2, "ERR_UNSUPPORTED")])
def test_pack_create_refuses_a_bad_attn_kernel(pkg, binding, kind, kernel, code):
    model = binding.Model(KD.variant_file(pkg, kind) if kind.endswith("h4") else XD.fixture_file(pkg, kind))
    with pytest.raises(binding.VitxError) as ei:
        binding.PackContext(model, device=0, max_tokens=64, max_images=2, dtype=binding.BF16, attn_kernel=kernel)
    assert ei.value.code == getattr(binding, code)
    model.close()
