"""The cls + mean head on packs, host only (include/vitx.h "packed batches", pool_head = 2): the chunk table, creation refusals, argument checks."""
import numpy as np
import pytest

import map_data as MD
import pack_mean_data as KD
import rect_data as XD

@pytest.mark.parametrize("D", KD.WIDTHS)
def test_chunks_against_the_definition(binding, D):
    R, W, _ = binding.pack_mean_chunks([0, KD.T + 1], KD.T, D)
    assert (R, W) == (128, 16 if D <= 768 else 8)
    cnts = KD.counts(R, W) + [4000] + [196] * 5
    R2, none, pc0 = binding.pack_mean_chunks(np.concatenate([[7], 7 + np.cumsum([KD.T + c for c in cnts])]), KD.T)
    assert (R2, none) == (R, None) and pc0.tolist() == [sum(-(-c // R) for c in cnts[:i]) for i in range(len(cnts) + 1)]

def test_creation_refusals_need_no_device(pkg, binding):
    cm = pkg.synth.cached_synthetic("vit_micro_patch14_56", head_scale=4.0, registers=4, head_pool=1)
    for path, pool_head, code in ((XD.fixture_file(pkg, "p16"), 2, binding.ERR_ARG), (MD.fixture_file(pkg), 2, binding.ERR_ARG), (cm, 0, binding.ERR_UNSUPPORTED),
                                  (cm, 1, binding.ERR_ARG), (cm, 3, binding.ERR_ARG)):
        model = binding.Model(path)
        with pytest.raises(binding.VitxError) as ei:
            binding.PackContext(model, device=0, max_tokens=64, max_images=2, dtype=binding.BF16, pool_head=pool_head)
        assert ei.value.code == code, (path, pool_head)
        model.close()

def test_op_argument_checks_come_before_the_device(binding):
    ok = dict(dtype=0, d_x=4096, d_row0=4096, n=2, T=5, D=128, d_w=4096, d_b=4096, eps=1e-6, d_cls=4096, d_mean=4096, d_z=4096)
    for change, code in [(dict(d_x=0), "ERR_ARG"), (dict(d_row0=0), "ERR_ARG"), (dict(d_w=0), "ERR_ARG"), (dict(d_cls=0, d_mean=0, d_z=0), "ERR_ARG"), (dict(n=0), "ERR_ARG"),
                         (dict(T=0), "ERR_ARG"), (dict(dtype=2), "ERR_ARG"), (dict(d_mean=4100), "ERR_ARG"), (dict(d_x=4104), "ERR_ARG"), (dict(d_row0=4098), "ERR_ARG"),
                         (dict(D=100), "ERR_UNSUPPORTED")]:
        with pytest.raises(binding.VitxError) as ei:
            binding.op_feat_pool_packed(**{**ok, **change})
        assert ei.value.code == getattr(binding, code), change
