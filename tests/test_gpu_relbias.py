"""attention_bias.hip (include/vitx.h "relative position bias") against float64, op and end to end; what the op's gate can see: test_cpu_relbias.py."""
import numpy as np
import pytest

import prefix_data as PD
import relbias_data as RB
from ref64 import PROB_TOL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("grid", RB.OP_GRIDS, ids=lambda g: "%dx%d" % g)
def test_op_against_float64_and_zero_table_against_generic(binding, torch_gpu, grid, dtype_name):
    """Three heads with a table each in +-4, two images: every element within RB.GATE of the float64 result; with an all-zero table the generic kernel's bytes."""
    torch = torch_gpu
    dt, tdt = (binding.F16, torch.float16) if dtype_name == "f16" else (binding.BF16, torch.bfloat16)
    qkv, table = RB.op_case(dtype_name, *grid)
    N, D = grid[0] * grid[1] + 1, 64 * RB.OP_H
    xq = torch.from_numpy(qkv).cuda().to(tdt)
    out, zero, want = (torch.full((RB.OP_IMG * N, D), float("nan"), dtype=tdt, device="cuda") for _ in range(3))
    for o, tab in ((out, table), (zero, 0 * table)):
        binding.attention_bias(dt, xq.data_ptr(), torch.from_numpy(tab).cuda().data_ptr(), o.data_ptr(), RB.OP_IMG, *grid, D, RB.OP_H)
    binding.check(binding.lib().vitx_op_attention_generic(dt, xq.data_ptr(), want.data_ptr(), RB.OP_IMG, N, D, RB.OP_H, None))
    torch.cuda.synchronize()
    ref = RB.attention64(qkv, table[:, RB.index(*grid)], RB.OP_IMG, RB.OP_H)
    err = float(np.abs(out.double().cpu().numpy() - ref).max())
    print(f"attention_bias {dtype_name} grid {grid}: max |d| {err:.3e} (gate {RB.GATE * np.abs(ref).max():.3e})")
    assert err <= RB.GATE * np.abs(ref).max()
    assert torch.equal(zero.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("shared,pool", [(False, False), (True, False), (False, True), (True, True)])
def test_forward_against_float64(pkg, binding, torch_gpu, shared, pool, dtype):
    """A table per layer and a shared one, the class-token head and the `pool` order-1 head, batches 3 and 1, under ref64's gate for the operand type."""
    path = RB.fixture_file(pkg, shared, pool)
    rnd = PD.f16_round if dtype == 0 else PD.bf16_round
    imgs = PD.exact_images(3, 64, seed=2)
    ref = RB.forward64(PD.file_tensors(pkg, path), imgs, wround=rnd, uround=rnd)
    model = binding.Model(path)
    assert model.rel_bias() == (1 if shared else RB.LAYERS, (2 * RB.GRID - 1) ** 2 + 3) and model.head_pool == (binding.POOL_MEAN_NORM if pool else 0)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=dtype)
    for n in (3, 1):
        p = ctx.forward(imgs[:n])
        d = float(np.abs(p - ref[:n]).max())
        print(f"rel_bias shared {shared} pool {pool} dtype {dtype} batch {n}: max|dprob| {d:.3e} (gate {PROB_TOL[dtype]})")
        assert np.isfinite(p).all() and d <= PROB_TOL[dtype]
    with pytest.raises(binding.VitxError, match="relative position bias"):
        ctx.attn_enable([0])
    ctx.close(); model.close()
