"""The staged packed attention kernel (attention_packed_staged.hip; include/vitx.h "packed batches"): head dim 64, K and V through LDS, the generic
kernel's bits.  Kernel ids through vitx_op_attention_packed_ex; the context through PackContext(attn_kernel=...)."""
import numpy as np
import pytest

import exact_data as X
import pack_data as KD
import rect_data as XD
from test_gpu_pack import SENT16, _bits, _pack, _raw, _tdt

pytestmark = pytest.mark.gpu

H, DM = 3, 192
COUNTS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 260, 577)      # 16-query tiles, 32-key steps, 64-key chunks (odd and even counts), 64-query blocks
EXACT_PACKS = ((15, 64, 65, 129), (193, 17))


def _run(binding, torch, dtype, kernel, qkv, counts, tail=0):
    """The kernel on a pack of `counts`: out [rows + tail][DM], the tail rows pre-filled with SENT16."""
    row0 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out = torch.full((int(row0[-1]) + tail, DM), SENT16, dtype=_tdt(torch, dtype), device="cuda")
    binding.op_attention_packed_ex(dtype, kernel, qkv.data_ptr(), out.data_ptr(), torch.from_numpy(row0).cuda().data_ptr(), len(counts), DM, H)
    return out, row0


@pytest.mark.parametrize("dtype", [0, 1])
def test_staged_has_the_generic_kernels_bits_per_image(binding, torch_gpu, dtype):
    """Every image's rows have the bits vitx_op_attention_generic writes for that image alone; 70 sentinel rows behind the pack keep their value; AUTO at
    this D is the staged kernel's buffer."""
    torch = torch_gpu
    order = [int(c) for c in np.random.default_rng(5).permutation(COUNTS)]
    for what, counts in (("shuffled", order), ("reversed", order[::-1]), ("300 x 2", [2] * 300), ("one image", [197])):
        g = torch.Generator(device="cuda").manual_seed(7 + dtype)
        qkv = (torch.randn((sum(counts), 3 * DM), device="cuda", generator=g) * 0.8).to(_tdt(torch, dtype))
        out, row0 = _run(binding, torch, dtype, binding.PACK_ATTN_STAGED, qkv, counts, tail=70)
        assert bool((out[row0[-1]:] == SENT16).all()), (what, "rows behind the pack were written")
        for i, N in enumerate(counts):
            one, o = qkv[row0[i]:row0[i + 1]].clone(), torch.zeros((N, DM), dtype=_tdt(torch, dtype), device="cuda")
            binding.check(binding.lib().vitx_op_attention_generic(dtype, one.data_ptr(), o.data_ptr(), 1, N, DM, H, None))
            bad = np.argwhere(_raw(out[row0[i]:row0[i + 1]]) != _raw(o))
            assert bad.size == 0, (what, i, N, bad[:5].tolist())
        auto, _ = _run(binding, torch, dtype, binding.PACK_ATTN_AUTO, qkv, counts, tail=70)
        assert torch.equal(auto.view(torch.int16), out.view(torch.int16)), what


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("counts", EXACT_PACKS, ids=str)
def test_staged_against_float64_on_exact_and_spread_data(binding, torch_gpu, counts, dtype_name):
    """Flat data (every numerator exactly 1: a leaked, dropped or counted pad key moves a row by two output ulps), every sign: torch.equal with the one
    correct output.  Spread data: every image against exact_data.attention_ref under exact_data.attention_bound."""
    torch = torch_gpu
    dtype = 0 if dtype_name == "f16" else 1
    tdt = _tdt(torch, dtype)
    for sign in X.FLAT_SIGNS:
        parts = [X.flat_qkv(1, N, H, 64, sign, X.attn_seed(1, N, H, 64) + 17 * sign) for N in counts]
        qkv = torch.from_numpy(np.concatenate([p[0] for p in parts])).cuda().to(tdt)
        want = torch.from_numpy(np.concatenate([X.flat_expected(c, N) for (_, c), N in zip(parts, counts)])).cuda().to(tdt)
        out, _ = _run(binding, torch, dtype, binding.PACK_ATTN_STAGED, qkv, counts)
        assert torch.equal(out, want), (counts, sign, torch.nonzero(out != want)[:5].tolist())
    x = torch.from_numpy(np.concatenate([X.spread_qkv(1, N, H, 64, X.attn_seed(1, N, H, 64)) for N in counts])).cuda().to(tdt)
    out, row0 = _run(binding, torch, dtype, binding.PACK_ATTN_STAGED, x, counts)
    for i, N in enumerate(counts):
        q, k, v = X.heads_of(x[row0[i]:row0[i + 1]].float(), 1, N, H, 64)
        ref, cond = X.attention_ref(q, k, v, 0.125, want_bound=True)
        bound = X.rows_of(X.attention_bound(ref, cond, dtype_name), 1, N, H, 64)
        worst = float(((out[row0[i]:row0[i + 1]].double() - X.rows_of(ref, 1, N, H, 64)).abs() / bound).max())
        print(f"staged {dtype_name} N {N}: {worst:.3f} of the bound")
        assert worst <= 1.0, (counts, i, N, worst)


@pytest.mark.parametrize("dtype", [0, 1])
def test_staged_poisoned_neighbours(binding, torch_gpu, dtype):
    """Every other image all-NaN, heads 0 and 2 of the clean images NaN, 64 NaN rows of qkv behind the pack: head 1 of every clean image is finite and
    has the bits of the clean run."""
    torch = torch_gpu
    counts = [37, 5, 64, 17, 130, 2, 33]
    rows = sum(counts)
    g = torch.Generator(device="cuda").manual_seed(3)
    clean = (torch.randn((rows + 64, 3 * DM), device="cuda", generator=g) * 0.8).to(_tdt(torch, dtype))
    poisoned = clean.clone()
    poisoned[rows:] = float("nan")
    a, row0 = _run(binding, torch, dtype, binding.PACK_ATTN_STAGED, clean, counts)
    for i in range(len(counts)):
        v = poisoned[row0[i]:row0[i + 1]].view(counts[i], 3, H, 64)
        if i % 2:
            v[:] = float("nan")
        else:
            v[:, :, 0] = float("nan"); v[:, :, 2] = float("nan")
    b, _ = _run(binding, torch, dtype, binding.PACK_ATTN_STAGED, poisoned, counts)
    for i in range(0, len(counts), 2):
        r = slice(int(row0[i]), int(row0[i + 1]))
        assert bool(torch.isfinite(b[r].view(-1, H, 64)[:, 1].float()).all()), i
        assert np.array_equal(_raw(a[r].view(-1, H, 64)[:, 1]), _raw(b[r].view(-1, H, 64)[:, 1])), i


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("kind", ["p16", "p14rope"])
def test_context_staged_is_generic_bit_for_bit(pkg, binding, torch_gpu, kind, dtype):
    """The mixed pack through a STAGED and a GENERIC context: equal bits of probabilities, logits and both features, equal launches and scratch
    bytes; the default context of a head-dim-64 model runs the staged kernel."""
    model = binding.Model(XD.fixture_file(pkg, kind))
    shapes, imgs = _pack(model.hparams.patch_size)
    res = {}
    for kern in (binding.PACK_ATTN_AUTO, binding.PACK_ATTN_GENERIC, binding.PACK_ATTN_STAGED):
        pack = binding.PackContext(model, device=0, max_tokens=256, max_images=8, dtype=dtype, attn_kernel=kern)
        pack.feat_enable(cls=True, tokens=True)
        p, lg = pack.forward(imgs)
        cls, tok = pack.feat_read()
        res[kern] = (pack.attn_kernel, pack.launches, pack.scratch_bytes, [_bits(a) for a in (p, lg, cls, np.concatenate([t.reshape(-1) for t in tok]))])
        pack.close()
    assert res[binding.PACK_ATTN_AUTO][0] == res[binding.PACK_ATTN_STAGED][0] == binding.PACK_ATTN_STAGED and res[binding.PACK_ATTN_GENERIC][0] == binding.PACK_ATTN_GENERIC
    gen, st = res[binding.PACK_ATTN_GENERIC], res[binding.PACK_ATTN_STAGED]
    assert gen[1:3] == st[1:3], (gen[1:3], st[1:3])
    assert np.isfinite(st[3][0].view(np.float32)).all()
    for name, x, y in zip(("probs", "logits", "cls", "tokens"), gen[3], st[3]):
        assert np.array_equal(x, y), (kind, dtype, name)
    model.close()


def test_context_on_head_dim_32(pkg, binding, torch_gpu):
    """A default context of a head-dim-32 model runs the generic kernel; STAGED is refused with ERR_UNSUPPORTED."""
    model = binding.Model(KD.variant_file(pkg, "p16h4"))
    pack = binding.PackContext(model, device=0, max_tokens=64, max_images=2, dtype=binding.BF16)
    assert pack.attn_kernel == binding.PACK_ATTN_GENERIC
    pack.close()
    with pytest.raises(binding.VitxError) as ei:
        binding.PackContext(model, device=0, max_tokens=64, max_images=2, dtype=binding.BF16, attn_kernel=binding.PACK_ATTN_STAGED)
    assert ei.value.code == binding.ERR_UNSUPPORTED and "128 / 4" in str(ei.value)
    model.close()
