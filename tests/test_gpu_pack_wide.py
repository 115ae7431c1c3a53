"""The staged packed attention of head dims 72 .. 128 (attention_packed_wide.hip; include/vitx.h "packed batches"): what VITX_PACK_ATTN_AUTO runs there.
The generic packed kernel's bits, float64, NaN neighbours, the one input that tells the two kernels apart, default contexts against GENERIC ones."""
import numpy as np
import pytest

import prefix_data as PD
import ref64 as R64
from pack_data import pack_of
from test_gpu_attention_wide import GUARD, _qkv, siglip_file
from test_gpu_pack import SENT16, _bits, _tdt

pytestmark = pytest.mark.gpu

COUNTS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 193, 577)      # every tile and chunk edge, partial chunks behind full ones: one launch


def _run(binding, torch, dtype, kernel, qkv, counts, D, H):
    """vitx_op_attention_packed_ex on a pack of `counts`: the output with GUARD canary rows in front of and behind the pack's rows, as 16-bit patterns."""
    row0 = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device="cuda")
    out = torch.full((2 * GUARD + sum(counts), D), SENT16, dtype=_tdt(torch, dtype), device="cuda")
    binding.op_attention_packed_ex(dtype, kernel, qkv.data_ptr(), out.data_ptr() + GUARD * D * 2, row0.data_ptr(), len(counts), D, H)
    return out.view(torch.int16)


def _same_with_canaries(torch, dtype, got, want, what):
    sent = torch.full((GUARD, got.shape[1]), SENT16, dtype=_tdt(torch, dtype), device="cuda").view(torch.int16)
    assert torch.equal(got[:GUARD], sent) and torch.equal(got[-GUARD:], sent), (what, "canary rows were written")
    assert torch.equal(got, want), (what, torch.nonzero(got != want)[:5].tolist())


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hd", [72, 80, 88, 96, 104, 112, 120, 128])
def test_auto_has_the_generic_kernels_bits(binding, torch_gpu, hd, dtype):
    """The whole buffer equals the generic packed kernel's; three launches agree (a wave that restaged a buffer another wave still reads would show)."""
    qkv = _qkv(torch_gpu, dtype, sum(COUNTS), 2 * hd, 100 * hd + dtype)
    want = _run(binding, torch_gpu, dtype, binding.PACK_ATTN_GENERIC, qkv, COUNTS, 2 * hd, 2)
    for launch in range(3):
        _same_with_canaries(torch_gpu, dtype, _run(binding, torch_gpu, dtype, binding.PACK_ATTN_AUTO, qkv, COUNTS, 2 * hd, 2), want, (hd, launch))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hd", [72, 128])
def test_auto_against_float64(binding, torch_gpu, hd, dtype):
    """max |out - float64| is at most the generic kernel's on the same input (equal bits: no margin), and below test_wide_against_float64's bound."""
    torch = torch_gpu
    H, D, counts = 2, 2 * hd, (33, 130, 65)
    qkv = _qkv(torch, dtype, sum(counts), D, 7 + hd + dtype)
    heads = [[x.view(-1, 3, H, hd)[:, j].transpose(0, 1) for j in range(3)] for x in torch.split(qkv.double(), counts)]
    ref = torch.cat([(torch.softmax(q @ k.transpose(1, 2) / np.sqrt(hd), dim=-1) @ v).transpose(0, 1).reshape(-1, D) for q, k, v in heads])
    auto, gen = (float((_run(binding, torch, dtype, kernel, qkv, counts, D, H)[GUARD:-GUARD].view(_tdt(torch, dtype)).double() - ref).abs().max())
                 for kernel in (binding.PACK_ATTN_AUTO, binding.PACK_ATTN_GENERIC))
    print(f"packed wide attention hd {hd} dtype {dtype} N {counts}: max |d| auto {auto:.3e}, generic {gen:.3e}")
    assert auto <= gen < 0.05 * float(ref.abs().max())


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hd", [72, 120])
def test_nan_neighbours_stay_out(binding, torch_gpu, hd, dtype):
    """The middle image all NaN and NaN rows of qkv behind the pack: images 0 and 2 have the bits they have alone.  Head 1's q, k and v NaN: heads 0
    and 2 keep the clean run's bits -- the pad dims of the score product and the half-live V tile hold nobody else's bytes."""
    torch = torch_gpu
    H, D, counts, A = 3, 3 * hd, (33, 130, 33), binding.PACK_ATTN_AUTO
    clean = _qkv(torch, dtype, sum(counts) + 64, D, 31 + hd + dtype)
    a = _run(binding, torch, dtype, A, clean, counts, D, H)[GUARD:-GUARD]
    assert bool(torch.isfinite(a.view(_tdt(torch, dtype)).float()).all())
    bad = clean.clone(); bad[33:163] = float("nan"); bad[196:] = float("nan")
    b = _run(binding, torch, dtype, A, bad, counts, D, H)[GUARD:-GUARD]
    for r in (slice(0, 33), slice(163, 196)):
        alone = _run(binding, torch, dtype, A, clean[r].clone(), (33,), D, H)[GUARD:-GUARD]
        assert torch.equal(b[r], alone) and torch.equal(a[r], alone), (hd, r)
    bad = clean.clone(); bad.view(-1, 3, H, hd)[:, :, 1] = float("nan")
    b = _run(binding, torch, dtype, A, bad, counts, D, H)[GUARD:-GUARD].view(-1, H, hd)
    assert torch.equal(a.view(-1, H, hd)[:, [0, 2]], b[:, [0, 2]]), (hd, "heads 0 and 2 moved")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hd", [72, 120])
def test_auto_runs_the_staged_kernel(binding, torch_gpu, hd, dtype):
    """N = 33, v[N - 1] of (image 1, head 1) = +Inf: the generic kernel multiplies the padding keys' probability 0 by that row (NaN everywhere in the
    block); a staged kernel reads zeros there and the block holds +Inf.  Every other (image, head) keeps the clean run's bits under both ids."""
    torch = torch_gpu
    H, D, n, N = 3, 3 * hd, 3, 33
    clean = _qkv(torch, dtype, n * N, D, 91 + hd + dtype)
    bad, other = clean.clone(), torch.ones((n, H), dtype=torch.bool, device="cuda")
    bad.view(n, N, 3, H, hd)[1, N - 1, 2, 1] = float("inf"); other[1, 1] = False
    for kernel in (binding.PACK_ATTN_AUTO, binding.PACK_ATTN_GENERIC):
        a, b = (_run(binding, torch, dtype, kernel, x, (N,) * n, D, H)[GUARD:-GUARD].view(n, N, H, hd).transpose(1, 2) for x in (clean, bad))
        assert torch.equal(a[other], b[other]), (kernel, "a neighbouring image or head moved")
        struck = b[1, 1].contiguous().view(_tdt(torch, dtype)).float()
        if kernel == binding.PACK_ATTN_AUTO:
            assert bool(torch.isposinf(struck).any()) and not bool(torch.isnan(struck).all()), "AUTO gave the generic kernel's all-NaN block"
        else:
            assert bool(torch.isnan(struck).all())


@pytest.mark.parametrize("dtype", [0, 1])
def test_auto_at_the_models_head_count(binding, torch_gpu, dtype):
    """D 1152, 16 heads of 72, unequal images: the descriptor length at every h up to 15, the search of the tables, more workgroups than a few CUs hold."""
    D, H, counts = 1152, 16, (729, 1, 196, 64)
    qkv = _qkv(torch_gpu, dtype, sum(counts), D, 72 + dtype)
    want = _run(binding, torch_gpu, dtype, binding.PACK_ATTN_GENERIC, qkv, counts, D, H)
    _same_with_canaries(torch_gpu, dtype, _run(binding, torch_gpu, dtype, binding.PACK_ATTN_AUTO, qkv, counts, D, H), want, counts)


def _contexts(binding, model, dtype, imgs, max_tokens, **kw):
    """Default against GENERIC context: equal launches, scratch bytes, class and token feature bits; the default reports STAGED.  -> both (probs, logits)."""
    res = {}
    for kern in (binding.PACK_ATTN_AUTO, binding.PACK_ATTN_GENERIC):
        pack = binding.PackContext(model, device=0, max_tokens=max_tokens, max_images=len(imgs), dtype=dtype, attn_kernel=kern, **kw)
        pack.feat_enable(cls=True, tokens=True)
        out, (cls, tok) = pack.forward(imgs), pack.feat_read()
        res[kern] = (pack.attn_kernel, pack.launches, pack.scratch_bytes, out, np.concatenate([_bits(t).reshape(-1) for t in [cls] + tok]))
        pack.close()
    auto, gen = res[binding.PACK_ATTN_AUTO], res[binding.PACK_ATTN_GENERIC]
    assert auto[0] == binding.PACK_ATTN_STAGED and gen[0] == binding.PACK_ATTN_GENERIC
    assert auto[1:3] == gen[1:3], (auto[1:3], gen[1:3])
    assert np.isfinite(auto[4].view(np.float32)).all() and np.array_equal(auto[4], gen[4]), "class or token features differ"
    return auto[3], gen[3]


@pytest.mark.parametrize("dtype", [0, 1])
def test_default_context_of_a_head_dim_72_model(pkg, binding, torch_gpu, dtype):
    """A class-token file with 16 heads of 72: equal bits of probabilities and logits too, probabilities within ref64.PROB_TOL of the float64 forward of
    every image alone.  Images: the file's own kind (test_gpu_head_dims.py), normalised synthetic u8 cut to four shapes: 6.5e-4 F16, 3.9e-3 bf16 measured;
    pack_data's exact pixels in [-4, 4) have 2.3 x that spread: BOTH contexts are 1.36e-3 off in F16 there, and the gate is not stated for such pixels."""
    path = pkg.synth.cached_synthetic("vit_mini_hd72_patch14_112", head_scale=4.0)
    model = binding.Model(path)
    shapes = [(14, 14), (112, 112), (70, 28), (126, 112)]                     # 2, 65, 11 and 73 token rows
    u8 = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(len(shapes), 126))
    imgs = [np.ascontiguousarray(u8[i][:h, :w]) for i, (h, w) in enumerate(shapes)]
    auto, gen = _contexts(binding, model, dtype, imgs, 256)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(auto, gen))
    t, rnd = PD.file_tensors(pkg, path), PD.f16_round if dtype == 0 else PD.bf16_round
    ref = np.concatenate([R64.forward64(t, im[None], 16, wround=rnd, uround=rnd, binding=binding)["probs"] for im in imgs])
    d = float(np.abs(auto[0] - ref).max())
    print(f"vit_mini_hd72 packed, dtype {dtype}: max|dprob| {d:.3e}")
    assert np.isfinite(auto[0]).all() and d <= R64.PROB_TOL[dtype]
    model.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_default_context_of_a_pooling_head_file(pkg, binding, torch_gpu, dtype):
    """The SigLIP-class file (D 576, 8 heads of 72, attention pooling): _contexts' comparison; its class feature is the pooled embedding."""
    model = binding.Model(siglip_file(pkg))
    _contexts(binding, model, dtype, pack_of([(28, 28), (14, 42), (56, 28)]), 16, pool_head=True)
    model.close()
