"""The LDS-staged attention of head dims 72 .. 128 (attention_wide.hip; include/vitx.h, vitx_op_attention_wide): the generic kernel's bits per (image,
head) with nothing written outside its rows, the float64 softmax(Q K^T / sqrt(hd)) V of the rounded operands with the generic kernel's own error as the
yardstick, and NaN neighbours (an image, a head) that stay out of a clean (image, head).  Then the model that needs it end to end: D 576, 8 heads
(head dim 72), an MLP of width 1000 from the file's `mlp` tensor (include/vitx.h "MLP width"), against tests/ref64.py under that file's gates."""
import numpy as np
import pytest

import prefix_data as PD
import ref64 as R64
import text_data as TD
import zs_data as Z
from test_cpu_mlp_width import F, H, mlp_file, siglip_file
from test_gpu_pack import SENT16, _bits, _tdt

pytestmark = pytest.mark.gpu

N_IMG, GUARD = 3, 70
COUNTS = (1, 15, 17, 32, 33, 63, 65, 129, 130, 193, 577)      # one tile, each side of the 16- and 32-key steps, a partial chunk behind a full one, many chunks


def _qkv(torch, dtype, rows, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn((rows, 3 * D), device="cuda", generator=g) * 0.8).to(_tdt(torch, dtype))


def _run(binding, torch, dtype, wide, qkv, n_img, N, D, H):
    """out with GUARD canary rows in front of and behind the n_img * N rows the kernel owns, as 16-bit patterns; the dispatcher where wide is None."""
    out = torch.full((2 * GUARD + n_img * N, D), SENT16, dtype=_tdt(torch, dtype), device="cuda")
    o = out.data_ptr() + GUARD * D * 2
    if wide is None:
        binding.check(binding.lib().vitx_op_attention(dtype, qkv.data_ptr(), o, n_img, N, D, H, None))
    elif wide:
        binding.op_attention_wide(dtype, qkv.data_ptr(), o, n_img, N, D, H)
    else:
        binding.check(binding.lib().vitx_op_attention_generic(dtype, qkv.data_ptr(), o, n_img, N, D, H, None))
    torch.cuda.synchronize()
    return out.view(torch.int16)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hd", [72, 80, 88, 96, 104, 112, 120, 128])
def test_wide_has_the_generic_kernels_bits(binding, torch_gpu, hd, dtype):
    """Every token count: the whole buffer, canary rows included, equals the generic kernel's; the dispatcher gives the same bits at these head dims."""
    torch = torch_gpu
    H, D = 2, 2 * hd
    for N in COUNTS:
        qkv = _qkv(torch, dtype, N_IMG * N, D, 100 * hd + N + dtype)
        want = _run(binding, torch, dtype, False, qkv, N_IMG, N, D, H)
        got = _run(binding, torch, dtype, True, qkv, N_IMG, N, D, H)
        sent = torch.full((GUARD, D), SENT16, dtype=_tdt(torch, dtype), device="cuda").view(torch.int16)
        assert torch.equal(got[:GUARD], sent) and torch.equal(got[-GUARD:], sent), (hd, N, "canary rows were written")
        assert torch.equal(got, want), (hd, N, torch.nonzero(got != want)[:5].tolist())
        assert torch.equal(_run(binding, torch, dtype, None, qkv, N_IMG, N, D, H), want), (hd, N, "vitx_op_attention")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hd", [72, 128])
def test_wide_against_float64(binding, torch_gpu, hd, dtype):
    """max |out - float64| of the wide kernel is at most the generic kernel's on the same inputs (equal bits: no margin)."""
    torch = torch_gpu
    H, D, N = 2, 2 * hd, 130
    qkv = _qkv(torch, dtype, N_IMG * N, D, 7 + hd + dtype)
    q, k, v = (qkv.double().view(N_IMG, N, 3, H, hd)[:, :, j].transpose(1, 2) for j in range(3))
    ref = (torch.softmax(q @ k.transpose(2, 3) / np.sqrt(hd), dim=-1) @ v).transpose(1, 2).reshape(N_IMG * N, D)
    err = {}
    for wide in (False, True):
        out = _run(binding, torch, dtype, wide, qkv, N_IMG, N, D, H)[GUARD:-GUARD].view(_tdt(torch, dtype))
        err[wide] = float((out.double() - ref).abs().max())
    print(f"wide attention hd {hd} {'f16' if dtype == 0 else 'bf16'} N {N}: max |d| wide {err[True]:.3e}, generic {err[False]:.3e}")
    assert err[True] <= err[False] < 0.05 * float(ref.abs().max())


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hd,N", [(72, 33), (72, 130), (128, 130)])
def test_wide_nan_neighbours_stay_out(binding, torch_gpu, hd, N, dtype):
    """Three heads, three images.  Image 1 all NaN: images 0 and 2 have the bits they have alone.  Head 1's q, k and v NaN: heads 0 and 2 keep the bits
    of the clean run -- at head dim 72 the pad pieces of the score product's K dimension (dims 72 .. 95) are zeros by construction, never head 1's bytes."""
    torch = torch_gpu
    H, D = 3, 3 * hd
    clean = _qkv(torch, dtype, N_IMG * N, D, 31 + hd + N + dtype)
    a = _run(binding, torch, dtype, True, clean, N_IMG, N, D, H)[GUARD:-GUARD]
    bad = clean.clone()
    bad[N:2 * N] = float("nan")
    b = _run(binding, torch, dtype, True, bad, N_IMG, N, D, H)[GUARD:-GUARD]
    for i in (0, 2):
        assert torch.equal(b[i * N:(i + 1) * N], _run(binding, torch, dtype, True, clean[i * N:(i + 1) * N].clone(), 1, N, D, H)[GUARD:-GUARD]), (hd, i)
    bad = clean.clone()
    bad.view(N_IMG * N, 3, H, hd)[:, :, 1] = float("nan")
    b = _run(binding, torch, dtype, True, bad, N_IMG, N, D, H)[GUARD:-GUARD].view(-1, H, hd)
    assert torch.equal(a.view(-1, H, hd)[:, [0, 2]], b[:, [0, 2]]) and bool(torch.isfinite(a.view(_tdt(torch, dtype)).float()).all())


# ------------------------------------------------------------------------------------------------ end to end: head dim 72 and the `mlp` width 1000
_REF = {}


def _ref(pkg, dtype):
    if dtype not in _REF:
        imgs = PD.exact_images(5, 56, seed=1)
        t = PD.file_tensors(pkg, mlp_file(pkg))
        _REF[dtype] = (imgs, R64.forward64(t, imgs, H, wround=PD.f16_round if dtype == 0 else PD.bf16_round, uround=PD.f16_round if dtype == 0 else PD.bf16_round))
    return _REF[dtype]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("context", ["image", "packed"])
def test_width_1000_model_against_float64(pkg, binding, torch_gpu, context, dtype):
    """Probabilities within ref64.PROB_TOL of the float64 forward; the image context of the same model filed at width 1024 with the zeros written out
    has the same bits (the padding rule is exact)."""
    imgs, ref = _ref(pkg, dtype)
    model = binding.Model(mlp_file(pkg))
    if context == "image":
        ctx = binding.Context(model, device=0, max_batch=5, dtype=dtype)
        p, lg = ctx.forward(imgs, want_logits=True)
        ctx.close()
        padded = binding.Model(mlp_file(pkg, pad_to=1024))
        assert padded.mlp_width == 1024
        ctx = binding.Context(padded, device=0, max_batch=5, dtype=dtype)
        p2, lg2 = ctx.forward(imgs, want_logits=True)
        ctx.close(); padded.close()
        assert np.array_equal(_bits(p), _bits(p2)) and np.array_equal(_bits(lg), _bits(lg2))
    else:
        pack = binding.PackContext(model, device=0, max_tokens=5 * 17, max_images=5, dtype=dtype)
        p, lg = pack.forward([im for im in imgs])
        pack.close()
    model.close()
    d = float(np.abs(p - ref["probs"]).max())
    print(f"mlp width {F} {context} dtype {dtype}: max|dprob| {d:.3e}, max|dlogit| {float(np.abs(lg - ref['logits']).max()):.3e}")
    assert np.isfinite(p).all() and d <= R64.PROB_TOL[dtype]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("context", ["image", "packed"])
def test_pooling_head_of_width_1000_against_float64(pkg, binding, torch_gpu, context, dtype):
    """The converted SiglipVisionModel of test_cpu_mlp_width (D 576, heads of 72, MLP 1000 in the blocks AND the attention-pooling head): the pooled
    embedding, L2-normalised, against ref64's float64 forward.  Gate: 3 x the error of the restatement with the device's operand roundings (the
    project's emulation factor, tests/test_gpu_text.py), maximum and mean."""
    imgs = PD.exact_images(3, 28, seed=2)
    t = PD.file_tensors(pkg, siglip_file(pkg))
    rnd = PD.f16_round if dtype == 0 else PD.bf16_round
    r64, rop = Z.normalise64(R64.forward64(t, imgs, H)["e"]), Z.normalise64(R64.forward64(t, imgs, H, wround=rnd, uround=rnd)["e"])
    model = binding.Model(siglip_file(pkg))
    if context == "image":
        ctx = binding.Context(model, device=0, max_batch=3, dtype=dtype)
        ctx.feat_enable(cls=True)
        ctx.forward(imgs)
        e = ctx.feat_read(3)[1]["cls"]
    else:
        ctx = binding.PackContext(model, device=0, max_tokens=12, max_images=3, dtype=dtype, pool_head=True)
        ctx.feat_enable(cls=True)
        ctx.forward([im for im in imgs])
        e = ctx.feat_read()[0]
    ctx.close(); model.close()
    a, b = np.abs(Z.normalise64(np.asarray(e, np.float64)) - r64), np.abs(rop - r64)
    print(f"pooling head, mlp width {F}, {context} dtype {dtype}: max|dev - R64| {a.max():.3e}, max|Rop - R64| {b.max():.3e}; mean {a.mean():.3e} / {b.mean():.3e}")
    assert np.isfinite(e).all() and a.max() <= 3 * b.max() and a.mean() <= 3 * b.mean()


@pytest.mark.parametrize("dtype", [0, 1])
def test_text_tower_of_width_1000(pkg, binding, torch_gpu, dtype):
    """text_data's micro CLIP text tower with intermediate_size 1000, converted with mlp_width=True: the gate of tests/test_gpu_text.py."""
    import torch
    import transformers
    torch.manual_seed(11)
    hf = transformers.CLIPTextModelWithProjection(transformers.CLIPTextConfig(**dict(TD.CLIP_CFG, intermediate_size=1000))).double().eval()
    path = R64.cached_file("text-clip-micro-mlp1000", lambda tmp: pkg.convert.convert_hf_text_model(hf, tmp, mlp_width=True))
    t, ids = PD.file_tensors(pkg, path), TD.prompts("clip")
    r64, rop = Z.normalise64(TD.forward64(t, ids)), Z.normalise64(TD.forward64(t, ids, wround=Z.ROUND[dtype], uround=Z.ROUND[dtype]))
    model = binding.Model(path)
    assert model.mlp_width == 1000
    ctx = binding.TextContext(model, max_prompts=TD.N_PROMPTS, dtype=dtype)
    dev = ctx.embed(ids, l2=True).astype(np.float64)
    ctx.close(); model.close()
    a, b = np.abs(dev - r64), np.abs(rop - r64)
    print(f"text mlp width 1000 dtype {dtype}: max|dev - R64| {a.max():.3e}, max|Rop - R64| {b.max():.3e}")
    assert np.isfinite(dev).all() and a.max() <= 3 * b.max() and a.mean() <= 3 * b.mean()
