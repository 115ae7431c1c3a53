"""The LDS-staged attention of head dims 72 .. 128 (attention_wide.hip; include/vitx.h, vitx_op_attention_wide): the generic kernel's bits per (image,
head) with nothing written outside its rows, the float64 softmax(Q K^T / sqrt(hd)) V of the rounded operands with the generic kernel's own error as the
yardstick, and NaN neighbours (an image, a head) that stay out of a clean (image, head).  Then the model that needs it end to end: D 576, 8 heads
(head dim 72), an MLP of width 1000 from the file's `mlp` tensor (include/vitx.h "MLP width"), against tests/ref64.py under that file's gates.
What equal bits cannot show is tested on its own: the model's 16 heads over several rounds of the device on flat data, repeated launches, the half-live last
V tile of head dims 72 and 120, an infinite last value row.  The exact designs at these head dims: test_gpu_exact.py, test_gpu_attention.py (family `wide`)."""
import functools

import numpy as np
import pytest

import exact_data as X
import prefix_data as PD
import ref64 as R64
import text_data as TD
import zs_data as Z
from test_cpu_mlp_width import F, H, mlp_file, siglip_file
from test_gpu_exact import _same
from test_gpu_pack import SENT16, _bits, _tdt

pytestmark = pytest.mark.gpu

N_IMG, GUARD = 3, 70
# one tile, each side of the 16- and 32-key steps, whole chunks (64, 128, 192: the last chunk is full) and their neighbours, a partial chunk behind a full one, many chunks
COUNTS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 192, 193, 577)


def _qkv(torch, dtype, rows, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn((rows, 3 * D), device="cuda", generator=g) * 0.8).to(_tdt(torch, dtype))


def _run(binding, torch, dtype, wide, qkv, n_img, N, D, H):
    """out with GUARD canary rows in front of and behind the n_img * N rows the kernel owns, as 16-bit patterns; wide: True, False (the generic kernel), "packed" (vitx_op_attention_packed), None (the dispatcher)."""
    out = torch.full((2 * GUARD + n_img * N, D), SENT16, dtype=_tdt(torch, dtype), device="cuda")
    o = out.data_ptr() + GUARD * D * 2
    if wide is None:
        binding.check(binding.lib().vitx_op_attention(dtype, qkv.data_ptr(), o, n_img, N, D, H, None))
    elif wide == "packed":            # the same images as one pack
        row0 = torch.arange(0, (n_img + 1) * N, N, dtype=torch.int32, device="cuda")
        binding.op_attention_packed(dtype, qkv.data_ptr(), o, row0.data_ptr(), n_img, D, H)
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


# ------------------------------------------------------------------------------------------------ what "the generic kernel's bits" cannot show
SO400M = (8, 729, 1152, 16)        # images, tokens, D, heads of the model the kernel exists for (head dim 72): 8 * 16 * 12 = 1536 workgroups, 40 MB of qkv


@functools.lru_cache(maxsize=1)
def _so400m_flat():
    n_img, N, D, H = SO400M
    qkv, c = X.flat_qkv(n_img, N, H, D // H, -1, 729)
    return qkv, X.flat_expected(c, N)


@pytest.mark.parametrize("dtype", [0, 1])
def test_wide_at_the_models_head_count_and_several_rounds(binding, torch_gpu, dtype):
    """16 heads of 72 at 729 tokens: the descriptor length (N * 3 D - h * DH) * 2 and the blockIdx split at every h up to 15, more workgroups than the
    device holds at once.  Flat data, sign -1 (a zero key counted in a row sum outweighs the real ones by e^24): the whole buffer is c, bit for bit.
    randn: the generic kernel's bits, canary rows intact; three launches on one input agree -- with one barrier per chunk of the double buffer, a
    wave that restaged a buffer another wave still reads shows as a difference between runs."""
    torch = torch_gpu
    n_img, N, D, H = SO400M
    qkv32, want = _so400m_flat()
    tdt = _tdt(torch, dtype)
    got = _run(binding, torch, dtype, True, torch.from_numpy(qkv32).cuda().to(tdt), n_img, N, D, H)[GUARD:-GUARD].view(tdt)
    _same(torch, got, torch.from_numpy(want).cuda().to(tdt), f"wide flat {SO400M} dtype {dtype}")
    qkv = _qkv(torch, dtype, n_img * N, D, 72 + dtype)
    want = _run(binding, torch, dtype, False, qkv, n_img, N, D, H)
    sent = torch.full((GUARD, D), SENT16, dtype=tdt, device="cuda").view(torch.int16)
    for launch in range(3):
        got = _run(binding, torch, dtype, True, qkv, n_img, N, D, H)
        assert torch.equal(got[:GUARD], sent) and torch.equal(got[-GUARD:], sent), (launch, "canary rows were written")
        assert torch.equal(got, want), (launch, torch.nonzero(got != want)[:5].tolist())


KERNELS = ((True, "wide"), (False, "generic"), ("packed", "packed"))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hd,N", [(72, 33), (72, 130), (120, 33), (120, 130)])
def test_half_live_v_tile_keeps_the_next_rows_bytes_out(binding, torch_gpu, hd, N, dtype):
    """Head dims 72 and 120: the last 16-dim tile of V^T is half live, and in the wide kernel its upper half holds the first 16 bytes of the NEXT key
    row of the same head.  Those bytes NaN (v[:, 0:8] of head 1, every key row): columns 0 .. 7 of head 1 are NaN, columns 8 .. DH - 1 of head 1 and
    all of heads 0 and 2 keep the clean run's bits, in the wide, the generic and the packed kernel."""
    torch = torch_gpu
    H, D = 3, 3 * hd
    clean = _qkv(torch, dtype, N_IMG * N, D, 53 + hd + N + dtype)
    bad = clean.clone()
    bad.view(N_IMG * N, 3, H, hd)[:, 2, 1, 0:8] = float("nan")
    for kernel, name in KERNELS:
        a = _run(binding, torch, dtype, kernel, clean, N_IMG, N, D, H)[GUARD:-GUARD].view(-1, H, hd)
        b = _run(binding, torch, dtype, kernel, bad, N_IMG, N, D, H)[GUARD:-GUARD].view(-1, H, hd)
        assert bool(torch.isfinite(a.view(_tdt(torch, dtype)).float()).all()), name
        assert torch.equal(a[:, [0, 2]], b[:, [0, 2]]), (name, "heads 0 and 2 moved")
        assert torch.equal(a[:, 1, 8:], b[:, 1, 8:]), (name, "columns 8 .. of head 1 moved", torch.nonzero(a[:, 1, 8:] != b[:, 1, 8:])[:5].tolist())
        assert bool(torch.isnan(b[:, 1, :8].contiguous().view(_tdt(torch, dtype)).float()).all()), (name, "columns 0 .. 7 of head 1 are not all NaN")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hd", [72, 120])
def test_a_nan_head_stays_out_of_its_neighbours_pad_dims(binding, torch_gpu, hd, dtype):
    """Head dims 72 and 120 pad the score product's K dimension to 96 and 128: the pad of q AND of k is the constant zero, never the next head's
    bytes (0 * NaN is NaN: one zero side is not enough).  Head 1's q, k and v NaN: heads 0 and 2 keep the clean run's bits in all three kernels."""
    torch = torch_gpu
    H, D, N = 3, 3 * hd, 33
    clean = _qkv(torch, dtype, N_IMG * N, D, 77 + hd + dtype)
    bad = clean.clone()
    bad.view(N_IMG * N, 3, H, hd)[:, :, 1] = float("nan")
    for kernel, name in KERNELS:
        a = _run(binding, torch, dtype, kernel, clean, N_IMG, N, D, H)[GUARD:-GUARD].view(-1, H, hd)
        b = _run(binding, torch, dtype, kernel, bad, N_IMG, N, D, H)[GUARD:-GUARD].view(-1, H, hd)
        assert torch.equal(a[:, [0, 2]], b[:, [0, 2]]), (name, "heads 0 and 2 moved")
        assert bool(torch.isnan(b[:, 1].contiguous().view(_tdt(torch, dtype)).float()).all()), name


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hd", [72, 120])
def test_a_key_with_an_infinite_dim_weighs_nothing_where_the_query_turns_from_it(binding, torch_gpu, hd, dtype):
    """k[j][0] = +Inf for one key of every (image, head): a query with q[0] < 0 scores it -Inf, float64 gives it the weight 0 and a finite row.  A pad
    piece of the score product that wrapped round to the key's piece 0 would add 0 * Inf = NaN to that score -- on finite data the zero pad of q hides
    such a piece completely.  Those rows are finite in all three kernels and have the generic kernel's bits."""
    torch = torch_gpu
    H, D, N = 2, 2 * hd, 65
    qkv = _qkv(torch, dtype, N_IMG * N, D, 19 + hd + dtype)
    x = qkv.view(N_IMG, N, 3, H, hd)
    x[:, 40, 1, :, 0] = float("inf")
    turned = (x[:, :, 0, :, 0].float() < 0)                                  # [image][query][head]
    assert bool(turned.any(dim=1).all()) and not bool((x[:, :, 0, :, 0] == 0).any())
    rows = {}
    for kernel, name in KERNELS:
        o = _run(binding, torch, dtype, kernel, qkv, N_IMG, N, D, H)[GUARD:-GUARD].view(N_IMG, N, H, hd)
        rows[name] = o[turned]
        assert bool(torch.isfinite(rows[name].view(_tdt(torch, dtype)).float()).all()), (name, "a row that gives the infinite key no weight is not finite")
    assert torch.equal(rows["wide"], rows["generic"]) and torch.equal(rows["packed"], rows["generic"])


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hd", [72, 120])
def test_an_infinite_last_value_row_stays_in_its_image_and_head(binding, torch_gpu, hd, dtype):
    """N = 33 (N % 32 != 0), v[N - 1] of (image 1, head 1) = +Inf: the one input on which the wide kernel's bits may differ from the generic kernel's
    (attention_wide.hip: keys past N are zeros there, the image's last row here).  Every other (image, head) keeps the clean run's bits in all three
    kernels; in the wide kernel the struck one holds no finite value -- float64 says +Inf everywhere (every weight is positive), a numerator that
    rounds to zero makes it NaN, and a finite element would be a key row that was dropped."""
    torch = torch_gpu
    H, D, N = 3, 3 * hd, 33
    clean = _qkv(torch, dtype, N_IMG * N, D, 91 + hd + dtype)
    bad = clean.clone()
    bad.view(N_IMG, N, 3, H, hd)[1, N - 1, 2, 1] = float("inf")
    other = torch.ones((N_IMG, H), dtype=torch.bool, device="cuda")
    other[1, 1] = False
    for kernel, name in KERNELS:
        a = _run(binding, torch, dtype, kernel, clean, N_IMG, N, D, H)[GUARD:-GUARD].view(N_IMG, N, H, hd).transpose(1, 2)
        b = _run(binding, torch, dtype, kernel, bad, N_IMG, N, D, H)[GUARD:-GUARD].view(N_IMG, N, H, hd).transpose(1, 2)
        assert torch.equal(a[other], b[other]), (name, "a neighbouring image or head moved")
        if name == "wide":
            assert not bool(torch.isfinite(b[1, 1].contiguous().view(_tdt(torch, dtype)).float()).any()), "a finite value in the struck (image, head)"


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
