"""Packed batches on the GPU (include/vitx.h "packed batches"): the variable-length attention against the generic kernel per image, bit for bit,
with poisoned neighbours; the packed rotary launch against vitx_op_rope per image; a pack of one shape against the rectangular context, bit for
bit; mixed packs against the float64 restatement of every image at its own shape (tests/rect_data.py) with every mutant outside the gate; pack
invariance; the table cache; the four opt-in parts set, dropped and set again in different orders; the refusals; vit_cli.py --pack."""
import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import arch_data as AD
import depth_data as DD
import map_data as MD
import pack_data as KD
import pack_u8_data as UD
import prefix_data as PD
import preproc_data as PPD
import rect_data as XD
import ref64 as R64
import text_data as TD
from ref64 import PROB_TOL
from test_gpu_arch import ROUND

pytestmark = pytest.mark.gpu

D, L = 128, 2
SENT = -12345.5            # f32 buffers
SENT16 = -640.0             # 16-bit buffers: exact in fp16 and bf16
COUNTS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129, 197, 260, 577)
GATE = PROB_TOL[1]          # the bf16 gate for both operand types: plain fp16 carries three more mantissa bits than bf16, so that gate bounds it
TOKEN_GATE = 2.5e-2         # rms(d) <= 2.5e-2 rms on the final norm's patch rows: the bf16 stage gate of tests/ref64.py, as test_gpu_rect.py applies it


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tdt(torch, dtype):
    return torch.float16 if dtype == 0 else torch.bfloat16


def _raw(t):
    """The 16-bit patterns of a device tensor, on the host."""
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the attention kernel alone
def _attention_pack(binding, torch, dtype, counts, Dm, H, seed, qkv=None):
    """(packed output rows, the same rows by vitx_op_attention_generic image by image, the rows behind the last segment), as 16-bit patterns."""
    row0 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rows = int(row0[-1])
    if qkv is None:
        g = torch.Generator(device="cuda").manual_seed(seed)
        qkv = (torch.randn((rows, 3 * Dm), device="cuda", generator=g) * 0.8).to(_tdt(torch, dtype))
    out = torch.full((rows + 70, Dm), SENT16, dtype=_tdt(torch, dtype), device="cuda")
    d_row0 = torch.from_numpy(row0).cuda()
    binding.op_attention_packed(dtype, qkv.data_ptr(), out.data_ptr(), d_row0.data_ptr(), len(counts), Dm, H)
    torch.cuda.synchronize()
    want = torch.zeros((rows, Dm), dtype=_tdt(torch, dtype), device="cuda")
    for i, N in enumerate(counts):
        one, o = qkv[row0[i]:row0[i + 1]].clone(), torch.zeros((N, Dm), dtype=_tdt(torch, dtype), device="cuda")
        binding.check(binding.lib().vitx_op_attention_generic(dtype, one.data_ptr(), o.data_ptr(), 1, N, Dm, H, None))
        want[row0[i]:row0[i + 1]] = o
    torch.cuda.synchronize()
    return _raw(out[:rows]), _raw(want), out[rows:].float().cpu().numpy()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("DH", [32, 64, 80, 128])
def test_attention_packed_is_the_generic_kernel_per_image(binding, torch_gpu, DH, dtype):
    """H = 3.  Token counts around every tile edge (16-query tiles, 32-key steps, 64-query blocks) in a seeded shuffled order and reversed, 300 images of
    2 tokens (the work-list search must find every image), one image alone: every image's rows have the bits vitx_op_attention_generic writes for
    that image alone (n_img = 1), and the rows behind the last segment keep their sentinel."""
    H = 3
    order = [int(c) for c in np.random.default_rng(5).permutation(COUNTS)]
    for what, counts in (("shuffled", order), ("reversed", order[::-1]), ("300 x 2", [2] * 300), ("one image", [197])):
        got, want, tail = _attention_pack(binding, torch_gpu, dtype, counts, H * DH, H, seed=DH + dtype)
        assert (tail == SENT16).all(), (what, "rows behind the last segment were written")
        bad = np.argwhere(got != want)
        assert bad.size == 0, (what, DH, dtype, bad[:5].tolist())


@pytest.mark.parametrize("dtype", [0, 1])
def test_attention_packed_poisoned_neighbours(binding, torch_gpu, dtype):
    """On the pattern of test_attention_poisoned_neighbours: every other image of the pack is NaN in q, k and v and every other head of the clean
    images too; the clean (image, head) outputs have the bits of the clean run and are finite -- no key of a neighbour, no dim of a neighbouring
    head reaches them."""
    torch = torch_gpu
    H, DH = 3, 80
    Dm = H * DH
    counts = [37, 5, 64, 17, 130, 2, 33]
    row0 = np.concatenate([[0], np.cumsum(counts)])
    g = torch.Generator(device="cuda").manual_seed(3)
    clean = (torch.randn((int(row0[-1]), 3 * Dm), device="cuda", generator=g) * 0.8).to(_tdt(torch, dtype))
    poisoned = clean.clone()
    for i in range(len(counts)):
        v = poisoned[row0[i]:row0[i + 1]].view(counts[i], 3, H, DH)
        if i % 2:
            v[:] = float("nan")
        else:
            v[:, :, 0] = float("nan"); v[:, :, 2] = float("nan")
    a = _attention_pack(binding, torch, dtype, counts, Dm, H, 0, qkv=clean)[0].reshape(-1, H, DH)
    outp = torch.zeros((int(row0[-1]), Dm), dtype=_tdt(torch, dtype), device="cuda")
    d_row0 = torch.from_numpy(row0.astype(np.int32)).cuda()
    binding.op_attention_packed(dtype, poisoned.data_ptr(), outp.data_ptr(), d_row0.data_ptr(), len(counts), Dm, H)
    torch.cuda.synchronize()
    b = _raw(outp).reshape(-1, H, DH)
    for i in range(0, len(counts), 2):
        rows = slice(int(row0[i]), int(row0[i + 1]))
        assert bool(torch.isfinite(outp[rows].view(-1, H, DH)[:, 1].float()).all()), i
        assert np.array_equal(a[rows, 1], b[rows, 1]), i


# ------------------------------------------------------------------------------------------------ 3. the packed rotary launch
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("Dm,H", [(128, 2), (128, 4), (96, 4)], ids=["hd64", "hd32", "hd24-narrow"])
def test_rope_packed_is_rope_per_image(binding, torch_gpu, Dm, H, dtype):
    """Grids 1 x 1, 1 x 7, 5 x 2 and 4 x 4 in one pack, prefix 5; head dims 64 and 32 (16-byte accesses) and 24 (the per-element form).  Every image's
    rows have the bits of vitx_op_rope on that image alone; v columns, prefix rows and the rows behind the pack are untouched."""
    torch = torch_gpu
    prefix, half = 5, Dm // H // 2
    patches = [1, 7, 10, 16]
    counts = [prefix + p for p in patches]
    row0 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    toff = (np.concatenate([[0], np.cumsum(patches)[:-1]]) * half).astype(np.int32)
    rows = int(row0[-1])
    rng = np.random.default_rng(Dm + H)
    ang = rng.uniform(-3.0, 3.0, (sum(patches), half))
    cos, sin = torch.from_numpy(np.cos(ang).astype(np.float32)).cuda(), torch.from_numpy(np.sin(ang).astype(np.float32)).cuda()
    g = torch.Generator(device="cuda").manual_seed(9)
    src = torch.randn((rows + 9, 3 * Dm), device="cuda", generator=g).to(_tdt(torch, dtype))
    got = src.clone()
    d_row0, d_toff = torch.from_numpy(row0).cuda(), torch.from_numpy(toff).cuda()
    binding.op_rope_packed(dtype, got.data_ptr(), cos.data_ptr(), sin.data_ptr(), d_row0.data_ptr(), d_toff.data_ptr(), len(counts), prefix, Dm, H)
    torch.cuda.synchronize()
    want = src.clone()
    at = 0
    for i, N in enumerate(counts):
        one = src[row0[i]:row0[i + 1]].clone()
        c, s = cos[at:at + patches[i]].clone(), sin[at:at + patches[i]].clone()
        binding.op_rope(dtype, one.data_ptr(), c.data_ptr(), s.data_ptr(), 1, N, prefix, Dm, H)
        want[row0[i]:row0[i + 1]] = one
        at += patches[i]
    torch.cuda.synchronize()
    a, b, s0 = _raw(got), _raw(want), _raw(src)
    assert np.array_equal(a, b), np.argwhere(a != b)[:5].tolist()
    assert np.array_equal(a[:, 2 * Dm:], s0[:, 2 * Dm:]) and np.array_equal(a[rows:], s0[rows:])
    for i in range(len(counts)):
        assert np.array_equal(a[row0[i]:row0[i] + prefix], s0[row0[i]:row0[i] + prefix]), i
    assert not np.array_equal(a[:rows, :2 * Dm], s0[:rows, :2 * Dm])


# ------------------------------------------------------------------------------------------------ 4. a pack of one shape is the rectangular context
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("kind", KD.VARIANTS)
def test_uniform_pack_is_the_rect_context_bit_for_bit(pkg, binding, torch_gpu, kind, dtype):
    """n = 5 images of one shape at head dim 32: both sides run the generic attention arithmetic, the same patch-embedding kernel and bit-identical
    GEMM families, so probabilities, logits, VITX_FEAT_CLS and VITX_FEAT_TOKENS of the last layer have equal bits."""
    model = binding.Model(KD.variant_file(pkg, kind))
    P = model.hparams.patch_size
    shape = KD.UNIFORM_SHAPE[P]
    n, gh, gw = 5, shape[0] // P, shape[1] // P
    imgs = XD.images(n, *shape)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, img_shape=shape, last_layer_all_rows=1)
    ctx.feat_enable(cls=True, tokens=True)
    p, lg = ctx.forward(imgs, want_logits=True)
    f = ctx.feat_read(n)[L - 1]
    pack = binding.PackContext(model, device=0, max_tokens=n * ctx.tokens, max_images=n, dtype=dtype)
    pack.feat_enable(cls=True, tokens=True)
    pp, plg = pack.forward(list(imgs))
    cls, tok = pack.feat_read()
    assert np.isfinite(pp).all() and pack.launches[1] == 1
    assert np.array_equal(_bits(pp), _bits(p)) and np.array_equal(_bits(plg), _bits(lg))
    assert np.array_equal(_bits(cls), _bits(f["cls"]))
    assert all(t.shape == (gh, gw, D) for t in tok)
    assert np.array_equal(_bits(np.stack(tok).reshape(n, gh * gw, D)), _bits(f["tokens"]))
    ctx.close(); pack.close(); model.close()


# ------------------------------------------------------------------------------------------------ 5. mixed packs against the restatement
_T = {}


def _tensors(pkg, kind):
    if kind not in _T:
        _T[kind] = PD.file_tensors(pkg, XD.fixture_file(pkg, kind))
    return _T[kind]


@functools.lru_cache(maxsize=None)
def _pack(P):
    shapes = KD.mixed_shapes(P)
    return shapes, KD.pack_of(shapes)


_REF = {}


def _ref(pkg, binding, kind, dtype, mutant=None):
    """The restatement of every image of the mixed pack alone, at its own shape: [(probs [C], final-norm patch rows [gh gw][D])], once per key."""
    key = (kind, dtype, mutant)
    if key not in _REF:
        t = _tensors(pkg, kind)
        T = 1 + (t["reg_token"].shape[1] if "reg_token" in t else 0)
        out = []
        for im in _pack(t["patch_embed.proj.weight"].shape[-1])[1]:
            r = R64.forward64(t, im[None], XD.HEADS, mutant=mutant, wround=ROUND[dtype], uround=ROUND[dtype], binding=binding)
            out.append((r["probs"][0], r["final"][0, T:]))
        _REF[key] = out
    return _REF[key]


def _distances(probs, tok, ref):
    """Per image: (max|dprob|, rms(d) / rms on the final norm's patch rows)."""
    out = []
    for p, t, (rp, rt) in zip(probs, tok, ref):
        t = t.reshape(rt.shape)
        out.append((float(np.abs(p - rp).max()), float(np.sqrt(((t - rt) ** 2).mean()) / np.sqrt((rt ** 2).mean()))))
    return out


def _run_pack(binding, model, dtype, shapes, imgs, max_grids=0):
    pack = binding.PackContext(model, device=0, max_tokens=256, max_images=8, dtype=dtype, max_grids=max_grids)
    pack.feat_enable(cls=True, tokens=True)
    p, lg = pack.forward(imgs)
    cls, tok = pack.feat_read()
    return pack, p, lg, cls, tok


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("kind", ["p16", "p14r4", "p14rope"])
def test_mixed_pack_against_the_restatement_and_every_mutant(pkg, binding, torch_gpu, kind, dtype):
    """Seven images of five grids in one forward (head dim 64).  Every image against ref64.forward64 of its own shape: probabilities inside the
    bf16 gate (both operand types) and the final norm's patch rows inside the bf16 stage gate; every mutant of rect_data fails one of the two for at
    least one image.  (Probabilities alone do not separate every mutant on shapes this small -- pos_transposed moves them by 0.016 at most on
    p14r4, computed on the restatement -- the patch rows do: 0.35 of their rms and more, 0.049 for rope_transposed.)"""
    model = binding.Model(XD.fixture_file(pkg, kind))
    t = _tensors(pkg, kind)
    shapes, imgs = _pack(model.hparams.patch_size)
    pack, p, lg, cls, tok = _run_pack(binding, model, dtype, shapes, imgs)
    assert np.isfinite(p).all() and pack.launches[1] == len(shapes)          # no two neighbours of the mixed pack share a shape
    d = _distances(p, tok, _ref(pkg, binding, kind, dtype))
    print(f"{kind} {'F16' if dtype == 0 else 'BF16'}: max|dprob| {max(a for a, _ in d):.3e} (gate {GATE}), patch rows rms(d) / rms {max(b for _, b in d):.3e} (gate {TOKEN_GATE})")
    assert all(a <= GATE and b <= TOKEN_GATE for a, b in d), d
    for mut in XD.mutants_of(t):
        dm = _distances(p, tok, _ref(pkg, binding, kind, dtype, mut))
        assert any(a > GATE or b > TOKEN_GATE for a, b in dm), (kind, dtype, mut, dm)
    pack.close(); model.close()


# ------------------------------------------------------------------------------------------------ 6. pack invariance
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("kind", ["p16", "p14r4", "p14rope"])
def test_pack_invariance_bit_for_bit(pkg, binding, torch_gpu, kind, dtype):
    """The mixed pack forward, reversed, every image alone, and every image between two images of all-NaN pixels: the same image has the same
    probabilities, logits and features in all four runs."""
    model = binding.Model(XD.fixture_file(pkg, kind))
    shapes, imgs = _pack(model.hparams.patch_size)
    pack, p, lg, cls, tok = _run_pack(binding, model, dtype, shapes, imgs)
    same = lambda i, q, g, c, k, where: (np.array_equal(_bits(q), _bits(p[i])) and np.array_equal(_bits(g), _bits(lg[i])) and np.array_equal(_bits(c), _bits(cls[i]))
                                         and np.array_equal(_bits(k), _bits(tok[i]))) or pytest.fail(f"image {i} differs {where}")
    assert np.isfinite(p).all() and np.isfinite(lg).all() and np.isfinite(cls).all() and all(np.isfinite(k).all() for k in tok)
    n = len(imgs)
    q, g = pack.forward(imgs[::-1]); c, k = pack.feat_read()
    for i in range(n):
        same(i, q[n - 1 - i], g[n - 1 - i], c[n - 1 - i], k[n - 1 - i], "in the reversed pack")
    for i in range(n):
        q, g = pack.forward(imgs[i:i + 1]); c, k = pack.feat_read()
        same(i, q[0], g[0], c[0], k[0], "alone")
        nan = np.full_like(imgs[(i + 1) % n], np.nan)
        q, g = pack.forward([nan, imgs[i], nan]); c, k = pack.feat_read()
        same(i, q[1], g[1], c[1], k[1], "between two NaN images")
    pack.close(); model.close()


# ------------------------------------------------------------------------------------------------ 7. the table cache
@pytest.mark.parametrize("kind", ["p16", "p14rope"])
def test_table_cache_eviction_and_rebuild(pkg, binding, torch_gpu, kind):
    """max_grids = 2: three calls whose grids force an eviction and a rebuild give the bits of a context with the default cache; a call with three
    distinct grids is refused before anything is launched (the output buffer keeps its sentinel)."""
    torch = torch_gpu
    model = binding.Model(XD.fixture_file(pkg, kind))
    P = model.hparams.patch_size
    a, b, c = (2 * P, 5 * P), (5 * P, 2 * P), (3 * P, 3 * P)
    calls = [[a, b, a], [c, c], [b, a], [c, a]]
    tokens = max(int(binding.pack_check(model, s, 10 ** 6, 8)[-1]) for s in calls)
    small = binding.PackContext(model, device=0, max_tokens=tokens, max_images=3, dtype=binding.BF16, max_grids=2)
    big = binding.PackContext(model, device=0, max_tokens=tokens, max_images=3, dtype=binding.BF16, max_grids=32)
    for s in calls:
        imgs = KD.pack_of(s, seed=11)
        (p1, l1), (p2, l2) = small.forward(imgs), big.forward(imgs)
        assert np.isfinite(p1).all() and np.array_equal(_bits(p1), _bits(p2)) and np.array_equal(_bits(l1), _bits(l2)), s
    three = [a, b, c]
    pix = torch.from_numpy(np.concatenate([i.ravel() for i in KD.pack_of(three)])).cuda()
    probs = torch.full((3, model.num_classes), SENT, dtype=torch.float32, device="cuda")
    with pytest.raises(binding.VitxError) as ei:
        small.forward_device(pix.data_ptr(), three, probs.data_ptr())
    assert ei.value.code == binding.ERR_ARG and "max_grids" in str(ei.value)
    torch.cuda.synchronize()
    assert bool((probs == SENT).all())
    big.forward_device(pix.data_ptr(), three, probs.data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(probs).all())
    small.close(); big.close(); model.close()


# ------------------------------------------------------------------------------------------------ 7b. the opt-in parts in any order
def test_parts_set_in_any_order_make_the_same_context(pkg, binding, torch_gpu):
    """The four opt-in parts that bring segment tables (dense head, depth head, u8 sources, attention rollout) on two contexts of the 4-head patch-16
    variant, bf16, the mixed pack fed from u8 originals of seven different sizes.  A turns them on as dense, depth, u8, rollout; B as rollout, u8, depth,
    dense, then takes depth off and sets it again, then u8 likewise.  The same forward_u8 call, twice, then has equal bits on both -- probabilities,
    logits, labels, scores, kept logits, depth maps, fine planes, offsets, class maps, rollout rows -- and the bits of its first run (the forward is
    deterministic), with equal launch counts and scratch bytes; and with the parts taken off in a third order each context is back at the scratch bytes
    it had before any part was set (its grids' tables built: a device call with no part on does that and allocates nothing else)."""
    torch = torch_gpu
    model = binding.Model(KD.variant_file(pkg, "p16h4"))
    shapes = KD.mixed_shapes(16)
    imgs = UD.originals()
    assert len(imgs) == len(shapes) and len({im.shape for im in imgs}) == len(imgs)
    mean, std = PPD.mean_std255(PPD.IMAGENET)
    pp = binding.Preproc.make(resize_a=16, resize_b=16, filter=PPD.PP_PIL_BICUBIC, mean255=mean, std255=std)
    tokens = int(binding.pack_check(model, shapes, 2 ** 31 - 1, len(shapes))[-1])
    rng = np.random.default_rng(12)
    W, b = (rng.standard_normal((5, D)) * 0.25).astype(np.float32), rng.standard_normal(5).astype(np.float32)
    wp, wc = ((rng.standard_normal((21, D)) * 0.05).astype(np.float32) for _ in range(2))
    db, bins = rng.standard_normal(21).astype(np.float32), DD.bins_ud(21)
    on = {"dense": lambda c: c.dense_set(W, b, None, score=True, logits=True),
          "depth": lambda c: c.depth_set(wp, wc, db, bins, None, 2, 3.0, 7.0, logits=True, fine=True),
          "u8": lambda c: c.u8_set(pp, max_src_bytes=sum(im.size for im in imgs)),
          "rollout": lambda c: c.attn_enable(None, rollout=True)}
    off = {"dense": lambda c: c.dense_set(None), "depth": lambda c: c.depth_set(None), "u8": lambda c: c.u8_set(None, 0), "rollout": lambda c: c.attn_disable()}
    A, B = (binding.PackContext(model, device=0, max_tokens=tokens, max_images=len(shapes), dtype=binding.BF16) for _ in range(2))
    pix = torch.zeros(sum(3 * h * w for h, w in shapes), dtype=torch.float32, device="cuda")
    probs = torch.zeros((len(shapes), model.num_classes), dtype=torch.float32, device="cuda")
    base = []
    for c in (A, B):
        c.forward_device(pix.data_ptr(), shapes, probs.data_ptr())
        torch.cuda.synchronize()
        base.append(c.scratch_bytes)
    assert base[0] == base[1]
    for part in ("dense", "depth", "u8", "rollout"):
        on[part](A)
    for part in ("rollout", "u8", "depth", "dense"):
        on[part](B)
    assert B.scratch_bytes == A.scratch_bytes > base[0]
    for part in ("depth", "u8"):
        off[part](B)
        assert base[0] < B.scratch_bytes < A.scratch_bytes, part
        on[part](B)
        assert B.scratch_bytes == A.scratch_bytes, part

    def run(c):
        """Every output of one forward_u8 call as a flat list of (name, array), and the counters."""
        p, lg = c.forward_u8(imgs, shapes)
        lab, sc, dlg = c.dense_read()
        dm, fn, plg, offs = c.depth_read()
        maps = c.attn_read()
        out = [("probs", p), ("logits", lg), ("offsets", offs)]
        for name, per_image in (("labels", lab), ("scores", sc), ("dense logits", dlg), ("depth", dm), ("fine", fn), ("depth logits", plg),
                                ("class maps", [m[0] for m in maps]), ("rollout", [m[1] for m in maps])):
            out += [(f"{name} of image {i}", a) for i, a in enumerate(per_image)]
        return out, (c.launches, c.scratch_bytes, c.dense_scratch_bytes(), c.depth_scratch_bytes())

    def same(x, y, what):
        assert len(x) == len(y)
        for (name, a), (_, b_) in zip(x, y):
            a, b_ = np.ascontiguousarray(a), np.ascontiguousarray(b_)
            assert a.shape == b_.shape and a.size and np.array_equal(a.view(np.uint8), b_.view(np.uint8)), (what, name)

    first = None
    for call in range(2):
        (oa, ca), (ob, cb) = run(A), run(B)
        assert all(np.isfinite(np.asarray(a, np.float64)).all() for _, a in oa)
        same(oa, ob, f"call {call}: A against B")
        assert ca == cb, (call, ca, cb)
        if first is None:
            first = oa
        else:
            same(first, oa, "A: the second call against the first")
    for c, was in zip((A, B), base):
        for part in ("u8", "dense", "rollout", "depth"):
            off[part](c)
        assert c.scratch_bytes == was
    A.close(); B.close(); model.close()


# ------------------------------------------------------------------------------------------------ 8. refusals at creation
def test_refusals_at_creation(pkg, binding, torch_gpu, tmp_path):
    def code(model, dtype=binding.BF16, max_tokens=64, max_images=2):
        with pytest.raises(binding.VitxError) as ei:
            binding.PackContext(model, device=0, max_tokens=max_tokens, max_images=max_images, dtype=dtype)
        return ei.value.code
    UNS, ARG = binding.ERR_UNSUPPORTED, binding.ERR_ARG
    ok = binding.Model(XD.fixture_file(pkg, "p16"))
    assert code(ok, dtype=binding.MXFP8) == UNS
    assert code(ok, max_tokens=2 ** 31 - 1) == UNS                                       # beyond the kernels' 32-bit window
    hp, t = XD.fixture_tensors(pkg, "p16")
    odd = str(tmp_path / "hd4.gguf")
    pkg.ggml_file.write_model(odd, dataclasses.replace(hp, num_attention_heads=32), t)   # head dim 4
    m = binding.Model(odd); assert code(m) == UNS; m.close()
    hp832 = pkg.ggml_file.HParams(832, 1, 13, 10, 16, 32)                                # D = 832 = 13 x 64: no LayerNorm width
    wide = str(tmp_path / "d832.gguf")
    pkg.ggml_file.write_model(wide, hp832, pkg.synth.make_weights(hp832, head_scale=4.0))
    m = binding.Model(wide); assert code(m) == UNS; m.close()
    for path in (pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0), MD.fixture_file(pkg), AD.fixture_file(pkg, "dinov2_erf")):
        m = binding.Model(path); assert code(m) == UNS, path; m.close()                   # ViTSTR, the attention-pooling head, the cls + mean head
    text = binding.Model(TD.text_file(pkg, "clip"))
    assert code(text) == ARG
    text.close()
    pack = binding.PackContext(ok, device=0, max_tokens=64, max_images=2, dtype=binding.BF16)      # and the plain case is accepted
    assert pack.forward([XD.images(1, 16, 48)[0]])[0].shape == (1, 10)
    pack.close(); ok.close()


# ------------------------------------------------------------------------------------------------ 9. end to end
def test_cli_pack_prints_the_lines_of_the_per_image_path(pkg, binding, torch_gpu):
    """vit_cli.py --pack --img-fit 32 on two golden assets, the 4-head patch-16 variant (both paths then run the same attention arithmetic): the
    printed top-k lines are those of the per-image --img-fit runs, image after image."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = KD.variant_file(pkg, "p16h4")
    files = [os.path.join(root, "tests", "golden", "assets", f) for f in ("tench.jpg", "kiwi.jpg")]
    cli = [sys.executable, os.path.join(root, "vit_cli.py"), "-m", src, "--dtype", "bf16", "--img-fit", "32"]
    single = []
    for f in files:
        r = subprocess.run(cli + ["-i", f], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        single.append(r.stdout)
    r = subprocess.run(cli + ["--pack", "-i", ",".join(files)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count(" > ") == 10 and r.stdout == "".join(single)
    bad = subprocess.run(cli[:-2] + ["--pack", "-i", ",".join(files)], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "--pack takes --img-fit" in bad.stderr
