"""A NaN or Inf image stays in its own outputs (include/vitx.h: "images are independent in every kernel"; data: tests/poison_data.py,
conditions: test_cpu_poison_data.py).

A kernel that stages a whole tile of keys reads, behind the last key of an image, the first rows of the NEXT image.  It masks their scores
to -inf, so their probabilities are exactly 0 -- and 0 . NaN and 0 . Inf are NaN in the P.V product.  Finite neighbours cannot show that
read, and a NaN planted behind the tensor is never fetched; here whole neighbouring images are NaN, +Inf, -Inf and, as the control that must
be harmless, the operand type's largest finite number.

  * op level, every attention family and entry point: three images, two heads, images {0, 2} poisoned and then image {1}.
      flat data    the clean images' rows equal c (text: the staircase) BIT FOR BIT in a NaN-filled buffer -- known without any device run;
      spread data  the clean images pass the float64 gates of test_gpu_attention.py and have the bits of the same launch with the finite
                   data in place of the poison.
    Token counts: the smallest at which a family has padded keys, and its tile-aligned count as a control (no padded key: it passes on any
    build).  On 197 tokens q, k and v are also poisoned one at a time, so a failure names the operand.
  * forward level, the main context: [A, P, B, P, C] with P all-NaN, one +Inf pixel, all 1e30: the clean images' outputs are finite and
    have the bits of the same call with finite images at the poisoned positions.

Rows of poisoned images are not asserted: the launch returns success, what it writes there is that image's business.
"""
import numpy as np
import pytest

import arch_data as AD
import exact_data as X
import map_data as MD
import poison_data as P
import prefix_data as PD
import rope_data as RD
import swiglu_data as SD
import test_gpu_attn_map as TM
import test_gpu_exact as TE
import test_gpu_rollout as TR
import test_gpu_text as TT
import text_data as TD
import wide_data as WD
import zs_data as Z

pytestmark = pytest.mark.gpu

n_img, H = P.N_IMG, P.HEADS
PARTS_N = 197                  # the token count at which q, k and v are also poisoned one at a time

# family -> [(tokens, head dim)]; CONTROLS: tile-aligned counts, no padded key in any tile the family stages
OP_CASES = {
    "persist": [(N, 64) for N in (193, 197, 207, 208, 209, 215, 223, 224)],
    "flow": [(N, 64) for N in (15, 63, 64, 65, 197, 577, 1025)],
    "stream": [(N, 64) for N in (15, 63, 64, 65, 197, 577, 1025)],
    "precise": [(N, 64) for N in (65, 197, 215, 224, 577)],
    "single": [(N, 64) for N in (17, 197, 224, 257, 577)],
    "auto": [(N, 64) for N in (197, 257, 289, 785)],
    "generic": [(17, 32), (65, 80), (33, 120)],
    "cls": [(197, 64), (65, 32)],
    "text_causal": [(33, 72), (77, 64)],
    "text_nomask": [(33, 72), (77, 64)],
}
CONTROLS = {"persist": (208, 224), "flow": (64,), "stream": (64,), "precise": (224,), "single": (224,)}
MAP_CASES = [(197, 64), (17, 32)]


def _op_params():
    out = []
    for family, cases in OP_CASES.items():
        for dn in ("f16", "bf16"):
            if family == "precise" and dn == "bf16":
                continue
            for N, hd in cases:
                tag = "_control" if N in CONTROLS.get(family, ()) else ""
                out.append(pytest.param(family, dn, N, hd, id=f"{family}-{dn}-N{N}_hd{hd}{tag}"))
    return out


def _run(binding, torch, family, dtype_name, x32, N, hd):
    """{entry point: output [n_img][rows per image][D]} of one launch on f32 values (rounded to the operand type on upload; `precise`: both
    entry points, the poison in both planes)."""
    if family.startswith("text"):
        outs = {family: TT._run(binding, torch, dtype_name, x32, n_img, N, H, hd, family == "text_causal")}
    else:
        outs = TE.attention_run(binding, torch, family, dtype_name, x32, n_img, N, H, hd)
    return {name: o.view(n_img, -1, H * hd) for name, o in outs.items()}


def _flat_data(family, N, hd, sign):
    """(qkv f32, the one correct output [n_img][rows][D] f32) of a sign: exact_data.flat_qkv, text_data.staircase_qkv for the text kernel."""
    seed = X.attn_seed(n_img, N, H, hd) + 17 * sign
    if family.startswith("text"):
        qkv, u = TD.staircase_qkv(n_img, N, H, hd, sign, seed)
        return qkv, TD.staircase_expected(u, N, family == "text_causal").reshape(n_img, N, H * hd)
    qkv, c = X.flat_qkv(n_img, N, H, hd, sign, seed)
    want = c.reshape(n_img, 1, H * hd) if family == "cls" else X.flat_expected(c, N).reshape(n_img, N, H * hd)
    return qkv, want


def _variants(dtype_name, N):
    """(label, poisoned images, (parts, images, value) for _apply, heads that stay clean or None for all) of every launch of a case."""
    out = []
    for images in P.IMAGE_SETS:
        for value in P.VALUES:
            out.append((f"images {images} {value}", images, ("qkv", images, P.value_of(value, dtype_name)), None))
        out.append((f"images {images} and the even heads nan", images, ("heads", images, float("nan")), P.clean_heads(H)))
    if N == PARTS_N:
        for part in "qkv":
            out.append((f"images {P.IMAGE_SETS[0]} nan in {part} only", P.IMAGE_SETS[0], (part, P.IMAGE_SETS[0], float("nan")), None))
    return out


def _apply(x32, N, hd, spec):
    parts, images, v = spec
    if parts == "heads":
        return P.poison_heads(x32, n_img, N, H, hd, images, v)
    return P.poison(x32, n_img, N, H, hd, images, v, parts)


def _cols(hd, heads):
    """Column mask [D] of the heads that are compared (None = all)."""
    keep = np.ones(H * hd, bool) if heads is None else np.zeros(H * hd, bool)
    for h in heads or ():
        keep[h * hd:(h + 1) * hd] = True
    return keep


@pytest.mark.parametrize("family,dtype_name,N,hd", _op_params())
def test_flat_clean_images_keep_the_one_correct_result(binding, torch_gpu, family, dtype_name, N, hd):
    """Flat data of the three signs (every key of an item carries the weight 1 / N; sign -1: a zero pad key in the row sum would outweigh
    all real keys by e^24): every row of a clean image equals c bit for bit, whatever its neighbours hold.  Every launch of the case runs;
    the failure lists all that differ."""
    torch = torch_gpu
    _, tdt, _ = TE._types(binding, torch, dtype_name)
    failed = []
    for sign in X.FLAT_SIGNS:
        qkv, want32 = _flat_data(family, N, hd, sign)
        want = torch.from_numpy(want32).cuda().to(tdt)
        for label, images, spec, heads in _variants(dtype_name, N):
            cols = torch.from_numpy(_cols(hd, heads)).cuda()
            for name, out in _run(binding, torch, family, dtype_name, _apply(qkv, N, hd, spec), N, hd).items():
                for b in P.clean_images(n_img, images):
                    got, ref = out[b][:, cols], want[b][:, cols]
                    if not torch.equal(got, ref):
                        bad = (got != ref).nonzero()
                        failed.append(f"{name} sign {sign} {label}: image {b}: {bad.shape[0]} of {got.numel()} elements differ, first at {tuple(bad[0].tolist())}: "
                                      f"got {got[tuple(bad[0].tolist())].item()!r}, want {ref[tuple(bad[0].tolist())].item()!r}")
    assert not failed, f"{family} {dtype_name} N {N} hd {hd}: {len(failed)} launches leak:\n  " + "\n  ".join(failed)


@pytest.mark.parametrize("family,dtype_name,N,hd", _op_params())
def test_spread_clean_images_pass_the_gates_and_keep_their_bits(binding, torch_gpu, family, dtype_name, N, hd):
    """randn * 0.8 data: the clean images of every poisoned launch lie inside the per-element bound and the mean gate of
    test_gpu_attention.py (float64 reference of the operands the kernel multiplies; f32 emulation of the definition) and have the bits of
    the launch on the finite data."""
    torch = torch_gpu
    _, tdt, _ = TE._types(binding, torch, dtype_name)
    scale = 1.0 / np.sqrt(hd)
    x32 = X.spread_qkv(n_img, N, H, hd, X.attn_seed(n_img, N, H, hd), "spread")
    x = torch.from_numpy(x32).cuda()
    q, k, v = X.heads_of(x if family == "precise" else x.to(tdt).float(), n_img, N, H, hd)
    if family.startswith("text"):
        causal = family == "text_causal"
        ref, cond = TD.masked_ref(q, k, v, scale, causal, want_bound=True)
        emu = TD.masked_emu(q, k, v, scale, dtype_name, causal)
    else:
        if family == "cls":
            q = q[:, :1]
        ref, cond = X.attention_ref(q, k, v, scale, want_bound=True)
        emu = X.attention_emu(q, k, v, scale, dtype_name, X.attention_schedule(family, dtype_name, N))
    bound = X.attention_bound(ref, cond, dtype_name)
    emu_worst, _ = X.attention_gate_ratios(emu, ref, bound, emu)
    assert emu_worst <= 0.5, f"the emulation needs {emu_worst:.3f} of the bound (k = {X.ATTN_K})"
    nq = q.shape[1]
    ref, bound, emu = (X.rows_of(t, n_img, nq, H, hd).view(n_img, nq, H * hd) for t in (ref, bound, emu))
    base = _run(binding, torch, family, dtype_name, x32, N, hd)
    failed = []
    for label, images, spec, heads in _variants(dtype_name, N):
        cols = torch.from_numpy(_cols(hd, heads)).cuda()
        for name, out in _run(binding, torch, family, dtype_name, _apply(x32, N, hd, spec), N, hd).items():
            for b in P.clean_images(n_img, images):
                got = out[b][:, cols]
                if not bool(torch.isfinite(got.float()).all()):
                    failed.append(f"{name} {label}: image {b}: {int((~torch.isfinite(got.float())).sum())} of {got.numel()} elements are not finite")
                    continue
                worst, mean = X.attention_gate_ratios(got, ref[b][:, cols], bound[b][:, cols], emu[b][:, cols])
                if worst > 1.0 or mean > X.ATTN_MEAN_FACTOR:
                    failed.append(f"{name} {label}: image {b}: an element at {worst:.3f} of its bound, mean error {mean:.3f} times the emulation's")
                if not torch.equal(got.view(torch.int16), base[name][b][:, cols].view(torch.int16)):
                    failed.append(f"{name} {label}: image {b}: the bits differ from the launch on finite data")
    assert not failed, f"{family} {dtype_name} N {N} hd {hd}: {len(failed)} launches leak:\n  " + "\n  ".join(failed)


# ------------------------------------------------------------------------------------------------ class-token map, head mean, rollout factor
def _maps(binding, torch, x32, mode, N, hd):
    """(class-token maps [n][H][N], head mean [n][N][N], rollout factor [n][N][N]) f32 of one buffer in the mode's operand layout."""
    dt, buf, lo_off = TR._operands(binding, torch, np.ascontiguousarray(x32), mode)
    cls = torch.full((n_img, H, N), float("nan"), dtype=torch.float32, device="cuda")
    mean = torch.full((n_img, N, N), float("nan"), dtype=torch.float32, device="cuda")
    fac = torch.full((n_img, N, N), float("nan"), dtype=torch.float32, device="cuda")
    binding.op_attention_map(dt, buf.data_ptr(), cls.data_ptr(), mean.data_ptr(), n_img, N, H * hd, H, lo_off=lo_off)
    binding.op_rollout_factor(dt, buf.data_ptr(), fac.data_ptr(), n_img, N, H * hd, H, lo_off=lo_off)
    torch.cuda.synchronize()
    return {"class-token map": cls, "head mean": mean, "rollout factor": fac}


@pytest.mark.parametrize("mode", ["bf16", "f16", "f16_planes"])
@pytest.mark.parametrize("N,hd", MAP_CASES)
def test_maps_and_rollout_factor_of_clean_images(binding, torch_gpu, N, hd, mode):
    """vitx_op_attention_map and vitx_op_rollout_factor are f32 softmaxes, so "exact" is one f32 ulp: on flat data every entry of a clean
    image's class-token map and head mean lies within one ulp of 1 / N and the factor within one ulp of 0.5 / N (+ 0.5 on the diagonal), the
    gates of test_attention_map_of_a_flat_softmax and test_factor_of_a_flat_softmax; on spread data maps and mean lie within 1e-5 of the
    float64 softmax (test_op_attention_map_against_float64's gate) and all three have the bits of the launch on finite data.  The maps use
    q and k only; the poison sits in v too (f16_planes: in both planes)."""
    torch = torch_gpu
    dtype_name = "bf16" if mode == "bf16" else "f16"
    eye = torch.eye(N, dtype=torch.bool, device="cuda")
    variants = [(label, images, spec) for label, images, spec, heads in _variants(dtype_name, N) if heads is None]
    failed = []
    for sign in X.FLAT_SIGNS:
        qkv, _ = X.flat_qkv(n_img, N, H, hd, sign, X.attn_seed(n_img, N, H, hd) + 17 * sign)
        for label, images, spec in variants:
            got = _maps(binding, torch, _apply(qkv, N, hd, spec), mode, N, hd)
            for b in P.clean_images(n_img, images):
                for name, m, val in (("class-token map", got["class-token map"][b], 1.0 / N), ("head mean", got["head mean"][b], 1.0 / N),
                                     ("rollout factor, diagonal", got["rollout factor"][b][eye], 0.5 + 0.5 / N), ("rollout factor, off the diagonal", got["rollout factor"][b][~eye], 0.5 / N)):
                    worst, ulp = float((m.double() - val).abs().max()), float(np.spacing(np.float32(val)))
                    if not worst <= ulp:                                          # (NaN fails)
                        failed.append(f"flat sign {sign} {label}: image {b}: {name} lies {worst / ulp:.2f} ulp from {val}")
    x32 = X.spread_qkv(n_img, N, H, hd, X.attn_seed(n_img, N, H, hd), "spread")
    base = _maps(binding, torch, x32, mode, N, hd)
    xt = torch.from_numpy(x32)
    if mode == "f16_planes":
        hi = xt.to(torch.float16); lo = ((xt - hi.float()) * 2048.0).to(torch.float16)
        vals = hi.double().numpy() + lo.double().numpy() * 2.0 ** -11
    else:
        vals = xt.to(torch.bfloat16 if mode == "bf16" else torch.float16).double().numpy()
    D = H * hd
    A = [TM._maps64(vals[b * N:(b + 1) * N, :D], vals[b * N:(b + 1) * N, D:2 * D], H) for b in range(n_img)]
    for label, images, spec in variants:
        got = _maps(binding, torch, _apply(x32, N, hd, spec), mode, N, hd)
        for b in P.clean_images(n_img, images):
            for name, want in (("class-token map", A[b][:, 0, :]), ("head mean", A[b].mean(axis=0))):
                err = float(np.abs(got[name][b].cpu().numpy().astype(np.float64) - want).max())
                if not err <= 1e-5:
                    failed.append(f"spread {label}: image {b}: {name} lies {err:.2e} from the float64 softmax")
            for name in got:
                if not torch.equal(got[name][b].view(torch.int32), base[name][b].view(torch.int32)):
                    failed.append(f"spread {label}: image {b}: the bits of the {name} differ from the launch on finite data")
    assert not failed, f"{mode} N {N} hd {hd}: {len(failed)} leaks:\n  " + "\n  ".join(failed)


# ================================================================================================ forward level: the main context
FILES = {
    "vit_tiny": lambda pkg: pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0),
    "micro": lambda pkg: pkg.synth.cached_synthetic(AD.MICRO, head_scale=4.0),
    "vit_erf": lambda pkg: AD.fixture_file(pkg, "vit_erf"),
    "dinov2_erf": lambda pkg: AD.fixture_file(pkg, "dinov2_erf"),
    "clip": lambda pkg: AD.fixture_file(pkg, "clip"),
    "siglip_map": lambda pkg: MD.fixture_file(pkg),
    "dinov3_rope": lambda pkg: RD.fixture_file(pkg),
    "swiglu": lambda pkg: SD.fixture_file(pkg, "g"),
    "registers": lambda pkg: pkg.synth.cached_synthetic(AD.MICRO, head_scale=4.0, registers=4, head_pool=1),
    "vitstr": lambda pkg: pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0),       # (the micro ViTSTR file has 17 tokens, fewer than the 25 its head reads: no context takes it)
    "zs_clip": lambda pkg: Z.model_file(pkg, "clip"),
}
MODES = {"bf16": (1, {}), "f16_fast": (0, {"f16_fast_attention": 1}), "f16": (0, {}), "mxfp8": (2, {})}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _images(model, ctx, n, seed):
    """n finite images of the context's shape, multiples of 1 / 16 (prefix_data.exact_images); one grey plane for a ViTSTR file."""
    imgs = PD.exact_images(n, ctx.img_size, seed=seed)
    return np.ascontiguousarray(imgs[..., 0]) if model.in_channels == 1 else imgs


def _outputs(ctx, imgs, maps, feats, head=None, repeat=1):
    """Everything one forward gives, {name: array [n][...]}: probabilities, logits, the class embedding and (if on) the token features, the
    class-token maps and the rollout row, the outputs of `head`.  repeat: the call is made that often (a graph context captures the second
    identical call and replays it from the third on); the last call's outputs are returned."""
    n = imgs.shape[0]
    for _ in range(repeat):
        probs, logits = ctx.forward(imgs, want_logits=True)
    out = {"probabilities": probs, "logits": logits}
    if feats:
        for layer, kinds in ctx.feat_read(n).items():
            for k, v in kinds.items():
                out[f"layer {layer} {k} features"] = v
    if maps:
        cls, roll = ctx.attn_read(n)
        out["class-token maps"], out["rollout row"] = cls, roll
    if head == "zeroshot":
        out["zero-shot probabilities"], out["zero-shot logits"] = ctx.zeroshot_read(n, want_logits=True)
    elif head == "gallery":
        out["neighbour indices"], out["neighbour scores"], out["neighbour votes"] = ctx.nn_read(n)
    elif head == "dense":
        out["label map"], out["label score"], out["patch logits"] = ctx.dense_read(n)
    elif head == "depth":
        out["depth map"], out["fine plane"], out["depth logits"], out["depth offsets"] = ctx.depth_read(n)
    return {k: v for k, v in out.items() if v is not None}


def _compare(got, want, clean, where, failed):
    for name in want:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        for p in clean:
            if g.dtype.kind == "f" and not np.isfinite(g[p]).all():
                failed.append(f"{where}: image {p}: {int((~np.isfinite(g[p])).sum())} of {g[p].size} values of the {name} are not finite")
            elif not np.array_equal(_bits(g[p]), _bits(w[p])):
                failed.append(f"{where}: image {p}: the {name} differ from the call with finite images ({int((_bits(g[p]) != _bits(w[p])).sum())} of {g[p].size} values)")


def _sandwich(binding, ctx, model, where, maps=True, feats=True, head=None, repeat=1, n=5, bad=None, tails=(False, True)):
    """[A, P, B, P, C] (or `bad` positions of n images) through one context, P = every kind of poisoned image in turn: the clean images'
    outputs are finite and have the bits of the call with finite images at the poisoned positions -- same batch size, same positions, so
    the same kernels and tiles.  tails: with the class-rows-only last layer (the class embedding alone) and with every row of it (token
    features of the last layer on); contexts that always evaluate every row run both all the same."""
    clean, bad = (P.sandwich(3) if bad is None else (tuple(p for p in range(n) if p not in bad), tuple(bad)))
    base = _images(model, ctx, n, seed=3)
    assert np.isfinite(base).all()
    failed = []
    if maps:
        ctx.attn_enable(None, rollout=True)
    for tokens in (tails if feats else (False,)):
        if feats:
            ctx.feat_enable(cls=True, tokens=tokens)
        want = _outputs(ctx, base, maps, feats, head, repeat)
        for p in clean:
            assert all(np.isfinite(v[p]).all() for v in want.values() if np.asarray(v).dtype.kind == "f"), f"{where}: the finite batch itself is not finite"
        for kind in P.IMAGE_POISONS:
            got = _outputs(ctx, P.poison_images(base, bad, kind), maps, feats, head, repeat)
            _compare(got, want, clean, f"{where}, P = {kind}{', token features on' if tokens else ''}", failed)
    assert not failed, f"{len(failed)} outputs of clean images moved:\n  " + "\n  ".join(failed)


@pytest.mark.parametrize("mode", list(MODES))
def test_forward_vit_tiny_at_197_tokens(pkg, binding, torch_gpu, mode):
    """vit_tiny_patch16_224: 197 tokens, the persistent attention kernels of every operand mode (an item stages 208 rows: 11 padded keys, the first 11 rows
    of the next image)."""
    dtype, opts = MODES[mode]
    model = binding.Model(FILES["vit_tiny"](pkg))
    ctx = binding.Context(model, 0, 5, dtype, **opts)
    assert ctx.tokens == 197
    _sandwich(binding, ctx, model, f"vit_tiny {mode}")
    ctx.close(); model.close()


@pytest.mark.parametrize("mode", ["bf16", "f16_fast", "f16"])
def test_forward_vit_tiny_at_362_tokens(pkg, binding, torch_gpu, mode):
    """The same file in a context with img_size 304: 362 tokens, the pipelined kernel (F16 parity: the two-pass `precise` build), 22 padded
    keys in the last 64-key chunk."""
    dtype, opts = MODES[mode]
    model = binding.Model(FILES["vit_tiny"](pkg))
    ctx = binding.Context(model, 0, 5, dtype, img_size=304, **opts)
    assert ctx.tokens == 362
    _sandwich(binding, ctx, model, f"vit_tiny at 304 {mode}")
    ctx.close(); model.close()


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("family", ["vit_erf", "dinov2_erf", "clip", "siglip_map", "dinov3_rope", "swiglu", "registers", "vitstr"])
def test_forward_of_every_model_family(pkg, binding, torch_gpu, family, mode):
    """One micro file of every model family the loaders know (17 tokens; 21 with registers, 16 without a class token; the ViTSTR file has
    197).  F16 parity runs the two-pass `precise` build (17 tokens: 47 padded keys), BF16 the single-pass kernel, which zeroes its
    padded rows: the control."""
    dtype, opts = MODES[mode]
    model = binding.Model(FILES[family](pkg))
    ctx = binding.Context(model, 0, 5, dtype, **opts)
    vitstr = model.seq_len > 0
    _sandwich(binding, ctx, model, f"{family} {mode}", maps=not vitstr and model.num_prefix > 0, feats=not vitstr)
    ctx.close(); model.close()


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_forward_two_streams_poison_on_each_side_of_the_cut(pkg, binding, torch_gpu, mode):
    """16 images on two sub-batch streams: the last image of the first sub-batch and the first of the second are poisoned (and image 1 and
    the one before the last): every other image keeps its bits."""
    dtype, opts = MODES[mode]
    model = binding.Model(FILES["micro"](pkg))
    n = 16
    ctx = binding.Context(model, 0, n, dtype, **opts)
    parts = ctx.split(n)
    assert len(parts) == 2 and min(parts) >= 3, parts
    cut = parts[0]
    _sandwich(binding, ctx, model, f"two streams {parts} {mode}", n=n, bad=sorted({1, cut - 1, cut, n - 2}))
    ctx.close(); model.close()


def test_forward_smallest_layernorm_fusing_batch(pkg, binding, torch_gpu):
    """The smallest batch at which proj and fc2 of a 512-wide fixture carry the LayerNorms (wide_data.batch_for): poisoned images at both
    ends, in a row block of their own neighbours and on either side of the cut; rows of a poisoned image share 256-row GEMM tiles, and
    their statistics exchange, with clean ones."""
    key = "vit_erf"
    N = WD.FIXTURES[key].tokens
    n, s1 = WD.batch_for(N)
    model = binding.Model(WD.fixture_file(pkg, key))
    ctx = binding.Context(model, 0, n, 1, streams=2, split_first=s1)
    assert ctx.ln_fusion_active() == 1 and ctx.split(n) == [s1, n - s1]
    _sandwich(binding, ctx, model, f"wide {key} bf16, batch {n} = {s1} + {n - s1}", maps=False, feats=True, n=n, bad=sorted({1, 3, s1 - 1, s1, n - 2}), tails=(False,))
    assert ctx.ln_fusion_active() == 1
    ctx.close(); model.close()


def test_forward_with_the_graph_option(pkg, binding, torch_gpu):
    """graph = 1: every batch is forwarded three times (captured at the second, replayed at the third): the replays of a poisoned batch
    leave the clean images the bits of the finite batch's replay."""
    model = binding.Model(FILES["vit_tiny"](pkg))
    ctx = binding.Context(model, 0, 5, 0, graph=1)
    _sandwich(binding, ctx, model, "vit_tiny f16 graph", maps=False, feats=False, repeat=3)
    assert ctx.graph_launches() >= 4                     # one replay per batch: the finite one and the three poisoned ones
    ctx.close(); model.close()


@pytest.mark.parametrize("head", ["zeroshot", "gallery", "dense", "depth"])
def test_forward_with_each_opt_in_head(pkg, binding, torch_gpu, head):
    """Each opt-in head on a micro file, random head weights: only the clean images' head outputs are compared (what a nearest-neighbour
    search or an arg-max makes of a NaN row is that image's business)."""
    model = binding.Model(FILES["zs_clip" if head == "zeroshot" else "micro"](pkg))
    ctx = binding.Context(model, 0, 5, 1)
    rng = np.random.default_rng(11)
    D = model.hparams.hidden_size
    if head == "zeroshot":
        ctx.zeroshot_set(Z.unit_rows(rng.standard_normal((7, Z.CLIP_E))), Z.SOFTMAX, 100.0, 0.0)
    elif head == "gallery":
        ctx.nn_set(Z.unit_rows(rng.standard_normal((40, ctx.nn_width(binding.NN_EMBED)))).astype(np.float32), 3, binding.NN_EMBED)
    elif head == "dense":
        ctx.dense_set((rng.standard_normal((5, D)) * 0.5).astype(np.float32), rng.standard_normal(5).astype(np.float32), None, score=True, logits=True)
    else:
        K = 8
        ctx.depth_set((rng.standard_normal((K, D)) * 0.5).astype(np.float32), (rng.standard_normal((K, D)) * 0.5).astype(np.float32), rng.standard_normal(K).astype(np.float32),
                      binding.depth_bins(K, 0.5, 10.0), None, 4, 0.5, 10.0, logits=True, fine=True)
    _sandwich(binding, ctx, model, f"micro bf16 with the {head} head", maps=False, feats=False, head=head)
    ctx.close(); model.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_a_clean_batch_after_a_full_batch_of_nan_has_the_bits_of_a_fresh_context(pkg, binding, torch_gpu, mode):
    """Call hygiene: max_batch all-NaN images leave NaN in every scratch row; a smaller clean batch must then give the bits of a context that
    never saw them -- nothing behind the batch (rows of earlier, larger calls) is ever read."""
    dtype, opts = MODES[mode]
    model = binding.Model(FILES["vit_tiny"](pkg))
    used, fresh = binding.Context(model, 0, 6, dtype, **opts), binding.Context(model, 0, 6, dtype, **opts)
    failed = []
    for ctx in (used, fresh):
        ctx.attn_enable(None, rollout=True); ctx.feat_enable(cls=True, tokens=True)
    nan = np.full_like(_images(model, used, 6, seed=1), np.nan)
    used.forward(nan)
    for n in (1, 3, 5):
        imgs = _images(model, used, n, seed=10 + n)
        _compare(_outputs(used, imgs, True, True), _outputs(fresh, imgs, True, True), range(n), f"vit_tiny {mode}: {n} clean images after 6 NaN images", failed)
        used.forward(nan)
    assert not failed, "\n  ".join(failed)
    used.close(); fresh.close(); model.close()
