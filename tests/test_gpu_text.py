"""The text tower on the GPU (include/vitx.h "the text tower"; data and conditions: tests/text_data.py, tests/test_cpu_text.py).

  * vitx_op_attention_text: the causal staircase and "future keys do not exist" bit for bit, spread / peaked data under exact_data's two gates;
  * vitx_op_text_embed and vitx_op_text_pool bit for bit (the pooled rows are vitx_op_layernorm's);
  * TextContext.embed on the two micro towers against the float64 restatement, batch invariance bit for bit, a bank made by the engine fed to
    vitx_zeroshot_set, and the refusals at creation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exact_data as X
import prefix_data as PD
import test_gpu_exact as TE
import text_data as TD
import zs_data as Z

pytestmark = pytest.mark.gpu

_DTYPES = ("f16", "bf16")


def _run(binding, torch, dtype_name, qkv32, n, T, H, hd, causal):
    dt, tdt, _ = TE._types(binding, torch, dtype_name)
    xq = torch.from_numpy(np.ascontiguousarray(qkv32)).cuda().to(tdt)
    out = torch.full((n * T, H * hd), float("nan"), dtype=tdt, device="cuda")
    binding.op_attention_text(dt, xq.data_ptr(), out.data_ptr(), n, T, H * hd, H, causal)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype_name", _DTYPES)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "nomask"])
@pytest.mark.parametrize("case", TD.ATTN_CASES, ids=TD.case_id)
def test_staircase_is_exact(binding, torch_gpu, case, causal, dtype_name):
    """Every numerator is exactly 1 and v[j] = (2 j + 1) u: causal row t is (t + 1) u, every unmasked row T u, the whole NaN-filled buffer,
    torch.equal.  One leaked, dropped or pad key moves a row by at least u: two output ulps."""
    torch = torch_gpu
    n, T, H, hd = case
    _, tdt, _ = TE._types(binding, torch, dtype_name)
    for sign in X.FLAT_SIGNS:
        qkv, u = TD.staircase_qkv(n, T, H, hd, sign, X.attn_seed(n, T, H, hd) + 17 * sign)
        want = torch.from_numpy(TD.staircase_expected(u, T, causal)).cuda().to(tdt)
        TE._same(torch, _run(binding, torch, dtype_name, qkv, n, T, H, hd, causal), want, f"{dtype_name} {case} causal {causal} sign {sign}")


@pytest.mark.parametrize("dtype_name", _DTYPES)
@pytest.mark.parametrize("case", TD.ATTN_CASES, ids=TD.case_id)
def test_future_keys_do_not_exist(binding, torch_gpu, case, dtype_name):
    """k and v of the rows behind a cut replaced by other random values, then by +-60000 (f16) / +-3e38 (bf16): causal rows up to the cut keep
    their bits, the rows behind it move (a kernel that ignored keys would pass the first half alone)."""
    torch = torch_gpu
    n, T, H, hd = case
    D = H * hd
    rng = np.random.default_rng(X.attn_seed(n, T, H, hd) + 5)
    base = rng.standard_normal((n, T, 3 * D)).astype(np.float32)
    first = _run(binding, torch, dtype_name, base.reshape(n * T, 3 * D), n, T, H, hd, True).reshape(n, T, D)
    big = 60000.0 if dtype_name == "f16" else 3e38
    for c in sorted({0, T // 2, max(T - 2, 0)}):
        if c >= T - 1:
            continue                                   # no row behind the cut (T = 1)
        for kind in ("random", "huge"):
            x = base.copy()
            fill = rng.standard_normal((n, T - 1 - c, 2 * D)).astype(np.float32)
            x[:, c + 1:, D:] = fill if kind == "random" else np.where(fill > 0, big, -big).astype(np.float32)
            out = _run(binding, torch, dtype_name, x.reshape(n * T, 3 * D), n, T, H, hd, True).reshape(n, T, D)
            TE._same(torch, out[:, :c + 1].contiguous().view(torch.int16), first[:, :c + 1].contiguous().view(torch.int16), f"{dtype_name} {case} cut {c} {kind}: rows up to the cut")
            assert not torch.equal(out[:, c + 1:].contiguous().view(torch.int16), first[:, c + 1:].contiguous().view(torch.int16)), f"{dtype_name} {case} cut {c} {kind}: the rows behind the cut did not move"


@pytest.mark.parametrize("dtype_name", _DTYPES)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "nomask"])
@pytest.mark.parametrize("case", [c for c in TD.ATTN_CASES if c[1] >= X.SPREAD_MIN_N], ids=TD.case_id)
def test_spread_softmax_within_the_derived_bound(binding, torch_gpu, case, causal, dtype_name):
    """exact_data's spread and peaked data against exact_data.attention_ref with the mask applied (text_data.masked_ref), under the two gates of
    tests/test_gpu_attention.py: attention_bound per element, ATTN_MEAN_FACTOR times the mean error of attention_emu in this kernel's
    (two-pass) schedule.  Neither takes a number from the kernel."""
    torch = torch_gpu
    n, T, H, hd = case
    _, tdt, _ = TE._types(binding, torch, dtype_name)
    scale = 1.0 / np.sqrt(hd)
    for kind in X.spread_kinds(T):
        x32 = X.spread_qkv(n, T, H, hd, X.attn_seed(n, T, H, hd), kind)
        x = torch.from_numpy(x32).cuda()
        q, k, v = X.heads_of(x.to(tdt).float(), n, T, H, hd)
        ref, cond = TD.masked_ref(q, k, v, scale, causal, want_bound=True)
        bound = X.attention_bound(ref, cond, dtype_name)
        emu = TD.masked_emu(q, k, v, scale, dtype_name, causal)
        emu_worst, _ = X.attention_gate_ratios(emu, ref, bound, emu)
        ref, bound, emu = (X.rows_of(t, n, T, H, hd) for t in (ref, bound, emu))
        out = _run(binding, torch, dtype_name, x32, n, T, H, hd, causal)
        assert bool(torch.isfinite(out.float()).all()), (case, kind)
        worst, mean = X.attention_gate_ratios(out, ref, bound, emu)
        print(f"TEXT_ATTN_GATE {dtype_name} {TD.case_id(case)} {'causal' if causal else 'nomask'} {kind}: emulation {emu_worst:.3f} of the bound, kernel {worst:.3f} of the bound, "
              f"mean error {mean:.3f} of the emulation's")
        assert emu_worst <= 0.5, f"{case} {kind} {dtype_name}: the emulation needs {emu_worst:.3f} of the bound"
        assert worst <= 1.0, f"{dtype_name} {case} {kind}: an element lies at {worst:.3f} of its bound"
        assert mean <= X.ATTN_MEAN_FACTOR, f"{dtype_name} {case} {kind}: mean error {mean:.3f} times the emulation's"


# ------------------------------------------------------------------------------------------------ front and pooling
@pytest.mark.parametrize("table", ["f16", "f32"])
@pytest.mark.parametrize("D", [64, 192, 768])
def test_token_embedding_is_exact(binding, torch_gpu, D, table):
    """X = f32(tok[ids]) + pos, one f32 add per element: numpy's bits, for an f16 table and an f32 table; ids include 0, V - 1 and repeats."""
    torch = torch_gpu
    V, T, n = 96, 24, 5
    rng = np.random.default_rng(D)
    tok = rng.standard_normal((V, D)).astype(np.float16 if table == "f16" else np.float32)
    pos = rng.standard_normal((T, D)).astype(np.float32)
    ids = rng.integers(0, V, (n, T)).astype(np.int32)
    ids[0, :4] = (0, V - 1, 0, V - 1); ids[1] = 7; ids[-1, -1] = V - 1
    want = tok[ids].astype(np.float32) + pos
    d_tok, d_pos, d_ids = (torch.from_numpy(a).cuda() for a in (tok, pos, ids))
    out = torch.full((n * T, D), float("nan"), device="cuda")
    binding.op_text_embed(table == "f16", d_tok.data_ptr(), d_pos.data_ptr(), d_ids.data_ptr(), out.data_ptr(), n, T, D)
    torch.cuda.synchronize()
    TE._same(torch, out, torch.from_numpy(want.reshape(n * T, D)).cuda(), f"text_embed D {D} {table}")


@pytest.mark.parametrize("dtype_name", _DTYPES)
@pytest.mark.parametrize("D", [64, 192, 768])
def test_pooled_rows_are_the_layernorm_rows(binding, torch_gpu, D, dtype_name):
    """vitx_op_text_pool at positions 0, T - 1 and mixed: the bits of vitx_op_layernorm on the same rows (the pin of tests/test_gpu_ln_pins.py)."""
    torch = torch_gpu
    dt, tdt, _ = TE._types(binding, torch, dtype_name)
    T, n, eps = 24, 9, 1e-5
    x = torch.from_numpy(X.hostile_matrix(D, rows_per_kind=24, seed=3)[0][:n * T]).cuda().contiguous()
    w, b = (torch.from_numpy(a).cuda() for a in X.ln_params(D, 1))
    full = torch.empty((n * T, D), dtype=tdt, device="cuda")
    binding.check(binding.lib().vitx_op_layernorm(dt, x.data_ptr(), w.data_ptr(), b.data_ptr(), full.data_ptr(), n * T, D, eps, None), "vitx_op_layernorm")
    for name, pooled in (("first", np.zeros(n, np.int32)), ("last", np.full(n, T - 1, np.int32)), ("mixed", (np.arange(n) * 7 % T).astype(np.int32))):
        d_p = torch.from_numpy(pooled).cuda()
        z = torch.full((n, D), float("nan"), dtype=tdt, device="cuda")
        binding.op_text_pool(dt, x.data_ptr(), d_p.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), n, T, D, eps)
        torch.cuda.synchronize()
        want = full.reshape(n, T, D)[torch.arange(n), torch.from_numpy(pooled.astype(np.int64))]
        TE._same(torch, z.view(torch.int16), want.contiguous().view(torch.int16), f"text_pool D {D} {dtype_name} {name}")


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def refs(pkg):
    """family -> (path, ids, R64, {dtype: Rop}): the float64 restatement of the 17 prompts, once for the module"""
    out = {}
    for family in ("clip", "siglip"):
        path = TD.text_file(pkg, family)
        t = PD.file_tensors(pkg, path)
        ids = TD.prompts(family)
        rop = {d: TD.forward64(t, ids, wround=Z.ROUND[d], uround=Z.ROUND[d]) for d in (0, 1)}
        out[family] = (path, ids, TD.forward64(t, ids), rop)
    return out


@pytest.mark.parametrize("dtype", [0, 1], ids=_DTYPES)
@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_embeddings_against_the_restatement(binding, torch_gpu, refs, family, dtype):
    """On L2-normalised embeddings: max|dev - R64| <= 3 max|Rop - R64| and the same for the mean; Rop = the restatement with the operand
    roundings the device makes, 3 = the project's emulation factor.  Measured ratios: DESIGN.md section 3."""
    path, ids, r64, rop = refs[family]
    model = binding.Model(path)
    ctx = binding.TextContext(model, max_prompts=TD.N_PROMPTS, dtype=dtype)
    dev = ctx.embed(ids, l2=True).astype(np.float64)
    raw = ctx.embed(ids).astype(np.float64)
    ctx.close(); model.close()
    a, b = np.abs(dev - Z.normalise64(r64)), np.abs(Z.normalise64(rop[dtype]) - Z.normalise64(r64))
    print(f"TEXT_E2E {family} {_DTYPES[dtype]}: max|dev - R64| {a.max():.3e}, max|Rop - R64| {b.max():.3e}, ratio {a.max() / b.max():.3f}; "
          f"mean {a.mean():.3e} / {b.mean():.3e}, ratio {a.mean() / b.mean():.3f}")
    assert np.isfinite(dev).all() and np.abs(np.linalg.norm(dev, axis=1) - 1).max() < 1e-6
    # VITX_TEXT_L2 is zs_embed_kernel's rule on the plain output, bit for bit: the f32 sum of squares in its order (zs_data.device_sumsq), IEEE
    # square root and division, unrounded
    raw32 = raw.astype(np.float32)
    want = raw32 / np.sqrt(Z.device_sumsq(raw32))[:, None]
    assert want.dtype == np.float32 and np.array_equal(dev.astype(np.float32).view(np.uint32), want.view(np.uint32))
    assert a.max() <= 3 * b.max() and a.mean() <= 3 * b.mean()


@pytest.mark.parametrize("dtype", [0, 1], ids=_DTYPES)
@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_a_prompt_has_the_same_bits_in_any_batch(binding, torch_gpu, refs, family, dtype):
    """One by one, as 17, and as 17 inside a max_prompts = 64 context with other prompts around them: np.array_equal embeddings."""
    path, ids, _, _ = refs[family]
    model = binding.Model(path)
    ctx = binding.TextContext(model, max_prompts=TD.N_PROMPTS, dtype=dtype)
    whole = ctx.embed(ids)
    single = np.concatenate([ctx.embed(ids[i:i + 1]) for i in range(len(ids))])
    big = binding.TextContext(model, max_prompts=64, dtype=dtype)
    assert big.shares_weights
    other = TD.prompts(family, n=40, seed=99)
    other[11:11 + len(ids)] = ids
    inside = big.embed(other)[11:11 + len(ids)]
    # a context large enough that fc1 pins the 128 x 256 ring tiles where the small contexts pin 64 x 128 (600 x T rows: 128 tiles of 128 x 256 and
    # more): the ring tilings multiply in the same K order, so the bits are the same here too (an observation across contexts,
    # the contract is per context)
    huge = binding.TextContext(model, max_prompts=600, dtype=dtype)
    far = huge.embed(other)[11:11 + len(ids)]
    ctx.close(); big.close(); huge.close(); model.close()
    assert np.array_equal(whole.view(np.uint32), single.view(np.uint32)), "one by one"
    assert np.array_equal(whole.view(np.uint32), inside.view(np.uint32)), "inside a batch of 40 of a 64-prompt context"
    assert np.array_equal(whole.view(np.uint32), far.view(np.uint32)), "inside a batch of 40 of a 600-prompt context (another ring tiling for fc1)"


@pytest.mark.parametrize("dtype", [0, 1], ids=_DTYPES)
@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_zero_shot_through_the_engine(pkg, binding, torch_gpu, refs, family, dtype):
    """binding.text_bank(TextContext, ids, groups) fed to vitx_zeroshot_set on the matching vision micro file: top-1 equals the float64
    restatement's (a bank made by zs_data.restate's rule from R64) on every image whose float64 top-2 margin exceeds twice
    zs_data.COS_BOUND * scale; such images are at least half of the 17 (tests/test_cpu_text.py checks that condition without a GPU)."""
    path, ids, r64, _ = refs[family]
    groups = TD.zs_groups()
    kind, scale, bias = TD.zs_constants(family)
    tmodel = binding.Model(path)
    tctx = binding.TextContext(tmodel, max_prompts=TD.N_PROMPTS, dtype=dtype)
    embeds, _, _, _ = binding.text_bank(tctx, ids, groups)
    tctx.close(); tmodel.close()
    emb = Z.embedding64(pkg, family)
    r = Z.restate(Z.normalise64(emb), TD.bank64(r64, groups), kind, scale, bias)
    top, mar = Z.margins(r["logits"])
    sure = mar > 2 * Z.COS_BOUND[dtype](emb.shape[1]) * scale
    assert sure.sum() * 2 >= Z.N_IMAGES
    vmodel = binding.Model(TD.zs_family_file(pkg, family))
    vctx = binding.Context(vmodel, max_batch=Z.N_IMAGES, dtype=dtype)
    vctx.zeroshot_set(embeds.astype(np.float32), kind, scale, bias)
    vctx.forward(Z.images())
    probs = vctx.zeroshot_read()
    vctx.close(); vmodel.close()
    got = probs.argmax(1)
    print(f"TEXT_ZS {family} {_DTYPES[dtype]}: {int(sure.sum())} of {Z.N_IMAGES} images with a sure margin; top-1 equal on {int((got == top)[sure].sum())} of them")
    assert (got == top)[sure].all()


def test_refusals_at_creation(pkg, binding, torch_gpu, tmp_path):
    """VITX_MXFP8, T = 129 and a head dim of 136 are refused when the context is created; an image model takes no text context and a text model no
    image context.  Nothing is launched after a refusal: a good context made afterwards works."""
    path = TD.text_file(pkg, "clip")
    model = binding.Model(path)
    with pytest.raises(binding.VitxError) as ei:
        binding.TextContext(model, 4, binding.MXFP8)
    assert ei.value.code == binding.ERR_UNSUPPORTED
    with pytest.raises(binding.VitxError) as ei:
        binding.Context(model, max_batch=1)
    assert ei.value.code == binding.ERR_ARG
    t = PD.file_tensors(pkg, path)
    for name, change in (("T129", dict(T=129)), ("hd136", dict(D=272))):
        p = str(tmp_path / f"{name}.gguf")
        TD.write_variant(pkg, t, p, **change)
        m = binding.Model(p)
        with pytest.raises(binding.VitxError) as ei:
            binding.TextContext(m, 4, binding.F16)
        assert ei.value.code == binding.ERR_UNSUPPORTED, (name, str(ei.value))
        m.close()
    ctx = binding.TextContext(model, 4, binding.F16)
    assert np.isfinite(ctx.embed(TD.prompts("clip", n=3))).all()
    ctx.close(); model.close()


@pytest.mark.parametrize("dtype", [0, 1], ids=_DTYPES)
def test_block_quantised_file_is_expanded_at_upload(pkg, binding, torch_gpu, dtype, tmp_path):
    """A q8_0 text file (vitx_quantize_file: the four block matrices and head.weight as blocks, the token table copied): the embeddings follow
    the restatement of the DEQUANTISED tensors under the same gate as the f16 file."""
    src, path = TD.text_file(pkg, "clip"), str(tmp_path / "q8.gguf")
    binding.quantize_file(src, path, 8)
    t = PD.file_tensors(pkg, path)
    ids = TD.prompts("clip")
    r64 = Z.normalise64(TD.forward64(t, ids))
    rop = Z.normalise64(TD.forward64(t, ids, wround=Z.ROUND[dtype], uround=Z.ROUND[dtype]))
    model = binding.Model(path)
    ctx = binding.TextContext(model, max_prompts=TD.N_PROMPTS, dtype=dtype)
    dev = ctx.embed(ids, l2=True).astype(np.float64)
    ctx.close(); model.close()
    a, b = np.abs(dev - r64), np.abs(rop - r64)
    print(f"TEXT_E2E q8_0 clip {_DTYPES[dtype]}: max {a.max():.3e} / {b.max():.3e}, mean {a.mean():.3e} / {b.mean():.3e}")
    assert a.max() <= 3 * b.max() and a.mean() <= 3 * b.mean()


@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_embed_refuses_bad_input_before_any_launch(binding, torch_gpu, refs, family):
    """vitx_text_embed and vitx_text_embed_device on a live context: an id < 0, an id >= V, a CLIP row without EOS, n = 0, n > max_prompts and
    unknown flags are VITX_ERR_ARG; the output buffer (host and device) keeps its fill, and the next good call gives the bits of a fresh context."""
    torch = torch_gpu
    path, ids, _, _ = refs[family]
    L = binding.lib()
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    model = binding.Model(path)
    info = model.text_info
    V, T, E = info["vocab"], info["tokens"], model.hparams.num_classes
    ctx = binding.TextContext(model, max_prompts=4, dtype=binding.BF16)
    good = np.ascontiguousarray(ids[:4])
    first = ctx.embed(good)
    cases = []
    for val, at in ((-1, (0, 0)), (V, (3, T - 1)), (V + 7, (1, 2)), (-2 ** 31, (2, 1))):
        x = good.copy(); x[at] = val
        cases.append((f"id {val}", x, 4, 0))
    if info["eos"] >= 0:
        x = good.copy(); x[2][x[2] == info["eos"]] = 1
        cases.append(("no EOS", x, 4, 0))
    cases += [("n = 0", good, 0, 0), ("n = -1", good, -1, 0), ("n > max_prompts", np.ascontiguousarray(ids[:5]), 5, 0), ("flags", good, 4, 2), ("flags", good, 4, -1)]
    host = np.full((5, E), 123.0, np.float32)
    dev = torch.full((5, E), 123.0, device="cuda")
    for name, x, n, flags in cases:
        assert L.vitx_text_embed(ctx._h, x.ctypes.data_as(i32p), n, flags, host.ctypes.data_as(fp)) == binding.ERR_ARG, name
        assert L.vitx_text_embed_device(ctx._h, x.ctypes.data_as(i32p), n, flags, dev.data_ptr(), None) == binding.ERR_ARG, name
    torch.cuda.synchronize()
    assert (host == 123.0).all() and bool((dev == 123.0).all())
    assert L.vitx_text_embed(ctx._h, None, 1, 0, host.ctypes.data_as(fp)) == binding.ERR_ARG and L.vitx_text_embed(ctx._h, good.ctypes.data_as(i32p), 1, 0, None) == binding.ERR_ARG
    again = ctx.embed(good)
    ctx.embed_device(good, dev.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(again.view(np.uint32), first.view(np.uint32)) and np.array_equal(dev[:4].cpu().numpy().view(np.uint32), first.view(np.uint32))
    ctx.close(); model.close()


def test_command_line_and_cpp_header(pkg, binding, torch_gpu, refs, tmp_path, capsys):
    """vit_cli.py --text-model: --text-embed writes TextContext.embed's rows; with -m and -i the bank is made in the same run and the image is
    classified against it (the labels and top-1 of Context.zeroshot_set with binding.text_bank).  examples/text_embed_main.cpp (vit_text_embed_batch
    of vit.h) prints the same embeddings."""
    from vitcpp_amd import cli
    path, ids, _, _ = refs["clip"]
    ids_path, out_path, lab_path = str(tmp_path / "ids.npy"), str(tmp_path / "e.npy"), str(tmp_path / "labels.txt")
    np.save(ids_path, ids)
    with open(lab_path, "w") as f:
        f.write("".join(f"thing {k}\n" for k in range(len(ids))))
    model = binding.Model(path)
    ctx = binding.TextContext(model, max_prompts=len(ids), dtype=binding.F16)
    want = ctx.embed(ids)
    bank = binding.text_bank(ctx, ids)
    ctx.close(); model.close()
    assert cli.main(["--text-model", path, "--zero-shot-ids", ids_path, "--text-embed", out_path]) == 0
    assert np.array_equal(np.load(out_path).view(np.uint32), want.view(np.uint32))
    capsys.readouterr()
    vision = TD.zs_family_file(pkg, "clip")
    image = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assets", "apple.jpg")
    assert cli.main(["-m", vision, "-i", image, "-k", "3", "--text-model", path, "--zero-shot-ids", ids_path, "--zero-shot-labels", lab_path]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith(" > ")]
    vmodel = binding.Model(vision)
    vctx = binding.Context(vmodel, max_batch=1, dtype=binding.F16)
    vctx.zeroshot_set(bank[0].astype(np.float32), *bank[1:])
    vctx.forward(binding.preprocess_ex(cli._decode(image), vmodel.preproc())[None] if vmodel.has_preproc else binding.preprocess(cli._decode(image), vmodel.img_size)[None])
    idx, val = binding.topk(vctx.zeroshot_read(1)[0], 3)
    vctx.close(); vmodel.close()
    assert lines == [f" > thing {i} : {p:.2f}" for i, p in zip(idx, val)]
    # the C++ header
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkgdir, exe, raw = os.path.join(root, "vit.cpp_amd"), str(tmp_path / "text_embed_main"), str(tmp_path / "ids.i32")
    r = subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(root, "examples", "text_embed_main.cpp"), "-I" + pkgdir, "-L" + pkgdir, "-lvitx", "-L/opt/rocm/lib",
                        "-Wl,-rpath," + pkgdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    ids.astype("<i4").tofile(raw)
    r = subprocess.run([exe, path, raw], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = np.array([[float(v) for v in l.split()[1:]] for l in r.stdout.splitlines() if l.startswith("embedding")], np.float32)
    assert np.array_equal(rows.view(np.uint32), want.view(np.uint32))                # %.9g round-trips an f32
    r = subprocess.run([exe, vision, raw], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "image model" in r.stderr
