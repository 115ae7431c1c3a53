"""Contexts at another image size than the file's (vitx_ctx_options::img_size / pos_interp, vitx_op_pos_embed_resample; include/vitx.h).

  1. the device resampler gives the host function's bits on every case of tests/resolution_data.py (which test_cpu_pos_resample.py
     checks against torch), inside NaN canaries;
  2. THE MAIN CHECK: a context at img_size = S' gives the bits -- probabilities and logits -- of an ordinary context on the file
     vitx_model_resize_file wrote for S': every parity result of the ordinary path carries over;
  3. the same for the opt-in outputs (class-token maps, rollout, features), with the shapes of the new token count;
  4. against the oracle on the resized file, F16, with the gates of test_gpu_e2e.test_forward_matches_oracle_f16;
  5. img_size equal to the file's is the context without options; two sizes of one loaded model share the weights;
  6. an image's bits do not depend on its batch;  7. errors;  8. the CLI and the C++ example."""
import os
import subprocess
import sys

import numpy as np
import pytest

import resolution_data as RD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_PROB = 1e-3        # test_gpu_e2e.TOL_PROB
MICRO, TINY, BASE = "vit_micro_patch16_64", "vit_tiny_patch16_224", "vit_base_patch16_224"

_files = {}


def _resized(pkg, binding, tmp_path_factory, name, S, interp):
    """The file vitx_model_resize_file writes for (model, S, interp), once per session."""
    key = (name, S, interp)
    if key not in _files:
        dst = str(tmp_path_factory.mktemp("resized") / f"{name}-{S}-{interp}.gguf")
        binding.resize_file(pkg.synth.cached_synthetic(name, head_scale=4.0), dst, S, interp)
        _files[key] = dst
    return _files[key]


def _images(pkg, n, S, seed=4321):          # the default seed of synth.synthetic_images_u8: the images of test_forward_matches_oracle_f16
    return pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, S, seed=seed))


def _forward(binding, path, imgs, dt, repeats=1, **options):
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=len(imgs), dtype=dt, **options)
    for _ in range(repeats):
        probs, logits = ctx.forward(imgs, want_logits=True)
    info = dict(img_size=ctx.img_size, tokens=ctx.tokens, graph_launches=ctx.graph_launches())
    ctx.close(); model.close()
    return probs, logits, info


def _same(a, b):
    return RD.bits_equal(a, b)


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("D", RD.WIDTHS)
@pytest.mark.parametrize("case", RD.CASES + [RD.IDENTITY], ids=RD.case_id)
@pytest.mark.parametrize("interp", [RD.BICUBIC, RD.BICUBIC_AA], ids=["bicubic", "bicubic_aa"])
def test_device_resampler_gives_the_host_bits(binding, torch_gpu, interp, case, D):
    torch = torch_gpu
    grid_in, grid_out = case
    pos = RD.table(grid_in, D)
    want = binding.pos_embed_resample(pos, grid_out, interp, grid_in)
    GUARD = 1024
    d_pos = torch.from_numpy(pos).cuda()
    buf = torch.full((2 * GUARD + want.size,), float("nan"), dtype=torch.float32, device="cuda")
    binding.op_pos_embed_resample(d_pos.data_ptr(), grid_in, D, grid_out, interp, buf.data_ptr() + 4 * GUARD)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.isnan(host[:GUARD]).all() and np.isnan(host[-GUARD:]).all()
    got = host[GUARD:-GUARD].reshape(want.shape)
    assert _same(got, want), f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {want.size} floats differ from the host function"
    if case == RD.IDENTITY:
        assert _same(got, pos)


def test_device_resampler_argument_errors(binding, torch_gpu):
    torch = torch_gpu
    L = binding.lib()
    d = torch.zeros(64 * 8, dtype=torch.float32, device="cuda")
    p = d.data_ptr()
    assert L.vitx_op_pos_embed_resample(None, 4, 4, 8, 6, 6, 0, p, None) == 3
    assert L.vitx_op_pos_embed_resample(p, 4, 4, 8, 6, 6, 0, None, None) == 3
    assert L.vitx_op_pos_embed_resample(p, 4, 0, 8, 6, 6, 0, p, None) == 3
    assert L.vitx_op_pos_embed_resample(p, 4, 4, 8, 6, 6, 2, p, None) == 3


# ------------------------------------------------------------------------------------------------ 2. context == ordinary context on the resized file
FORWARD_CASES = (
    [(MICRO, S, 5, dt, ip, {}) for S in (32, 96, 128) for dt in ("F16", "BF16") for ip in (RD.BICUBIC, RD.BICUBIC_AA)] +
    # token counts 101, 257, 401, 577: the single-pass, pipelined and streaming attention families
    [(TINY, S, 6, dt, RD.BICUBIC_AA if S == 160 else RD.BICUBIC, {}) for S in (160, 256, 320, 384) for dt in ("F16", "BF16")] +
    # two streams, LayerNorm-fusing GEMMs
    [(BASE, 384, 32, dt, RD.BICUBIC, {}) for dt in ("F16", "BF16")] +
    [(TINY, 384, 6, "MXFP8", RD.BICUBIC, {}),
     (TINY, 256, 4, "BF16", RD.BICUBIC, {"graph": 1}),
     (TINY, 320, 6, "F16", RD.BICUBIC_AA, {"last_layer_all_rows": 1}),
     (TINY, 160, 6, "BF16", RD.BICUBIC, {"last_layer_all_rows": 1})]
)


@pytest.mark.parametrize("name,S,n,dt,interp,options", FORWARD_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[3]}-i{c[4]}" + "".join(f"-{k}" for k in c[5]) for c in FORWARD_CASES])
def test_context_at_img_size_gives_the_bits_of_the_resized_file(pkg, binding, torch_gpu, tmp_path_factory, name, S, n, dt, interp, options):
    dtype = getattr(binding, dt)
    src = pkg.synth.cached_synthetic(name, head_scale=4.0)
    imgs = _images(pkg, n, S)
    repeats = 4 if options.get("graph") else 1              # the graph is captured the second time a call repeats
    p0, l0, i0 = _forward(binding, _resized(pkg, binding, tmp_path_factory, name, S, interp), imgs, dtype, repeats, **options)
    p1, l1, i1 = _forward(binding, src, imgs, dtype, repeats, img_size=S, pos_interp=interp, **options)
    P = pkg.synth.CONFIGS[name][4]
    assert (i1["img_size"], i1["tokens"]) == (S, (S // P) ** 2 + 1) == (i0["img_size"], i0["tokens"])
    assert np.isfinite(p1).all() and np.abs(p1.sum(1) - 1).max() < 1e-4
    assert _same(p1, p0) and _same(l1, l0)
    if options.get("graph"):
        assert i1["graph_launches"] >= 1 and i0["graph_launches"] >= 1
    # and the other convention is another table: the option is not ignored
    if name == MICRO and dt == "F16":
        p2, l2, _ = _forward(binding, src, imgs, dtype, img_size=S, pos_interp=1 - interp)
        assert not _same(l2, l1)


# ------------------------------------------------------------------------------------------------ 3. opt-in outputs
@pytest.mark.parametrize("name,S,n,dt", [(MICRO, 96, 5, "F16"), (TINY, 256, 3, "BF16")])
def test_maps_rollout_and_features_follow_the_context_geometry(pkg, binding, torch_gpu, tmp_path_factory, name, S, n, dt):
    dtype = getattr(binding, dt)
    hp = pkg.synth.hparams_for(name)
    g = S // hp.patch_size
    N, D, H, L = g * g + 1, hp.hidden_size, hp.num_attention_heads, hp.num_hidden_layers
    imgs = _images(pkg, n, S, seed=3)
    res = []
    for path, opt in ((_resized(pkg, binding, tmp_path_factory, name, S, RD.BICUBIC), {}), (pkg.synth.cached_synthetic(name, head_scale=4.0), dict(img_size=S))):
        model = binding.Model(path)
        ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, **opt)
        ctx.attn_enable([0, L - 1], rollout=True)
        probs = ctx.forward(imgs)
        cls, roll = ctx.attn_read(n)
        grid = ctx.attn_grid(roll)
        ctx.attn_disable()
        ctx.feat_enable(cls=True, mean=True, tokens=True, layers=[0, L - 1])
        probs_f = ctx.forward(imgs)
        feats = ctx.feat_read(n)
        ctx.feat_disable()
        ctx.trace_enable([0])
        ctx.forward(imgs)
        trace = ctx.trace_read()
        res.append((probs, cls, roll, grid, probs_f, feats, trace))
        ctx.close(); model.close()
    (p0, c0, r0, g0, pf0, f0, t0), (p1, c1, r1, g1, pf1, f1, t1) = res
    assert c1.shape == (n, 2, H, N) and r1.shape == (n, N) and g1.shape == (n, g, g) and t1.shape == (L + 1, 1, N, D)
    assert np.abs(c1.sum(-1) - 1).max() < 1e-4 and np.abs(r1.sum(-1) - 1).max() < 1e-4
    assert _same(p1, p0) and _same(c1, c0) and _same(r1, r0) and _same(g1, g0) and _same(pf1, pf0) and _same(t1, t0)
    for l in (0, L - 1):
        assert f1[l]["cls"].shape == (n, D) and f1[l]["mean"].shape == (n, D) and f1[l]["tokens"].shape == (n, N - 1, D)
        for k in ("cls", "mean", "tokens"):
            assert _same(f1[l][k], f0[l][k]), (l, k)


# ------------------------------------------------------------------------------------------------ 4. the oracle
@pytest.mark.parametrize("name,S,n,all_decided", [(MICRO, 32, 5, True), (MICRO, 96, 5, False), (MICRO, 128, 5, True), (TINY, 160, 6, None), (TINY, 384, 6, None)])
def test_resized_context_matches_oracle_f16(pkg, binding, oracle, torch_gpu, tmp_path_factory, name, S, n, all_decided):
    """Gates of test_forward_matches_oracle_f16.  Top-1 equality only on the rows the oracle decides (top-1 minus top-2 > 2 TOL_PROB); the
    micro model decides all 5 rows at 32 and 128; the tiny model's 1000-class head has margins of 6e-5 .. 4e-4 at every resampled size, so no
    top-1 claim is made there."""
    imgs = _images(pkg, n, S)
    probs, logits, _ = _forward(binding, pkg.synth.cached_synthetic(name, head_scale=4.0), imgs, binding.F16, img_size=S, pos_interp=RD.BICUBIC)
    ref_logits, ref_probs = oracle.OracleModel(_resized(pkg, binding, tmp_path_factory, name, S, RD.BICUBIC)).forward(imgs, oracle.REF)
    dp, dl = float(np.abs(probs - ref_probs).max()), float(np.abs(logits - ref_logits).max())
    srt = np.sort(ref_probs, -1)
    decided = (srt[:, -1] - srt[:, -2]) > 2 * TOL_PROB
    print(f"{name} at {S}: max|dprob| = {dp:.2e} (gate {TOL_PROB:.0e}), max|dlogit| = {dl:.2e} (gate 2.5e-2), rows decided {int(decided.sum())}/{n}, "
          f"smallest margin {float((srt[:, -1] - srt[:, -2]).min()):.2e}")
    assert np.isfinite(probs).all() and np.abs(probs.sum(1) - 1).max() < 1e-4
    assert dp <= TOL_PROB
    assert dl <= 2.5e-2
    if all_decided is not None:
        assert ((probs.argmax(1) == ref_probs.argmax(1)) | ~decided).all()
    if all_decided:
        assert decided.all()


# ------------------------------------------------------------------------------------------------ 5. the default path, shared weights
@pytest.mark.parametrize("dt", ["F16", "BF16"])
def test_img_size_of_the_file_is_the_context_without_options(pkg, binding, torch_gpu, dt):
    path = pkg.synth.cached_synthetic(TINY, head_scale=4.0)
    imgs = _images(pkg, 6, 224, seed=2)
    p0, l0, _ = _forward(binding, path, imgs, getattr(binding, dt))
    for interp in (RD.BICUBIC, RD.BICUBIC_AA):
        p1, l1, i1 = _forward(binding, path, imgs, getattr(binding, dt), img_size=224, pos_interp=interp)
        assert (i1["img_size"], i1["tokens"]) == (224, 197) and _same(p1, p0) and _same(l1, l0)


def test_two_sizes_of_one_loaded_model_share_the_weights(pkg, binding, torch_gpu):
    path = pkg.synth.cached_synthetic(TINY, head_scale=4.0)
    x224, x384 = _images(pkg, 4, 224, seed=5), _images(pkg, 4, 384, seed=6)
    alone = {}
    for S, x in ((224, x224), (384, x384)):
        alone[S] = _forward(binding, path, x, binding.BF16, img_size=S)[:2]
    model = binding.Model(path)
    a = binding.Context(model, device=0, max_batch=4, dtype=binding.BF16)
    b = binding.Context(model, device=0, max_batch=4, dtype=binding.BF16, img_size=384)
    assert not a.shares_weights() and b.shares_weights()
    assert a.weight_bytes() == b.weight_bytes() > 0
    assert (a.img_size, a.tokens, b.img_size, b.tokens) == (224, 197, 384, 577)
    for _ in range(2):                                     # interleaved
        pa, la = a.forward(x224, want_logits=True)
        pb, lb = b.forward(x384, want_logits=True)
        assert _same(pa, alone[224][0]) and _same(la, alone[224][1])
        assert _same(pb, alone[384][0]) and _same(lb, alone[384][1])
    # the resized context first, the file-sized one second: the shared set holds the FILE's table either way
    a.close(); b.close(); model.close()
    model = binding.Model(path)
    b = binding.Context(model, device=0, max_batch=4, dtype=binding.BF16, img_size=384)
    a = binding.Context(model, device=0, max_batch=4, dtype=binding.BF16)
    assert not b.shares_weights() and a.shares_weights()
    assert _same(a.forward(x224), alone[224][0]) and _same(b.forward(x384), alone[384][0])
    a.close(); b.close(); model.close()


# ------------------------------------------------------------------------------------------------ 6. batch invariance
@pytest.mark.parametrize("dt", ["F16", "BF16"])
def test_bits_at_a_resampled_size_do_not_depend_on_the_batch(pkg, binding, torch_gpu, dt):
    path = pkg.synth.cached_synthetic(TINY, head_scale=4.0)
    S, n = 256, 24
    imgs = _images(pkg, n, S, seed=9)
    model = binding.Model(path)
    big = binding.Context(model, device=0, max_batch=n, dtype=getattr(binding, dt), img_size=S)
    assert len(big.split(n)) == 2
    pb, lb = big.forward(imgs, want_logits=True)
    rows = big.boundary_rows(n)
    big.close()
    one = binding.Context(model, device=0, max_batch=1, dtype=getattr(binding, dt), img_size=S)
    for k in rows:
        p1, l1 = one.forward(imgs[k:k + 1], want_logits=True)
        assert _same(p1[0], pb[k]) and _same(l1[0], lb[k]), k
    one.close(); model.close()


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors_through_the_binding(pkg, binding, torch_gpu):
    model = binding.Model(pkg.synth.cached_synthetic(MICRO, head_scale=4.0))
    for opt in (dict(img_size=40), dict(img_size=-64), dict(img_size=96, pos_interp=2), dict(img_size=96, pos_interp=-1)):
        with pytest.raises(binding.VitxError, match="invalid argument"):
            binding.Context(model, device=0, max_batch=1, **opt)
    ctx = binding.Context(model, device=0, max_batch=2, img_size=96)
    with pytest.raises(ValueError, match="96, 96, 3"):
        ctx.forward(_images(pkg, 2, 64))                    # the file's size on a resized context: refused before the ABI
    assert ctx.forward(_images(pkg, 2, 96)).shape == (2, 10)
    ctx.close(); model.close()
    vitstr = binding.Model(pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0))
    with pytest.raises(binding.VitxError, match="unsupported"):
        binding.Context(vitstr, device=0, max_batch=1, img_size=384)
    ok = binding.Context(vitstr, device=0, max_batch=1, img_size=224)        # its own size is its ordinary context
    assert ok.img_size == 224
    ok.close(); vitstr.close()


# ------------------------------------------------------------------------------------------------ 8. interfaces
def test_cli_img_size_prints_the_top_k_of_the_resized_file(pkg, binding, torch_gpu, tmp_path, tmp_path_factory):
    src = pkg.synth.cached_synthetic(MICRO, head_scale=4.0)
    u8 = pkg.synth.synthetic_images_u8(1, 80, seed=4)[0]
    (tmp_path / "img.ppm").write_bytes(b"P6\n80 80\n255\n" + np.ascontiguousarray(u8, np.uint8).tobytes())
    cli = [sys.executable, os.path.join(ROOT, "vit_cli.py"), "-i", str(tmp_path / "img.ppm"), "-k", "3"]
    pgm = tmp_path / "map.pgm"
    emb = tmp_path / "tok.npy"
    r1 = subprocess.run(cli + ["-m", src, "--img-size", "96", "--attn-map", str(pgm), "--embed", str(emb), "--embed-kind", "tokens"], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    r0 = subprocess.run(cli + ["-m", _resized(pkg, binding, tmp_path_factory, MICRO, 96, RD.BICUBIC)], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stderr
    assert r1.stdout.count(" > ") == 3 and r1.stdout == r0.stdout
    assert "(96 x 96)" in r1.stderr
    assert pgm.read_bytes().startswith(b"P5\n96 96\n255\n") and len(pgm.read_bytes()) == len(b"P5\n96 96\n255\n") + 96 * 96
    assert np.load(emb).shape == (1, 36, 128)
    # the binding gives the same top-k
    model = binding.Model(src)
    ctx = binding.Context(model, device=0, max_batch=1, dtype=binding.F16, img_size=96)
    idx, val = binding.topk(ctx.forward(binding.preprocess(u8, 96)[None])[0], 3)
    assert r1.stdout == "".join(f" > {model.label(i)} : {p:.2f}\n" for i, p in zip(idx, val))
    ctx.close(); model.close()
    bad = subprocess.run(cli + ["-m", src, "--img-size", "50"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "patch size" in bad.stderr


def test_cpp_example_embed_main_at_another_img_size(pkg, binding, torch_gpu, tmp_path):
    """examples/embed_main.cpp --img-size through vit.cpp_amd/vit.h (vit_state::img_size): the embedding it writes is the binding's."""
    pkgdir = os.path.join(ROOT, "vit.cpp_amd")
    exe = str(tmp_path / "embed_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "examples", "embed_main.cpp"), "-I" + pkgdir, "-L" + pkgdir, "-lvitx", "-L/opt/rocm/lib",
                        "-Wl,-rpath," + pkgdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assets = os.path.join(ROOT, "tests", "golden", "assets")
    files = sorted(f for f in os.listdir(assets) if f.lower().endswith((".jpg", ".jpeg", ".png")))
    a, b = os.path.join(assets, files[0]), os.path.join(assets, files[1])
    path = pkg.synth.cached_synthetic(TINY, head_scale=4.0)
    model = binding.Model(path)
    for S in (160, 0):
        out = tmp_path / f"emb{S}.bin"
        r = subprocess.run([exe, path, a, b, "--out", str(out)] + (["--img-size", str(S)] if S else []), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "embedding: 192 floats per image" in r.stdout
        side = S or 224
        ctx = binding.Context(model, device=0, max_batch=2, dtype=binding.F16, img_size=S)
        ctx.feat_enable(cls=True, l2=True)
        ctx.forward(np.stack([binding.preprocess(binding.load_image(f), side) for f in (a, b)]))
        want = ctx.feat_read(2)[11]["cls"][0]
        ctx.close()
        assert _same(np.fromfile(out, np.float32), want), S
    r = subprocess.run([exe, path, a, b, "--img-size", "100"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "not a positive multiple" in r.stderr
    model.close()
