"""The attention-pooling (MAP) head of a model without a class token on the MI355X (include/vitx.h "no class token and the attention-pooling
head"): the pooling kernel against float64, its leaks and drops, batch invariance, the patch embedding without a prefix row, and the forward end
to end against tests/ref64.py's restatement (pinned to transformers' SiglipVisionModel in tests/test_cpu_map_head.py)."""
import functools

import numpy as np
import pytest

import arch_data as AD
import map_data as MD
import prefix_data as PD
import ref64 as R64
from ref64 import PROB_TOL, stage_errors, stage_ok

pytestmark = pytest.mark.gpu

D, L, H, P, S, N = 128, 2, 2, 14, 56, 16            # arch_data.MICRO without its class token
ROUND = {0: PD.f16_round, 1: PD.bf16_round}
COS_GPU, COS_CPU = MD.COS_GPU, MD.COS_CPU      # the gates on e and their provenance: tests/map_data.py


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ the pooling kernel on its own
def _pool_inputs(n_img, n_tok, d, h, seed, gap=3):
    """x [n_img][n_tok + gap][d] with 1e30 / NaN sentinel rows between the images, LayerNorm weights, u with scores of unit spread."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n_img, n_tok + gap, d)) * (0.5 + rng.random((n_img, n_tok + gap, 1))) + 0.3 * rng.standard_normal((1, 1, d))).astype(np.float32)
    x[:, n_tok:] = np.float32(1e30)
    x[:, n_tok + 1:] = np.float32(np.nan)
    w = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    u = (rng.standard_normal((h, d)) * 2.0 / np.sqrt(d)).astype(np.float32)
    return x, w, b, u


def _features(binding, torch, dx, dw, db, n_img, n_tok, d, gap):
    """F [n_img][n_tok][d] f32 from the existing feature kernel (tokens, first = 0): the LayerNorm's own error stays outside the pooling bound."""
    F = torch.zeros((n_img, n_tok, d), dtype=torch.float32, device="cuda")
    binding.op_features_ex(dx.data_ptr(), d, (n_tok + gap) * d, dw.data_ptr(), db.data_ptr(), 0, 0, F.data_ptr(), n_tok * d, n_img, n_tok, 0, d, 1e-6)
    return F.cpu().numpy()


def _run_pool(binding, torch, x, w, b, u, n_img, n_tok, d, h, gap=3, want_p=True, extra=1):
    dx, dw, db, du = (_dev(torch, a) for a in (x, w, b, u))
    SENT = -12345.5
    M = torch.full((n_img + extra, h, d), SENT, dtype=torch.float32, device="cuda")
    Pr = torch.full((n_img + extra, h, n_tok), SENT, dtype=torch.float32, device="cuda")
    binding.op_attention_pool(dx.data_ptr(), d, (n_tok + gap) * d, dw.data_ptr(), db.data_ptr(), 1e-6, du.data_ptr(), M.data_ptr(), Pr.data_ptr() if want_p else 0, n_img, n_tok, d, h)
    torch.cuda.synchronize()
    M, Pr = M.cpu().numpy(), Pr.cpu().numpy()
    assert (M[n_img:] == SENT).all() and (Pr[n_img:] == SENT).all(), "rows past n_img were written"
    assert want_p or (Pr == SENT).all()
    F = _features(binding, torch, dx, dw, db, n_img, n_tok, d, gap)
    return M[:n_img], Pr[:n_img], F


def _check_pool(M, Pr, F, u, where):
    """The issue's bound: per element of M_h, 4e-6 sum_t p_t |F[t][k]| + 2 max_t delta_t sum_t p_t |F[t][k] - M[k]| + 1e-6 with
    delta_t = 2e-6 sum_k |u_k F[t][k]| + 1e-6 (the GEMM accumulation convention of tests/test_gpu_arch.py:163; the second term is the first-order
    sensitivity of a softmax-weighted mean to score error); |dp| <= 2 delta p + 1e-7."""
    F64, u64 = F.astype(np.float64), u.astype(np.float64)
    want, p = MD.pool64(F64, u64)
    delta = (2e-6 * np.einsum("hk,ntk->nht", np.abs(u64), np.abs(F64)) + 1e-6).max(-1)                    # [n][H]
    spread = np.einsum("nht,nhtk->nhk", p, np.abs(F64[:, None] - want[:, :, None]))
    tol = 4e-6 * np.einsum("nht,ntk->nhk", p, np.abs(F64)) + 2 * delta[..., None] * spread + 1e-6
    assert np.isfinite(M).all() and np.isfinite(Pr).all(), where
    r_m = float((np.abs(M - want) / tol).max())
    r_p = float((np.abs(Pr - p) / (2 * delta[..., None] * p + 1e-7)).max()) if Pr is not None else 0.0
    print(f"{where}: worst |dM| / tol {r_m:.3f}, worst |dp| / tol {r_p:.3f}  (largest p {p.max():.3f})")
    assert r_m <= 1.0 and r_p <= 1.0, (where, r_m, r_p)
    return want, p, tol


# N in {1, 16, 63, 64, 65, 196, 577, 1024}, D in {128, 192, 768, 1152}, H in {1, 2, 3, 12, 16}, n_img in {1, 3}, each once; then the kernel's own
# edges: 4 waves x 2 rows per step (N = 3, 4, 5 and 7, 8, 9; one row per step above 1024 columns is D 1152's path), head groups (one workgroup
# each) of 4 at D 768 (H = 12, 13: 3 and 4 groups), of 2 at D 1152 (H = 9, 16), of 12 at D 128 and 192 (H = 1, 2, 3 and 32 = 12 + 12 + 8)
POOL_CASES = [(1, 1, 128, 2), (3, 16, 128, 2), (1, 63, 192, 3), (1, 64, 128, 1), (1, 65, 768, 12), (3, 196, 768, 13), (1, 577, 1152, 16), (1, 1024, 128, 32),
              (1, 3, 128, 2), (1, 4, 128, 2), (1, 5, 1152, 9), (1, 7, 192, 3), (1, 8, 128, 2), (1, 9, 128, 2)]


@pytest.mark.parametrize("n_img,n_tok,d,h", POOL_CASES)
def test_op_attention_pool_against_float64(binding, torch_gpu, n_img, n_tok, d, h):
    x, w, b, u = _pool_inputs(n_img, n_tok, d, h, seed=n_tok * 7 + d + h)
    M, Pr, F = _run_pool(binding, torch_gpu, x, w, b, u, n_img, n_tok, d, h)
    _check_pool(M, Pr, F, u, f"n {n_img} N {n_tok} D {d} H {h}")
    M2, _, _ = _run_pool(binding, torch_gpu, x, w, b, u, n_img, n_tok, d, h, want_p=False)       # the same bits without the probabilities
    assert np.array_equal(_bits(M), _bits(M2))


@pytest.mark.parametrize("t_hot", [0, 19, 8], ids=["first", "last", "step-edge"])
def test_op_attention_pool_leaks_and_drops(binding, torch_gpu, t_hot):
    """Row t_hot alone carries head H-1's score, so M_{H-1} must be F[t_hot]; heads 0 and H-2 have opposite u, so a kernel that used the wrong
    head's vector fails; the rows between the images hold 1e30 and NaN and must reach no output (tests/test_gpu_attention.py's convention)."""
    torch = torch_gpu
    n_img, n_tok, d, h, gap = 3, 20, 128, 4, 3
    x, w, b, u = _pool_inputs(n_img, n_tok, d, h, seed=50 + t_hot)
    dx, dw, db = (_dev(torch, a) for a in (x, w, b))
    F = _features(binding, torch, dx, dw, db, n_img, n_tok, d, gap)
    u[h - 2] = -u[0]
    f = F[1, t_hot].astype(np.float64)
    u[h - 1] = (40.0 * f / (f @ f)).astype(np.float32)                # image 1: s[t_hot] = 40, every other row a few units
    M, Pr, F2 = _run_pool(binding, torch, x, w, b, u, n_img, n_tok, d, h, gap=gap)
    assert np.array_equal(_bits(F), _bits(F2))
    want, p, tol = _check_pool(M, Pr, F, u, f"hot row {t_hot}")
    assert p[1, h - 1, t_hot] > 1 - 1e-9
    assert (np.abs(M[1, h - 1] - F[1, t_hot]) <= tol[1, h - 1]).all(), "M of the one-hot head is not the hot row"
    assert (np.abs(want[:, 0] - want[:, h - 2]) > 10 * (tol[:, 0] + tol[:, h - 2])).any(axis=-1).all(), "the opposite heads must be told apart"


def test_op_attention_pool_opposite_first_and_last_head(binding, torch_gpu):
    """Heads 0 and H-1 have opposite u (H = 13 at D 768: they sit in different head groups): a kernel that used the wrong head's vector gives the
    other head's M, which lies far outside the bound -- checked on the device output itself."""
    n_img, n_tok, d, h = 2, 20, 768, 13
    x, w, b, u = _pool_inputs(n_img, n_tok, d, h, seed=77)
    u[h - 1] = -u[0]
    M, Pr, F = _run_pool(binding, torch_gpu, x, w, b, u, n_img, n_tok, d, h)
    want, p, tol = _check_pool(M, Pr, F, u, "opposite heads 0 and H-1")
    swapped = np.abs(M[:, 0] - want[:, h - 1]) / tol[:, 0]
    assert (swapped.max(-1) > 10).all(), "head 0's M must not pass as head H-1's"


def test_op_attention_pool_batch_invariance(binding, torch_gpu):
    """M of image i in a batch of 1, 3 and 8 is bit-identical, whatever its position."""
    torch = torch_gpu
    n_tok, d, h, gap = 37, 192, 3, 3
    x, w, b, u = _pool_inputs(8, n_tok, d, h, seed=9)
    M8, P8, _ = _run_pool(binding, torch, x, w, b, u, 8, n_tok, d, h)
    for first, n in ((0, 1), (5, 1), (7, 1), (0, 3), (4, 3)):
        Mi, Pi, _ = _run_pool(binding, torch, x[first:first + n], w, b, u, n, n_tok, d, h)
        assert np.array_equal(_bits(Mi), _bits(M8[first:first + n])) and np.array_equal(_bits(Pi), _bits(P8[first:first + n])), (first, n)


# ------------------------------------------------------------------------------------------------ patch embedding without a prefix row
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("patch,size,d,n_img", [(14, 56, 128, 9), (16, 48, 192, 15)])      # 144 and 135 patch rows: a 128-row tile ends inside an image
def test_op_patch_embed_without_a_prefix_row(binding, torch_gpu, dtype, patch, size, d, n_img):
    torch = torch_gpu
    g = size // patch
    tpi = g * g
    rng = np.random.default_rng(size + dtype)
    rnd = ROUND[dtype]
    w = rnd((rng.standard_normal((d, 3 * patch * patch)) * 0.05).astype(np.float32))
    bias = (rng.standard_normal(d) * 0.1).astype(np.float32)
    pos = (rng.standard_normal((tpi, d)) * 0.5).astype(np.float32)
    imgs = PD.exact_images(n_img, size, seed=size)
    SENT = np.float32(-12345.5)
    X = torch.full((n_img * tpi + 300, d), float(SENT), dtype=torch.float32, device="cuda")
    dv = [_dev(torch, a) for a in (imgs, w, bias, pos)]
    binding.op_patch_embed(dtype, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), 0, 0, 0, X.data_ptr(), n_img, size, patch, 3, d)
    x = X.cpu().numpy()
    assert (x[n_img * tpi:] == SENT).all(), "rows behind the last token row were written"
    x = x[:n_img * tpi].reshape(n_img, tpi, d)
    a64 = imgs.astype(np.float64).reshape(n_img, g, patch, g, patch, 3).transpose(0, 1, 3, 5, 2, 4).reshape(n_img, tpi, -1)
    want = a64 @ w.astype(np.float64).T + bias + pos                   # row b * N is patch 0 + pos[0], not a class row
    tol = (np.abs(a64) @ np.abs(w.astype(np.float64)).T) * 2e-6 + 1e-6 + np.abs(want) * 2e-7 + 1e-7          # tests/test_gpu_registers.py:101
    err = np.abs(x - want)
    print(f"patch rows, patch {patch} size {size} D {d} dtype {dtype}: worst err / tol {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), float((err / tol).max())


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _images():
    return PD.exact_images(17, S, seed=1)


_REF = {}


def _ref(pkg, dtype, path=None, **mutant):
    """The restatement of all 17 images, once per (file, operand type, mutant); dtype None: no operand rounding."""
    key = (path, dtype, tuple(sorted(mutant.items())))
    if key not in _REF:
        t = PD.file_tensors(pkg, path or MD.fixture_file(pkg))
        rnd = {} if dtype is None else dict(wround=ROUND[dtype], uround=ROUND[dtype])
        _REF[key] = (t, R64.forward64(t, _images(), H, **rnd, **mutant))
    return _REF[key]


@pytest.mark.parametrize("dtype", [0, 1])
def test_forward_against_the_restatement(pkg, binding, torch_gpu, dtype):
    """Batches 1, 3 and 17 (two sub-batch streams): the trace stage by stage, the pooled embedding through VITX_FEAT_CLS (1 - cos, worst image), the
    head operand RNE(e), the probabilities; the flat-softmax and wrong-activation restatements lie outside the same gates; MEAN and TOKENS cover
    all N rows."""
    t, ref = _ref(pkg, dtype)
    _, exact = _ref(pkg, None)
    imgs = _images()
    model = binding.Model(MD.fixture_file(pkg))
    assert (model.head_pool, model.num_prefix) == (binding.POOL_MAP, 0)
    ctx = binding.Context(model, device=0, max_batch=17, dtype=dtype)
    assert ctx.tokens == N and ctx.prefix == 0 and len(ctx.split(17)) == 2
    plain = {n: ctx.forward(imgs[:n], want_logits=True) for n in (1, 3, 17)}
    for n in (1, 3, 17):
        d = float(np.abs(plain[n][0] - ref["probs"][:n]).max())
        print(f"dtype {dtype} batch {n}: max|dprob| {d:.3e}")
        assert d <= PROB_TOL[dtype], (n, d)
    assert np.array_equal(_bits(plain[17][0][:3]), _bits(plain[3][0])) and np.array_equal(_bits(plain[17][0][:1]), _bits(plain[1][0]))
    ids = ctx.boundary_rows(17)
    ctx.trace_enable(ids)
    ctx.forward(imgs)
    x = ctx.trace_read()
    ctx.trace_enable([])
    assert x.shape == (L + 1, len(ids), N, D)
    d0 = float(np.abs(x[0] - ref["trace"][0][ids]).max()); g0 = 2e-5 * max(1.0, float(np.abs(ref["trace"][0]).max()))
    print(f"dtype {dtype} stage 0: max|d| {d0:.3e} (gate {g0:.3e})")
    assert d0 <= g0                                                    # row b * N is patch 0 + pos[0]
    for il, (e_max, e_rms) in enumerate(stage_errors(x, ref["trace"][:, ids]), 1):
        print(f"dtype {dtype} stage {il}: max|d| / rms {e_max:.3e}, rms(d) / rms {e_rms:.3e}")
        assert stage_ok(e_max, e_rms, dtype), (il, e_max, e_rms)
    # the pooled embedding
    ctx.feat_enable(cls=True, mean=True, tokens=True)
    p17, lg17 = ctx.forward(imgs, want_logits=True)
    f = ctx.feat_read(17)[L - 1]
    e, mean, tok = f["cls"], f["mean"], f["tokens"]
    assert e.shape == (17, D) and mean.shape == (17, D) and tok.shape == (17, N, D)
    assert np.array_equal(_bits(p17), _bits(plain[17][0])), "features must not change the forward of a context that evaluates every row anyway"
    cos = MD.one_minus_cos(e, exact["e"])
    gate = MD.cos_gate(dtype)
    print(f"dtype {dtype}: 1 - cos(e, restatement) worst image {cos.max():.3e}  (gate {gate:.3e}; against the rounded restatement {MD.one_minus_cos(e, ref['e']).max():.3e})")
    assert cos.max() <= gate
    ml = MD.mean_length(e, exact["e"])
    lgate = MD.len_gate(dtype)
    print(f"dtype {dtype}: mean |e| / |e_restatement| - 1 = {ml:+.3e}  (gate {lgate:.3e})")
    assert abs(ml) <= lgate
    # The mutants of the restatement lie outside the same gates, both operand types: flat softmax by the direction of e (1 - cos), the wrong
    # activation in the MLPs (QuickGELU for tanh-GELU), which mostly rescales e, by its mean length (tests/map_data.py LEN)
    for name, mut in (("flat softmax", dict(flat=True)), ("QuickGELU for tanh", dict(activation=AD.ACT_QUICK))):
        _, m = _ref(pkg, None, **mut)
        cm, dp, lm = float(MD.one_minus_cos(e, m["e"]).min()), float(np.abs(p17 - m["probs"]).max()), MD.mean_length(e, m["e"])
        print(f"dtype {dtype}: {name} mutant: 1 - cos(e) best image {cm:.3e} (gate {gate:.3e}), mean length {lm:+.3e} (gate {lgate:.3e}), max|dprob| {dp:.3e} (gate {PROB_TOL[dtype]:.0e})")
        assert cm > gate or abs(lm) > lgate or dp > PROB_TOL[dtype], name
    # RNE(e) is the head GEMM's operand: the logits are its product with the rounded head to GEMM accumulation noise (tests/test_gpu_arch.py:163), far
    # inside what an unrounded or differently rounded operand would give
    z = ROUND[dtype](e).astype(np.float64)
    hw = ROUND[dtype](t["head.weight"]).astype(np.float64)
    want = z @ hw.T + t["head.bias"].astype(np.float64)
    tol = 2e-6 * (np.abs(z) @ np.abs(hw).T) + 1e-6
    r = float((np.abs(lg17 - want) / tol).max())
    unrounded = float((np.abs(e.astype(np.float64) @ hw.T + t["head.bias"] - want) / tol).max())
    print(f"dtype {dtype}: logits against RNE(e) . head: worst err / tol {r:.3f}  (the unrounded e would be at {unrounded:.1f})")
    assert r <= 1.0 and unrounded > 2.0
    # MEAN and TOKENS cover all N rows: the tokens are the final norm of the traced stream, the mean is theirs
    i = ids.index(16) if 16 in ids else 0
    F64 = AD.layernorm64(x[L][i].astype(np.float64), t["norm.weight"].astype(np.float64), t["norm.bias"].astype(np.float64), 1e-6)
    assert np.abs(tok[ids[i]] - F64).max() <= 1e-4 and np.abs(mean - tok.astype(np.float64).mean(1)).max() <= 1e-5
    # l2: a unit vector along e
    ctx.feat_enable(cls=True, l2=True)
    ctx.forward(imgs[:3])
    e2 = ctx.feat_read(3)[L - 1]["cls"]
    assert np.abs(np.linalg.norm(e2.astype(np.float64), axis=1) - 1).max() <= 1e-6 and np.abs(e2 - e[:3] / np.linalg.norm(e[:3].astype(np.float64), axis=1)[:, None]).max() <= 1e-6
    with pytest.raises(binding.VitxError) as ei:                       # the pooled embedding exists for the last layer only
        ctx.feat_enable(cls=True, layers=[0, 1])
    assert ei.value.code == binding.ERR_ARG
    ctx.close(); model.close()


def test_batches_graph_replay_and_two_contexts(pkg, binding, torch_gpu):
    """Batches 1, 5 and 64 against batch 1 bit for bit (probabilities and e); a hipGraph replay gives the same bits; two contexts of one model share
    the weights and agree."""
    rng_imgs = PD.exact_images(64, S, seed=2)
    model = binding.Model(MD.fixture_file(pkg))
    ctx = binding.Context(model, device=0, max_batch=64, dtype=1)
    ctx.feat_enable(cls=True)
    p64 = ctx.forward(rng_imgs); e64 = ctx.feat_read(64)[L - 1]["cls"].copy()
    assert len(ctx.split(64)) == 2
    p5 = ctx.forward(rng_imgs[:5]); e5 = ctx.feat_read(5)[L - 1]["cls"].copy()
    assert np.array_equal(_bits(p5), _bits(p64[:5])) and np.array_equal(_bits(e5), _bits(e64[:5]))
    for i in (0, 4, 31, 32, 63):
        p1 = ctx.forward(rng_imgs[i:i + 1]); e1 = ctx.feat_read(1)[L - 1]["cls"]
        assert np.array_equal(_bits(p1), _bits(p64[i:i + 1])) and np.array_equal(_bits(e1), _bits(e64[i:i + 1])), i
    ctx2 = binding.Context(model, device=0, max_batch=5, dtype=1, graph=1)
    assert ctx2.shares_weights()
    outs = [ctx2.forward(rng_imgs[:5]) for _ in range(4)]
    assert ctx2.graph_launches() >= 1
    for o in outs:
        assert np.array_equal(_bits(o), _bits(p5))
    ctx2.close(); ctx.close(); model.close()


def test_unsupported_cases(pkg, binding, torch_gpu, tmp_path):
    model = binding.Model(MD.fixture_file(pkg))
    with pytest.raises(binding.VitxError) as ei:
        binding.Context(model, device=0, max_batch=2, dtype=binding.MXFP8)
    assert ei.value.code == binding.ERR_UNSUPPORTED
    with pytest.raises(binding.VitxError) as ei:                       # the second part of the feature: not here yet
        binding.Context(model, device=0, max_batch=2, dtype=1, img_size=70)
    assert ei.value.code == binding.ERR_UNSUPPORTED and "class row" in str(ei.value)
    ctx = binding.Context(model, device=0, max_batch=2, dtype=1)
    with pytest.raises(binding.VitxError) as ei:
        ctx.attn_enable([0])
    assert ei.value.code == binding.ERR_UNSUPPORTED and "class token" in str(ei.value)
    ctx.close(); model.close()
    hp, t = MD.fixture_tensors(pkg)                                    # a one-channel (ViTSTR) file with the extension
    t["patch_embed.proj.weight"] = np.ascontiguousarray(t["patch_embed.proj.weight"][:, :1])
    path = str(tmp_path / "grey.gguf")
    pkg.ggml_file.write_model(path, hp, t, ftype=1)
    grey = binding.Model(path)
    assert grey.in_channels == 1
    with pytest.raises(binding.VitxError) as ei:
        binding.Context(grey, device=0, max_batch=2, dtype=0)
    assert ei.value.code == binding.ERR_UNSUPPORTED
    grey.close()


def test_q8_0_file_matches_the_restatement_on_dequantised_weights(pkg, binding, torch_gpu, tmp_path):
    """q8_0 blocks, attn_pool.* untouched."""
    q8 = str(tmp_path / "q8.gguf")
    binding.quantize_file(MD.fixture_file(pkg), q8, 8)
    t, ref = _ref(pkg, 0, path=q8)
    assert np.array_equal(t["attn_pool.kv.weight"], PD.file_tensors(pkg, MD.fixture_file(pkg))["attn_pool.kv.weight"])
    imgs = _images()[:3]
    model = binding.Model(q8)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=0)
    ctx.feat_enable(cls=True)
    p = ctx.forward(imgs)
    e = ctx.feat_read(3)[L - 1]["cls"]
    d = float(np.abs(p - ref["probs"][:3]).max()); c = float(MD.one_minus_cos(e, ref["e"][:3]).max())
    print(f"q8_0: max|dprob| {d:.3e}, 1 - cos(e) {c:.3e}")
    assert d <= PROB_TOL[0] and c <= MD.cos_gate(0)
    ctx.close(); model.close()
