"""The mean-pool head (include/vitx.h): vitx_op_pool_mean on exact, ordinary and NaN data; files with `pool` end to end against ref64.forward64."""
import numpy as np
import pytest

import exact_data as X
import prefix_data as PD
import ref64 as R64

pytestmark = pytest.mark.gpu

C = 64                                      # VITX_POOL_MEAN_CHUNK_ROWS
WIDTHS = (64, 768, 1152)                    # the smallest LayerNorm width, ViT-B, and a width whose statistics are not tiled
ROUND = {0: PD.f16_round, 1: PD.bf16_round}
NAME, H = "vit_micro_patch14_56", 2


def _run(torch, binding, x, first, w, b, dtype=1, m_pad=None, n=None):
    """The first n images of x [..][N][D] f32 (all of them by default) -> (m, e [n][D] f32, z [m_pad][D] as int16 bits, torch's RNE of e as int16 bits)."""
    (n, N, D), m_pad = (n or x.shape[0], *x.shape[1:]), m_pad or n or x.shape[0]
    dx, dw, db = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (x, w, b))
    m, e = torch.full((n, D), 7.0, device="cuda"), torch.full((n, D), 7.0, device="cuda")
    z = torch.full((m_pad, D), 7.0, device="cuda", dtype=torch.bfloat16 if dtype else torch.float16)
    binding.op_pool_mean(dtype, dx.data_ptr(), D, N * D, dw.data_ptr(), db.data_ptr(), X.LN_EPS, m.data_ptr(), e.data_ptr(), z.data_ptr(), n, m_pad, N, first, D)
    return m.cpu().numpy(), e.cpu().numpy(), z.view(torch.int16).cpu().numpy(), e.to(z.dtype).view(torch.int16).cpu().numpy()


@pytest.mark.parametrize("n_img", [1, 3])
@pytest.mark.parametrize("first", [0, 1, 5])
@pytest.mark.parametrize("Np", [1, C - 1, C, C + 1, 2 * C + 3])
@pytest.mark.parametrize("D", WIDTHS)
def test_pool_mean_exact_on_integer_rows(binding, torch_gpu, D, Np, first, n_img):
    """|x| <= 2^10 integers, Np <= 2^12: every partial sum is exact in f32, so m = f32(sum) / f32(Np) bit for bit.  The prefix rows and a canary image behind
    the last one hold 2^20: a row read too many moves m.  z = torch's RNE of the returned e; the pad rows of z are zero."""
    rng = np.random.default_rng(D + 7 * Np + first)
    x = np.full((n_img + 1, first + Np, D), 2.0 ** 20, np.float32)
    x[:n_img, first:] = rng.integers(-1024, 1025, (n_img, Np, D))
    w, b = X.ln_params(D)
    m, e, z, z_want = _run(torch_gpu, binding, x, first, w, b, m_pad=n_img + 2, n=n_img)
    want = x[:n_img, first:].astype(np.float64).sum(1).astype(np.float32) / np.float32(Np)
    assert np.array_equal(m.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(z[:n_img], z_want) and not z[n_img:].any()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("D,Np,first", [(64, 131, 1), (768, 196, 5), (1152, 65, 0)])
def test_pool_mean_ordinary_rows_within_the_f32_bounds(binding, torch_gpu, D, Np, first, dtype):
    """Normal rows.  m: an f32 sum of Np terms in any order is within (Np 2^-24) mean|x| of the exact mean, the division adds 2^-24 |m|.  e against
    ref64.layernorm64 of the float64 mean under the feature tests' bound of a final-norm row (feature_data.features64: ln_bound, ulp_out 2^-23)."""
    x = np.random.default_rng(D).standard_normal((3, first + Np, D)).astype(np.float32)
    w, b = X.ln_params(D)
    m, e, z, z_want = _run(torch_gpu, binding, x, first, w, b, dtype)
    rows = x[:, first:].astype(np.float64); m64 = rows.mean(1)
    mb = Np * 2.0 ** -24 * np.abs(rows).mean(1) + 2.0 ** -24 * np.abs(m64)
    assert (np.abs(m - m64) <= mb).all()
    e64, (_, rstd, xmax) = R64.layernorm64(m64, w.astype(np.float64), b.astype(np.float64), X.LN_EPS), X.layernorm64(m64, w, b)
    bound = X.ln_bound(e64, w, rstd, xmax, 2.0 ** -23)
    assert (np.abs(e - e64) <= bound).all(), float((np.abs(e - e64) / bound).max())
    assert np.array_equal(z, z_want)


@pytest.mark.parametrize("D", WIDTHS)
def test_pool_mean_bits_do_not_depend_on_the_batch(binding, torch_gpu, D):
    """An image's m, e, z alone == at every position of a batch of 3 whose other images are NaN."""
    N, first = 2 * C + 3 + 5, 5
    img = np.random.default_rng(D).standard_normal((1, N, D)).astype(np.float32)
    w, b = X.ln_params(D)
    alone = _run(torch_gpu, binding, img, first, w, b)[:3]
    for pos in range(3):
        x = np.full((3, N, D), np.nan, np.float32)
        x[pos] = img[0]
        got = _run(torch_gpu, binding, x, first, w, b)[:3]
        for a, g in zip(alone, got):
            assert np.array_equal(a[0].view(a.dtype.str.replace("f", "u")), g[pos].view(g.dtype.str.replace("f", "u"))), pos


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("cls,R", [(True, 4), (False, 4), (False, 0)])
@pytest.mark.parametrize("order", [0, 1])
def test_mean_pool_files_end_to_end(pkg, binding, torch_gpu, order, cls, R, dtype):
    """Stage 0 (a class-less file's registers as they are, the rows under the stage-0 gate), the later stages under ref64's gates, the probabilities under
    PROB_TOL against the head computed here from the restatement's last stage, RNE(VITX_FEAT_CLS) == the head operand: the logits of a host head on it."""
    path = pkg.synth.cached_synthetic(NAME, head_scale=4.0, registers=R, head_pool=3 + order, cls_token=cls)
    t, rnd, T, imgs = PD.file_tensors(pkg, path), ROUND[dtype], int(cls) + R, PD.exact_images(3, 56, seed=1)
    ref = R64.forward64(t, imgs, H, pos=t["pos_embed"][0].astype(np.float64), wround=rnd, uround=rnd)
    ctx = binding.Context(binding.Model(path), device=0, max_batch=4, dtype=dtype)
    ctx.feat_enable(cls=True, mean=True); ctx.trace_enable([0, 1, 2])
    probs, logits = ctx.forward(imgs, want_logits=True)
    x, f = ctx.trace_read(), ctx.feat_read(3)[1]
    if not cls and R:
        assert np.array_equal(x[0][:, :R].view(np.uint32), np.broadcast_to(t["reg_token"][0], (3, R, 128)).astype(np.float32).view(np.uint32))
    assert np.abs(x[0] - ref["embed"]).max() <= 2e-5 * max(1.0, float(np.abs(ref["embed"]).max()))      # tests/test_gpu_registers.py, stage 0
    for il, (e_max, e_rms) in enumerate(R64.stage_errors(x, ref["trace"]), 1):
        assert R64.stage_ok(e_max, e_rms, dtype), (il, e_max, e_rms)
    z = ref["mean"] if order == 0 else R64.layernorm64(ref["trace"][-1][:, T:].mean(1), t["norm.weight"].astype(np.float64), t["norm.bias"].astype(np.float64), 1e-6)
    e_max, e_rms = R64.stage_errors(np.stack([z, f["cls"]])[:, None], np.stack([z, z])[:, None])[0]
    assert R64.stage_ok(e_max, e_rms, dtype), (e_max, e_rms)
    assert order == 1 or np.array_equal(f["cls"].view(np.uint32), f["mean"].view(np.uint32))
    hw = rnd(t["head.weight"]).astype(np.float64)
    lg = rnd(z).astype(np.float64) @ hw.T + t["head.bias"]
    p = np.exp(lg - lg.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
    assert np.abs(probs - p).max() <= R64.PROB_TOL[dtype], float(np.abs(probs - p).max())
    want = rnd(f["cls"]).astype(np.float64) @ hw.T + t["head.bias"]
    tol = (np.abs(rnd(f["cls"])) @ np.abs(hw).T) * 2e-6 + 1e-6                                                  # tests/test_gpu_registers.py: the head on RNE(features)
    assert (np.abs(logits - want) <= tol).all(), float((np.abs(logits - want) / tol).max())
