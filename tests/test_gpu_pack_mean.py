"""The cls + mean head and VITX_FEAT_MEAN on packs on the MI355X (include/vitx.h "packed batches", pool_head = 2): csrc/features_packed.hip against
float64 and the row kernels, its independence of position and neighbours, a pack of a DINOv2-class file end to end against ref64.forward64."""
import numpy as np
import pytest

import exact_data as X
import feature_data as FD
import map_data as MD
import pack_mean_data as KD
import prefix_data as PD
import ref64 as R64

pytestmark = pytest.mark.gpu
SENT = -12345.5
T16 = {0: "float16", 1: "bfloat16"}
NAME, H, P, SHAPES = "vit_micro_patch14_56", 2, 14, [(56, 56), (56, 112), (462, 56)]      # 16, 32 and 33 x 4 = 132 patch rows: two chunks
ROUND = {0: PD.f16_round, 1: PD.bf16_round}

def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)

def _run(binding, torch, x, row0, w, b, dtype):
    """vitx_op_feat_pool_packed on a pack: (cls [n][D], mean [n][D], z [n][2 D] as f32); sentinels behind every output, x unchanged, z's pad rows zero."""
    n, D, m_pad = len(row0) - 1, x.shape[1], -(-(len(row0) - 1) // 8) * 8
    dx, dw, db, dr = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, w, b, row0))
    cls, mean = (torch.full((n + 1, D), SENT, dtype=torch.float32, device="cuda") for _ in range(2))
    z = torch.full((m_pad + 1, 2 * D), SENT, dtype=getattr(torch, T16[dtype]), device="cuda")
    binding.op_feat_pool_packed(dtype, dx.data_ptr(), dr.data_ptr(), n, KD.T, D, dw.data_ptr(), db.data_ptr(), 1e-6, cls.data_ptr(), mean.data_ptr(), z.data_ptr())
    sent16 = torch.tensor(SENT).to(z.dtype).float().item()
    cls, mean, z = cls.cpu().numpy(), mean.cpu().numpy(), z.float().cpu().numpy()
    assert (cls[n] == SENT).all() and (mean[n] == SENT).all() and (z[m_pad] == sent16).all(), "a row behind an output was written"
    assert np.array_equal(dx.cpu().numpy().view(np.uint32), x.view(np.uint32)), "the residual stream was written"
    assert not z[n:m_pad].any(), "pad rows of z are not zero"
    return cls[:n], mean[:n], z[:n]

@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("D", KD.WIDTHS)
def test_op_against_float64_and_the_row_kernels(binding, torch_gpu, D, dtype):
    torch, t16 = torch_gpu, getattr(torch_gpu, T16[dtype])
    R, W, _ = binding.pack_mean_chunks([0, KD.T + 1], KD.T, D)
    cnts = KD.counts(R, W)
    x, row0 = KD.pack(KD.image_rows(D, cnts))
    w, b = X.ln_params(D)
    cls, mean, z = _run(binding, torch, x, row0, w, b, dtype)
    # the launch's own rows through the two row kernels: the f32 final norm and the operand rows
    dx, dw, db = (torch.from_numpy(a).cuda() for a in (x, w, b))
    F, U = torch.zeros_like(dx), torch.zeros(dx.shape, dtype=t16, device="cuda")
    binding.op_layernorm_f32(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), F.data_ptr(), len(x), D)
    binding.check(binding.lib().vitx_op_layernorm(dtype, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), U.data_ptr(), len(x), D, 1e-6, None))
    torch.cuda.synchronize()
    F, U = F.cpu().numpy(), U.float().cpu().numpy()
    assert np.array_equal(_bits(cls), _bits(F[row0[:-1]])), "cls is not the f32 final norm of the class row"
    assert np.array_equal(_bits(z[:, :D]), _bits(U[row0[:-1]])), "the operand's class half is not the operand row of the class row"
    assert np.array_equal(_bits(z[:, D:]), _bits(torch.from_numpy(mean).to(t16).float().numpy())), "the operand's mean half is not RNE(mean)"
    for i, c in enumerate(cnts):
        m64, mb = FD.mean_bound(F[None, row0[i] + KD.T:row0[i + 1]])
        print(f"D {D} dtype {dtype} image {i} ({c} patch rows): max |mean - mean64| / bound = {float((np.abs(mean[i] - m64[0]) / np.maximum(mb[0], 1e-300)).max()):.3f}")
        assert np.isfinite(mean[i]).all() and (np.abs(mean[i] - m64[0]) <= mb[0]).all(), (i, c)

@pytest.mark.parametrize("D", KD.WIDTHS)
def test_position_neighbours_and_what_lies_behind(binding, torch_gpu, D):
    """Every image alone, the pack reversed, one image all NaN (NaN rows lie in front of and behind every pack): the clean images keep their bits."""
    R, W, _ = binding.pack_mean_chunks([0, KD.T + 1], KD.T, D)
    blocks = KD.image_rows(D, KD.counts(R, W))
    w, b = X.ln_params(D)
    n = len(blocks)
    run = lambda bl: [_bits(o) for o in _run(binding, torch_gpu, *KD.pack(bl), w, b, 0)]
    full, rev = run(blocks), run(blocks[::-1])
    assert all(np.isfinite(o.view(np.float32)).all() for o in full)
    poisoned = run([np.full_like(bl, np.nan) if i == 5 else bl for i, bl in enumerate(blocks)])
    for i in range(n):
        alone = run([blocks[i]])
        for k, name in enumerate(("cls", "mean", "z")):
            assert np.array_equal(alone[k][0], full[k][i]) and np.array_equal(rev[k][n - 1 - i], full[k][i]), (name, i, "alone or reversed")
            assert i == 5 or np.array_equal(poisoned[k][i], full[k][i]), (name, i, "beside a NaN image")

@pytest.mark.parametrize("dtype", [0, 1])
def test_pack_end_to_end(pkg, binding, torch_gpu, dtype):
    path = pkg.synth.cached_synthetic(NAME, head_scale=4.0, registers=4, head_pool=1)
    t = PD.file_tensors(pkg, path)
    rng = np.random.default_rng(41)
    imgs = [(rng.integers(-64, 64, (h, w, 3)) / 16.0).astype(np.float32) for h, w in SHAPES]
    model, cls_model = binding.Model(path), binding.Model(pkg.synth.cached_synthetic(NAME, head_scale=4.0, registers=4, head_pool=0))
    mk = lambda m, **kw: binding.PackContext(m, device=0, max_tokens=sum(5 + (h // P) * (w // P) for h, w in SHAPES), max_images=3, dtype=dtype, **kw)
    pack, cls_pack = mk(model, pool_head=binding.PACK_POOL_CLS_MEAN), mk(cls_model)
    pack.forward([imgs[0]]); cls_pack.forward([imgs[0]])
    assert pack.launches[0] == cls_pack.launches[0] + 1, "one launch more than a class-token pack of the same tower"
    pack.feat_enable(cls=False, tokens=True, mean=True)
    p, lg = pack.forward(imgs)
    mean, tok = pack.feat_read_mean(), pack.feat_read()[1]
    for k, img in enumerate(imgs):
        ref = R64.forward64(t, img[None], H, binding=binding, wround=ROUND[dtype], uround=ROUND[dtype])
        dp, dl = float(np.abs(p[k] - ref["probs"][0]).max()), float(np.abs(lg[k] - ref["logits"][0]).max())
        m64, mb = FD.mean_bound(tok[k].reshape(1, -1, tok[k].shape[-1]))
        # max|dlogit| is printed, not checked: ref64 holds no logit gate and none is invented here; the probabilities and both argmaxes are the check
        print(f"dtype {dtype} image {k} {img.shape[:2]}: max|dprob| {dp:.3e} (gate {R64.PROB_TOL[dtype]:.0e}), max|dlogit| {dl:.3e}")
        assert p[k].argmax() == ref["probs"][0].argmax() == lg[k].argmax() and dp <= R64.PROB_TOL[dtype]
        assert (np.abs(mean[k] - m64[0]) <= mb[0]).all()
        p1, lg1 = pack.forward([img])
        assert np.array_equal(_bits(p1[0]), _bits(p[k])) and np.array_equal(_bits(lg1[0]), _bits(lg[k])) and np.array_equal(_bits(pack.feat_read_mean()[0]), _bits(mean[k])), k
    # VITX_FEAT_MEAN on the class-token pack (tokens on before and after, for the bound's rows): two launches more and the mean under its bound; off
    # again: the bits and the launch count of before, the scratch of before + the two buffers a pack keeps (include/vitx.h)
    cls_pack.feat_enable(cls=False, tokens=True)
    cls_pack.forward(imgs)                    # the call that builds the grids' tables counts their launches and bytes: not the baseline
    p0, n0, bytes0 = _bits(cls_pack.forward(imgs)[0]), cls_pack.launches[0], cls_pack.scratch_bytes
    cls_pack.feat_enable(cls=False, tokens=True, mean=True)
    p_on, n_on = _bits(cls_pack.forward(imgs)[0]), cls_pack.launches[0]
    cmean, ctok = cls_pack.feat_read_mean(), cls_pack.feat_read()[1]
    for k in range(3):
        m64, mb = FD.mean_bound(ctok[k].reshape(1, -1, ctok[k].shape[-1]))
        assert (np.abs(cmean[k] - m64[0]) <= mb[0]).all(), k
    cls_pack.feat_enable(cls=False, tokens=True)
    kept = (3 + (cls_pack.max_tokens // 128 + 3)) * 128 * 4
    assert n_on == n0 + 2 and np.array_equal(p_on, p0) and np.array_equal(_bits(cls_pack.forward(imgs)[0]), p0)
    assert (cls_pack.launches[0], cls_pack.scratch_bytes) == (n0, bytes0 + kept)
    # recorded, not pinned: a pack of the file's own shape beside a rectangular context that evaluates every row (its mean has another order)
    own = PD.exact_images(3, 56, seed=1)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=dtype, last_layer_all_rows=1)
    print(f"dtype {dtype}: worst |logit - logit of the image context|, one-shape pack: {float(np.abs(pack.forward(list(own))[1] - ctx.forward(own, want_logits=True)[1]).max()):.3e}")
    ctx.close(); pack.close(); cls_pack.close(); model.close(); cls_model.close()

def test_refusals_that_need_a_device(pkg, binding, torch_gpu):
    torch = torch_gpu
    model = binding.Model(MD.fixture_file(pkg))
    pack = binding.PackContext(model, device=0, max_tokens=64, max_images=2, dtype=binding.BF16, pool_head=1)
    with pytest.raises(binding.VitxError) as ei:
        pack.feat_enable(mean=True)
    assert ei.value.code == binding.ERR_ARG
    pack.close(); model.close()
    x, w, out = torch.zeros((16, 128), device="cuda"), torch.ones(128, device="cuda"), torch.zeros((8, 256), device="cuda")
    row0 = torch.tensor([0, KD.T + 3, 2 * KD.T + 3], dtype=torch.int32, device="cuda")       # image 1 has no patch row: the table is read back, nothing is launched
    with pytest.raises(binding.VitxError) as ei:
        binding.op_feat_pool_packed(0, x.data_ptr(), row0.data_ptr(), 2, KD.T, 128, w.data_ptr(), w.data_ptr(), 1e-6, 0, out.data_ptr(), 0)
    assert ei.value.code == binding.ERR_ARG and not out.any()
