"""Zero-shot classification on the MI355X (include/vitx.h "zero-shot classification"): the kernels bit for bit on exact data, pad rows and columns
that never leak, hostile rows, probabilities against float64 on the engine's own logits, the forward end to end on a CLIP-class and a SigLIP-class
micro file, the invariants (batch, position, cut, streams, bank replaced), and every error.  The restatement is tests/zs_data.py, pinned to
transformers in tests/test_cpu_zeroshot.py."""
import ctypes as C

import numpy as np
import pytest

import arch_data as AD
import zs_data as Z

pytestmark = pytest.mark.gpu

SENT = -12345.5
TDT = {0: "float16", 1: "bfloat16"}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _up(v, m):
    return (v + m - 1) // m * m


def _run(binding, torch, z, t, dtype, kind, scale, bias, z_stride=None, poison=False):
    """vitx_op_zeroshot on z [n][E] f32 and the bank t [K][E] (f32 values already exact in the operand type).  The gap between z's rows (z_stride >
    E) holds NaN; probs / logits carry one sentinel row behind the n real ones.  poison: the operand scratch and the whole accumulator scratch
    (pad rows, pad columns, the bias row) start as NaN and +-inf.  Returns probs, logits [n][K], the operand rows a [n_pad][E] as f32, and the
    accumulator scratch [n_pad + 1][K_pad] as left behind."""
    n, E = z.shape
    K = t.shape[0]
    k_pad, n_pad = _up(K, 128), _up(n, 256)
    zs = z_stride or E
    zb = np.full((n, zs), np.nan, np.float32); zb[:, :E] = z
    tb = np.zeros((k_pad, E), np.float32); tb[:K] = t
    tdt = getattr(torch, TDT[dtype])
    d_z = torch.from_numpy(zb).cuda()
    d_t = torch.from_numpy(tb).cuda().to(tdt)
    assert np.array_equal(d_t.float().cpu().numpy(), tb), "the bank must be exact in the operand type"
    if poison:
        pat = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")], device="cuda")
        d_a = pat.repeat(n_pad * E // 4).reshape(n_pad, E).to(tdt)
        d_acc = pat.repeat((n_pad + 1) * k_pad // 4).reshape(n_pad + 1, k_pad).clone()
    else:
        d_a = torch.zeros((n_pad, E), dtype=tdt, device="cuda")
        d_acc = torch.zeros((n_pad + 1, k_pad), dtype=torch.float32, device="cuda")
    before = d_acc.cpu().numpy().copy()
    d_p = torch.full((n + 1, K), SENT, dtype=torch.float32, device="cuda")
    d_l = torch.full((n + 1, K), SENT, dtype=torch.float32, device="cuda")
    binding.op_zeroshot(dtype, d_z.data_ptr(), zs, d_t.data_ptr(), d_a.data_ptr(), d_acc.data_ptr(), d_p.data_ptr(), d_l.data_ptr(), n, K, E, kind, scale, bias)
    torch.cuda.synchronize()
    p, l, a, acc = d_p.cpu().numpy(), d_l.cpu().numpy(), d_a.float().cpu().numpy(), d_acc.cpu().numpy()
    assert (p[n:] == SENT).all() and (l[n:] == SENT).all(), "rows past n were written"
    assert not a[n:].any(), "the operand pad rows must be written as zeros"
    assert not acc[n_pad].any(), "the bias row must be zeros"
    # pad rows and pad columns of the accumulator scratch are neither written nor read: still what they were (bit for bit, NaN included)
    assert np.array_equal(_bits(acc[n:n_pad]), _bits(before[n:n_pad])) and np.array_equal(_bits(acc[:n, K:]), _bits(before[:n, K:]))
    return p[:n], l[:n], a, acc


# ------------------------------------------------------------------------------------------------ 1. bit for bit on exact data
def _exact_case(n, K, seed):
    """z = +-2^k (k per row), so ss = 64 4^k, nrm = 2^(k + 3), a = +-1/8; bank entries j/8, |j| <= 8; scale 4, bias 3/8.  Every product is a
    multiple of 2^-6 and sum |a t| <= 8: any partial sum in any order is an integer below 2^10 times 2^-6 -- exact in f32; so is c * 4 + 3/8."""
    rng = np.random.default_rng(seed)
    E = 64
    k = rng.integers(-12, 13, (n, 1))
    z = (rng.choice([-1.0, 1.0], (n, E)) * 2.0 ** k).astype(np.float32)
    t = (rng.integers(-8, 9, (K, E)) / 8.0).astype(np.float32)
    a = np.sign(z) / 8
    prod = np.abs(a[:, None, :].astype(np.float64) * t[None].astype(np.float64))
    assert (prod * 64 == np.rint(prod * 64)).all() and prod.sum(-1).max() * 64 < 2 ** 24          # every partial sum: an integer / 64 below 2^24
    return z, t, a


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 257])
def test_logits_bit_for_bit_on_exact_data(binding, torch_gpu, dtype, K):
    scale, bias = 4.0, 0.375
    for n, stride in ((1, 64), (3, 80), (129, 64), (129, 80)):            # 129 rows cross a row tile of every GEMM family; 80: a row stride above E
        z, t, a = _exact_case(n, K, seed=K * 1000 + n)
        assert np.array_equal(Z.device_operand(z, dtype), a.astype(np.float32))
        for kind in (Z.SOFTMAX, Z.SIGMOID):
            p, l, a_dev, _ = _run(binding, torch_gpu, z, t, dtype, kind, scale, bias, z_stride=stride)
            want = Z.restate(a, t, kind, scale, bias)
            assert np.array_equal(want["logits"], want["logits"].astype(np.float32).astype(np.float64))      # the restatement's logits are f32 values
            assert np.array_equal(_bits(a_dev[:n]), _bits(a)), (n, stride, "operand rows")
            assert np.array_equal(_bits(l), _bits(want["logits"].astype(np.float32))), (n, stride, kind, "logits")
            err = float(np.abs(p / want["probs"] - 1).max())
            assert np.isfinite(p).all() and err < 2e-6, (n, stride, kind, err)
            if kind == Z.SOFTMAX:
                assert np.abs(p.astype(np.float64).sum(1) - 1).max() < 1e-6


# ------------------------------------------------------------------------------------------------ 2. pad columns and rows never leak
@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
def test_pad_rows_and_columns_never_leak(binding, torch_gpu, dtype):
    """K = 65 leaves 63 pad columns in the accumulator rows; with them, the pad rows and the operand scratch full of NaN and +-inf the outputs are
    the same bits, the probabilities finite and the softmax rows sum to 1."""
    for n in (3, 129):
        z, t, a = _exact_case(n, 65, seed=65000 + n)
        for kind in (Z.SOFTMAX, Z.SIGMOID):
            p0, l0, _, _ = _run(binding, torch_gpu, z, t, dtype, kind, 4.0, 0.375, z_stride=80)
            p1, l1, _, _ = _run(binding, torch_gpu, z, t, dtype, kind, 4.0, 0.375, z_stride=80, poison=True)
            assert np.array_equal(_bits(l0), _bits(l1)) and np.array_equal(_bits(p0), _bits(p1)), (n, kind)
            assert np.isfinite(p1).all() and np.isfinite(l1).all()
            assert np.array_equal(_bits(l1), _bits(Z.restate(a, t, kind, 4.0, 0.375)["logits"].astype(np.float32)))
            if kind == Z.SOFTMAX:
                assert np.abs(p1.astype(np.float64).sum(1) - 1).max() < 1e-6


# ------------------------------------------------------------------------------------------------ 3. hostile rows
@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
def test_all_zero_embedding(binding, torch_gpu, dtype):
    """a = 0: every logit equals bias exactly, the softmax is uniform to the last bit of 1 / K for K a power of two (row 1 is an ordinary row)."""
    rng = np.random.default_rng(5)
    for K in (64, 1024):
        z = np.zeros((2, 128), np.float32); z[1] = rng.standard_normal(128)
        t = Z.ROUND[dtype](Z.unit_rows(rng.standard_normal((K, 128))))
        for kind in (Z.SOFTMAX, Z.SIGMOID):
            p, l, a, _ = _run(binding, torch_gpu, z, t, dtype, kind, 50.0, -1.75)
            assert not a[0].any() and np.array_equal(_bits(l[0]), _bits(np.full(K, -1.75)))
            if kind == Z.SOFTMAX:
                assert np.array_equal(_bits(p[0]), _bits(np.full(K, 1.0 / K)))
            assert np.ptp(l[1]) > 1.0 and np.isfinite(p).all()


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
def test_one_huge_and_many_tiny_entries(binding, torch_gpu, dtype):
    """z = one entry of 1e15 among entries of 1e-15 .. 1e-12 (and a row of 1e-18s, a row at 5e17: ss of 1e-34 and 1e38, towards both ends of f32): the operand rows are
    the f32 rule's bit for bit (zs_data.device_operand), the logits the restatement's within f32 accumulation."""
    rng = np.random.default_rng(6)
    E, K = 256, 130
    z = (rng.standard_normal((4, E)) * 10.0 ** rng.uniform(-15, -12, (4, E))).astype(np.float32)
    z[0, 77] = 1e15; z[1, 255] = -1e15
    z[2] = (rng.standard_normal(E) * 1e-18).astype(np.float32)
    z[3] = (rng.standard_normal(E) * 5e17).astype(np.float32)
    t = Z.ROUND[dtype](Z.unit_rows(rng.standard_normal((K, E))))
    want_a = Z.device_operand(z, dtype)
    assert abs(want_a[0, 77]) == 1 and np.abs(np.linalg.norm(want_a[2:].astype(np.float64), axis=1) - 1).max() < 1e-2
    for kind in (Z.SOFTMAX, Z.SIGMOID):
        p, l, a, _ = _run(binding, torch_gpu, z, t, dtype, kind, 30.0, 0.5)
        assert np.array_equal(_bits(a[:4]), _bits(want_a))
        want = Z.restate(want_a, t, kind, 30.0, 0.5)
        r = float((np.abs(l - want["logits"]) / Z.logit_tol(want_a, t, 30.0, 0.5)).max())
        print(f"dtype {dtype} kind {kind}: logits, worst err / tol {r:.3f}")
        assert r <= 1.0 and np.isfinite(p).all()


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
def test_logits_spread_over_80(binding, torch_gpu, dtype):
    """z = e_0 and bank rows (c_k, sqrt(1 - c_k^2), 0, ...) with c_k = k / 128 - 1, scale 80: logits -80 .. 80 in steps of 5/8.  The softmax does not
    overflow; the sigmoid is exactly 0 or 1 only where the float64 value rounds there in f32 (l = 16.875 lies where 1 + expf(-l) already rounds to 1)."""
    K, E = 257, 64
    c = np.arange(K) / 128.0 - 1.0
    t = np.zeros((K, E), np.float32); t[:, 0] = c; t[:, 1] = Z.ROUND[dtype](np.sqrt(1 - c * c).astype(np.float32))
    assert np.array_equal(Z.ROUND[dtype](t), t)
    z = np.zeros((2, E), np.float32); z[0, 0] = 3.0; z[1, 0] = -0.5
    for kind in (Z.SOFTMAX, Z.SIGMOID):
        p, l, a, _ = _run(binding, torch_gpu, z, t, dtype, kind, 80.0, 0.0)
        assert np.array_equal(l[0], (c * 80).astype(np.float32)) and np.array_equal(l[1], (-c * 80).astype(np.float32))      # (values: the sign of a zero logit is not pinned)
        want = Z.probs64(l.astype(np.float64), kind)
        assert np.isfinite(p).all()
        if kind == Z.SOFTMAX:
            assert np.abs(p.astype(np.float64).sum(1) - 1).max() < 1e-6 and p[0, -1] > 0.46 and p[1, 0] > 0.46
            assert np.abs(p - want).max() < 1e-6
        else:
            w32 = want.astype(np.float32)
            assert ((p == 1) <= (w32 == 1)).all() and ((p == 0) <= (w32 == 0)).all()
            assert (p == 1).any() and not (p == 0).any() and (p[0] < 1e-34).any()       # e^-80 = 1.8e-35 is an f32 value: nothing may flush to 0
            assert np.abs(p / want - 1).max() < 1e-6


# ------------------------------------------------------------------------------------------------ 4. probabilities on random data
_MEASURED = []


@pytest.mark.parametrize("kind", [Z.SOFTMAX, Z.SIGMOID], ids=["softmax", "sigmoid"])
@pytest.mark.parametrize("E,K", [(64, 1000), (512, 4099), (64, 4099), (512, 1000)])
def test_probabilities_on_random_data(binding, torch_gpu, E, K, kind):
    """Unit Gaussian z, bf16.  The logits come off the MFMA in f32 (checked within f32 accumulation of the restatement's); the probabilities are
    compared with the restatement evaluated on the engine's OWN logits.  The gate is measured, not fixed: CPU torch's f32 softmax / sigmoid of the same
    logits against the same float64 values, times 4 (the device expf is another <= 1 ulp implementation)."""
    import torch
    dtype, n, scale, bias = 1, 5, 16.0, -1.0
    rng = np.random.default_rng(E + K + kind)
    z = rng.standard_normal((n, E)).astype(np.float32)
    t = Z.ROUND[dtype](Z.unit_rows(rng.standard_normal((K, E))))
    p, l, a, _ = _run(binding, torch_gpu, z, t, dtype, kind, scale, bias)
    want_a = Z.device_operand(z, dtype)
    assert np.array_equal(_bits(a[:n]), _bits(want_a))
    r = float((np.abs(l - Z.restate(want_a, t, kind, scale, bias)["logits"]) / Z.logit_tol(want_a, t, scale, bias)).max())
    want = Z.probs64(l.astype(np.float64), kind)
    lt = torch.from_numpy(l)
    ref = (torch.softmax(lt, dim=-1) if kind == Z.SOFTMAX else torch.sigmoid(lt)).numpy()
    e_dev, e_ref = float(np.abs(p / want - 1).max()), float(np.abs(ref / want - 1).max())
    print(f"E {E} K {K} {'softmax' if kind == Z.SOFTMAX else 'sigmoid'}: logits err / tol {r:.3f}; max relative error of the probabilities: device {e_dev:.3e}, CPU torch f32 {e_ref:.3e} (gate {4 * e_ref:.3e})")
    assert r <= 1.0
    assert e_dev <= 4 * e_ref


# ------------------------------------------------------------------------------------------------ 5. end to end
def _embedding_and_zeroshot(binding, ctx, family, imgs):
    """One forward: (z = the engine's own f32 embedding, zero-shot probs, zero-shot logits, the forward's probs and logits)."""
    if family == "siglip":
        ctx.feat_enable(cls=True)
    p, lg = ctx.forward(imgs, want_logits=True)
    n = imgs.shape[0]
    z = lg if family == "clip" else ctx.feat_read(n)[ctx.model.hparams.num_hidden_layers - 1]["cls"].copy()
    zp, zl = ctx.zeroshot_read(n, want_logits=True)
    if family == "siglip":
        ctx.feat_disable()
    return z, zp, zl, p, lg


_BANK = {}


def _bank(pkg, family):
    if family not in _BANK:
        _BANK[family] = Z.bank(family, Z.embedding64(pkg, family))
    return _BANK[family]


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_forward_end_to_end(pkg, binding, torch_gpu, family, dtype):
    """The new path isolated: the engine's own f32 embedding of the same forward (logits for the CLIP-class file, VITX_FEAT_CLS for the SigLIP-class
    one) goes through the restatement; the pre-scale cosines agree within the operand type's bound (both operands rounded once + f32 accumulation),
    top-1 is equal wherever the restatement's top-2 margin exceeds twice the logit bound -- at least 3 of every 4 images."""
    t, kind, scale, bias = _bank(pkg, family)
    imgs = Z.images()
    model = binding.Model(Z.model_file(pkg, family))
    ctx = binding.Context(model, device=0, max_batch=Z.N_IMAGES, dtype=dtype)
    E = model.num_classes if family == "clip" else model.hparams.hidden_size
    assert E == t.shape[1] and len(ctx.split(Z.N_IMAGES)) == 2
    ctx.zeroshot_set(t, kind, scale, bias)
    z, zp, zl, _, _ = _embedding_and_zeroshot(binding, ctx, family, imgs)
    want = Z.restate(Z.normalise64(z), t, kind, scale, bias)
    bound = Z.COS_BOUND[dtype](E)
    d_cos = float(np.abs((zl.astype(np.float64) - bias) / scale - want["cos"]).max())
    d_log = float(np.abs(zl - want["logits"]).max())
    top, mar = Z.margins(want["logits"])
    sure = mar > 2 * bound * scale
    print(f"{family} dtype {dtype}: max|dcos| {d_cos:.3e} (bound {bound:.3e}), max|dlogit| {d_log:.3e} (bound {bound * scale:.3e}); "
          f"{int(sure.sum())} of {len(sure)} images with a top-2 margin above {2 * bound * scale:.3f} ({mar.min():.3f} .. {mar.max():.3f})")
    assert d_log <= bound * scale and d_cos <= bound * (1 + 1e-3)
    assert sure.mean() >= 0.75
    assert np.array_equal(zl.argmax(1)[sure], top[sure])
    rows = np.flatnonzero(sure)
    assert (zp[rows, top[rows]] == zp[rows].max(1)).all()            # (a saturated sigmoid row holds several 1.0s: the maximum, not a unique argmax)
    assert np.abs(zp / Z.probs64(zl.astype(np.float64), kind) - 1).max() < 1e-5
    # the operand rows are the f32 rule's on the engine's own embedding: the logits are the restatement's on ROUNDED operands within f32 accumulation
    a = Z.device_operand(z, dtype)
    tr = Z.ROUND[dtype](t)
    r = float((np.abs(zl - Z.restate(a, tr, kind, scale, bias)["logits"]) / Z.logit_tol(a, tr, scale, bias)).max())
    print(f"{family} dtype {dtype}: logits against the restatement on the rounded operands: worst err / tol {r:.3f}")
    assert r <= 1.0
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 6. invariants
def _hip_read(ptr, shape):
    out = np.empty(shape, np.float32)
    assert C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) == 0
    return out


@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_invariants(pkg, binding, torch_gpu, family):
    t, kind, scale, bias = _bank(pkg, family)
    K = t.shape[0]
    imgs = Z.images()
    n = Z.N_IMAGES
    model = binding.Model(Z.model_file(pkg, family))
    ctx = binding.Context(model, device=0, max_batch=n, dtype=1)
    cut = ctx.split(n)
    assert len(cut) == 2
    assert ctx.zeroshot_device() == (0, 0)
    plain = ctx.forward(imgs, want_logits=True)
    ctx.zeroshot_set(t, kind, scale, bias)
    assert binding.lib().vitx_zeroshot_classes(ctx._h) == K and binding.lib().vitx_zeroshot_images(ctx._h) == 0
    _, zp, zl, p, lg = _embedding_and_zeroshot(binding, ctx, family, imgs)
    # the forward's own outputs: the same bits with a bank set and without
    assert np.array_equal(_bits(p), _bits(plain[0])) and np.array_equal(_bits(lg), _bits(plain[1]))
    # the device buffer is what read returns: [capacity][2][K], probabilities then logits
    ptr, k_dev = ctx.zeroshot_device()
    dev = _hip_read(ptr, (n, 2, K))
    assert k_dev == K and np.array_equal(_bits(dev[:, 0]), _bits(zp)) and np.array_equal(_bits(dev[:, 1]), _bits(zl))
    assert np.array_equal(_bits(ctx.zeroshot_read(n)), _bits(zp))             # without the logits
    # batch 1 at both ends and on both sides of the cut; a 3-image batch
    for i in sorted({0, cut[0] - 1, cut[0], n - 1}):
        _, p1, l1, _, _ = _embedding_and_zeroshot(binding, ctx, family, imgs[i:i + 1])
        assert np.array_equal(_bits(p1), _bits(zp[i:i + 1])) and np.array_equal(_bits(l1), _bits(zl[i:i + 1])), i
    _, p3, l3, _, _ = _embedding_and_zeroshot(binding, ctx, family, imgs[5:8])
    assert np.array_equal(_bits(p3), _bits(zp[5:8])) and np.array_equal(_bits(l3), _bits(zl[5:8]))
    # the bank replaced (other classes, other kind, other scale) and set back
    other = Z.unit_rows(np.random.default_rng(9).standard_normal((K + 7, t.shape[1])))
    ctx.zeroshot_set(other, 1 - kind, 7.0, 0.25)
    assert binding.lib().vitx_zeroshot_images(ctx._h) == 0
    _, po, lo, _, _ = _embedding_and_zeroshot(binding, ctx, family, imgs)
    assert po.shape == (n, K + 7) and not np.array_equal(lo[:, :K], zl)
    ctx.zeroshot_set(t, kind, scale, bias)
    _, pb, lb, _, _ = _embedding_and_zeroshot(binding, ctx, family, imgs)
    assert np.array_equal(_bits(pb), _bits(zp)) and np.array_equal(_bits(lb), _bits(zl))
    # profiling: three launches per sub-batch while the bank is set, none after it is switched off (and its buffers are gone)
    ctx.profile_enable(True)
    ctx.forward(imgs)
    pr = {e["name"]: e for e in ctx.profile_read()}
    assert pr["zeroshot"]["launches"] == 3 * len(cut)
    ctx.zeroshot_set(None)
    assert ctx.zeroshot_device() == (0, 0) and binding.lib().vitx_zeroshot_images(ctx._h) == 0
    p_off = ctx.forward(imgs)
    assert "zeroshot" not in [e["name"] for e in ctx.profile_read()]
    ctx.profile_enable(False)
    assert np.array_equal(_bits(p_off), _bits(plain[0]))
    with pytest.raises(binding.VitxError) as ei:
        ctx.zeroshot_read()
    assert ei.value.code == binding.ERR_ARG
    ctx.close()
    # one stream: the same bits as two
    ctx1 = binding.Context(model, device=0, max_batch=n, dtype=1, streams=1)
    assert len(ctx1.split(n)) == 1
    ctx1.zeroshot_set(t, kind, scale, bias)
    _, p1s, l1s, _, _ = _embedding_and_zeroshot(binding, ctx1, family, imgs)
    assert np.array_equal(_bits(p1s), _bits(zp)) and np.array_equal(_bits(l1s), _bits(zl))
    ctx1.close(); model.close()


def test_graph_cache_is_bypassed_while_a_bank_is_set(pkg, binding, torch_gpu):
    t, kind, scale, bias = _bank(pkg, "clip")
    imgs = Z.images()[:5]
    model = binding.Model(Z.model_file(pkg, "clip"))
    ctx = binding.Context(model, device=0, max_batch=5, dtype=1, graph=1)
    ctx.zeroshot_set(t, kind, scale, bias)
    outs = [ctx.forward(imgs) for _ in range(4)]
    assert ctx.graph_launches() == 0
    zp = ctx.zeroshot_read(5)
    ctx.zeroshot_set(None)
    again = [ctx.forward(imgs) for _ in range(4)]
    assert ctx.graph_launches() >= 1
    for o in outs + again:
        assert np.array_equal(_bits(o), _bits(outs[0]))
    assert np.isfinite(zp).all()
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors(pkg, binding, torch_gpu):
    L = binding.lib()
    fp = C.POINTER(C.c_float)
    t, kind, scale, bias = _bank(pkg, "siglip")
    K, E = t.shape
    tp = t.ctypes.data_as(fp)
    model = binding.Model(Z.model_file(pkg, "siglip"))
    ctx = binding.Context(model, device=0, max_batch=4, dtype=1)
    h = ctx._h
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    assert L.vitx_zeroshot_set(h, None, 3, E, kind, scale, bias) == A                 # NULL bank with K > 0
    assert L.vitx_zeroshot_set(h, tp, 0, E, kind, scale, bias) == A                   # K < 1 with a bank
    assert L.vitx_zeroshot_set(h, tp, -1, E, kind, scale, bias) == A
    assert L.vitx_zeroshot_set(h, None, -1, E, kind, scale, bias) == A
    assert L.vitx_zeroshot_set(h, tp, K, 64, kind, scale, bias) == A                  # not the context's width (128)
    assert L.vitx_zeroshot_set(h, tp, K, 10, kind, scale, bias) == A                  # (the head's class count is not the width of a pooled-head context)
    assert L.vitx_zeroshot_set(h, tp, K, E, 2, scale, bias) == A and L.vitx_zeroshot_set(h, tp, K, E, -1, scale, bias) == A
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert L.vitx_zeroshot_set(h, tp, K, E, kind, bad, bias) == A and L.vitx_zeroshot_set(h, tp, K, E, kind, scale, bad) == A
    for bad in (np.nan, np.inf):
        tb = t.copy(); tb[K - 1, E - 1] = bad
        assert L.vitx_zeroshot_set(h, tb.ctypes.data_as(fp), K, E, kind, scale, bias) == A
        assert "[%d][%d]" % (K - 1, E - 1) in L.vitx_last_error().decode()
    assert L.vitx_zeroshot_set(h, tp, binding.zeroshot_max_classes(E) + 1, E, kind, scale, bias) == U       # refused before the bank is read
    assert L.vitx_zeroshot_classes(h) == 0 and L.vitx_zeroshot_device(h) is None      # nothing above left a bank behind
    buf = np.empty(4 * K, np.float32)
    assert L.vitx_zeroshot_read(h, buf.ctypes.data_as(fp), None, buf.size) == A       # off
    ctx.zeroshot_set(t, kind, scale, bias)
    assert L.vitx_zeroshot_read(h, buf.ctypes.data_as(fp), None, buf.size) == A       # before any forward with the bank set
    ctx.forward(Z.images()[:3])
    assert L.vitx_zeroshot_images(h) == 3
    assert L.vitx_zeroshot_read(h, buf.ctypes.data_as(fp), None, 3 * K - 1) == A      # too small
    assert L.vitx_zeroshot_read(h, None, None, buf.size) == A
    assert L.vitx_zeroshot_read(h, buf.ctypes.data_as(fp), None, 3 * K) == 0
    ctx.close(); model.close()
    # a width that is not a multiple of 64: arch_data's CLIP-class file has 10 "classes"
    m10 = binding.Model(AD.fixture_file(pkg, "clip"))
    c10 = binding.Context(m10, device=0, max_batch=2, dtype=1)
    t10 = Z.unit_rows(np.random.default_rng(1).standard_normal((3, 10)))
    with pytest.raises(binding.VitxError) as ei:
        c10.zeroshot_set(t10)
    assert ei.value.code == U and "multiple of 64" in str(ei.value)
    c10.close(); m10.close()
    # a ViTSTR context
    st = binding.Model(pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0))
    cs = binding.Context(st, device=0, max_batch=1, dtype=0)
    with pytest.raises(binding.VitxError) as ei:
        cs.zeroshot_set(Z.unit_rows(np.random.default_rng(1).standard_normal((3, 64))))
    assert ei.value.code == U and "ViTSTR" in str(ei.value)
    cs.close(); st.close()


def test_zero_shot_takes_one_pass(pkg, binding, torch_gpu):
    """A forward of more images than one pass of the kernels takes is refused while a bank is set, before anything runs."""
    torch = torch_gpu
    L = binding.lib()
    name = "vit_micro_patch8_224"                        # 785 tokens: the F16 parity mode's window holds 3339 images
    model = binding.Model(Z.clip_file(pkg, name=name))
    big = 3400
    ctx = binding.Context(model, device=0, max_batch=big, dtype=binding.F16, streams=1)
    limit = ctx.split(big)[0]
    assert limit < big
    ctx.zeroshot_set(Z.unit_rows(np.random.default_rng(2).standard_normal((5, Z.CLIP_E))), Z.SOFTMAX, 100.0, 0.0)
    n = limit + 1
    x = torch.zeros((n, 224, 224, 3), dtype=torch.float32, device="cuda")            # sized for the call: memory-safe even if the check were gone
    p = torch.zeros((n, model.num_classes), dtype=torch.float32, device="cuda")
    assert L.vitx_forward_device(ctx._h, x.data_ptr(), n, p.data_ptr(), None, None) == binding.ERR_ARG
    assert "one pass" in L.vitx_last_error().decode() and L.vitx_zeroshot_images(ctx._h) == 0
    ctx.close(); model.close()


def test_a_refused_set_leaves_the_bank_in_place(pkg, binding, torch_gpu):
    """A vitx_zeroshot_set that is refused for its arguments (a NaN in the bank) leaves the bank that was set: the next forward gives the same bits."""
    L = binding.lib()
    t, kind, scale, bias = _bank(pkg, "clip")
    imgs = Z.images()[:5]
    model = binding.Model(Z.model_file(pkg, "clip"))
    ctx = binding.Context(model, device=0, max_batch=5, dtype=1)
    ctx.zeroshot_set(t, kind, scale, bias)
    ctx.forward(imgs)
    zp, zl = ctx.zeroshot_read(5, want_logits=True)
    bad = t.copy(); bad[1, 2] = np.nan
    with pytest.raises(binding.VitxError) as ei:
        ctx.zeroshot_set(bad, kind, scale, bias)
    assert ei.value.code == binding.ERR_ARG
    ctx.forward(imgs)
    assert L.vitx_zeroshot_images(ctx._h) == 5 and L.vitx_zeroshot_classes(ctx._h) == t.shape[0]
    zp2, zl2 = ctx.zeroshot_read(5, want_logits=True)
    assert np.array_equal(_bits(zp2), _bits(zp)) and np.array_equal(_bits(zl2), _bits(zl))
    ctx.close(); model.close()
