"""The dense head on the MI355X (include/vitx.h "dense prediction"): the label kernel against the host function bit for bit on every shape and on
hostile data, the whole op bit for bit on exact data and under the f32 inner-product bound on ordinary data, the forward end to end on the synthetic
families, the invariants (batch, position, cut, streams, last_layer_all_rows, bank + gallery + head), the behaviour while a head is set and every
error.  The restatement is tests/dense_data.py, pinned to the host function and to torch's F.interpolate in tests/test_cpu_dense.py."""
import ctypes as C

import numpy as np
import pytest

import dense_data as DD
import prefix_data as PD
import zs_data as Z

pytestmark = pytest.mark.gpu

TDT = {0: "float16", 1: "bfloat16"}
CAN_U8, CAN_F = 0xA5, -12345.5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _up(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ 1. the label kernel on given logits
def _run_labels(binding, torch, d_lg, ld, n, gh, gw, K, oh, ow, off_u8, off_f):
    """Labels and scores between poisoned canaries; off_u8 / off_f: where the outputs start inside their buffers (bytes / floats), so that both the
    packed stores and the element-by-element path of a row off the pack's boundary run."""
    px = n * oh * ow
    d_lab = torch.full((off_u8 + px + 64,), CAN_U8, dtype=torch.uint8, device="cuda")
    d_sc = torch.full((off_f + px + 16,), CAN_F, dtype=torch.float32, device="cuda")
    binding.op_dense_labels(d_lg.data_ptr(), ld, n, gh, gw, K, oh, ow, d_lab.data_ptr() + off_u8, d_sc.data_ptr() + 4 * off_f)
    torch.cuda.synchronize()
    lab, sc = d_lab.cpu().numpy(), d_sc.cpu().numpy()
    assert (lab[:off_u8] == CAN_U8).all() and (lab[off_u8 + px:] == CAN_U8).all(), "a label canary was written"
    assert (sc[:off_f] == CAN_F).all() and (sc[off_f + px:] == CAN_F).all(), "a score canary was written"
    return lab[off_u8:off_u8 + px].reshape(n, oh, ow), sc[off_f:off_f + px].view(np.uint32).reshape(n, oh, ow)


def test_label_kernel_equals_the_host_function_bit_for_bit(binding, torch_gpu):
    """Every shape of dense_data.cases() on hostile data, ld = K_pad with the pad columns full of +inf and NaN; batches of 1 and 3 images (a wrong image
    stride shows in the second image); output buffers on and off the 4-byte / 16-byte boundaries."""
    torch = torch_gpu
    cases = DD.cases()
    ran = 0
    for i, (gh, gw, oh, ow, K, n) in enumerate(cases):
        ld = DD.pad_to(K)
        lg = DD.hostile(n, gh, gw, K, ld, seed=i)
        d_lg = torch.from_numpy(lg).cuda()
        for nn_ in sorted({1, n}):
            sub = np.ascontiguousarray(lg.reshape(n, gh * gw, ld)[n - nn_:].reshape(nn_ * gh * gw, ld))       # the LAST image alone: it holds the cell of NaNs
            want_lab, want_sc = binding.dense_labels_host(sub, nn_, gh, gw, K, oh, ow)
            d_sub = d_lg if nn_ == n else torch.from_numpy(sub).cuda()
            for off_u8, off_f in ((64, 16), (61, 17)) if ran % 3 == 0 or nn_ == n else ((64, 16),):
                lab, bits = _run_labels(binding, torch, d_sub, ld, nn_, gh, gw, K, oh, ow, off_u8, off_f)
                tag = (gh, gw, oh, ow, K, nn_, off_u8)
                assert np.array_equal(lab, want_lab), tag
                assert np.array_equal(bits, want_sc.view(np.uint32)), tag
                ran += 1
        # without a score buffer: the same labels
        d_lab = torch.full((n * oh * ow,), CAN_U8, dtype=torch.uint8, device="cuda")
        binding.op_dense_labels(d_lg.data_ptr(), ld, n, gh, gw, K, oh, ow, d_lab.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_lab.cpu().numpy().reshape(n, oh, ow), binding.dense_labels_host(lg, n, gh, gw, K, oh, ow, want_score=False)[0])
    assert ran > 80


def test_label_kernel_takes_any_row_stride(binding, torch_gpu):
    """ld above K_pad, and the smallest ld there is (K rounded up to 4): the columns behind K hold NaN and +inf and are never compared."""
    torch = torch_gpu
    for (gh, gw, oh, ow, K, n, ld) in ((2, 3, 32, 48, 21, 3, 24), (14, 14, 37, 37, 150, 2, 152), (2, 3, 5, 17, 129, 3, 388), (1, 5, 16, 80, 2, 3, 4)):
        lg = DD.hostile(n, gh, gw, K, ld, seed=ld)
        want_lab, want_sc = binding.dense_labels_host(lg, n, gh, gw, K, oh, ow)
        assert np.array_equal(want_lab, DD.labels(lg, n, gh, gw, K, oh, ow)[0])
        lab, bits = _run_labels(binding, torch, torch.from_numpy(lg).cuda(), ld, n, gh, gw, K, oh, ow, 64, 16)
        assert np.array_equal(lab, want_lab) and np.array_equal(bits, want_sc.view(np.uint32)), (gh, gw, oh, ow, K, ld)


# ------------------------------------------------------------------------------------------------ 2. the op: operand rows -> GEMM -> labels
def _run_op(binding, torch, a, w, bias, dtype, n, gh, gw, oh, ow):
    """vitx_op_dense on operand rows a [n gh gw][Dc] and the head w [K][Dc] (both exact in the operand type), bias [K].  The operand's pad rows and the
    whole logit buffer start as NaN and +-inf.  Returns the logit buffer [M_pad][K_pad], labels, score bits."""
    rows, Dc = a.shape
    K = w.shape[0]
    m_pad, k_pad = _up(rows, 256), _up(K, 128)
    tdt = getattr(torch, TDT[dtype])
    pat = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")], device="cuda")
    d_a = pat.repeat(m_pad * Dc // 4).reshape(m_pad, Dc).to(tdt)
    d_a[:rows] = torch.from_numpy(a).cuda().to(tdt)
    assert np.array_equal(d_a[:rows].float().cpu().numpy(), a), "the operand must be exact in the operand type"
    wb = np.zeros((k_pad, Dc), np.float32); wb[:K] = w
    d_w = torch.from_numpy(wb).cuda().to(tdt)
    assert np.array_equal(d_w.float().cpu().numpy(), wb), "the head must be exact in the operand type"
    bb = np.zeros(k_pad, np.float32); bb[:K] = bias
    d_b = torch.from_numpy(bb).cuda()
    d_lg = pat.repeat(m_pad * k_pad // 4).reshape(m_pad, k_pad).clone()
    px = n * oh * ow
    d_lab = torch.full((px + 64,), CAN_U8, dtype=torch.uint8, device="cuda")
    d_sc = torch.full((px + 16,), CAN_F, dtype=torch.float32, device="cuda")
    binding.op_dense(dtype, d_a.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), d_lg.data_ptr(), n, gh, gw, K, Dc, oh, ow, d_lab.data_ptr(), d_sc.data_ptr())
    torch.cuda.synchronize()
    assert not d_a[rows:].float().cpu().numpy().any(), "the operand pad rows must be written as zeros"
    lab, sc = d_lab.cpu().numpy(), d_sc.cpu().numpy()
    assert (lab[px:] == CAN_U8).all() and (sc[px:] == CAN_F).all()
    return d_lg.cpu().numpy(), lab[:px].reshape(n, oh, ow), sc[:px].view(np.uint32).reshape(n, oh, ow)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("Dc", [64, 192, 768 * 4])
def test_op_bit_for_bit_on_exact_data(binding, torch_gpu, Dc, dtype):
    for (n, gh, gw, oh, ow, K) in ((3, 2, 3, 32, 48, 21), (1, 14, 14, 37, 37, 150), (2, 16, 37, 16, 37, 129)):
        rows = n * gh * gw
        a, w, bias = DD.exact_head(rows, K, Dc, seed=Dc + K)
        want = DD.patch_logits64(a, w, bias).astype(np.float32)
        assert np.array_equal(want.astype(np.float64), DD.patch_logits64(a, w, bias))           # exact in f32
        lg, lab, bits = _run_op(binding, torch_gpu, a, w, bias, dtype, n, gh, gw, oh, ow)
        tag = (Dc, dtype, n, gh, gw, K)
        assert np.array_equal(_bits(lg[:rows, :K]), _bits(want)), tag
        want_lab, want_bits = DD.labels(want, n, gh, gw, K, oh, ow)
        assert np.array_equal(lab, want_lab) and np.array_equal(bits, want_bits), tag


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("Dc", [64, 192, 768 * 4])
def test_op_on_ordinary_data_under_the_bound(binding, torch_gpu, Dc, dtype):
    """Reference: float64 on the rounded operands, so what is left is the f32 accumulation of Dc products and the bias: at most
    (Dc + 1) 2^-24 (sum |a_i w_i| + |bias|) whatever the order.  The labels are the host function's on the device's own logits, bit for bit."""
    n, gh, gw, oh, ow, K = 3, 5, 7, 40, 56, 150
    rows = n * gh * gw
    rng = np.random.default_rng(Dc + dtype)
    a = Z.ROUND[dtype](rng.standard_normal((rows, Dc)).astype(np.float32))
    w = Z.ROUND[dtype]((rng.standard_normal((K, Dc)) * 0.05).astype(np.float32))
    bias = rng.standard_normal(K).astype(np.float32)
    lg, lab, bits = _run_op(binding, torch_gpu, a, w, bias, dtype, n, gh, gw, oh, ow)
    got = lg[:rows, :K]
    want = DD.patch_logits64(a, w, bias)
    bound = (Dc + 1) * 2.0 ** -24 * (np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T + np.abs(bias)[None, :])
    worst = float((np.abs(got - want) / bound).max())
    print(f"Dc {Dc} dtype {dtype}: max |logit - float64| / bound = {worst:.3e}")
    assert worst <= 1.0
    want_lab, want_sc = binding.dense_labels_host(np.ascontiguousarray(lg[:rows]), n, gh, gw, K, oh, ow)       # the device's own rows, pad columns and all
    assert np.array_equal(lab, want_lab) and np.array_equal(bits, want_sc.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. end to end
MICRO = "vit_micro_patch14_56"
K_E2E = 21


def _family(pkg, family):
    """(model file, context options, images): the synthetic families at the smallest grids they allow."""
    import map_data as MD
    import rect_data as XD
    import rope_data as RD
    if family == "cls":
        return pkg.synth.cached_synthetic(MICRO, head_scale=4.0), {}, PD.exact_images(9, 56, seed=2)
    if family == "registers":
        return pkg.synth.cached_synthetic(MICRO, head_scale=4.0, registers=4), {}, PD.exact_images(9, 56, seed=3)
    if family == "map":
        return MD.fixture_file(pkg), {}, PD.exact_images(9, 56, seed=4)
    if family == "rope":
        return RD.fixture_file(pkg), {}, PD.exact_images(9, 56, seed=5)
    if family == "rect":
        rng = np.random.default_rng(6)
        return XD.fixture_file(pkg, "p14r4"), {"img_shape": (28, 70)}, (rng.integers(-64, 64, (9, 28, 70, 3)) / 16.0).astype(np.float32)
    if family == "tiny4":           # twelve layers: four of them concatenated, the published form
        return pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0), {}, PD.exact_images(3, 224, seed=7)
    raise KeyError(family)


def _head(K, Dc, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((K, Dc)) * 0.25).astype(np.float32), rng.standard_normal(K).astype(np.float32)


E2E = [(f, l, d) for f, l in [("cls", None), ("cls", [0, 1]), ("registers", [0, 1]), ("map", None), ("rope", [0, 1]), ("rect", [1]), ("tiny4", [8, 9, 10, 11])] for d in (0, 1)]
E2E.append(("tiny4", [8, 11], 2))            # a VITX_MXFP8 context: its operand type is bf16, as its head's is


@pytest.mark.parametrize("family,layers,dtype", E2E, ids=[f"{f}-{'last' if l is None else '+'.join(map(str, l))}-{('f16', 'bf16', 'mxfp8')[d]}" for f, l, d in E2E])
def test_forward_end_to_end(pkg, binding, torch_gpu, family, layers, dtype):
    """With VITX_FEAT_TOKENS of the same layers on in the same forward: the kept patch logits equal, bit for bit, vitx_op_dense applied to
    RNE(tokens) concatenated -- the operand IS RNE of the feature -- and lie under the f32 inner-product bound of the float64 product of the rounded
    operands; the labels and scores equal the host function applied to the kept logits."""
    path, opts, imgs = _family(pkg, family)
    n = imgs.shape[0]
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, **opts)
    L_, D = model.hparams.num_hidden_layers, model.hparams.hidden_size
    sel = [L_ - 1] if layers is None else layers
    gh, gw = ctx.grid_hw
    Dc = D * len(sel)
    W, b = _head(K_E2E, Dc, seed=len(sel))
    op_dtype = 1 if dtype == 2 else dtype
    ctx.dense_set(W, b, layers, score=True, logits=True)
    assert ctx.dense_shape() == tuple(ctx.img_shape) and binding.lib().vitx_dense_classes(ctx._h) == K_E2E and binding.lib().vitx_dense_images(ctx._h) == 0
    ctx.feat_enable(cls=False, tokens=True, layers=sel)
    ctx.forward(imgs)
    feats = ctx.feat_read(n)
    lab, score, kept = ctx.dense_read(n)
    oh, ow = ctx.dense_shape()
    assert lab.shape == (n, oh, ow) and kept.shape == (n, gh * gw, K_E2E)
    a = np.concatenate([binding.round_operand(feats[l]["tokens"], op_dtype) for l in sel], axis=2).reshape(n * gh * gw, Dc)
    wr = binding.round_operand(W, op_dtype)
    lg_op, lab_op, bits_op = _run_op(binding, torch_gpu, a, wr, b, op_dtype, n, gh, gw, oh, ow)
    assert np.array_equal(_bits(kept.reshape(-1, K_E2E)), _bits(lg_op[:n * gh * gw, :K_E2E])), "the operand is not RNE(VITX_FEAT_TOKENS)"
    want = DD.patch_logits64(a, wr, b)
    bound = (Dc + 1) * 2.0 ** -24 * (np.abs(a).astype(np.float64) @ np.abs(wr).astype(np.float64).T + np.abs(b)[None, :])
    assert (np.abs(kept.reshape(-1, K_E2E) - want) <= bound).all()
    padded = np.full((n * gh * gw, DD.pad_to(K_E2E)), np.nan, np.float32); padded[:, :K_E2E] = kept.reshape(-1, K_E2E)
    want_lab, want_sc = binding.dense_labels_host(padded, n, gh, gw, K_E2E, oh, ow)
    assert np.array_equal(lab, want_lab) and np.array_equal(_bits(score), want_sc.view(np.uint32))
    assert np.array_equal(lab, lab_op) and np.array_equal(_bits(score), bits_op)
    assert len(np.unique(lab)) > 1, "a label map of one class checks nothing"
    # the device buffer is what read returns
    ptr, shape = ctx.dense_device()
    dev = np.empty((n, oh, ow), np.uint8)
    assert C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(dev.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), dev.nbytes, 2) == 0
    assert shape == (oh, ow) and np.array_equal(dev, lab)
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 4. invariants
def test_invariants(pkg, binding, torch_gpu):
    imgs = Z.images()
    n = Z.N_IMAGES
    model = binding.Model(Z.model_file(pkg, "clip"))
    D = model.hparams.hidden_size
    W, b = _head(K_E2E, D, seed=9)
    W2, b2 = _head(K_E2E, 2 * D, seed=10)
    ref = binding.Context(model, device=0, max_batch=n, dtype=1, last_layer_all_rows=1)
    all_rows = ref.forward(imgs, want_logits=True)
    ref.close()
    ctx = binding.Context(model, device=0, max_batch=n, dtype=1)
    cut = ctx.split(n)
    assert len(cut) == 2
    plain = ctx.forward(imgs, want_logits=True)
    assert ctx.dense_device() == (0, (0, 0)) and ctx.dense_scratch_bytes() == 0

    def run(x):
        p, lg = ctx.forward(x, want_logits=True)
        return ctx.dense_read(x.shape[0]) + (p, lg)

    def same(r, lab, score, kept, rows=slice(None)):
        return np.array_equal(r[0], lab[rows]) and np.array_equal(_bits(r[1]), _bits(score[rows])) and np.array_equal(_bits(r[2]), _bits(kept[rows]))

    ctx.dense_set(W, b, None, out_shape=(61, 75), score=True, logits=True)          # the last layer: every row of it is evaluated
    lab, score, kept, p, lg = run(imgs)
    assert np.array_equal(_bits(p), _bits(all_rows[0])) and np.array_equal(_bits(lg), _bits(all_rows[1])), "not the bits of a last_layer_all_rows = 1 context"
    for i in sorted({0, cut[0] - 1, cut[0], n - 1}):                                 # batch 1; position 3 of a batch of 7 (one sub-batch: another cut)
        assert same(run(imgs[i:i + 1]), lab, score, kept, slice(i, i + 1)), i
        others = [j for j in range(n) if j != i][:6]
        r7 = run(imgs[others[:3] + [i] + others[3:]])
        assert np.array_equal(r7[0][3], lab[i]) and np.array_equal(_bits(r7[1][3]), _bits(score[i])) and np.array_equal(_bits(r7[2][3]), _bits(kept[i])), i
    # a head that leaves the last layer alone leaves the class-rows-only tail alone: the context's own bits
    ctx.dense_set(W, b, [0])
    r0 = run(imgs)
    assert np.array_equal(_bits(r0[3]), _bits(plain[0])) and np.array_equal(_bits(r0[4]), _bits(plain[1])) and r0[1] is None and r0[2] is None
    # a bank, a gallery and a head together: each equals its solo result
    ctx.dense_set(W2, b2, [0, 1], out_shape=(61, 75), score=True, logits=True)
    solo = run(imgs)
    bank = Z.unit_rows(np.random.default_rng(3).standard_normal((24, Z.CLIP_E)))
    gallery = Z.unit_rows(np.random.default_rng(4).standard_normal((40, Z.CLIP_E)))
    ctx.zeroshot_set(bank, Z.SOFTMAX, 100.0, 0.0)
    ctx.nn_set(gallery, 5, binding.NN_LOGITS)
    three = run(imgs)
    zs3, nn3 = ctx.zeroshot_read(n), ctx.nn_read(n)
    assert same(three, *solo[:3]) and np.array_equal(_bits(three[3]), _bits(all_rows[0]))
    ctx.dense_set(None)
    assert ctx.dense_device() == (0, (0, 0)) and ctx.dense_scratch_bytes() == 0 and binding.lib().vitx_dense_classes(ctx._h) == 0
    # (the bank and the gallery read the logits row; with the head off the last layer is class rows only again, so their solo results come from an
    # all-rows context below)
    ctx.zeroshot_set(None); ctx.nn_set(None)
    off = ctx.forward(imgs, want_logits=True)
    assert np.array_equal(_bits(off[0]), _bits(plain[0])) and np.array_equal(_bits(off[1]), _bits(plain[1]))
    ctx.close()
    ctxa = binding.Context(model, device=0, max_batch=n, dtype=1, last_layer_all_rows=1)
    ctxa.zeroshot_set(bank, Z.SOFTMAX, 100.0, 0.0)
    ctxa.nn_set(gallery, 5, binding.NN_LOGITS)
    ctxa.forward(imgs)
    zs1, nn1 = ctxa.zeroshot_read(n), ctxa.nn_read(n)
    assert np.array_equal(_bits(zs3), _bits(zs1)) and np.array_equal(nn3[0], nn1[0]) and np.array_equal(_bits(nn3[1]), _bits(nn1[1]))
    ctxa.close()
    # one stream: the same bits as two
    ctx1 = binding.Context(model, device=0, max_batch=n, dtype=1, streams=1)
    assert len(ctx1.split(n)) == 1
    ctx1.dense_set(W2, b2, [0, 1], out_shape=(61, 75), score=True, logits=True)
    ctx1.forward(imgs)
    assert same(ctx1.dense_read(n), *solo[:3])
    ctx1.close(); model.close()


# ------------------------------------------------------------------------------------------------ 5. behaviour while a head is set
def test_behaviour_while_a_head_is_set(pkg, binding, torch_gpu):
    L = binding.lib()
    imgs = Z.images()[:5]
    model = binding.Model(Z.model_file(pkg, "clip"))
    D = model.hparams.hidden_size
    W, b = _head(K_E2E, D, seed=11)
    ctx = binding.Context(model, device=0, max_batch=5, dtype=1, graph=1)
    ctx.dense_set(W, b, [0])                                   # the last layer is not selected: the forward's bits do not move
    outs = [ctx.forward(imgs) for _ in range(4)]
    assert ctx.graph_launches() == 0, "the graph cache must be bypassed while a head is set"
    first = ctx.dense_read(5)[0]
    s1 = ctx.dense_scratch_bytes()
    assert s1 > 0 and s1 % (_up(5 * 16, 256) * (D * 2 + 128 * 4)) == 0          # per slice: 80 patch rows padded to 256, operand + logit scratch
    # set again: the head is replaced (another K, two layers, another shape), the count of images starts again
    W2, b2 = _head(150, 2 * D, seed=12)
    ctx.dense_set(W2, b2, [0, 1], out_shape=(9, 200), score=True)
    assert (L.vitx_dense_classes(ctx._h), ctx.dense_shape(), L.vitx_dense_images(ctx._h)) == (150, (9, 200), 0)
    with pytest.raises(binding.VitxError) as ei:
        ctx.dense_read()
    assert ei.value.code == binding.ERR_ARG
    ctx.forward(imgs)
    lab2, sc2, none = ctx.dense_read(5)
    assert lab2.shape == (5, 9, 200) and sc2 is not None and none is None and lab2.max() < 150 and len(np.unique(lab2)) > 1
    # the profile: per sub-batch one operand launch per layer, the GEMM, the label kernel
    ctx.profile_enable(True)
    ctx.forward(imgs)
    pr = {e["name"]: e for e in ctx.profile_read()}
    assert pr["dense"]["launches"] == (2 + 1 + 1) * len(ctx.split(5))
    # off: freed, the scratch returns to 0, the graph cache is used again, the forward's bits never moved
    ctx.dense_set(None)
    ctx.forward(imgs)
    assert "dense" not in [e["name"] for e in ctx.profile_read()]
    ctx.profile_enable(False)
    assert ctx.dense_scratch_bytes() == 0 and ctx.dense_device() == (0, (0, 0))
    again = [ctx.forward(imgs) for _ in range(4)]
    assert ctx.graph_launches() >= 1
    for o in outs + again:
        assert np.array_equal(_bits(o), _bits(outs[0]))
    ctx.dense_set(W, b, [0])
    ctx.forward(imgs)
    assert np.array_equal(ctx.dense_read(5)[0], first)
    ctx.close(); model.close()


def test_the_dense_head_takes_one_pass(pkg, binding, torch_gpu):
    """A forward of more images than one pass of the kernels takes is refused while a head is set, before anything runs."""
    torch = torch_gpu
    L = binding.lib()
    model = binding.Model(Z.clip_file(pkg, name="vit_micro_patch8_224"))             # 785 tokens: the F16 parity mode's window holds 3339 images
    big = 3400
    ctx = binding.Context(model, device=0, max_batch=big, dtype=binding.F16, streams=1)
    limit = ctx.split(big)[0]
    assert limit < big
    W, b = _head(2, model.hparams.hidden_size, seed=13)
    ctx.dense_set(W, b, [0], out_shape=(28, 28))
    n = limit + 1
    x = torch.zeros((n, 224, 224, 3), dtype=torch.float32, device="cuda")            # sized for the call: memory-safe even if the check were gone
    p = torch.zeros((n, model.num_classes), dtype=torch.float32, device="cuda")
    assert L.vitx_forward_device(ctx._h, x.data_ptr(), n, p.data_ptr(), None, None) == binding.ERR_ARG
    assert "one pass" in L.vitx_last_error().decode() and L.vitx_dense_images(ctx._h) == 0
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors(pkg, binding, torch_gpu):
    L = binding.lib()
    fp = C.POINTER(C.c_float)
    model = binding.Model(Z.model_file(pkg, "clip"))
    ctx = binding.Context(model, device=0, max_batch=4, dtype=1)
    h = ctx._h
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    D, L_ = model.hparams.hidden_size, model.hparams.num_hidden_layers
    K = 5
    W, b = _head(K, D, seed=14)
    W2, _ = _head(K, 2 * D, seed=15)
    wp, bp, wp2 = W.ctypes.data_as(fp), b.ctypes.data_as(fp), W2.ctypes.data_as(fp)
    assert L.vitx_dense_set(h, None, None, 3, D, 0, 0, 0, 0) == A                       # NULL weights with K > 0
    assert L.vitx_dense_set(h, wp, bp, 0, D, 0, 0, 0, 0) == A and L.vitx_dense_set(h, wp, bp, -1, D, 0, 0, 0, 0) == A       # K < 1
    assert L.vitx_dense_set(h, wp2, bp, K, 2 * D, 0, 0, 0, 0) == A                      # mask 0 = one layer: Dc must be D
    assert L.vitx_dense_set(h, wp, bp, K, D, 3, 0, 0, 0) == A                           # two layers: Dc must be 2 D
    assert L.vitx_dense_set(h, wp, bp, K, D, 1 << L_, 0, 0, 0) == A                     # a layer at L
    assert L.vitx_dense_set(h, wp2, bp, K, 2 * D, (1 << L_) | 1, 0, 0, 0) == A
    assert L.vitx_dense_set(h, wp, bp, K, D, 1, 0, 0, 4) == A and L.vitx_dense_set(h, wp, bp, K, D, 1, 0, 0, -1) == A       # unknown flags
    assert L.vitx_dense_set(h, wp, bp, K, D, 1, 56, 0, 0) == A and L.vitx_dense_set(h, wp, bp, K, D, 1, -56, -56, 0) == A
    for bad in (np.nan, np.inf):
        wb = W.copy(); wb[K - 1, D - 1] = bad
        assert L.vitx_dense_set(h, wb.ctypes.data_as(fp), bp, K, D, 1, 0, 0, 0) == A
        assert "[%d][%d]" % (K - 1, D - 1) in L.vitx_last_error().decode()
        bb = b.copy(); bb[2] = bad
        assert L.vitx_dense_set(h, wp, bb.ctypes.data_as(fp), K, D, 1, 0, 0, 0) == A
    big = np.zeros((257, D), np.float32)
    assert L.vitx_dense_set(h, big.ctypes.data_as(fp), None, 257, D, 1, 0, 0, 0) == U   # K > 256
    assert L.vitx_dense_set(h, wp, bp, K, D, 1, 3, 56, 0) == U and L.vitx_dense_set(h, wp, bp, K, D, 1, 56, 3, 0) == U        # below the 4 x 4 grid
    assert L.vitx_dense_set(h, wp, bp, K, D, 1, 8193, 56, 0) == U and L.vitx_dense_set(h, wp, bp, K, D, 1, 56, 8193, 0) == U
    assert L.vitx_dense_classes(h) == 0 and L.vitx_dense_device(h) is None and L.vitx_dense_scratch_bytes(h) == 0         # nothing above left a head behind
    lab = np.empty((4, 56, 56), np.uint8); sc = np.empty((4, 56, 56), np.float32)
    u8 = C.POINTER(C.c_uint8)
    assert L.vitx_dense_read(h, lab.ctypes.data_as(u8), None, None) == A                # off
    # more than 4 layers needs a deeper file
    m12 = binding.Model(pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0))
    c12 = binding.Context(m12, device=0, max_batch=1, dtype=1)
    w5 = np.zeros((2, 5 * 192), np.float32)
    assert L.vitx_dense_set(c12._h, w5.ctypes.data_as(fp), None, 2, 5 * 192, 0b11111, 0, 0, 0) == A and "at most 4" in L.vitx_last_error().decode()
    c12.close(); m12.close()
    ctx.dense_set(W, b, [1])
    assert L.vitx_dense_read(h, lab.ctypes.data_as(u8), None, None) == A                # before any forward with the head set
    ctx.forward(Z.images()[:3])
    assert L.vitx_dense_images(h) == 3
    assert L.vitx_dense_read(h, None, None, None) == A
    assert L.vitx_dense_read(h, lab.ctypes.data_as(u8), sc.ctypes.data_as(fp), None) == A          # a score without VITX_DENSE_SCORE
    assert L.vitx_dense_read(h, lab.ctypes.data_as(u8), None, sc.ctypes.data_as(fp)) == A          # logits without VITX_DENSE_LOGITS
    assert L.vitx_dense_read(h, lab.ctypes.data_as(u8), None, None) == 0
    ctx.close(); model.close()
    # (the byte window of vitx_dense_set is not reached here: the operand rows are at most 4 D x 2 bytes and the logit rows at most 256 x 4, while the
    # pass itself is bound by the fc1 rows of 4 D x 2 bytes -- a context that leaves the window takes millions of patch rows, gigabytes of staging.
    # The same check of vitx_op_dense, which needs no context, is made in tests/test_cpu_dense.py.)
    # a ViTSTR context
    st = binding.Model(pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0))
    cs = binding.Context(st, device=0, max_batch=1, dtype=0)
    with pytest.raises(binding.VitxError) as ei:
        cs.dense_set(np.zeros((2, 192), np.float32), None, None)
    assert ei.value.code == U and "ViTSTR" in str(ei.value)
    cs.close(); st.close()


def test_a_refused_set_leaves_the_head_in_place(pkg, binding, torch_gpu):
    """A vitx_dense_set that is refused for its arguments (a NaN weight) leaves the head that was set: the next forward gives the same bits."""
    L = binding.lib()
    imgs = Z.images()[:5]
    model = binding.Model(Z.model_file(pkg, "clip"))
    D = model.hparams.hidden_size
    W, b = _head(K_E2E, D, seed=11)
    ctx = binding.Context(model, device=0, max_batch=5, dtype=1)
    ctx.dense_set(W, b, [1], score=True, logits=True)
    ctx.forward(imgs)
    labels, score, logits = ctx.dense_read(5)
    bad = W.copy(); bad[3, 5] = np.nan
    with pytest.raises(binding.VitxError) as ei:
        ctx.dense_set(bad, b, [1], score=True, logits=True)
    assert ei.value.code == binding.ERR_ARG
    ctx.forward(imgs)
    assert L.vitx_dense_images(ctx._h) == 5 and L.vitx_dense_classes(ctx._h) == K_E2E
    labels2, score2, logits2 = ctx.dense_read(5)
    assert np.array_equal(labels2, labels) and np.array_equal(_bits(score2), _bits(score)) and np.array_equal(_bits(logits2), _bits(logits))
    ctx.close(); model.close()
