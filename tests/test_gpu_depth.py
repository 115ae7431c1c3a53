"""The depth head on the MI355X (include/vitx.h "depth estimation"): the two kernels against the host function bit for bit on every shape and on
hostile data, the raw operand rows, the whole op bit for bit on exact data and under the f32 inner-product bound on ordinary data, the forward end
to end on the synthetic families, the invariants (batch, position, cut, streams, last_layer_all_rows, bank + gallery + dense head + depth head),
the behaviour while a head is set and every error.  The restatement is tests/depth_data.py, pinned to the host function and to torch in
tests/test_cpu_depth.py."""
import ctypes as C

import numpy as np
import pytest

import depth_data as XD
import prefix_data as PD
import zs_data as Z

pytestmark = pytest.mark.gpu

TDT = {0: "float16", 1: "bfloat16"}
CAN = -12345.5
LO, HI = float(XD.LO), float(XD.HI)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _up(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ 1. the two kernels on given logits
def _run_kernels(binding, torch, d_lg, ld, d_off, d_bins, n, gh, gw, K, u, oh, ow, shift):
    """Fine plane and depth map between poisoned canaries; shift: floats by which both outputs start off their buffers' 16-byte boundary, so that the
    packed stores and the element-by-element path both run."""
    fpx, px = n * u * gh * u * gw, n * oh * ow
    d_fine = torch.full((16 + shift + fpx + 16,), CAN, dtype=torch.float32, device="cuda")
    d_out = torch.full((16 + shift + px + 16,), CAN, dtype=torch.float32, device="cuda")
    o = 16 + shift
    binding.op_depth_fine(d_lg.data_ptr(), ld, d_off.data_ptr() if d_off is not None else 0, d_bins.data_ptr(), n, gh, gw, K, u, d_fine.data_ptr() + 4 * o)
    binding.op_depth_resize(d_fine.data_ptr() + 4 * o, n, u * gh, u * gw, oh, ow, LO, HI, d_out.data_ptr() + 4 * o)
    torch.cuda.synchronize()
    f, d = d_fine.cpu().numpy(), d_out.cpu().numpy()
    assert (f[:o] == CAN).all() and (f[o + fpx:] == CAN).all(), "a canary of the fine plane was written"
    assert (d[:o] == CAN).all() and (d[o + px:] == CAN).all(), "a canary of the depth map was written"
    return d[o:o + px].view(np.uint32).reshape(n, oh, ow), f[o:o + fpx].view(np.uint32).reshape(n, u * gh, u * gw)


def test_kernels_equal_the_host_function_bit_for_bit(binding, torch_gpu):
    """Every shape of depth_data.cases() on hostile and on ordinary data, ld = K_pad with pad columns of +inf and NaN; with offsets (a row per image)
    and without; the whole batch and its last image alone (a wrong image stride shows); outputs on and off the 16-byte boundary."""
    torch = torch_gpu
    ran = 0
    for i, (gh, gw, u, K, oh, ow, n) in enumerate(XD.cases()):
        ld = XD.pad_to(K)
        for make in (XD.hostile, XD.normal):
            lg, off, bins = make(n, gh, gw, K, ld, seed=i)
            d_bins = torch.from_numpy(bins).cuda()
            for nn_ in sorted({1, n}):
                sub = np.ascontiguousarray(lg.reshape(n, gh * gw, ld)[n - nn_:].reshape(nn_ * gh * gw, ld))
                sub_off = np.ascontiguousarray(off[n - nn_:])
                d_sub, d_off = torch.from_numpy(sub).cuda(), torch.from_numpy(sub_off).cuda()
                for with_off in (True, False) if make is XD.hostile else (True,):
                    want_d, want_f = binding.depth_host(sub, sub_off if with_off else None, bins, nn_, gh, gw, K, u, oh, ow, LO, HI)
                    for shift in (0, 1) if nn_ == n else (1,):
                        d, f = _run_kernels(binding, torch, d_sub, ld, d_off if with_off else None, d_bins, nn_, gh, gw, K, u, oh, ow, shift)
                        tag = (gh, gw, u, K, oh, ow, nn_, make.__name__, with_off, shift)
                        assert np.array_equal(f, _bits(want_f)), tag
                        assert np.array_equal(d, _bits(want_d)), tag
                        ran += 1
    assert ran > 150


def test_kernels_see_the_mutants(binding, torch_gpu):
    """The kernels' result on the mutants' shapes is the unmutated restatement's (which tests/test_cpu_depth.py shows to differ from every mutant)."""
    torch = torch_gpu
    for shape in ((2, 3, 4, 5, 16, 37, 3), (3, 5, 2, 64, 17, 37, 2)):
        gh, gw, u, K, oh, ow, n = shape
        i = XD.cases().index(shape)
        lg, off, bins = XD.hostile(n, gh, gw, K, XD.pad_to(K), seed=i)
        want_d, want_f = XD.depth(lg, off, bins, n, gh, gw, K, u, oh, ow, XD.LO, XD.HI)
        d, f = _run_kernels(binding, torch, torch.from_numpy(lg).cuda(), XD.pad_to(K), torch.from_numpy(off).cuda(), torch.from_numpy(bins).cuda(), n, gh, gw, K, u, oh, ow, 0)
        assert np.array_equal(d, want_d) and np.array_equal(f, want_f)
        for m in XD.MUTANTS:
            if m == "xy_swapped" and gh == 2:
                continue
            assert not np.array_equal(d, XD.depth(lg, off, bins, n, gh, gw, K, u, oh, ow, XD.LO, XD.HI, mutant=m)[0]), m


def test_kernels_take_any_row_stride(binding, torch_gpu):
    """ld above K_pad, and the smallest ld there is (K rounded up to 4): the columns behind K hold NaN and +inf and never reach a sum."""
    torch = torch_gpu
    for (gh, gw, u, K, oh, ow, n, ld) in ((2, 3, 4, 21, 32, 48, 3, 24), (14, 14, 1, 150, 17, 37, 2, 152), (2, 3, 2, 129, 5, 17, 3, 388), (1, 5, 4, 2, 16, 80, 3, 4), (3, 5, 4, 256, 16, 63, 2, 384)):
        lg, off, bins = XD.hostile(n, gh, gw, K, ld, seed=ld)
        want_d, want_f = binding.depth_host(lg, off, bins, n, gh, gw, K, u, oh, ow, LO, HI)
        assert np.array_equal(_bits(want_d), XD.depth(lg, off, bins, n, gh, gw, K, u, oh, ow, XD.LO, XD.HI)[0])
        d, f = _run_kernels(binding, torch, torch.from_numpy(lg).cuda(), ld, torch.from_numpy(off).cuda(), torch.from_numpy(bins).cuda(), n, gh, gw, K, u, oh, ow, 1)
        assert np.array_equal(d, _bits(want_d)) and np.array_equal(f, _bits(want_f)), (gh, gw, u, K, ld)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
def test_raw_rows_are_rounded_to_nearest_even(binding, torch_gpu, dtype):
    """vitx_op_depth_rows with row strides and a column offset: every element RNE of its f32, nothing else written; halfway cases, overflow, NaN."""
    torch = torch_gpu
    rows, D, ldx, ldy, col = 37, 72, 80, 160, 8
    rng = np.random.default_rng(dtype)
    x = (rng.standard_normal((rows, ldx)) * 3).astype(np.float32)
    one = np.float32(1.0)
    ulp = np.float32(2.0 ** -10 if dtype == 0 else 2.0 ** -7)
    x[0, :8] = [one + ulp / 2, one + 3 * ulp / 2, -(one + ulp / 2), np.inf, -np.inf, 1e30, 1e-30, -0.0]      # ties to even, overflow (fp16), tiny values
    d_x = torch.from_numpy(x).cuda()
    tdt = getattr(torch, TDT[dtype])
    d_y = torch.full((rows, ldy), 7.0, dtype=tdt, device="cuda")
    binding.op_depth_rows(dtype, d_x.data_ptr(), ldx, d_y.data_ptr() + 2 * col, ldy, rows, D)
    torch.cuda.synchronize()
    y = d_y.float().cpu().numpy()
    want = d_x[:, :D].to(tdt).float().cpu().numpy()
    assert np.array_equal(_bits(y[:, col:col + D]), _bits(want))
    assert (y[:, :col] == 7.0).all() and (y[:, col + D:] == 7.0).all()
    assert want[0, 0] == 1.0 and want[0, 1] == one + 2 * ulp and want[0, 2] == -1.0              # the halfway cases went to the even neighbour


# ------------------------------------------------------------------------------------------------ 2. the op: operand rows -> GEMMs -> depth
def _run_op(binding, torch, a, acls, wp, wc, bias, bins, dtype, n, gh, gw, u, oh, ow):
    """vitx_op_depth on patch rows a [n gh gw][Dc], class rows acls [n][Dc] or None, the halves wp / wc [K][Dc] (all exact in the operand type), bias
    and bins [K].  The pad rows of both operands and both result buffers start as NaN and +-inf.  Returns logits [M_pad + 1][K_pad], offsets
    [n_pad][K_pad] or None, depth bits, fine bits."""
    rows, Dc = a.shape
    K = wp.shape[0]
    m_pad, n_pad, k_pad = _up(rows, 256), _up(n, 256), _up(K, 128)
    tdt = getattr(torch, TDT[dtype])
    pat = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")], device="cuda")

    def operand(x, pad):
        d = pat.repeat(pad * Dc // 4).reshape(pad, Dc).to(tdt)
        d[:x.shape[0]] = torch.from_numpy(x).cuda().to(tdt)
        assert np.array_equal(d[:x.shape[0]].float().cpu().numpy(), x), "the operand must be exact in the operand type"
        return d

    def matrix(w):
        wb = np.zeros((k_pad, Dc), np.float32); wb[:K] = w
        d = torch.from_numpy(wb).cuda().to(tdt)
        assert np.array_equal(d.float().cpu().numpy(), wb), "the head must be exact in the operand type"
        return d
    d_a, d_wp = operand(a, m_pad), matrix(wp)
    d_ac, d_wc = (operand(acls, n_pad), matrix(wc)) if wc is not None else (None, None)
    bb = np.zeros(k_pad, np.float32); bb[:K] = bias
    d_b, d_bins = torch.from_numpy(bb).cuda(), torch.from_numpy(np.ascontiguousarray(bins, np.float32)).cuda()
    d_lg = pat.repeat((m_pad + 1) * k_pad // 4).reshape(m_pad + 1, k_pad).clone()
    d_off = pat.repeat(n_pad * k_pad // 4).reshape(n_pad, k_pad).clone() if wc is not None else None
    fpx, px = n * u * gh * u * gw, n * oh * ow
    d_fine = torch.full((fpx + 16,), CAN, dtype=torch.float32, device="cuda")
    d_out = torch.full((px + 16,), CAN, dtype=torch.float32, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else 0
    binding.op_depth(dtype, ptr(d_a), ptr(d_wp), ptr(d_ac), ptr(d_wc), ptr(d_b), ptr(d_bins), ptr(d_lg), ptr(d_off), n, gh, gw, K, Dc, u, oh, ow, LO, HI, ptr(d_fine), ptr(d_out))
    torch.cuda.synchronize()
    assert not d_a[rows:].float().cpu().numpy().any(), "the patch operand's pad rows must be written as zeros"
    if wc is not None:
        assert not d_ac[n:].float().cpu().numpy().any(), "the class operand's pad rows must be written as zeros"
    f, d = d_fine.cpu().numpy(), d_out.cpu().numpy()
    assert (f[fpx:] == CAN).all() and (d[px:] == CAN).all()
    return (d_lg.cpu().numpy(), d_off.cpu().numpy() if d_off is not None else None, d[:px].view(np.uint32).reshape(n, oh, ow), f[:fpx].view(np.uint32).reshape(n, u * gh, u * gw))


def _host_of(binding, lg_rows, off_rows, bias, bins, n, gh, gw, K, u, oh, ow):
    """The host function on the device's own logit rows [rows][K_pad] and offsets rows (None: the bias for every image), pad columns and all."""
    k_pad = lg_rows.shape[1]
    if off_rows is None:
        off_rows = np.zeros((n, k_pad), np.float32); off_rows[:, :K] = bias
    return binding.depth_host(np.ascontiguousarray(lg_rows), np.ascontiguousarray(off_rows[:n]), bins, n, gh, gw, K, u, oh, ow, LO, HI)


@pytest.mark.parametrize("cls_half", [True, False], ids=["class", "noclass"])
@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("Dc", [64, 192, 768 * 4])
def test_op_bit_for_bit_on_exact_data(binding, torch_gpu, Dc, dtype, cls_half):
    for (n, gh, gw, u, oh, ow, K) in ((3, 2, 3, 4, 32, 48, 21), (1, 14, 14, 4, 56, 61, 256), (2, 3, 5, 2, 16, 37, 129)):
        rows = n * gh * gw
        a, acls, wp, wc, bias = XD.exact_head(rows, n, K, Dc, seed=Dc + K)
        scale = np.float32(1.0 / 8)                                            # logits of a few units at Dc = 3072; products multiples of 1 / 512: still exact
        wp, wc = wp * scale, wc * scale
        bins = XD.bins_ud(K)
        want_lg = (a.astype(np.float64) @ wp.astype(np.float64).T).astype(np.float32)
        want_off = (bias.astype(np.float64)[None, :] + acls.astype(np.float64) @ wc.astype(np.float64).T).astype(np.float32) if cls_half else np.tile(bias, (n, 1))
        assert np.array_equal(want_lg.astype(np.float64), a.astype(np.float64) @ wp.astype(np.float64).T)       # exact in f32
        lg, off, d, f = _run_op(binding, torch_gpu, a, acls if cls_half else None, wp, wc if cls_half else None, bias, bins, dtype, n, gh, gw, u, oh, ow)
        tag = (Dc, dtype, cls_half, n, gh, gw, K)
        assert np.array_equal(_bits(lg[:rows, :K]), _bits(want_lg)), tag
        if cls_half:
            assert np.array_equal(_bits(off[:n, :K]), _bits(want_off)), tag
        want_d, want_f = XD.depth(want_lg, want_off, bins, n, gh, gw, K, u, oh, ow, XD.LO, XD.HI)
        assert np.array_equal(f, want_f) and np.array_equal(d, want_d), tag
        assert len(np.unique(d)) > 2, "a constant depth map checks nothing"


@pytest.mark.parametrize("cls_half", [True, False], ids=["class", "noclass"])
@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("Dc", [64, 192, 768 * 4])
def test_op_on_ordinary_data_under_the_bound(binding, torch_gpu, Dc, dtype, cls_half):
    """Reference: float64 on the rounded operands, so what is left is the f32 accumulation of Dc products and the bias: at most
    (Dc + 1) 2^-24 (sum |a_i w_i| + |bias|) whatever the order.  The depth is the host function's on the device's own logits and offsets, bit for bit."""
    n, gh, gw, u, oh, ow, K = 3, 5, 7, 4, 40, 56, 150
    rows = n * gh * gw
    rng = np.random.default_rng(Dc + dtype)
    a = Z.ROUND[dtype](rng.standard_normal((rows, Dc)).astype(np.float32))
    acls = Z.ROUND[dtype](rng.standard_normal((n, Dc)).astype(np.float32))
    wp = Z.ROUND[dtype]((rng.standard_normal((K, Dc)) * 0.05).astype(np.float32))
    wc = Z.ROUND[dtype]((rng.standard_normal((K, Dc)) * 0.05).astype(np.float32))
    bias = rng.standard_normal(K).astype(np.float32)
    bins = XD.bins_ud(K)
    lg, off, d, f = _run_op(binding, torch_gpu, a, acls if cls_half else None, wp, wc if cls_half else None, bias, bins, dtype, n, gh, gw, u, oh, ow)
    f64 = lambda x: x.astype(np.float64)
    worst = float((np.abs(lg[:rows, :K] - f64(a) @ f64(wp).T) / ((Dc + 1) * 2.0 ** -24 * (np.abs(f64(a)) @ np.abs(f64(wp)).T))).max())
    print(f"Dc {Dc} dtype {dtype}: max |logit - float64| / bound = {worst:.3e}")
    assert worst <= 1.0
    if cls_half:
        bound = (Dc + 1) * 2.0 ** -24 * (np.abs(f64(acls)) @ np.abs(f64(wc)).T + np.abs(bias)[None, :])
        worst = float((np.abs(off[:n, :K] - (f64(acls) @ f64(wc).T + f64(bias)[None, :])) / bound).max())
        print(f"Dc {Dc} dtype {dtype}: max |offset - float64| / bound = {worst:.3e}")
        assert worst <= 1.0
    want_d, want_f = _host_of(binding, lg[:rows], off, bias, bins, n, gh, gw, K, u, oh, ow)
    assert np.array_equal(f, _bits(want_f)) and np.array_equal(d, _bits(want_d))


# ------------------------------------------------------------------------------------------------ 3. end to end
MICRO = "vit_micro_patch14_56"
K_E2E = 21


def _family(pkg, family):
    """(model file, images): the synthetic families at the smallest grids they allow."""
    if family == "cls":
        return pkg.synth.cached_synthetic(MICRO, head_scale=4.0), PD.exact_images(9, 56, seed=2)
    if family == "registers":
        return pkg.synth.cached_synthetic(MICRO, head_scale=4.0, registers=4), PD.exact_images(9, 56, seed=3)
    if family == "tiny4":           # twelve layers: four of them concatenated, the published form
        return pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0), PD.exact_images(3, 224, seed=7)
    if family == "tiny4reg":
        return pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0, registers=4), PD.exact_images(3, 224, seed=8)
    raise KeyError(family)


def _head(K, Dc, seed, scale=0.05):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((K, Dc)) * scale).astype(np.float32), (rng.standard_normal((K, Dc)) * scale).astype(np.float32),
            rng.standard_normal(K).astype(np.float32), XD.bins_ud(K))


E2E = [(f, l, d, nm) for f, l in [("cls", None), ("registers", [0, 1]), ("tiny4", [2, 5, 8, 11]), ("tiny4reg", [8, 11])] for d in (0, 1) for nm in (False, True)]
E2E += [("tiny4", [2, 11], 2, False), ("tiny4", None, 2, True)]            # VITX_MXFP8 contexts (no register tokens): their operand type is bf16


@pytest.mark.parametrize("family,layers,dtype,norm", E2E,
                         ids=[f"{f}-{'last' if l is None else '+'.join(map(str, l))}-{('f16', 'bf16', 'mxfp8')[d]}-{'norm' if nm else 'raw'}" for f, l, d, nm in E2E])
def test_forward_end_to_end(pkg, binding, torch_gpu, family, layers, dtype, norm):
    """With VITX_DEPTH_LOGITS: the kept patch logits and offsets lie under the f32 inner-product bound of the float64 products of RNE(features) x
    RNE(W) -- the features being VITX_FEAT_TOKENS / VITX_FEAT_CLS of the same forward (normed) or the residual stream of vitx_trace_read (raw) -- and
    the depth map and the fine plane equal the host function applied to the kept logits and offsets, bit for bit."""
    path, imgs = _family(pkg, family)
    n = imgs.shape[0]
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype)
    L_, D = model.hparams.num_hidden_layers, model.hparams.hidden_size
    sel = [L_ - 1] if layers is None else layers
    gh, gw = ctx.grid_hw
    Np, T, Dc, u = gh * gw, ctx.prefix, D * len(sel), 4
    wp, wc, bias, bins = _head(K_E2E, Dc, seed=len(sel), scale=0.25 if norm else 0.05)
    op_dtype = 1 if dtype == 2 else dtype
    lo, hi = 3.0, 7.0
    ctx.depth_set(wp, wc, bias, bins, layers, u, lo, hi, norm=norm, logits=True, fine=True)
    oh, ow = ctx.img_shape
    assert ctx.depth_shape() == (oh, ow, u * gh, u * gw) and binding.lib().vitx_depth_bins(ctx._h) == K_E2E and binding.lib().vitx_depth_images(ctx._h) == 0
    if norm:
        ctx.feat_enable(cls=True, tokens=True, layers=sel)
        ctx.forward(imgs)
        feats = ctx.feat_read(n)
        rows = [feats[l]["tokens"] for l in sel]; crow = [feats[l]["cls"] for l in sel]
    else:
        ctx.trace_enable(list(range(n)))
        ctx.forward(imgs)
        tr = ctx.trace_read()
        rows = [tr[l + 1][:, T:, :] for l in sel]; crow = [tr[l + 1][:, 0, :] for l in sel]
    depth, fine, kept, koff = ctx.depth_read(n)
    assert depth.shape == (n, oh, ow) and fine.shape == (n, u * gh, u * gw) and kept.shape == (n, Np, K_E2E) and koff.shape == (n, K_E2E)
    f64 = lambda x: x.astype(np.float64)
    a = np.concatenate([binding.round_operand(r, op_dtype) for r in rows], axis=2).reshape(n * Np, Dc)
    ac = np.concatenate([binding.round_operand(r, op_dtype) for r in crow], axis=1)
    wpr, wcr = binding.round_operand(wp, op_dtype), binding.round_operand(wc, op_dtype)
    bound = (Dc + 1) * 2.0 ** -24 * (np.abs(f64(a)) @ np.abs(f64(wpr)).T)
    assert (np.abs(kept.reshape(-1, K_E2E) - f64(a) @ f64(wpr).T) <= bound).all(), "the patch logits are not the products of RNE(features) x RNE(Wp)"
    bound = (Dc + 1) * 2.0 ** -24 * (np.abs(f64(ac)) @ np.abs(f64(wcr)).T + np.abs(bias)[None, :])
    assert (np.abs(koff - (f64(ac) @ f64(wcr).T + f64(bias)[None, :])) <= bound).all(), "the offsets are not bias + RNE(class features) x RNE(Wc)"
    k_pad = XD.pad_to(K_E2E)
    lgp = np.full((n * Np, k_pad), np.nan, np.float32); lgp[:, :K_E2E] = kept.reshape(-1, K_E2E)
    ofp = np.full((n, k_pad), np.nan, np.float32); ofp[:, :K_E2E] = koff
    want_d, want_f = binding.depth_host(lgp, ofp, bins, n, gh, gw, K_E2E, u, oh, ow, lo, hi)
    assert np.array_equal(_bits(fine), _bits(want_f)) and np.array_equal(_bits(depth), _bits(want_d))
    assert len(np.unique(depth)) > 2 and np.isfinite(depth).all() and depth.min() >= lo and depth.max() <= hi
    # the device buffer is what read returns
    ptr, shape = ctx.depth_device()
    dev = np.empty((n, oh, ow), np.float32)
    assert C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(dev.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), dev.nbytes, 2) == 0
    assert shape == (oh, ow) and np.array_equal(_bits(dev), _bits(depth))
    ctx.close(); model.close()


def test_a_head_without_a_class_half_on_a_map_file(pkg, binding, torch_gpu):
    """No class token (VITX_POOL_MAP): a class half is VITX_ERR_UNSUPPORTED; without one the offsets are the bias and the patch rows start at row 0."""
    import map_data as MD
    imgs = PD.exact_images(5, 56, seed=4)
    model = binding.Model(MD.fixture_file(pkg))
    ctx = binding.Context(model, device=0, max_batch=5, dtype=1)
    D = model.hparams.hidden_size
    wp, wc, bias, bins = _head(K_E2E, D, seed=21, scale=0.25)
    with pytest.raises(binding.VitxError) as ei:
        ctx.depth_set(wp, wc, bias, bins, None, 4, 3.0, 7.0)
    assert ei.value.code == binding.ERR_UNSUPPORTED and "class token" in str(ei.value) and ctx.depth_scratch_bytes() == 0
    ctx.depth_set(wp, None, bias, bins, None, 4, 3.0, 7.0, norm=True, logits=True, fine=True)
    ctx.feat_enable(cls=False, tokens=True)
    ctx.forward(imgs)
    gh, gw = ctx.grid_hw
    tok = ctx.feat_read(5)[model.hparams.num_hidden_layers - 1]["tokens"]
    depth, fine, kept, koff = ctx.depth_read(5)
    assert np.array_equal(_bits(koff), _bits(np.tile(bias, (5, 1))))
    a, wr = binding.round_operand(tok, 1).reshape(5 * gh * gw, D).astype(np.float64), binding.round_operand(wp, 1).astype(np.float64)
    assert (np.abs(kept.reshape(-1, K_E2E) - a @ wr.T) <= (D + 1) * 2.0 ** -24 * (np.abs(a) @ np.abs(wr).T)).all()
    want_d, want_f = binding.depth_host(np.ascontiguousarray(np.pad(kept.reshape(-1, K_E2E), ((0, 0), (0, 3)))), np.ascontiguousarray(np.pad(koff, ((0, 0), (0, 3)))), bins, 5, gh, gw,
                                        K_E2E, 4, *ctx.img_shape, 3.0, 7.0)
    assert np.array_equal(_bits(depth), _bits(want_d)) and np.array_equal(_bits(fine), _bits(want_f))
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 4. invariants
def test_invariants(pkg, binding, torch_gpu):
    imgs = Z.images()
    n = Z.N_IMAGES
    model = binding.Model(Z.model_file(pkg, "clip"))
    D = model.hparams.hidden_size
    wp, wc, bias, bins = _head(K_E2E, D, seed=9)
    wp2, wc2, bias2, bins2 = _head(K_E2E, 2 * D, seed=10)
    ref = binding.Context(model, device=0, max_batch=n, dtype=1, last_layer_all_rows=1)
    all_rows = ref.forward(imgs, want_logits=True)
    ref.close()
    ctx = binding.Context(model, device=0, max_batch=n, dtype=1)
    cut = ctx.split(n)
    assert len(cut) == 2
    plain = ctx.forward(imgs, want_logits=True)
    assert ctx.depth_device() == (0, (0, 0)) and ctx.depth_scratch_bytes() == 0

    def run(x):
        p, lg = ctx.forward(x, want_logits=True)
        return ctx.depth_read(x.shape[0]) + (p, lg)

    def same(r, ref_, rows=slice(None)):
        return all(np.array_equal(_bits(r[j]), _bits(ref_[j][rows])) for j in range(4))

    ctx.depth_set(wp, wc, bias, bins, None, 4, 3.0, 7.0, out_shape=(61, 75), logits=True, fine=True)      # the last layer: every row of it is evaluated
    full = run(imgs)
    assert np.array_equal(_bits(full[4]), _bits(all_rows[0])) and np.array_equal(_bits(full[5]), _bits(all_rows[1])), "not the bits of a last_layer_all_rows = 1 context"
    assert len(np.unique(full[0])) > 2
    for i in sorted({0, cut[0] - 1, cut[0], n - 1}):                                 # batch 1; position 3 of a batch of 7 (one sub-batch: another cut)
        assert same(run(imgs[i:i + 1]), full, slice(i, i + 1)), i
        others = [j for j in range(n) if j != i][:6]
        r7 = run(imgs[others[:3] + [i] + others[3:]])
        assert all(np.array_equal(_bits(r7[j][3]), _bits(full[j][i])) for j in range(4)), i
    # a head that leaves the last layer alone leaves the class-rows-only tail alone: the context's own bits
    ctx.depth_set(wp, wc, bias, bins, [0], 2, 3.0, 7.0)
    r0 = run(imgs)
    assert np.array_equal(_bits(r0[4]), _bits(plain[0])) and np.array_equal(_bits(r0[5]), _bits(plain[1])) and r0[1] is None and r0[2] is None and r0[3] is None
    # a bank, a gallery, a dense head and a depth head together: each equals its solo result
    ctx.depth_set(wp2, wc2, bias2, bins2, [0, 1], 4, 3.0, 7.0, out_shape=(61, 75), logits=True, fine=True)
    solo = run(imgs)
    ctx.depth_set(None)
    dw = (np.random.default_rng(5).standard_normal((K_E2E, 2 * D)) * 0.25).astype(np.float32)
    ctx.dense_set(dw, bias2, [0, 1], out_shape=(61, 75), score=True, logits=True)
    ctx.forward(imgs)
    dense_solo = ctx.dense_read(n)
    ctx.depth_set(wp2, wc2, bias2, bins2, [0, 1], 4, 3.0, 7.0, out_shape=(61, 75), logits=True, fine=True)
    bank = Z.unit_rows(np.random.default_rng(3).standard_normal((24, Z.CLIP_E)))
    gallery = Z.unit_rows(np.random.default_rng(4).standard_normal((40, Z.CLIP_E)))
    ctx.zeroshot_set(bank, Z.SOFTMAX, 100.0, 0.0)
    ctx.nn_set(gallery, 5, binding.NN_LOGITS)
    four = run(imgs)
    zs4, nn4, dn4 = ctx.zeroshot_read(n), ctx.nn_read(n), ctx.dense_read(n)
    assert same(four, solo) and np.array_equal(_bits(four[4]), _bits(all_rows[0]))
    assert np.array_equal(dn4[0], dense_solo[0]) and np.array_equal(_bits(dn4[1]), _bits(dense_solo[1])) and np.array_equal(_bits(dn4[2]), _bits(dense_solo[2]))
    ctx.depth_set(None)
    assert ctx.depth_device() == (0, (0, 0)) and ctx.depth_scratch_bytes() == 0 and binding.lib().vitx_depth_bins(ctx._h) == 0
    ctx.forward(imgs)
    dn3 = ctx.dense_read(n)
    assert np.array_equal(dn3[0], dense_solo[0]) and np.array_equal(_bits(dn3[1]), _bits(dense_solo[1]))
    ctx.dense_set(None); ctx.zeroshot_set(None); ctx.nn_set(None)
    off = ctx.forward(imgs, want_logits=True)
    assert np.array_equal(_bits(off[0]), _bits(plain[0])) and np.array_equal(_bits(off[1]), _bits(plain[1]))
    ctx.close()
    ctxa = binding.Context(model, device=0, max_batch=n, dtype=1, last_layer_all_rows=1)
    ctxa.zeroshot_set(bank, Z.SOFTMAX, 100.0, 0.0)
    ctxa.nn_set(gallery, 5, binding.NN_LOGITS)
    ctxa.forward(imgs)
    zs1, nn1 = ctxa.zeroshot_read(n), ctxa.nn_read(n)
    assert np.array_equal(_bits(zs4), _bits(zs1)) and np.array_equal(nn4[0], nn1[0]) and np.array_equal(_bits(nn4[1]), _bits(nn1[1]))
    ctxa.close()
    # one stream: the same bits as two
    ctx1 = binding.Context(model, device=0, max_batch=n, dtype=1, streams=1)
    assert len(ctx1.split(n)) == 1
    ctx1.depth_set(wp2, wc2, bias2, bins2, [0, 1], 4, 3.0, 7.0, out_shape=(61, 75), logits=True, fine=True)
    ctx1.forward(imgs)
    assert same(ctx1.depth_read(n), solo)
    ctx1.close(); model.close()


# ------------------------------------------------------------------------------------------------ 5. behaviour while a head is set
def test_behaviour_while_a_head_is_set(pkg, binding, torch_gpu):
    L = binding.lib()
    imgs = Z.images()[:5]
    model = binding.Model(Z.model_file(pkg, "clip"))
    D = model.hparams.hidden_size
    wp, wc, bias, bins = _head(K_E2E, D, seed=11)
    ctx = binding.Context(model, device=0, max_batch=5, dtype=1, graph=1)
    ctx.depth_set(wp, wc, bias, bins, [0], 4, 3.0, 7.0)          # the last layer is not selected: the forward's bits do not move
    outs = [ctx.forward(imgs) for _ in range(4)]
    assert ctx.graph_launches() == 0, "the graph cache must be bypassed while a head is set"
    first = ctx.depth_read(5)[0]
    s1 = ctx.depth_scratch_bytes()
    per_slice = _up(5 * 16, 256) * (D * 2 + 128 * 4) + 256 * (D * 2 + 128 * 4)          # 80 patch rows and the class rows, each padded to 256: operand + f32 scratch
    assert s1 > 0 and s1 % per_slice == 0
    # set again: the head is replaced (another K, two layers, no class half, another shape), the count of images starts again
    wp2, _, bias2, bins2 = _head(150, 2 * D, seed=12)
    ctx.depth_set(wp2, None, bias2, bins2, [0, 1], 2, 1.0, 9.0, out_shape=(9, 200), norm=True)
    assert (L.vitx_depth_bins(ctx._h), ctx.depth_shape(), L.vitx_depth_images(ctx._h)) == (150, (9, 200, 8, 8), 0)
    with pytest.raises(binding.VitxError) as ei:
        ctx.depth_read()
    assert ei.value.code == binding.ERR_ARG
    ctx.forward(imgs)
    d2, f2, lg2, off2 = ctx.depth_read(5)
    assert d2.shape == (5, 9, 200) and f2 is None and lg2 is None and off2 is None and d2.min() >= 1.0 and d2.max() <= 9.0 and len(np.unique(d2)) > 2
    # the profile: per sub-batch one operand launch per layer, the GEMM, the two kernels -- every launch of the feature is class "depth"
    ctx.profile_enable(True)
    ctx.forward(imgs)
    pr = {e["name"]: e for e in ctx.profile_read()}
    assert pr["depth"]["launches"] == (2 + 1 + 2) * len(ctx.split(5))
    ctx.depth_set(wp, wc, bias, bins, [0], 4, 3.0, 7.0)          # with a class half: one more GEMM
    ctx.forward(imgs)
    pr = {e["name"]: e for e in ctx.profile_read()}
    assert pr["depth"]["launches"] == (2 + 2 + 2) * len(ctx.split(5))          # patch rows, class rows; two GEMMs; two kernels
    # off: freed, the scratch returns to 0, no "depth" class, the graph cache is used again, the forward's bits never moved
    ctx.depth_set(None)
    ctx.forward(imgs)
    assert "depth" not in [e["name"] for e in ctx.profile_read()]
    ctx.profile_enable(False)
    assert ctx.depth_scratch_bytes() == 0 and ctx.depth_device() == (0, (0, 0))
    again = [ctx.forward(imgs) for _ in range(4)]
    assert ctx.graph_launches() >= 1
    for o in outs + again:
        assert np.array_equal(_bits(o), _bits(outs[0]))
    ctx.depth_set(wp, wc, bias, bins, [0], 4, 3.0, 7.0)
    ctx.forward(imgs)
    assert np.array_equal(_bits(ctx.depth_read(5)[0]), _bits(first))
    ctx.close(); model.close()


def test_the_depth_head_takes_one_pass(pkg, binding, torch_gpu):
    """A forward of more images than one pass of the kernels takes is refused while a head is set, before anything runs."""
    torch = torch_gpu
    L = binding.lib()
    model = binding.Model(Z.clip_file(pkg, name="vit_micro_patch8_224"))             # 785 tokens: the F16 parity mode's window holds 3339 images
    big = 3400
    ctx = binding.Context(model, device=0, max_batch=big, dtype=binding.F16, streams=1)
    limit = ctx.split(big)[0]
    assert limit < big
    wp, _, bias, bins = _head(2, model.hparams.hidden_size, seed=13)
    ctx.depth_set(wp, None, bias, bins, [0], 1, 1.0, 9.0, out_shape=(28, 28))
    n = limit + 1
    x = torch.zeros((n, 224, 224, 3), dtype=torch.float32, device="cuda")            # sized for the call: memory-safe even if the check were gone
    p = torch.zeros((n, model.num_classes), dtype=torch.float32, device="cuda")
    assert L.vitx_forward_device(ctx._h, x.data_ptr(), n, p.data_ptr(), None, None) == binding.ERR_ARG
    assert "one pass" in L.vitx_last_error().decode() and L.vitx_depth_images(ctx._h) == 0
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors(pkg, binding, torch_gpu):
    L = binding.lib()
    fp, cf = C.POINTER(C.c_float), C.c_float
    model = binding.Model(Z.model_file(pkg, "clip"))
    ctx = binding.Context(model, device=0, max_batch=4, dtype=1)
    h = ctx._h
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    D, L_ = model.hparams.hidden_size, model.hparams.num_hidden_layers
    K = 5
    wp, wc, b, bins = _head(K, D, seed=14)
    wp2 = _head(K, 2 * D, seed=15)[0]
    P = lambda x: x.ctypes.data_as(fp) if x is not None else None

    def ds(Wp=wp, Wc=wc, bias=b, bn=bins, K_=K, Dc=D, mask=1, u=4, lo=1.0, hi=9.0, oh=0, ow=0, flags=0):
        return L.vitx_depth_set(h, P(Wp), P(Wc), P(bias), P(bn), K_, Dc, mask, u, cf(lo), cf(hi), oh, ow, flags)
    assert ds(Wp=None, K_=3) == A and ds(bn=None) == A                       # NULL weights with K > 0, NULL bins
    assert ds(K_=0) == A and ds(K_=-1) == A                                  # K < 1
    assert ds(Wp=wp2, Wc=None, Dc=2 * D, mask=0) == A                         # mask 0 = one layer: Dc must be D
    assert ds(mask=3) == A                                                   # two layers: Dc must be 2 D
    assert ds(mask=1 << L_) == A and ds(Wp=wp2, Wc=None, Dc=2 * D, mask=(1 << L_) | 1) == A       # a layer at L
    assert ds(flags=8) == A and ds(flags=-1) == A                            # unknown flags
    assert ds(oh=56) == A and ds(oh=-56, ow=-56) == A                        # one side 0, negative sides
    assert ds(lo=9.5) == A and ds(lo=float("nan")) == A and ds(hi=float("inf")) == A
    for bad in (np.nan, np.inf):
        for which in ("Wp", "Wc"):
            w = (wp if which == "Wp" else wc).copy(); w[K - 1, D - 1] = bad
            assert ds(**{which: w}) == A and "[%d][%d]" % (K - 1, D - 1) in L.vitx_last_error().decode()
        bb = b.copy(); bb[2] = bad
        assert ds(bias=bb) == A
        bn = bins.copy(); bn[3] = bad
        assert ds(bn=bn) == A
    for bad in (0.0, -1.0):                                                  # a bin <= 0
        bn = bins.copy(); bn[0] = bad
        assert ds(bn=bn) == A and "bin [0]" in L.vitx_last_error().decode()
    big = np.zeros((257, D), np.float32); bigb = np.ones(257, np.float32)
    assert ds(Wp=big, Wc=None, bias=None, bn=bigb, K_=257) == U              # K > 256
    assert ds(u=3) == U and ds(u=0) == U and ds(u=8) == U                    # u not in {1, 2, 4}
    assert ds(oh=15, ow=56) == U and ds(oh=56, ow=15) == U                   # below the 16 x 16 fine plane of the 4 x 4 grid
    assert ds(oh=15, ow=56, u=2) == 0 and ds(Wp=None, Wc=None, bias=None, bn=None, K_=0, Dc=0, mask=0) == 0      # ... which u = 2 fits; then off
    assert ds(oh=8193, ow=56) == U and ds(oh=56, ow=8193) == U
    assert L.vitx_depth_bins(h) == 0 and L.vitx_depth_device(h) is None and L.vitx_depth_scratch_bytes(h) == 0          # nothing above left a head behind
    dep = np.empty((4, 56, 56), np.float32); sc = np.empty((4, 16 * 16 * 16), np.float32)
    assert L.vitx_depth_read(h, P(dep), None, None, None) == A               # off
    # more than 4 layers needs a deeper file
    m12 = binding.Model(pkg.synth.cached_synthetic("vit_tiny_patch16_224", head_scale=4.0))
    c12 = binding.Context(m12, device=0, max_batch=1, dtype=1)
    w5 = np.zeros((2, 5 * 192), np.float32)
    assert L.vitx_depth_set(c12._h, P(w5), None, None, P(np.ones(2, np.float32)), 2, 5 * 192, 0b11111, 4, cf(1.0), cf(2.0), 0, 0, 0) == A and "at most 4" in L.vitx_last_error().decode()
    c12.close(); m12.close()
    ctx.depth_set(wp, wc, b, bins, [1], 4, 1.0, 9.0)
    assert L.vitx_depth_read(h, P(dep), None, None, None) == A               # before any forward with the head set
    ctx.forward(Z.images()[:3])
    assert L.vitx_depth_images(h) == 3
    assert L.vitx_depth_read(h, None, None, None, None) == A
    assert L.vitx_depth_read(h, P(dep), P(sc), None, None) == A              # the fine plane without VITX_DEPTH_FINE
    assert L.vitx_depth_read(h, P(dep), None, P(sc), None) == A and L.vitx_depth_read(h, P(dep), None, None, P(sc)) == A      # logits / offsets without VITX_DEPTH_LOGITS
    assert L.vitx_depth_read(h, P(dep), None, None, None) == 0
    ctx.close(); model.close()
    # (the byte window of vitx_depth_set is not reached here, as with vitx_dense_set: the pass itself is bound by the fc1 rows first.  The same check
    # of vitx_op_depth, which needs no context, is made in tests/test_cpu_depth.py.)
    # a ViTSTR context
    st = binding.Model(pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0))
    cs = binding.Context(st, device=0, max_batch=1, dtype=0)
    with pytest.raises(binding.VitxError) as ei:
        cs.depth_set(np.zeros((2, 192), np.float32), None, None, np.ones(2, np.float32))
    assert ei.value.code == U and "ViTSTR" in str(ei.value)
    cs.close(); st.close()


def test_a_refused_set_leaves_the_head_in_place(pkg, binding, torch_gpu):
    """A vitx_depth_set that is refused for its arguments (upsample = 3) leaves the head that was set: the next forward gives the same bits."""
    L = binding.lib()
    imgs = Z.images()[:5]
    model = binding.Model(Z.model_file(pkg, "clip"))
    D = model.hparams.hidden_size
    wp, wc, bias, bins = _head(K_E2E, D, seed=11)
    ctx = binding.Context(model, device=0, max_batch=5, dtype=1)
    ctx.depth_set(wp, wc, bias, bins, [1], 4, 3.0, 7.0, logits=True, fine=True)
    ctx.forward(imgs)
    first = ctx.depth_read(5)
    with pytest.raises(binding.VitxError) as ei:
        ctx.depth_set(wp, wc, bias, bins, [1], 3, 3.0, 7.0, logits=True, fine=True)
    assert ei.value.code == binding.ERR_UNSUPPORTED
    ctx.forward(imgs)
    assert L.vitx_depth_images(ctx._h) == 5 and L.vitx_depth_bins(ctx._h) == K_E2E
    again = ctx.depth_read(5)
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a), _bits(b))
    ctx.close(); model.close()
