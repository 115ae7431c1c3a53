"""The three rollout kernels on their own (vitx_op_rollout_factor, vitx_op_rollout_step, vitx_op_rollout_row; attention_map.hip), element for
element.  Data, mutants and bounds: tests/rollout_data.py; the conditions these tests rest on are proven by tests/test_cpu_rollout_data.py:

  * exact data (small integers over a power of two) has ONE correct f32 result in any summation order: whole buffers are compared bit for
    bit, at token counts on both sides of every build edge of the step kernel, with every N % 4, and each of nine faults of a tiled in-place
    product (dropped K tail, unwritten last row block / column group, transposed or swapped operands, another image's r, the in-place
    hazard, missing zero padding) changes at least one element of the expected buffer of every case where it can occur;
  * ordinary data (non-negative row-stochastic factors with peaked rows) is held to the componentwise bound of an f32 inner product,
    N 2^-23 (|a| . |r|)_ij -- no figure is taken from the kernels; an f32 evaluation of the definition needs less than half of it;
  * every output is allocated with a NaN image (or NaN gaps) behind it that must keep its bits, and every read-only operand must keep its.

Every buffer a kernel may address is allocated in full, also in the argument-check test."""
import numpy as np
import pytest

import exact_data as X
import rollout_data as R

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = 3, 5


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(torch, t):
    return t.contiguous().view(torch.int32)


def _nan_tail(torch, a, extra=1):
    """a [n][...] on the device with `extra` images of NaN behind it: ([n + extra][...], the view of the first n)."""
    buf = torch.full((a.shape[0] + extra,) + tuple(a.shape[1:]), float("nan"), dtype=torch.float32, device="cuda")
    buf[:a.shape[0]] = _dev(torch, a)
    return buf


def _same_bits(torch, got, want, what):
    """Whole-buffer bit comparison that names the first differing element."""
    g, w = _bits(torch, got), _bits(torch, want)
    if torch.equal(g, w):
        return
    idx = (g != w).nonzero()
    first = tuple(int(v) for v in idx[0])
    raise AssertionError(f"{what}: {idx.shape[0]} of {g.numel()} elements differ, the first at {first}: got {float(got[first])!r}, expected {float(want[first])!r}")


# ------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("N", R.STEP_N)
def test_step_on_exact_data_is_the_product_bit_for_bit(binding, torch_gpu, N):
    """a <- a . r on rollout_data.step_exact: the whole a buffer is the one correct product, the NaN image behind it and all of r keep
    their bits.  Then the forward's ping-pong: fresh data with the two buffers' roles exchanged is exact as well."""
    torch = torch_gpu
    n = R.n_images(N)
    nan = torch.full((1, N, N), float("nan"), dtype=torch.float32, device="cuda")
    bufs = [torch.empty((n + 1, N, N), dtype=torch.float32, device="cuda") for _ in range(2)]
    for launch in (0, 1):
        a, r, exp = R.step_exact(N, seed=launch)
        ab, rb = bufs[launch], bufs[1 - launch]
        ab[:n] = _dev(torch, a); rb[:n] = _dev(torch, r); ab[n:] = nan; rb[n:] = nan
        r_before = rb.clone()
        binding.op_rollout_step(ab.data_ptr(), rb.data_ptr(), n, N)
        torch.cuda.synchronize()
        _same_bits(torch, ab[:n], _dev(torch, exp), f"N {N} launch {launch}: a . r")
        assert torch.equal(ab[:n], _dev(torch, exp))
        _same_bits(torch, ab[n:], nan, f"N {N} launch {launch}: the image behind a")
        _same_bits(torch, rb, r_before, f"N {N} launch {launch}: r")


@pytest.mark.parametrize("N", R.STEP_ORDINARY_N)
def test_step_on_ordinary_factors_within_the_inner_product_bound(binding, torch_gpu, N):
    """|got - ref64| <= N 2^-23 (|a| . |r|)_ij (rollout_data.step_bound), ref64 the float64 product of the same f32 operands computed on the
    device; and image 1 launched alone has the bits it has in the batch.  Measured ratios: DESIGN.md section 3."""
    torch = torch_gpu
    n = R.n_images(N)
    f, r0 = R.step_ordinary(N)
    a, r = _nan_tail(torch, f[0]), _nan_tail(torch, r0)
    a1, r1 = a[1:2].clone(), r[1:2].clone()
    ref = a[:n].double() @ r[:n].double()
    bound = R.step_bound(N, a[:n].double().abs() @ r[:n].double().abs())
    r_before = r.clone()
    binding.op_rollout_step(a.data_ptr(), r.data_ptr(), n, N)
    binding.op_rollout_step(a1.data_ptr(), r1.data_ptr(), 1, N)
    torch.cuda.synchronize()
    ratio = float(((a[:n].double() - ref).abs() / bound).max())
    print(f"ROLLOUT_GATE step N {N} images {n}: worst ratio {ratio:.4f} of N 2^-23 (|a| . |r|)")
    assert ratio <= 1.0, (N, ratio)
    assert torch.isnan(a[n:]).all()
    _same_bits(torch, r, r_before, f"N {N}: r")
    _same_bits(torch, a1[0], a[1], f"N {N}: image 1 alone against image 1 in the batch of {n}")


@pytest.mark.parametrize("N", [122, 577])
def test_chain_of_four_steps_within_four_times_the_bound(binding, torch_gpu, N):
    """R_l = A^_l . R_(l-1), l = 1 .. 4, each in place over its factor as the forward chains them: within 4 N 2^-23 of the float64 chain,
    relative to the product of the absolute values (the chain itself: nothing is negative)."""
    torch = torch_gpu
    n = R.n_images(N)
    f, r0 = R.step_ordinary(N, steps=4)
    cur = _dev(torch, r0)
    ref, absref = cur.double(), cur.double().abs()
    for l in range(4):
        a = _dev(torch, f[l])
        ref, absref = a.double() @ ref, a.double().abs() @ absref
        binding.op_rollout_step(a.data_ptr(), cur.data_ptr(), n, N)
        cur = a
    torch.cuda.synchronize()
    ratio = float(((cur.double() - ref).abs() / (4 * R.step_bound(N, absref))).max())
    print(f"ROLLOUT_GATE chain of 4 N {N} images {n}: worst ratio {ratio:.4f} of 4 N 2^-23 |A4| |A3| |A2| |A1| |R0|")
    assert ratio <= 1.0, (N, ratio)
    assert float((cur.double().sum(dim=-1) - 1.0).abs().max()) <= 1e-4            # rows of a product of row-stochastic factors sum to 1


# ------------------------------------------------------------------------------------------------ the factor
def _operands(binding, torch, x, mode):
    """x [rows][3 D] f32 -> (dtype id, device buffer, lo_off) in the mode's operand layout (test_op_attention_map_against_float64's)."""
    rows, width = x.shape
    xt = _dev(torch, x)
    if mode == "bf16":
        return binding.BF16, xt.to(torch.bfloat16), 0
    if mode == "f16":
        return binding.F16, xt.to(torch.float16), 0
    hi = xt.to(torch.float16); lo = ((xt - hi.float()) * 2048.0).to(torch.float16)
    pad = 8
    buf = torch.full((2 * (rows + pad), width), float("nan"), dtype=torch.float16, device="cuda")        # NaN rows behind each plane: never read
    buf[:rows] = hi; buf[rows + pad:2 * rows + pad] = lo
    return binding.F16, buf, (rows + pad) * width


def _factor_and_mean(binding, torch, x, mode, n, N, D, H):
    dt, buf, lo_off = _operands(binding, torch, x, mode)
    mean = torch.full((n, N, N), float("nan"), dtype=torch.float32, device="cuda")
    fac = torch.full((n + 1, N, N), float("nan"), dtype=torch.float32, device="cuda")
    binding.op_attention_map(dt, buf.data_ptr(), 0, mean.data_ptr(), n, N, D, H, lo_off=lo_off)
    binding.op_rollout_factor(dt, buf.data_ptr(), fac.data_ptr(), n, N, D, H, lo_off=lo_off)
    torch.cuda.synchronize()
    return fac, mean


@pytest.mark.parametrize("mode", R.FACTOR_MODES)
@pytest.mark.parametrize("hd", R.FACTOR_HD)
@pytest.mark.parametrize("N", R.FACTOR_N)
def test_factor_is_half_the_head_mean_plus_half_the_identity_bit_for_bit(binding, torch_gpu, N, hd, mode):
    """On the ordinary qkv of test_op_attention_map_against_float64 (which holds the head mean to float64): every entry of the factor is
    float32(0.5) * mean + float32(0.5) * [i == j], evaluated in numpy float32 from the mean vitx_op_attention_map returns for the same
    buffer.  Bit for bit: the two forms of the kernel differ only in that last expression, and libvitx.so is built with -ffp-contract=off --
    vit.cpp_amd/Makefile puts it into CXXFLAGS, which its csrc/%.hip rule passes to every device object (halving is exact, so a contracted
    form would give the same bits here anyway: tests/test_cpu_rollout_data.py).  The NaN image behind the output keeps its bits."""
    torch = torch_gpu
    n, H = R.n_images(N), 2
    D = H * hd
    fac, mean = _factor_and_mean(binding, torch, R.ordinary_qkv(n, N, D, H), mode, n, N, D, H)
    want = _dev(torch, R.factor_of_mean(mean.cpu().numpy()))
    assert bool(torch.isfinite(mean).all())
    _same_bits(torch, fac[:n], want, f"N {N} hd {hd} {mode}: factor")
    assert bool(torch.isnan(fac[n:]).all())
    assert float((fac[:n].double().sum(dim=-1) - 1.0).abs().max()) <= 1e-5
    assert float(fac[:n].diagonal(dim1=1, dim2=2).min()) >= 0.5                   # the identity's half sits on the diagonal of every image


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("i", range(len(R.FACTOR_N)))
def test_factor_of_a_flat_softmax(binding, torch_gpu, i, mode):
    """exact_data.flat_qkv: every probability is 1 / N, so the diagonal lies within one f32 ulp of 0.5 + 0.5 / N and every other entry
    within one ulp of 0.5 / N."""
    torch = torch_gpu
    N, hd, H = R.FACTOR_N[i], R.FACTOR_HD[i % len(R.FACTOR_HD)], 2
    n = R.n_images(N)
    eye = torch.eye(N, dtype=torch.bool, device="cuda").expand(n, N, N)
    for sign in X.FLAT_SIGNS:
        qkv, _ = X.flat_qkv(n, N, H, hd, sign, X.attn_seed(n, N, H, hd) + 17 * sign)
        fac, _mean = _factor_and_mean(binding, torch, qkv, mode, n, N, H * hd, H)
        f = fac[:n].double()
        for name, sel, val in (("diagonal", eye, 0.5 + 0.5 / N), ("off-diagonal", ~eye, 0.5 / N)):
            if not bool(sel.any()):
                continue
            worst = float((f[sel] - val).abs().max())
            ulp = float(np.spacing(np.float32(val)))
            assert worst <= ulp, f"N {N} hd {hd} {mode} sign {sign}: a {name} entry lies {worst / ulp:.2f} ulp from {val}"
        assert bool(torch.isnan(fac[n:]).all())


# ------------------------------------------------------------------------------------------------ the last factor's row
def _row_buffers(torch, cls, r, N, H, cls_gap, out_gap):
    """cls rows cls_stride = H N + cls_gap apart and output rows N + out_gap apart, NaN in every gap; r with a NaN image behind it."""
    n = cls.shape[0]
    cb = torch.full((n, H * N + cls_gap), float("nan"), dtype=torch.float32, device="cuda")
    cb[:, :H * N] = _dev(torch, cls).reshape(n, H * N)
    ob = torch.full((n, N + out_gap), float("nan"), dtype=torch.float32, device="cuda")
    rb = None if r is None else _nan_tail(torch, r)
    return cb, ob, rb


@pytest.mark.parametrize("with_r", [True, False], ids=["r", "r_null"])
@pytest.mark.parametrize("N", R.ROW_EXACT_N)
def test_row_on_exact_data_is_exact_and_keeps_the_gaps(binding, torch_gpu, N, with_r):
    """rollout_data.row_exact, strides larger than the rows: the whole output buffer -- the N floats of every row and the NaN gaps between
    them -- has the expected bits; cls and r keep theirs.  r NULL (a one-layer model): the output is w itself."""
    torch = torch_gpu
    cls, r, w, out = R.row_exact(N)
    n, H = cls.shape[0], cls.shape[1]
    cb, ob, rb = _row_buffers(torch, cls, r if with_r else None, N, H, cls_gap=5, out_gap=3)
    want = ob.clone(); want[:, :N] = _dev(torch, out if with_r else w)
    cls_before, r_before = cb.clone(), (rb.clone() if with_r else None)
    binding.op_rollout_row(cb.data_ptr(), cb.shape[1], rb.data_ptr() if with_r else 0, ob.data_ptr(), ob.shape[1], n, N, H)
    torch.cuda.synchronize()
    _same_bits(torch, ob, want, f"N {N} H {H} {'w . r' if with_r else 'w'}")
    _same_bits(torch, cb, cls_before, "cls")
    if with_r:
        _same_bits(torch, rb, r_before, "r")


@pytest.mark.parametrize("N,H", R.ROW_ORDINARY)
def test_row_on_ordinary_maps_within_the_derived_bounds(binding, torch_gpu, N, H):
    """Softmax rows of H in {3, 12} heads and a row-stochastic r against float64 (rollout_data.row_bounds): w within (H + 2) 2^-24 w_j
    (r NULL), the product within N 2^-23 (w . |r|)_k."""
    torch = torch_gpu
    cls, r = R.row_ordinary(N, H)
    n = cls.shape[0]
    w64 = _dev(torch, R.row_w64(cls))
    out64 = torch.einsum("bj,bjk->bk", w64, _dev(torch, r).double())
    bw, bo = R.row_bounds(N, H, w64, out64)
    got = {}
    for with_r in (False, True):
        cb, ob, rb = _row_buffers(torch, cls, r if with_r else None, N, H, cls_gap=0, out_gap=1)
        binding.op_rollout_row(cb.data_ptr(), cb.shape[1], rb.data_ptr() if with_r else 0, ob.data_ptr(), ob.shape[1], n, N, H)
        torch.cuda.synchronize()
        assert bool(torch.isnan(ob[:, N:]).all())
        got[with_r] = ob[:, :N].double()
    rw = float(((got[False] - w64).abs() / bw).max())
    ro = float(((got[True] - out64).abs() / bo).max())
    print(f"ROLLOUT_GATE row N {N} H {H}: w worst ratio {rw:.4f} of (H + 2) 2^-24 w, product worst ratio {ro:.4f} of N 2^-23 (w . |r|)")
    assert rw <= 1.0 and ro <= 1.0, (N, H, rw, ro)


# ------------------------------------------------------------------------------------------------ argument checks
def test_every_refusal_comes_before_any_launch(binding, torch_gpu):
    """Every refusal of include/vitx.h leaves the sentinel-filled outputs untouched; a good call afterwards still works.  The buffers hold
    what the refused shapes would address."""
    torch = torch_gpu
    L = binding.lib()
    NMAX = R.MAX_TOKENS + 1
    SENT = -777.25
    q = torch.zeros((2 * NMAX * 3 * 512,), dtype=torch.float16, device="cuda")
    o = torch.full((2 * NMAX * NMAX,), SENT, dtype=torch.float32, device="cuda")
    o2 = torch.full((2 * NMAX * NMAX,), SENT, dtype=torch.float32, device="cuda")
    qp, op, o2p = q.data_ptr(), o.data_ptr(), o2.data_ptr()
    F16, BF16 = binding.F16, binding.BF16
    factor = [
        ((F16, None, 0, op, 2, 10, 128, 2, None), ERR_ARG), ((F16, qp, 0, None, 2, 10, 128, 2, None), ERR_ARG),
        ((F16, qp, 0, op, 0, 10, 128, 2, None), ERR_ARG), ((F16, qp, 0, op, 2, 0, 128, 2, None), ERR_ARG),
        ((F16, qp, 0, op, 2, 10, 128, 0, None), ERR_ARG), ((F16, qp, 0, op, 2, 10, 0, 2, None), ERR_ARG),
        ((F16, qp, 0, op, 2, -3, 128, 2, None), ERR_ARG), ((7, qp, 0, op, 2, 10, 128, 2, None), ERR_ARG),
        ((BF16, qp, 2 * 10 * 384, op, 2, 10, 128, 2, None), ERR_ARG),             # planes: F16 only
        ((F16, qp, 100, op, 2, 10, 128, 2, None), ERR_ARG),                       # lo inside hi
        ((F16, qp, 0, op, 2, 10, 100, 4, None), ERR_UNSUPPORTED),                 # head dim 25
        ((F16, qp, 0, op, 2, 10, 512, 2, None), ERR_UNSUPPORTED),                 # head dim 256
        ((F16, qp, 0, op, 2, NMAX, 128, 2, None), ERR_UNSUPPORTED),               # above 1024 tokens
    ]
    for args, rc in factor:
        assert L.vitx_op_rollout_factor(*args) == rc, args
    step = [
        ((None, o2p, 2, 10, None), ERR_ARG), ((op, None, 2, 10, None), ERR_ARG), ((op, o2p, 0, 10, None), ERR_ARG), ((op, o2p, 2, 0, None), ERR_ARG),
        ((op, o2p, -1, 10, None), ERR_ARG), ((op, o2p, 2, NMAX, None), ERR_UNSUPPORTED),
        ((op, op, 2, 10, None), ERR_ARG),                                         # r is a
        ((op, op + 4 * 199, 2, 10, None), ERR_ARG),                               # r begins in a's last row
        ((op + 4 * 199, op, 2, 10, None), ERR_ARG),                               # a begins in r's last row
    ]
    for args, rc in step:
        assert L.vitx_op_rollout_step(*args) == rc, args
    row = [
        ((None, 40, o2p, op, 10, 2, 10, 4, None), ERR_ARG), ((o2p, 40, None, None, 10, 2, 10, 4, None), ERR_ARG),
        ((o2p, 40, None, op, 10, 0, 10, 4, None), ERR_ARG), ((o2p, 40, None, op, 10, 2, 0, 4, None), ERR_ARG), ((o2p, 40, None, op, 10, 2, 10, 0, None), ERR_ARG),
        ((o2p, 39, None, op, 10, 2, 10, 4, None), ERR_ARG),                       # cls_stride < H N
        ((o2p, 40, None, op, 9, 2, 10, 4, None), ERR_ARG),                        # out_stride < N
        ((o2p, 2 * NMAX, None, op, NMAX, 2, NMAX, 2, None), ERR_UNSUPPORTED),
    ]
    for args, rc in row:
        assert L.vitx_op_rollout_row(*args) == rc, args
    torch.cuda.synchronize()
    assert bool((o == SENT).all()) and bool((o2 == SENT).all())
    # adjacent buffers do not overlap: a step whose r ends where a begins runs
    a, r, exp = R.step_exact(17)
    both = torch.cat([_dev(torch, r), _dev(torch, a)])
    n = a.shape[0]
    assert L.vitx_op_rollout_step(both[n:].data_ptr(), both.data_ptr(), n, 17, None) == 0
    torch.cuda.synchronize()
    _same_bits(torch, both[n:], _dev(torch, exp), "a step after the refusals")
    _same_bits(torch, both[:n], _dev(torch, r), "r after the step")
