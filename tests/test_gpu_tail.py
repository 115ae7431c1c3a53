"""The three kernel families the user-visible result comes straight out of -- class softmax, device top-k, block dequant -- on data that
leaves one correct result (tests/tail_data.py; conditions: test_cpu_tail_data.py).

  * softmax_kernel: every argument of the exponential with the numerators known bit for bit and the probabilities inside the bound the
    kernel's own arithmetic allows; flat, routed and shifted rows bit for bit; ld > cols with NaN / +inf in the pad columns.
  * topk_kernel (vitx_op_topk): ties across position k, signed zeros, infinities and NaNs, against the numpy order and vitx_topk.
  * dequant kernels (vitx_op_dequant, vitx_op_dequant_jobs): every code at every position, scales no quantiser writes, the four-job
    launch of the forward, bit for bit over the whole padded destination.

Every output buffer has GUARD elements in front and behind that must come back bit-unchanged; every input has hostile values around it.
Reach for these when a change touches the reductions, the rounding points, the tie rule, a bit gather or the job table.
"""
import ctypes as C

import numpy as np
import pytest

import tail_data as T

pytestmark = pytest.mark.gpu

GUARD = 1024                        # elements in front of and behind every buffer
OUT_FILL32, OUT_FILL16 = 0x5a5a5a5a, 0x5a5a


def _status(binding, rc, what):
    assert rc == 0, f"{what}: status {rc}: {binding.lib().vitx_last_error().decode()}"


def _out_buffer(torch, n, bits16=False):
    """(whole buffer, body view) of n elements between two guards, all sentinel."""
    buf = torch.full((n + 2 * GUARD,), OUT_FILL16 if bits16 else OUT_FILL32, dtype=torch.int16 if bits16 else torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(torch, buf, n, what):
    fill = OUT_FILL16 if buf.dtype == torch.int16 else OUT_FILL32
    assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), f"{what}: a guard element was written"


# ------------------------------------------------------------------------------------------------------------------
# softmax
# ------------------------------------------------------------------------------------------------------------------
def _pad_pattern(torch, cols, ld):
    c = torch.arange(cols, ld, device="cuda")
    return torch.where((c & 1) == 0, torch.tensor(float("nan"), device="cuda"), torch.tensor(float("inf"), device="cuda"))


def _softmax(binding, torch, dt, body, cols, what):
    """body: [rows][ld] f32 on the device, pad columns already hostile.  +inf in front of and behind the logits.  Returns probs [rows][cols] (a view
    of the guarded output buffer, guards checked)."""
    rows, ld = body.shape
    src = torch.full((rows * ld + 2 * GUARD,), float("inf"), device="cuda")
    src[GUARD:GUARD + rows * ld] = body.reshape(-1)
    buf, out = _out_buffer(torch, rows * cols)
    rc = binding.lib().vitx_op_softmax_dt(dt, src.data_ptr() + GUARD * 4, out.data_ptr(), rows, cols, ld, None)
    torch.cuda.synchronize()
    _status(binding, rc, what)
    _guards_intact(torch, buf, rows * cols, what)
    return out.view(torch.float32).view(rows, cols)


@pytest.mark.parametrize("perturbed", [False, True], ids=["on_grid", "off_grid"])
@pytest.mark.parametrize("dtype", [T.F16, T.BF16], ids=["f16", "bf16"])
def test_softmax_every_argument_of_the_exponential(binding, torch_gpu, dtype, perturbed):
    """Every value of the operand type in [-20, 0] as x - max (less the 1.4 % / 0.02 % whose exp lies within 64 f32 ulps of a rounding tie), so
    e_i = rnd<T>(expf(rnd<T>(x_i - max))) is known exactly -- f16 subnormals and the 171 f16 zeros included -- and p = e / sum e must hold
    |p - p_ref| <= p_ref * (ceil(cols / 256) + 10) * 2^-24 (tail_data.softmax_gate).  A kernel without the outer rounding misses that by a
    factor of thousands; off_grid moves every argument an eighth of a spacing off the type's values, where one without the inner
    rounding does too."""
    torch = torch_gpu
    cols = 1000
    logits, e64, p_ref = T.exp_case(dtype, perturbed=perturbed)
    p = _softmax(binding, torch, dtype, torch.from_numpy(logits.copy()).cuda(), cols, "softmax exp sweep").cpu().numpy()
    assert np.isfinite(p).all()
    ratio = T.softmax_gate_ratio(p, p_ref, cols)
    wrong_zero = int((p.view(np.uint32)[e64 == 0] != 0).sum())
    print(f"  dtype {dtype} perturbed {perturbed}: worst |p - p_ref| / (p_ref * gate) = {ratio:.3f}; entries with e = 0 that are not +0: {wrong_zero}")
    assert ratio <= 1.0, ratio
    assert wrong_zero == 0
    assert (p.view(np.uint32)[e64 > 0] != 0).all()


@pytest.mark.parametrize("dtype", [T.F16, T.BF16], ids=["f16", "bf16"])
def test_softmax_flat_rows(binding, torch_gpu, dtype):
    """All logits of a row equal: every numerator is 1, the sum is the integer cols, and every probability is float32(1) / float32(cols) bit
    for bit -- at every column count around the block's 256 threads and the waves' 64 lanes, ld = cols, cols + 1 and the padded width."""
    torch = torch_gpu
    for rows, cols, ld in T.sm_shapes():
        want = int(np.array([np.float32(1) / np.float32(cols)], np.float32).view(np.int32)[0])
        body = torch.empty((rows, ld), device="cuda")
        body[:, cols:] = _pad_pattern(torch, cols, ld)
        for level in T.SM_LEVELS:
            body[:, :cols] = level
            p = _softmax(binding, torch, dtype, body, cols, f"flat rows {rows} cols {cols} ld {ld} level {level}")
            bad = p.view(torch.int32) != want
            assert not bool(bad.any()), f"rows {rows} cols {cols} ld {ld} level {level}: {int(bad.sum())} entries are not float32(1) / {cols}, first at {tuple(bad.nonzero()[0].tolist())}"


@pytest.mark.parametrize("dtype", [T.F16, T.BF16], ids=["f16", "bf16"])
def test_softmax_routed_rows(binding, torch_gpu, dtype):
    """One column 0, all others -200: exactly 1.0 there and +0 elsewhere; the hot column moves through every lane and wave."""
    torch = torch_gpu
    for rows, cols, ld in T.sm_shapes():
        hot = torch.from_numpy(T.routed_hot(rows, cols)).cuda()
        r = torch.arange(rows, device="cuda")
        body = torch.empty((rows, ld), device="cuda")
        body[:, cols:] = _pad_pattern(torch, cols, ld)
        body[:, :cols] = -200.0
        body[r, hot] = 0.0
        want = torch.zeros((rows, cols), device="cuda"); want[r, hot] = 1.0
        p = _softmax(binding, torch, dtype, body, cols, f"routed rows {rows} cols {cols} ld {ld}")
        bad = p.view(torch.int32) != want.view(torch.int32)
        assert not bool(bad.any()), f"rows {rows} cols {cols} ld {ld}: {int(bad.sum())} entries differ, first at {tuple(bad.nonzero()[0].tolist())}"


@pytest.mark.parametrize("dtype", [T.F16, T.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("rows,cols,ld", [(37, 1000, 1024), (9, 257, 258), (3, 21843, 21843)])
def test_softmax_shift_invariance(binding, torch_gpu, dtype, rows, cols, ld):
    """Integer logits, integer shifts: every x - max is the same exact integer, so the three outputs are the same bits."""
    torch = torch_gpu
    x = torch.from_numpy(T.shift_logits(rows, cols, rows + cols)).cuda()
    outs = []
    for s in T.SHIFTS:
        body = torch.empty((rows, ld), device="cuda")
        body[:, cols:] = _pad_pattern(torch, cols, ld)
        body[:, :cols] = x + s
        outs.append(_softmax(binding, torch, dtype, body, cols, f"shift {s}").clone())
    assert bool(torch.isfinite(outs[1]).all()) and float(outs[1].sum(1).sub(1).abs().max()) < 1e-5
    for s, o in zip(T.SHIFTS, outs):
        assert torch.equal(o.view(torch.int32), outs[1].view(torch.int32)), f"shift {s}: {int((o.view(torch.int32) != outs[1].view(torch.int32)).sum())} entries differ from the unshifted result"


# ------------------------------------------------------------------------------------------------------------------
# top-k
# ------------------------------------------------------------------------------------------------------------------
def _host_topk(L, row, k):
    idx = np.full(k, -7, np.int32); val = np.zeros(k, np.float32)
    assert L.vitx_topk(row.ctypes.data_as(C.POINTER(C.c_float)), row.size, k, idx.ctypes.data_as(C.POINTER(C.c_int32)), val.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return val.view(np.uint32), idx


@pytest.mark.parametrize("kind", T.TK_KINDS)
def test_topk_order(binding, torch_gpu, kind):
    """vitx_op_topk against the numpy order and vitx_topk, value bits and class, at every width around the wave's 64 lanes, k up to the whole
    row, row counts around the four rows of a block.  The rows in front of and behind the input hold 2.0."""
    torch = torch_gpu
    L = binding.lib()
    for cols in T.TK_COLS:
        allrows = T.topk_rows(kind, cols)
        src = torch.full((allrows.size + 2 * GUARD,), T.TK_GUARD, device="cuda")
        for k in T.tk_ks(cols):
            vals, idx = T.topk_expected(allrows, k)
            for r in range(allrows.shape[0]):
                hv, hi = _host_topk(L, np.ascontiguousarray(allrows[r]), k)
                assert np.array_equal(hv, vals[r]) and np.array_equal(hi, idx[r]), f"vitx_topk: {kind} cols {cols} k {k} row {r}"
            want = np.stack([vals.view(np.int32), idx], axis=2)                       # [rows][k][2]
            for rows in T.TK_ROWS:
                what = f"{kind} cols {cols} k {k} rows {rows}"
                src[GUARD:GUARD + rows * cols] = torch.from_numpy(allrows[:rows].reshape(-1).view(np.int32).copy()).cuda().view(torch.float32)
                src[GUARD + rows * cols:GUARD + allrows.size] = T.TK_GUARD
                buf, out = _out_buffer(torch, rows * k * 2)
                rc = L.vitx_op_topk(src.data_ptr() + GUARD * 4, rows, cols, k, out.data_ptr(), None)
                torch.cuda.synchronize()
                _status(binding, rc, what)
                _guards_intact(torch, buf, rows * k * 2, what)
                got = out.cpu().numpy().reshape(rows, k, 2)
                if not np.array_equal(got, want[:rows]):
                    r, i = np.argwhere((got != want[:rows]).any(2))[0]
                    pytest.fail(f"{what}: row {r} position {i}: got class {got[r, i, 1]} value bits {int(got[r, i, 0]) & 0xffffffff:#010x}, "
                                f"want class {want[r, i, 1]} value bits {int(want[r, i, 0]) & 0xffffffff:#010x}")


# ------------------------------------------------------------------------------------------------------------------
# dequant
# ------------------------------------------------------------------------------------------------------------------
def _upload_blocks(torch, qtype, blocks):
    """Blocks in the file layout -> what the kernels read, between 0xff bytes (an f16 scale of 0xffff is a NaN).  Returns (keep-alive
    tensors, blocks pointer, scales pointer or None)."""
    def guarded(a):
        raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)
        t = torch.full((raw.size + 2 * GUARD,), 0xff, dtype=torch.uint8, device="cuda")
        t[GUARD:GUARD + raw.size] = torch.from_numpy(raw.copy()).cuda()
        return t
    if qtype == T.Q4_0:
        qs, ds = T.split_q4_0(blocks)
        tq, td = guarded(qs), guarded(ds)
        return (tq, td), tq.data_ptr() + GUARD, td.data_ptr() + GUARD
    t = guarded(blocks)
    return (t,), t.data_ptr() + GUARD, None


def _dequant(binding, torch, dtype, qtype, blocks, N, n_pad, K, what):
    """vitx_op_dequant into a guarded buffer: the whole destination [n_pad][K] as 16-bit patterns."""
    keep, pb, ps = _upload_blocks(torch, qtype, blocks)
    buf, out = _out_buffer(torch, n_pad * K, bits16=True)
    rc = binding.lib().vitx_op_dequant(dtype, qtype, pb, ps, out.data_ptr(), N, n_pad, K, None)
    torch.cuda.synchronize()
    _status(binding, rc, what)
    _guards_intact(torch, buf, n_pad * K, what)
    return out.cpu().numpy().view(np.uint16).reshape(n_pad, K)


def _same_bits(got, want, what):
    if not np.array_equal(got, want):
        r, c = np.argwhere(got != want)[0]
        pytest.fail(f"{what}: {int((got != want).sum())} of {want.size} elements differ; first at row {r} column {c} (position {c % 32} of block {c // 32}): "
                    f"got {got[r, c]:#06x}, want {want[r, c]:#06x}")


@pytest.mark.parametrize("dtype", [T.F16, T.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("qtype", T.QTYPES)
def test_dequant_every_code_at_every_position(binding, torch_gpu, qtype, dtype):
    """Block b holds code (b + i) % n_codes at position i: a nibble, a qh bit or a byte taken from the wrong place changes some element.
    Once with d = 1, m = 0 (the result is the code itself), once with a scale whose products round."""
    N, K = T.sweep_shape(qtype)
    for d_bits, m_bits in T.SWEEP_SCALES:
        blocks = T.sweep_blocks(qtype, d_bits, m_bits)
        got = _dequant(binding, torch_gpu, dtype, qtype, blocks, N, N + 3, K, "code sweep")
        _same_bits(got, T.dequant_bits(qtype, blocks, dtype, N, N + 3, K), f"qtype {qtype} d {d_bits:#06x} m {m_bits:#06x}")


@pytest.mark.parametrize("dtype", [T.F16, T.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("qtype", T.QTYPES)
def test_dequant_hostile_scales_and_shapes(binding, torch_gpu, qtype, dtype):
    """Scales (and minima) no quantiser writes -- zeros of both signs, subnormals, +-65504 (f16 results overflow to inf), random patterns --
    one per row, at N = 1, 5, 200, n_pad = N, N + 3 and the next multiple of 256, K = 32, 64, 448; pad rows are +0."""
    sc = T.hostile_scales()
    for N, n_pad, K in T.dq_shapes():
        blocks = T.scaled_blocks(qtype, N, K, N + K, sc)
        got = _dequant(binding, torch_gpu, dtype, qtype, blocks, N, n_pad, K, "hostile scales")
        _same_bits(got, T.dequant_bits(qtype, blocks, dtype, N, n_pad, K), f"qtype {qtype} N {N} n_pad {n_pad} K {K}")


@pytest.mark.parametrize("dtype", [T.F16, T.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("qtype", T.QTYPES)
def test_dequant_nonfinite_scales(binding, torch_gpu, qtype, dtype):
    """inf and NaN scales: NaN where the reference has NaN (0 * inf, inf - inf, anything with a NaN), the same bits everywhere else."""
    N, blocks = T.nonfinite_blocks(qtype)
    K, n_pad = 64, N + 3
    got = _dequant(binding, torch_gpu, dtype, qtype, blocks, N, n_pad, K, "non-finite scales")
    want = T.dequant_bits(qtype, blocks, dtype, N, n_pad, K)
    nan = T.is_nan_bits(want, dtype)
    assert nan.any() and np.array_equal(T.is_nan_bits(got, dtype), nan)
    _same_bits(np.where(nan, 0, got), np.where(nan, 0, want), f"qtype {qtype}")


@pytest.mark.parametrize("dtype", [T.F16, T.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("qtype", T.HAS_MIN)
def test_dequant_rounds_to_f32_first(binding, torch_gpu, qtype, dtype):
    """code * d + m is rounded to f32 and THEN to the operand type: elements on which rounding the exact sum at once gives another value
    (tail_data.double_rounding_blocks; a contracted multiply-add, by contrast, cannot show: test_cpu_tail_data.py)."""
    blocks, found = T.double_rounding_blocks(qtype, dtype)
    assert found >= T.DOUBLE_ROUNDING_WANT[(qtype, dtype)]
    if not found:
        return
    got = _dequant(binding, torch_gpu, dtype, qtype, blocks, found, found + 3, 32, "double rounding")
    _same_bits(got, T.dequant_bits(qtype, blocks, dtype, found, found + 3, 32), f"qtype {qtype}")


@pytest.mark.parametrize("dtype", [T.F16, T.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("qtype", T.QTYPES)
def test_dequant_jobs(binding, torch_gpu, qtype, dtype):
    """vitx_op_dequant_jobs with 1 .. 4 matrices shaped like a layer at D = 64, ragged pads, all destinations in ONE buffer with guards
    between them: every destination is the single-job expansion of the same blocks (and the reference), every guard is untouched."""
    torch = torch_gpu
    sc = T.hostile_scales()
    shapes = [(N, T.job_n_pad(N, j), K) for j, (N, K) in enumerate(T.JOB_SHAPES)]
    blocks = [T.scaled_blocks(qtype, N, K, 100 + j, sc) for j, (N, _, K) in enumerate(shapes)]
    single = [_dequant(binding, torch, dtype, qtype, blocks[j], *shapes[j], f"single job {j}") for j in range(4)]
    for j in range(4):
        _same_bits(single[j], T.dequant_bits(qtype, blocks[j], dtype, *shapes[j]), f"qtype {qtype} single job {j}")
    ups = [_upload_blocks(torch, qtype, b) for b in blocks]
    for njobs in (1, 2, 3, 4):
        sizes = [shapes[j][1] * shapes[j][2] for j in range(njobs)]
        offs = [GUARD + sum(sizes[:j]) + j * GUARD for j in range(njobs)]
        total = sum(sizes) + (njobs + 1) * GUARD
        buf = torch.full((total,), OUT_FILL16, dtype=torch.int16, device="cuda")
        vp, ip = C.c_void_p * njobs, C.c_int * njobs
        rc = binding.lib().vitx_op_dequant_jobs(dtype, qtype, njobs, vp(*[ups[j][1] for j in range(njobs)]), vp(*[ups[j][2] for j in range(njobs)]),
                                                vp(*[buf.data_ptr() + 2 * offs[j] for j in range(njobs)]), ip(*[shapes[j][0] for j in range(njobs)]),
                                                ip(*[shapes[j][1] for j in range(njobs)]), ip(*[shapes[j][2] for j in range(njobs)]), None)
        torch.cuda.synchronize()
        _status(binding, rc, f"{njobs} jobs")
        got = buf.cpu().numpy().view(np.uint16)
        covered = np.zeros(total, bool)
        for j in range(njobs):
            covered[offs[j]:offs[j] + sizes[j]] = True
            _same_bits(got[offs[j]:offs[j] + sizes[j]].reshape(shapes[j][1], shapes[j][2]), single[j], f"qtype {qtype}, {njobs} jobs, job {j}")
        assert (got[~covered] == OUT_FILL16).all(), f"qtype {qtype}, {njobs} jobs: a guard element between the destinations was written"
