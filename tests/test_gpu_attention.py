"""Attention kernels on data with ORDINARY softmax weights (tests/exact_data.py; conditions: test_cpu_exact_data.py).

The routing and dominant-token tests make every softmax one-hot: a key that leaks or goes missing with an ordinary weight, a softmax scale
that is a little off, or a padded key counted in the row sum changes nothing there.  Two designs close that:

  * flat: every key of an (image, head) is the same vector, so every numerator is exactly 1, every partial sum an integer, and the output
    is the per-column constant c BIT FOR BIT while every key carries the weight 1 / N.  Whole buffers, torch.equal, no tolerance.  A
    dropped key moves every row; with sign = -1 a zero pad key in the row sum outweighs all real keys by e^24.
  * spread / peaked: randn data against the float64 attention of the operands the kernel multiplies, under a per-element bound made of
    the output ulp and the first-order effect of the numerator and exponent-argument rounding, and a mean gate of three times the mean
    error of an f32 EMULATION OF THE DEFINITION.  Neither gate takes a number from the kernels; test_cpu_exact_data.py shows that one
    leaked key, one dropped key and a 2 % scale error each break a gate on every case.
"""
import numpy as np
import pytest

import exact_data as X
import test_gpu_exact as TE

pytestmark = pytest.mark.gpu


def _params(cases):
    return [(f, dn, c) for f in cases if f != "map" for dn in ("f16", "bf16") for c in cases[f] if not (f == "precise" and dn == "bf16")]


_ids = lambda p: p if isinstance(p, str) else "n%d_N%d_H%d_hd%d" % p


@pytest.mark.parametrize("family,dtype_name,case", _params(X.FLAT_CASES), ids=_ids)
def test_attention_flat_softmax_is_exact(binding, torch_gpu, family, dtype_name, case):
    """Every family and entry point (`precise`: vitx_op_attention_f32 and vitx_op_attention_planes, whose lo plane is zero on this data;
    `cls`: row 0) on flat data of the three signs: the whole output buffer, pre-filled with NaN, equals c.  Every family normalises AFTER
    P.V ((P.V) * (1 / sum) with exact integer P.V = N c and sum = N), so no family needs another expected buffer."""
    torch = torch_gpu
    n_img, N, H, hd = case
    _, tdt, _ = TE._types(binding, torch, dtype_name)
    for sign in X.FLAT_SIGNS:
        qkv, c = X.flat_qkv(n_img, N, H, hd, sign, X.attn_seed(n_img, N, H, hd) + 17 * sign)
        want = torch.from_numpy(c.reshape(n_img, H * hd) if family == "cls" else X.flat_expected(c, N)).cuda().to(tdt)
        for name, out in TE.attention_run(binding, torch, family, dtype_name, qkv, n_img, N, H, hd).items():
            TE._same(torch, out, want, f"{name} {dtype_name} {case} sign {sign}")


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
@pytest.mark.parametrize("case", X.FLAT_CASES["map"], ids=_ids)
def test_attention_map_of_a_flat_softmax(binding, torch_gpu, case, dtype_name):
    """vitx_op_attention_map on the flat inputs: an f32 softmax of N equal scores.  Every class-token entry and every head-mean entry lies
    within one f32 ulp of 1 / N, and every row sums to 1 within N such ulps (the head mean takes at most 1024 tokens)."""
    torch = torch_gpu
    n_img, N, H, hd = case
    dt, tdt, _ = TE._types(binding, torch, dtype_name)
    ulp = float(np.spacing(np.float32(1.0 / N)))
    for sign in X.FLAT_SIGNS:
        qkv, _ = X.flat_qkv(n_img, N, H, hd, sign, X.attn_seed(n_img, N, H, hd) + 17 * sign)
        xq = torch.from_numpy(qkv).cuda().to(tdt)
        cls = torch.full((n_img, H, N), float("nan"), device="cuda")
        mean = torch.full((n_img, N, N), float("nan"), device="cuda") if N <= 1024 else None
        binding.op_attention_map(dt, xq.data_ptr(), cls.data_ptr(), mean.data_ptr() if mean is not None else 0, n_img, N, H * hd, H)
        torch.cuda.synchronize()
        for name, m in (("class-token map", cls), ("head mean", mean)):
            if m is None:
                continue
            m = m.double()
            worst = float((m - 1.0 / N).abs().max())
            assert worst <= ulp, f"{name} {dtype_name} {case} sign {sign}: an entry lies {worst / ulp:.2f} ulp from 1 / N"
            rows = float((m.sum(dim=-1) - 1.0).abs().max())
            assert rows <= N * ulp, f"{name} {dtype_name} {case} sign {sign}: a row sums to 1 +- {rows / ulp:.1f} ulp"


@pytest.mark.parametrize("family,dtype_name,case", _params(X.SPREAD_CASES), ids=_ids)
def test_attention_spread_softmax_within_the_derived_bound(binding, torch_gpu, family, dtype_name, case):
    """randn * 0.8 (hundreds of keys carry weight) and the same with q * 3 (ten or so do) against exact_data.attention_ref of the operands
    the kernel multiplies (rounded to the operand type; the f32 values for `precise`), all of it in float64 on the device, no case capped:
      per element  |got - ref64| <= |ref64| ulp_out + k u sum_j w_ij (2 + |s_ij - max_i|) |v_jd - ref64_id| + 1e-7   (exact_data.attention_bound),
      whole buffer mean|got - ref64| <= 3 mean|emu - ref64|,  emu = exact_data.attention_emu in the family's schedule,
    and, so that k is not a guess, the emulation itself stays below half of the bound.  Measured ratios: DESIGN.md section 3."""
    torch = torch_gpu
    n_img, N, H, hd = case
    _, tdt, _ = TE._types(binding, torch, dtype_name)
    scale = 1.0 / np.sqrt(hd)
    schedule = X.attention_schedule(family, dtype_name, N)
    for kind in X.spread_kinds(N):
        x32 = X.spread_qkv(n_img, N, H, hd, X.attn_seed(n_img, N, H, hd), kind)
        x = torch.from_numpy(x32).cuda()
        q, k, v = X.heads_of(x if family == "precise" else x.to(tdt).float(), n_img, N, H, hd)
        if family == "cls":
            q = q[:, :1]
        ref, cond = X.attention_ref(q, k, v, scale, want_bound=True)
        bound = X.attention_bound(ref, cond, dtype_name)
        emu = X.attention_emu(q, k, v, scale, dtype_name, schedule)
        emu_worst, _ = X.attention_gate_ratios(emu, ref, bound, emu)
        # The CPU conditions sample the query rows of these cases: here every row.  They are conditions on the data of a case, not on a family:
        # `cls` keeps one row per item, too few to stand for the case, and shares its large case with the families that keep all rows.
        if N > X.CPU_FULL_MAX_N and family != "cls":
            for fault, out in X.attention_faults(q, k, v, scale, n_img, H).items():
                worst, mean = X.attention_gate_ratios(out, ref, bound, emu)
                assert worst > 1.0 or mean > X.ATTN_MEAN_FACTOR, f"{case} {kind} {dtype_name} {schedule}: fault '{fault}' passes both gates ({worst:.2f}, {mean:.2f})"
        nq = q.shape[1]
        ref, bound, emu = (X.rows_of(t, n_img, nq, H, hd) for t in (ref, bound, emu))
        for name, out in TE.attention_run(binding, torch, family, dtype_name, x32, n_img, N, H, hd).items():
            assert bool(torch.isfinite(out.float()).all()), (name, case, kind)
            worst, mean = X.attention_gate_ratios(out, ref, bound, emu)
            print(f"ATTN_GATE {name} {dtype_name} {schedule} n{n_img}_N{N}_H{H}_hd{hd} {kind}: emulation {emu_worst:.3f} of the bound, kernel {worst:.3f} of the bound, "
                  f"mean error {mean:.3f} of the emulation's")
            assert emu_worst <= 0.5, f"{case} {kind} {dtype_name} {schedule}: the emulation needs {emu_worst:.3f} of the bound (k = {X.ATTN_K})"
            assert worst <= 1.0, f"{name} {dtype_name} {case} {kind}: an element lies at {worst:.3f} of its bound"
            assert mean <= X.ATTN_MEAN_FACTOR, f"{name} {dtype_name} {case} {kind}: mean error {mean:.3f} times the emulation's"
