"""Cases, references and gates shared by tests/test_cpu_pos_resample.py and tests/test_gpu_resolution.py (vitx_pos_embed_resample,
vitx_model_resize_file, vitx_ctx_options::img_size).

The reference of the resampler is CPU torch F.interpolate(mode="bicubic", align_corners=False) evaluated in float64 on the f32 input,
antialias False (VITX_POS_BICUBIC) or True (VITX_POS_BICUBIC_AA).  The gate per case comes from torch itself, not from the code under test:
    max |ours - torch64| <= 4 * max |torch32 - torch64|,   floor 4 * 2^-23 * max |pos|
(the factor 4 allows another summation order over the 16 taps and differently rounded coefficients, both a few ulp of max |pos|; the floor
covers the sizes where torch's own f32 result happens to be exact).  The two conventions differ by 1e-3 .. 5e-2 on these inputs, four to
five orders of magnitude above the gate: each case also asserts that the OTHER convention is more than 100 gates away."""
import numpy as np

BICUBIC, BICUBIC_AA = 0, 1
WIDTHS = (192, 130)          # 130: not a multiple of 4 (the kernel's scalar path), let alone 64
# ((gy_in, gx_in), (gy_out, gx_out)); the identity case is separate (exact equality)
CASES = [((14, 14), (24, 24)), ((14, 14), (16, 16)), ((14, 14), (10, 10)), ((14, 14), (7, 7)), ((14, 14), (37, 37)),
         ((4, 4), (2, 2)), ((4, 4), (6, 6)), ((4, 4), (8, 8)), ((14, 14), (12, 20))]
IDENTITY = ((14, 14), (14, 14))


def case_id(c):
    (a, b), (p, q) = c
    return f"{a}x{b}-{p}x{q}"


def table(grid_in, D, seed=0):
    """[1 + gy * gx][D] f32 ~ N(0, 0.02^2): the scale of a trained ViT position table."""
    gy, gx = grid_in
    rng = np.random.default_rng(1000 * seed + 31 * D + 7 * gy + gx)
    return (rng.standard_normal((1 + gy * gx, D)) * 0.02).astype(np.float32)


def torch_resample(pos, grid_in, grid_out, interp, f64):
    """torch's F.interpolate on the grid rows of pos (the class row is not part of it): [gy' * gx'][D] in float64 or float32."""
    import torch
    import torch.nn.functional as F
    D = pos.shape[1]
    t = torch.from_numpy(np.ascontiguousarray(pos[1:])).to(torch.float64 if f64 else torch.float32)
    t = t.reshape(1, grid_in[0], grid_in[1], D).permute(0, 3, 1, 2)
    o = F.interpolate(t, size=tuple(grid_out), mode="bicubic", align_corners=False, antialias=(interp == BICUBIC_AA))
    return o.permute(0, 2, 3, 1).reshape(-1, D).numpy()


def gate(pos, grid_in, grid_out, interp):
    """(torch64 reference, gate) of one case."""
    r64 = torch_resample(pos, grid_in, grid_out, interp, True)
    r32 = torch_resample(pos, grid_in, grid_out, interp, False)
    g = max(4.0 * float(np.abs(r32.astype(np.float64) - r64).max()), 4.0 * 2.0 ** -23 * float(np.abs(pos).max()))
    return r64, g


def check_against_torch(ours, pos, grid_in, grid_out, interp, label=""):
    """The whole per-case statement: class row bit-equal, within the gate of this convention, more than 100 gates from the other one."""
    assert ours.shape == (1 + grid_out[0] * grid_out[1], pos.shape[1]) and ours.dtype == np.float32
    assert np.array_equal(ours[0].view(np.uint32), pos[0].view(np.uint32)), "class row is not a bit copy"
    r64, g = gate(pos, grid_in, grid_out, interp)
    dev = float(np.abs(ours[1:].astype(np.float64) - r64).max())
    other = torch_resample(pos, grid_in, grid_out, 1 - interp, True)
    far = float(np.abs(ours[1:].astype(np.float64) - other).max())
    print(f"{label} interp={interp} D={pos.shape[1]} {case_id((grid_in, grid_out))}: max|ours - torch64| = {dev:.3e}  gate = {g:.3e}  "
          f"to the other convention = {far:.3e} ({far / g:.0f} gates)")
    assert dev <= g, (dev, g)
    assert far > 100.0 * g, (far, g)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
