"""attention_window.hip (include/vitx.h "windowed attention and decomposed relative position") on its own: the generic kernel's bits with zero tables,
float64 with random ones, the sharp cases of window_data.SHARP, and isolation.  D 128, two heads, canary rows around `out`."""
import numpy as np
import pytest

import prefix_data as PD
import window_data as WD
from ref64 import PROB_TOL, stage_errors, stage_ok

pytestmark = pytest.mark.gpu
DTYPES = ["f16", "bf16"]


def _types(binding, torch, dtype_name):
    return (binding.F16, torch.float16) if dtype_name == "f16" else (binding.BF16, torch.bfloat16)


def _window(binding, torch, dtype_name, qkv, Rh, Rw, bias, n, grid, win):
    """out [n * gh gw][D] on the device; qkv may hold more rows than the launch covers."""
    dt, tdt = _types(binding, torch, dtype_name)
    x, th, tw = (torch.from_numpy(np.ascontiguousarray(a)).cuda().to(tdt) for a in (qkv, Rh, Rw))
    tb = torch.from_numpy(bias).float().cuda()
    out = torch.full((n * grid[0] * grid[1] + 4, WD.D), 7.0, dtype=tdt, device="cuda")
    binding.attention_window(dt, x.data_ptr(), th.data_ptr(), tw.data_ptr(), tb.data_ptr(), out[2:].data_ptr(), n, grid, win, WD.D, WD.H)
    torch.cuda.synchronize()
    assert bool((out[:2] == 7).all()) and bool((out[-2:] == 7).all())
    return out[2:-2]


def _generic(binding, torch, dtype_name, qkv, n, N):
    dt, tdt = _types(binding, torch, dtype_name)
    x = torch.from_numpy(np.ascontiguousarray(qkv)).cuda().to(tdt)
    out = torch.full((n * N, WD.D), float("nan"), dtype=tdt, device="cuda")
    binding.check(binding.lib().vitx_op_attention_generic(dt, x.data_ptr(), out.data_ptr(), n, N, WD.D, WD.H, None))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("grid,ws", [(g, None) for g in WD.GLOBAL] + [((8, 12), 4)], ids=str)
def test_zero_tables_have_the_generic_kernels_bits(binding, torch_gpu, grid, ws, dtype_name):
    """One global window: vitx_op_attention_generic at N = gh gw.  Windows of a grid without pads: the generic kernel on each window's rows as an image."""
    win = (ws, ws) if ws else grid
    qkv, Rh, Rw, bias = WD.case(dtype_name, grid, win, tables=0.0)
    got = _window(binding, torch_gpu, dtype_name, qkv, Rh, Rw, bias, 2, grid, win)
    rows = WD.window_rows(2, grid, ws) if ws else np.arange(len(qkv)).reshape(2, -1)
    want = _generic(binding, torch_gpu, dtype_name, qkv[rows.ravel()], len(rows), rows.shape[1])
    assert torch_gpu.equal(got[torch_gpu.from_numpy(rows.ravel()).cuda()].view(torch_gpu.int16), want.view(torch_gpu.int16))


SHARP_CASES = [(g, w, {}) for g, w in WD.F64_CASES] + [WD.SHARP[k] for k in WD.SHARP]


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("grid,win,kw", SHARP_CASES, ids=["%dx%d-%dx%d" % (g + w) for g, w in WD.F64_CASES] + list(WD.SHARP))
def test_against_float64(binding, torch_gpu, grid, win, kw, dtype_name):
    args = WD.case(dtype_name, grid, win, **kw)
    ref = WD.attention64(*args, 2, grid, win)
    err = float(np.abs(_window(binding, torch_gpu, dtype_name, *args, 2, grid, win).double().cpu().numpy() - ref).max())
    print(f"attention_window {dtype_name} grid {grid} window {win} {kw}: max |d| {err:.3e} (gate {WD.GATE * np.abs(ref).max():.3e})")
    assert err <= WD.GATE * np.abs(ref).max()


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("grid,win", [((5, 7), (3, 3)), ((9, 8), (9, 8))], ids=str)
def test_a_nan_image_and_nan_rows_behind_the_buffer_stay_out(binding, torch_gpu, grid, win, dtype_name):
    qkv, Rh, Rw, bias = WD.case(dtype_name, grid, win, n_img=3)
    G = grid[0] * grid[1]
    alone = _window(binding, torch_gpu, dtype_name, qkv[2 * G:], Rh, Rw, bias, 1, grid, win)
    dirty = np.concatenate([qkv, np.full((70, 3 * WD.D), np.nan, np.float32)])
    dirty[G:2 * G] = np.nan
    got = _window(binding, torch_gpu, dtype_name, dirty, Rh, Rw, bias, 3, grid, win)
    clean = _window(binding, torch_gpu, dtype_name, qkv, Rh, Rw, bias, 3, grid, win)
    i16 = torch_gpu.int16
    assert torch_gpu.equal(got[:G].view(i16), clean[:G].view(i16)) and torch_gpu.equal(got[2 * G:].view(i16), clean[2 * G:].view(i16))
    assert torch_gpu.equal(got[2 * G:].view(i16), alone.view(i16)) and bool(got[G:2 * G].isnan().all())


@pytest.mark.parametrize("dtype", [0, 1])
def test_forward_against_float64(pkg, binding, torch_gpu, dtype):
    """The synthetic file (layer 1 global, windows of 3 on a 5 x 5 grid, identity final norm): probabilities and VITX_FEAT_TOKENS under ref64's gates,
    batch 3 against batch 1 bit for bit, the named refusals of a live context."""
    path = WD.fixture_file(pkg)
    rnd = PD.f16_round if dtype == 0 else PD.bf16_round
    imgs = PD.exact_images(3, WD.IMG, seed=2)
    tok64, ref = WD.forward64(PD.file_tensors(pkg, path), imgs, wround=rnd, uround=rnd)
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=dtype)
    ctx.feat_enable(cls=False, tokens=True)
    p3 = ctx.forward(imgs)
    t3 = ctx.feat_read(3)[WD.LAYERS - 1]["tokens"]
    p1 = ctx.forward(imgs[:1])
    t1 = ctx.feat_read(1)[WD.LAYERS - 1]["tokens"]
    e_max, e_rms = stage_errors(np.stack([tok64, t3]), np.stack([tok64, tok64]))[0]
    print(f"window forward dtype {dtype}: max|dprob| {np.abs(p3 - ref).max():.3e} (gate {PROB_TOL[dtype]}), tokens max/rms {e_max:.3e} rms/rms {e_rms:.3e}")
    assert np.isfinite(p3).all() and np.abs(p3 - ref).max() <= PROB_TOL[dtype] and stage_ok(e_max, e_rms, dtype)
    assert np.array_equal(p3[:1], p1) and np.array_equal(t3[:1], t1)
    with pytest.raises(binding.VitxError, match="windowed attention"):
        ctx.attn_enable([0])
    with pytest.raises(binding.VitxError, match="identity_final_norm"):      # the dense head reads the final norm, which this file has not
        ctx.dense_set(np.ones((2, WD.D), np.float32))
    ctx.close(); model.close()
