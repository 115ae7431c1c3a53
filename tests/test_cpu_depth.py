"""The depth head without a GPU (include/vitx.h "depth estimation"): the host function vitx_depth_host against the numpy restatement of
tests/depth_data.py bit for bit, the restatement against torch in mmseg's own order, the mutants the GPU test must be able to see, the bin
centres, the converter and the head file's round trip, and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import depth_data as XD


def _host(binding, lg, off, bins, n, gh, gw, K, u, oh, ow, lo=XD.LO, hi=XD.HI):
    d, f = binding.depth_host(lg, off, bins, n, gh, gw, K, u, oh, ow, float(lo), float(hi))
    return d.view(np.uint32), f.view(np.uint32)


def test_host_function_equals_the_restatement_bit_for_bit(binding):
    """Hostile data on every shape (ld = K_pad, pad columns of +inf and NaN in logits and offsets), with and without offsets; ordinary data too."""
    cases = XD.cases()
    assert len(cases) > 30
    for i, (gh, gw, u, K, oh, ow, n) in enumerate(cases):
        ld = XD.pad_to(K)
        for make in (XD.hostile, XD.normal):
            lg, off, bins = make(n, gh, gw, K, ld, seed=i)
            for o in (off, None):
                want_d, want_f = XD.depth(lg, o, bins, n, gh, gw, K, u, oh, ow, XD.LO, XD.HI)
                d, f = _host(binding, lg, o, bins, n, gh, gw, K, u, oh, ow)
                tag = (gh, gw, u, K, oh, ow, n, make.__name__, o is None)
                assert np.array_equal(f, want_f), tag
                assert np.array_equal(d, want_d), tag


def test_hostile_data_does_what_it_is_meant_to(binding):
    """On one shape, each property by name."""
    n, gh, gw, K, u, oh, ow = 3, 3, 5, 5, 4, 42, 70
    ld = XD.pad_to(K)
    lg, off, bins = XD.hostile(n, gh, gw, K, ld, seed=1)
    d, f = _host(binding, lg, off, bins, n, gh, gw, K, u, oh, ow)
    fine, dep = f.view(np.float32), d.view(np.float32)
    nan_f = np.isnan(fine)
    assert nan_f[1].sum() > 0 and (f[nan_f] == 0x7fc00000).all() and (d[np.isnan(dep)] == 0x7fc00000).all()     # +inf: S and Tm both inf
    assert nan_f[0].sum() > nan_f[1].sum()                                     # the NaN logit of image 0 adds NaNs of its own
    # the fine cell (fh - 1, 0) reads grid cell (gh - 1, 0) alone (both weights 1 and 0) and every v_k < 0 there: (0.1 sum bins) / (0.1 K)
    S = np.float32(0); T = np.float32(0)
    for k in range(K):
        S = np.float32(S + np.float32(0.1)); T = np.float32(T + np.float32(np.float32(0.1) * bins[k]))
    assert (fine[:, u * gh - 1, 0] == np.float32(T / S)).all() and abs(float(T / S) - float(bins.astype(np.float64).mean())) < 1e-5
    # the first bin alone / the last bin alone: depths outside the clamp, which the depth map shows as its bounds
    assert (fine[1:, 0, 0] < XD.LO).all() and (fine[:, -1, -1] > XD.HI).all()
    assert (dep[1:, 0, 0] == XD.LO).all() and (dep[:, -1, -1] == XD.HI).all()
    assert np.nanmin(dep) == XD.LO and np.nanmax(dep) == XD.HI
    # -inf is clipped to 0 where its weight is positive, and a NaN where the weight is exactly 0: the clip alone leaves numbers around that cell
    P = lg.reshape(n, gh, gw, ld)
    assert np.isneginf(P[1, gh // 2, gw - 1, (K // 2 + 1) % K]) and np.isfinite(fine[1, u * (gh // 2) + u // 2, -1])
    assert np.isinf(P[..., K:]).any() and np.isnan(P[..., K:]).any() and np.isnan(off[:, K:]).any()
    assert len({off[i, :K].tobytes() for i in range(n)}) == n                  # a different offset row per image


def test_mutants_change_the_expected_map(binding):
    """Each mistake of depth_data.MUTANTS changes the expected map -- the host function's -- on shapes the GPU test runs: the GPU test can notice."""
    shape = {m: (2, 3, 4, 5, 16, 37, 3) for m in XD.MUTANTS}
    shape["xy_swapped"] = (3, 5, 2, 64, 17, 37, 2)
    cases = XD.cases()
    for m in XD.MUTANTS:
        gh, gw, u, K, oh, ow, n = shape[m]
        assert shape[m] in cases, m
        i = cases.index(shape[m])
        lg, off, bins = XD.hostile(n, gh, gw, K, XD.pad_to(K), seed=i)
        want_d, want_f = XD.depth(lg, off, bins, n, gh, gw, K, u, oh, ow, XD.LO, XD.HI)
        assert np.array_equal(want_d, _host(binding, lg, off, bins, n, gh, gw, K, u, oh, ow)[0])
        got_d, got_f = XD.depth(lg, off, bins, n, gh, gw, K, u, oh, ow, XD.LO, XD.HI, mutant=m)
        changed = int((want_d != got_d).sum())
        print(f"{m}: {changed} of {want_d.size} depths change")
        assert changed >= 1, m
        if m not in ("clamp_missing", "upsample_skipped"):
            assert got_f.shape == want_f.shape and (want_f != got_f).any(), m


@pytest.mark.parametrize("gh,gw,oh,ow", [(3, 5, 42, 70), (16, 16, 224, 224), (37, 37, 518, 518)])
def test_restatement_against_torch_in_mmseg_order(binding, gh, gw, oh, ow):
    """mmseg's depth head: F.interpolate of the logits x u, relu, + 0.1, division by the sum, einsum with the bins, F.interpolate to the output, clamp --
    in float64 and in float32, K = 256, u = 4.  Every summand is positive, so each sequential sum carries at most K 2^-24 relative error, S and Tm
    together 2 K; 64 covers the two resamplings at |logit| <= 4.  Allowed: (2 K + 64) 2^-24 max(bins)."""
    import torch
    import torch.nn.functional as Fn
    K, u, n = 256, 4, 1
    lg, off, bins = XD.normal(n, gh, gw, K, K, seed=gh)
    taps = lg.reshape(n, gh * gw, K) + off[:, None, :K]
    assert np.abs(taps).max() <= 4.0, "the bound's condition"
    lo, hi = 0.001, 10.0
    got_bits, _ = XD.depth(lg, off, bins, n, gh, gw, K, u, oh, ow, lo, hi)
    got = got_bits.view(np.float32).astype(np.float64)
    host_bits, _ = _host(binding, lg, off, bins, n, gh, gw, K, u, oh, ow, lo, hi)
    assert np.array_equal(host_bits, got_bits)
    bound = (2 * K + 64) * 2.0 ** -24 * float(bins.max())
    for dt in (torch.float64, torch.float32):
        x = torch.from_numpy(np.ascontiguousarray(taps.reshape(n, gh, gw, K).transpose(0, 3, 1, 2))).to(dt)
        x = Fn.interpolate(x, size=(u * gh, u * gw), mode="bilinear", align_corners=False)
        x = torch.relu(x) + 0.1
        x = x / x.sum(dim=1, keepdim=True)
        d = torch.einsum("ikmn,k->imn", x, torch.from_numpy(bins).to(dt)).unsqueeze(1)
        d = Fn.interpolate(d, size=(oh, ow), mode="bilinear", align_corners=False)
        d = torch.clamp(d, min=lo, max=hi)[:, 0].double().numpy()
        worst = float(np.abs(got - d).max())
        print(f"{gh}x{gw} -> {oh}x{ow} {dt}: max |restatement - torch| = {worst / (2.0 ** -24 * float(bins.max())):.1f} x 2^-24 max(bins), allowed {2 * K + 64}")
        assert worst <= bound


def test_bin_centres(binding):
    ud = binding.depth_bins(256, 0.001, 10.0, "UD")
    assert ud.dtype == np.float32 and ud.shape == (256,) and ud[0] == np.float32(0.001) and ud[-1] == np.float32(10.0)
    assert np.array_equal(ud, np.linspace(0.001, 10.0, 256).astype(np.float32)) and (np.diff(ud) > 0).all()
    sid = binding.depth_bins(64, 0.001, 80.0, "SID")
    assert np.array_equal(sid, np.logspace(np.log10(0.001), np.log10(80.0), 64).astype(np.float32)) and (np.diff(sid) > 0).all()
    assert abs(float(sid[1] / sid[0]) - float(sid[-1] / sid[-2])) < 1e-4
    assert binding.depth_bins(1, 2.0, 2.0)[0] == 2.0
    for bad in ((0, 1.0, 2.0, "UD"), (4, 0.0, 2.0, "UD"), (4, 3.0, 2.0, "SID"), (4, 1.0, 2.0, "log")):
        with pytest.raises(ValueError):
            binding.depth_bins(*bad)


def test_converter_round_trip_and_refused_widths(pkg, binding, tmp_path):
    import torch
    convert = pkg.convert
    K, D, layers = 6, 16, [2, 5, 8, 11]
    m = len(layers)
    rng = np.random.default_rng(0)
    W = rng.standard_normal((K, 2 * m * D, 1, 1)).astype(np.float32)
    b = rng.standard_normal(K).astype(np.float32)
    sd = {"decode_head.conv_depth.weight": torch.from_numpy(W), "decode_head.conv_depth.bias": torch.from_numpy(b), "backbone.cls_token": torch.zeros(1, 1, D)}
    head = convert.depth_head(sd, layers, D, 0.001, 10.0, "UD", 4)
    assert head["wp"].shape == (K, m * D) and head["wc"].shape == (K, m * D) and head["layers"] == layers and not head["norm"]
    for j in range(m):                                                          # per layer: the D patch columns first, then the D class columns
        assert np.array_equal(head["wp"][:, j * D:(j + 1) * D], W[:, 2 * j * D:(2 * j + 1) * D, 0, 0])
        assert np.array_equal(head["wc"][:, j * D:(j + 1) * D], W[:, (2 * j + 1) * D:(2 * j + 2) * D, 0, 0])
    assert np.array_equal(head["bias"], b) and np.array_equal(head["bins"], binding.depth_bins(K, 0.001, 10.0, "UD"))
    path = str(tmp_path / "head.npz")
    convert.write_depth_head(path, head)
    back = binding.depth_head(path)
    for k in ("wp", "wc", "bias", "bins"):
        assert np.array_equal(back[k], head[k]), k
    assert (back["layers"], back["upsample"], back["min_depth"], back["max_depth"], back["norm"]) == (layers, 4, 0.001, 10.0, False)
    # without the class half: a width of m D
    sd1 = {"state_dict": {"decode_head.conv_depth.weight": torch.from_numpy(W[:, :m * D, 0, 0].copy()), "decode_head.conv_depth.bias": torch.from_numpy(b)}}
    h1 = convert.depth_head(sd1, layers, D, 0.5, 80.0, "SID", 2, norm=True)
    assert h1["wc"] is None and np.array_equal(h1["wp"], W[:, :m * D, 0, 0]) and np.array_equal(h1["bins"], binding.depth_bins(K, 0.5, 80.0, "SID"))
    convert.write_depth_head(path, h1)
    b1 = binding.depth_head(path)
    assert b1["wc"] is None and b1["norm"] is True and b1["upsample"] == 2 and np.array_equal(b1["wp"], h1["wp"])
    # any other width is refused by name
    with pytest.raises(ValueError, match="decode_head.conv_depth.weight has width 128"):
        convert.depth_head(sd, layers, 24)
    with pytest.raises(ValueError, match="decode_head.conv_depth.weight has width 128"):
        convert.depth_head(sd, layers[:3], D)
    with pytest.raises(ValueError, match="layers"):
        convert.depth_head(sd, [3, 2], D)
    with pytest.raises(ValueError, match="conv_depth"):
        convert.depth_head({"weight": torch.zeros(2, 16)}, [0], 16)
    np.savez(path, wp=head["wp"])
    with pytest.raises(ValueError, match="a depth head file holds"):
        binding.depth_head(path)
    # the command line
    ck = str(tmp_path / "ckpt.pth")
    torch.save(sd, ck)
    assert convert.main(["--depth-head-in", ck, "--depth-head-out", path, "--depth-layers", "2,5,8,11", "--depth-hidden", str(D), "--depth-max", "80", "--depth-bins", "SID",
                         "--depth-upsample", "2", "--depth-norm"]) == 0
    cli = binding.depth_head(path)
    assert np.array_equal(cli["wp"], head["wp"]) and np.array_equal(cli["wc"], head["wc"]) and cli["layers"] == layers and cli["norm"] is True and cli["upsample"] == 2
    assert cli["max_depth"] == 80.0 and np.array_equal(cli["bins"], binding.depth_bins(K, 0.001, 80.0, "SID"))


def test_argument_checks_need_no_device(binding):
    L = binding.lib()
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    raw = np.zeros(6 * 128 + 4, np.float32)
    lg = raw[(-raw.ctypes.data // 4) % 4:][:6 * 128].reshape(6, 128)          # 16-byte aligned rows
    assert lg.ctypes.data % 16 == 0
    bins = np.ones(256, np.float32); out = np.zeros((64, 64), np.float32); fine = np.zeros((64, 64), np.float32)
    p, b, q, f = lg.ctypes.data, bins.ctypes.data, out.ctypes.data, fine.ctypes.data
    cf = C.c_float
    # (logits, ld, offsets, bins, n, gh, gw, K, u): the fine plane's checks, shared by the host function and the device entry point
    host = lambda lgp, ld, offp, bp, n, gh, gw, K, u, oh=32, ow=48, lo=1.0, hi=2.0, dst=q: L.vitx_depth_host(lgp, ld, offp, bp, n, gh, gw, K, u, oh, ow, cf(lo), cf(hi), dst, None)
    dev = lambda lgp, ld, offp, bp, n, gh, gw, K, u, dst=f: L.vitx_op_depth_fine(lgp, ld, offp, bp, n, gh, gw, K, u, dst, None)   # refused before any device call
    for fn in (host, dev):
        assert fn(None, 128, None, b, 1, 2, 3, 21, 4) == A and fn(p, 128, None, None, 1, 2, 3, 21, 4) == A and fn(p, 128, None, b, 1, 2, 3, 21, 4, dst=None) == A
        assert fn(p, 128, None, b, 0, 2, 3, 21, 4) == A and fn(p, 128, None, b, 1, 0, 3, 21, 4) == A and fn(p, 128, None, b, 1, 2, 0, 21, 4) == A
        assert fn(p, 128, None, b, 1, 2, 3, 0, 4) == A                           # K < 1
        assert fn(p, 20, None, b, 1, 2, 3, 21, 4) == A and fn(p, 126, None, b, 1, 2, 3, 21, 4) == A       # ld below K rounded up to 4; no multiple of 4
        assert fn(p, 260, None, b, 1, 2, 3, 257, 4) == U                         # K > 256
        assert fn(p, 128, None, b, 1, 2, 3, 21, 3) == U and fn(p, 128, None, b, 1, 2, 3, 21, 0) == U and fn(p, 128, None, b, 1, 2, 3, 21, 8) == U
        assert b"not 1, 2 or 4" in L.vitx_last_error()
        assert fn(p, 128, None, b, 65536, 2, 3, 21, 4) == U
    assert dev(p + 4, 128, None, b, 1, 2, 3, 21, 4) == A and dev(p, 128, p + 4, b, 1, 2, 3, 21, 4) == A   # off a 16-byte boundary
    # the depth map's checks
    assert host(p, 128, None, b, 1, 2, 3, 21, 4, oh=7) == U and host(p, 128, None, b, 1, 2, 3, 21, 4, ow=11) == U      # below the fine plane 8 x 12
    assert host(p, 128, None, b, 1, 2, 3, 21, 4, oh=8193) == U and host(p, 128, None, b, 1, 2, 3, 21, 4, ow=8193) == U
    assert host(p, 128, None, b, 1, 2, 3, 21, 4, lo=3.0, hi=2.0) == A and host(p, 128, None, b, 1, 2, 3, 21, 4, lo=float("nan")) == A
    assert host(p, 128, None, b, 1, 2, 3, 21, 4, hi=float("inf")) == A
    assert host(p, 24, None, b, 1, 2, 3, 21, 4, oh=8, ow=12) == 0                # ld = K rounded up to 4 is enough; output = the fine plane
    rs = lambda src, n, fh, fw, oh, ow, lo, hi, dst: L.vitx_op_depth_resize(src, n, fh, fw, oh, ow, cf(lo), cf(hi), dst, None)
    assert rs(None, 1, 8, 12, 32, 48, 1.0, 2.0, q) == A and rs(f, 1, 8, 12, 32, 48, 1.0, 2.0, None) == A and rs(f, 0, 8, 12, 32, 48, 1.0, 2.0, q) == A
    assert rs(f, 1, 0, 12, 32, 48, 1.0, 2.0, q) == A and rs(f, 1, 8, 12, 32, 48, 2.5, 2.0, q) == A and rs(f, 1, 8, 12, 32, 48, 1.0, float("nan"), q) == A
    assert rs(f + 2, 1, 8, 12, 32, 48, 1.0, 2.0, q) == A and rs(f, 1, 8, 12, 32, 48, 1.0, 2.0, q + 1) == A           # off a 4-byte boundary
    assert rs(f, 1, 8, 12, 7, 48, 1.0, 2.0, q) == U and rs(f, 1, 8, 12, 32, 11, 1.0, 2.0, q) == U and rs(f, 1, 8, 12, 8193, 48, 1.0, 2.0, q) == U
    assert rs(f, 65536, 8, 12, 32, 48, 1.0, 2.0, q) == U
    # vitx_op_depth: refused before any device call
    def z(dtype=1, a=p, wp=p, acls=None, wc=None, bias=p, bn=b, lgp=p, offp=None, n=1, gh=2, gw=3, K=21, Dc=64, u=4, oh=32, ow=48, lo=1.0, hi=2.0, fn=f, dst=q):
        return L.vitx_op_depth(dtype, a, wp, acls, wc, bias, bn, lgp, offp, n, gh, gw, K, Dc, u, oh, ow, cf(lo), cf(hi), fn, dst, None)
    assert z(a=None) == A and z(wp=None) == A and z(bias=None) == A and z(bn=None) == A and z(lgp=None) == A and z(fn=None) == A and z(dst=None) == A
    assert z(dtype=2) == A and z(Dc=0) == A and z(K=0) == A
    assert z(acls=p) == A and z(wc=p) == A and z(acls=p, wc=p) == A             # the class half: rows and matrix together, and somewhere to put the offsets
    assert z(a=p + 4) == A and z(dst=q + 1) == A and z(lo=3.0) == A
    assert z(Dc=96) == U and z(K=257) == U and z(u=3) == U and z(oh=7) == U
    assert z(n=65535, gh=64, gw=64, oh=256, ow=256) == U and b"byte window" in L.vitx_last_error()
    # vitx_op_depth_rows
    rw = lambda dtype, x, ldx, y, ldy, rows, D: L.vitx_op_depth_rows(dtype, x, ldx, y, ldy, rows, D, None)
    assert rw(1, None, 64, p, 64, 1, 64) == A and rw(2, p, 64, p, 64, 1, 64) == A and rw(1, p, 32, p, 64, 1, 64) == A and rw(1, p + 4, 64, p, 64, 1, 64) == A
    assert rw(1, p, 64, p, 64, 1, 12) == U and rw(1, p, 66, p, 64, 1, 64) == U and rw(1, p, 64, p, 68, 1, 64) == U
    # vitx_depth_set and its readers without a context
    assert L.vitx_depth_set(None, None, None, None, None, 0, 0, 0, 4, cf(1.0), cf(2.0), 0, 0, 0) == A
    assert L.vitx_depth_bins(None) == 0 and L.vitx_depth_images(None) == 0 and L.vitx_depth_scratch_bytes(None) == 0 and L.vitx_depth_device(None) is None
