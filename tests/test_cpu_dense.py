"""The dense head without a GPU (include/vitx.h "dense prediction"): the host function vitx_dense_labels_host against the numpy restatement of
tests/dense_data.py bit for bit, the restatement against torch's F.interpolate, the mutants the GPU test must be able to see, the converter's
BatchNorm fold against torch's own modules, the head file's round trip, and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import dense_data as DD


def _host(binding, lg, n, gh, gw, K, oh, ow):
    lab, sc = binding.dense_labels_host(lg, n, gh, gw, K, oh, ow)
    return lab, sc.view(np.uint32)


def test_host_function_equals_the_restatement_bit_for_bit(binding):
    """Hostile data on every shape: ties, zeros of both signs, NaN planes, cells of NaNs, infinities, pad columns of +inf and NaN (ld = K_pad)."""
    cases = DD.cases()
    assert len(cases) > 30
    for i, (gh, gw, oh, ow, K, n) in enumerate(cases):
        ld = DD.pad_to(K)
        lg = DD.hostile(n, gh, gw, K, ld, seed=i)
        want_lab, want_bits = DD.labels(lg, n, gh, gw, K, oh, ow)
        lab, bits = _host(binding, lg, n, gh, gw, K, oh, ow)
        tag = (gh, gw, oh, ow, K, n)
        assert np.array_equal(lab, want_lab), tag
        assert np.array_equal(bits, want_bits), tag
        assert lab.max() < K, tag
        lab2, none = binding.dense_labels_host(lg, n, gh, gw, K, oh, ow, want_score=False)          # without scores: the same labels
        assert none is None and np.array_equal(lab2, lab), tag


def test_hostile_data_does_what_it_is_meant_to(binding):
    """On one shape, each property by name: the lowest index wins a tie, a NaN plane never wins against a number, a pixel of NaNs gets class 0, the
    infinities meet a zero weight (the score of such a pixel's class is a NaN: it ranks last), zeros of both signs tie."""
    n, gh, gw, K, oh, ow = 2, 14, 14, 21, 37, 37
    ld = DD.pad_to(K)
    lg = DD.hostile(n, gh, gw, K, ld, seed=3)
    lab, bits = _host(binding, lg, n, gh, gw, K, oh, ow)
    v = DD.values(lg, n, gh, gw, K, oh, ow)
    others = np.where(np.isnan(v), -np.inf, v)[..., [k for k in range(K) if k not in (1, K - 1)]].max(-1)
    tie = (v[..., 1] == v[..., K - 1]) & (v[..., 1] > others)
    assert tie.sum() > 100 and (lab[tie] == 1).all()                             # classes 1 and K - 1 are equal and on top: class 1 wins
    assert np.isnan(v[0, ..., 0]).all() and (lab[0] != 0)[~np.isnan(v[0]).all(-1)].all()        # the NaN plane of image 0
    dead = np.isnan(v).all(-1)
    assert dead.sum() > 0 and (lab[dead] == 0).all() and (bits[dead] == 0x7fc00000).all()       # pixels of NaNs only
    assert (lab[1] == 0).sum() > dead[1].sum()                                   # ... while class 0 does win elsewhere in image 1
    # the corner pixel reads cell (0, 0) alone (both weights 1 and 0): the zeros of both signs tie, class 0 wins
    assert lab[1, 0, 0] == 0 and (bits[1, 0, 0] & 0x7fffffff) == 0
    # +inf times a zero weight: at scale 1 every second weight is 0, so the class with +inf in one cell is a NaN in the neighbouring pixels
    lg1 = DD.hostile(1, 4, 4, 5, 128, seed=1)
    v1 = DD.values(lg1, 1, 4, 4, 5, 4, 4)
    assert np.isnan(v1[0, :, :, 2]).sum() >= 2 and np.isinf(v1[0, 2, 2, 2])
    lab1, _ = _host(binding, lg1, 1, 4, 4, 5, 4, 4)
    assert np.array_equal(lab1, DD.labels(lg1, 1, 4, 4, 5, 4, 4)[0]) and lab1[0, 2, 2] == 2


def test_mutants_change_the_expected_map(binding):
    """Each mistake of dense_data.MUTANTS changes at least one label of the expected map -- the host function's -- on the shapes the GPU test runs: the
    GPU test can notice."""
    shapes = {"pad_leak": (2, 3, 32, 48, 21), "last_dropped": (2, 3, 32, 48, 21), "tie_high": (2, 3, 32, 48, 21), "clamp_g2": (2, 3, 32, 48, 21), "xy_swapped": (3, 5, 224, 17, 150)}
    assert set(shapes) == set(DD.MUTANTS)
    for m, (gh, gw, oh, ow, K) in shapes.items():
        assert (gh, gw, oh, ow, K) in [c[:5] for c in DD.cases()]
        i = [c[:5] for c in DD.cases()].index((gh, gw, oh, ow, K))
        n = DD.cases()[i][5]
        lg = DD.hostile(n, gh, gw, K, DD.pad_to(K), seed=i)
        want, _ = DD.labels(lg, n, gh, gw, K, oh, ow)
        assert np.array_equal(want, _host(binding, lg, n, gh, gw, K, oh, ow)[0])
        got, _ = DD.labels(lg, n, gh, gw, K, oh, ow, mutant=m)
        changed = int((want != got).sum())
        print(f"{m}: {changed} of {want.size} labels change")
        assert changed >= 1, m


def test_restatement_against_torch_interpolate(binding):
    """F.interpolate(mode="bilinear", align_corners=False) on the CPU, seeded normal logits at K = 21.  Each form rounds a convex combination of the four
    taps at three levels, so two values differ by at most 16 2^-24 max |tap| (a margin of about 2 over both); the labels agree on every pixel whose
    float64 top-two gap exceeds that bound, and those left out are at most 0.1 % of the map."""
    import torch
    import torch.nn.functional as Fn
    K = 21
    for (gh, gw, oh, ow, seed) in ((14, 14, 224, 224, 0), (14, 14, 37, 37, 1), (3, 5, 224, 17, 2), (16, 37, 16, 37, 3)):
        lg = DD.normal(2, gh, gw, K, K, seed=seed)
        P = lg.reshape(2, gh, gw, K)
        planes = torch.from_numpy(np.ascontiguousarray(P.transpose(0, 3, 1, 2)))
        t32 = Fn.interpolate(planes, size=(oh, ow), mode="bilinear", align_corners=False).numpy().transpose(0, 2, 3, 1)
        t64 = Fn.interpolate(planes.double(), size=(oh, ow), mode="bilinear", align_corners=False).numpy().transpose(0, 2, 3, 1)
        v = DD.values(lg, 2, gh, gw, K, oh, ow)
        y0, y1, _, _ = DD.axis(gh, oh)
        x0, x1, _, _ = DD.axis(gw, ow)
        A = np.abs(P)
        taps = np.maximum(np.maximum(A[:, y0][:, :, x0], A[:, y0][:, :, x1]), np.maximum(A[:, y1][:, :, x0], A[:, y1][:, :, x1]))
        bound = 16 * 2.0 ** -24 * taps
        assert (np.abs(v.astype(np.float64) - t32) <= bound).all()
        lab, _ = DD.labels(lg, 2, gh, gw, K, oh, ow)
        assert np.array_equal(lab, _host(binding, np.ascontiguousarray(np.pad(lg, ((0, 0), (0, 3)), constant_values=np.nan)), 2, gh, gw, K, oh, ow)[0])
        top2 = np.sort(t64, axis=-1)[..., -2:]
        sure = (top2[..., 1] - top2[..., 0]) > bound.max(-1)
        left_out = 1.0 - sure.mean()
        print(f"{gh}x{gw} -> {oh}x{ow}: {100 * left_out:.4f} % of the pixels left out")
        assert left_out <= 1e-3
        assert np.array_equal(lab[sure], t64.argmax(-1)[sure]) and np.array_equal(t32.argmax(-1)[sure], t64.argmax(-1)[sure])


def test_batchnorm_fold_and_refused_width(pkg):
    import torch
    convert = pkg.convert
    K, D, layers = 7, 16, [2, 5, 8, 11]
    Dc = D * len(layers)
    g = torch.Generator().manual_seed(0)
    bn = torch.nn.BatchNorm2d(Dc).double()
    conv = torch.nn.Conv2d(Dc, K, 1).double()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(Dc, generator=g, dtype=torch.float64) + 0.5); bn.bias.copy_(torch.randn(Dc, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(Dc, generator=g, dtype=torch.float64)); bn.running_var.copy_(torch.rand(Dc, generator=g, dtype=torch.float64) + 0.1)
        conv.weight.copy_(torch.randn(K, Dc, 1, 1, generator=g, dtype=torch.float64)); conv.bias.copy_(torch.randn(K, generator=g, dtype=torch.float64))
    bn.eval(); conv.eval()
    sd = {f"decode_head.bn.{k}": v for k, v in bn.state_dict().items()}
    sd.update({f"decode_head.conv_seg.{k}": v for k, v in conv.state_dict().items()})
    sd["backbone.cls_token"] = torch.zeros(1, 1, D)                               # other keys of a checkpoint are ignored
    # the fold itself, before its rounding to f32, against torch in float64
    x = torch.randn(3, Dc, 4, 5, generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = conv(bn(x)).numpy()
    gam = sd["decode_head.bn.weight"].numpy() / np.sqrt(sd["decode_head.bn.running_var"].numpy() + 1e-5)
    head = convert.dense_head(sd, layers, hidden_size=D)
    assert head["weight"].shape == (K, Dc) and head["weight"].dtype == np.float32 and head["layers"] == layers and head["names"] is None
    W64 = conv.weight.detach().numpy()[:, :, 0, 0] * gam[None, :]
    b64 = conv.bias.detach().numpy() + conv.weight.detach().numpy()[:, :, 0, 0] @ (bn.bias.detach().numpy() - bn.running_mean.numpy() * gam)
    got = np.einsum("kc,nchw->nkhw", W64, x.numpy()) + b64[None, :, None, None]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(head["weight"], W64.astype(np.float32)) and np.array_equal(head["bias"], b64.astype(np.float32))
    # a plain pair is taken as it is; {"state_dict": ...} wrappers are looked into
    plain = convert.dense_head({"state_dict": {"weight": torch.from_numpy(W64), "bias": torch.from_numpy(b64)}}, layers)
    assert np.array_equal(plain["weight"], head["weight"]) and np.array_equal(plain["bias"], head["bias"])
    # a width that does not match the backbone is refused by name
    with pytest.raises(ValueError, match="decode_head.conv_seg.weight has width 64"):
        convert.dense_head(sd, layers, hidden_size=32)
    with pytest.raises(ValueError, match="decode_head.conv_seg.weight has width 64"):
        convert.dense_head(sd, layers[:3], hidden_size=D)
    with pytest.raises(ValueError, match="layers"):
        convert.dense_head(sd, [3, 2], hidden_size=D)


def test_head_file_round_trip(pkg, binding, tmp_path):
    convert = pkg.convert
    rng = np.random.default_rng(0)
    head = {"weight": rng.standard_normal((5, 32)).astype(np.float32), "bias": rng.standard_normal(5).astype(np.float32), "layers": [1, 3],
            "names": ["sky", "road", "tree", "grass", "a name with spaces"]}
    path = str(tmp_path / "head.npz")
    convert.write_dense_head(path, head)
    back = binding.dense_head(path)
    assert np.array_equal(back["weight"], head["weight"]) and np.array_equal(back["bias"], head["bias"])
    assert back["layers"] == [1, 3] and back["names"] == head["names"]
    del head["names"]
    convert.write_dense_head(path, head)
    assert binding.dense_head(path)["names"] is None
    np.savez(path, weight=head["weight"])
    with pytest.raises(ValueError, match="weight, bias and layers"):
        binding.dense_head(path)
    # the command line: a torch-saved state dict in, the same file out
    import torch
    ck = str(tmp_path / "ckpt.pth")
    torch.save({"weight": torch.from_numpy(head["weight"]), "bias": torch.from_numpy(head["bias"])}, ck)
    assert convert.main(["--dense-head-in", ck, "--dense-head-out", path, "--dense-layers", "1,3", "--dense-hidden", "16"]) == 0
    cli = binding.dense_head(path)
    assert np.array_equal(cli["weight"], head["weight"]) and cli["layers"] == [1, 3]


def test_argument_checks_need_no_device(binding):
    L = binding.lib()
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    raw = np.zeros(6 * 128 + 4, np.float32)
    lg = raw[(-raw.ctypes.data // 4) % 4:][:6 * 128].reshape(6, 128); lab = np.zeros((32, 48), np.uint8)       # 16-byte aligned rows
    assert lg.ctypes.data % 16 == 0
    p, q = lg.ctypes.data, lab.ctypes.data
    host = lambda *a: L.vitx_dense_labels_host(*a, None)
    dev = lambda *a: L.vitx_op_dense_labels(*a, None, None)                       # refused before any device call: host pointers do no harm
    for f in (host, dev):
        assert f(None, 128, 1, 2, 3, 21, 32, 48, q) == A and f(p, 128, 1, 2, 3, 21, 32, 48, None) == A
        assert f(p, 128, 0, 2, 3, 21, 32, 48, q) == A and f(p, 128, 1, 0, 3, 21, 32, 48, q) == A and f(p, 128, 1, 2, 0, 21, 32, 48, q) == A
        assert f(p, 128, 1, 2, 3, 0, 32, 48, q) == A                             # K < 1
        assert f(p, 20, 1, 2, 3, 21, 32, 48, q) == A and f(p, 126, 1, 2, 3, 21, 32, 48, q) == A       # ld below K rounded up to 4; ld no multiple of 4
        assert f(p, 260, 1, 2, 3, 257, 32, 48, q) == U                           # K > 256
        assert f(p, 128, 1, 2, 3, 21, 1, 48, q) == U and f(p, 128, 1, 2, 3, 21, 32, 2, q) == U        # smaller than the grid
        assert f(p, 128, 1, 2, 3, 21, 8193, 48, q) == U and f(p, 128, 1, 2, 3, 21, 32, 8193, q) == U
        assert f(p, 128, 65536, 2, 3, 21, 32, 48, q) == U
        assert b"upsampling only" in L.vitx_last_error() or b"images" in L.vitx_last_error()
    assert L.vitx_op_dense_labels(p + 4, 128, 1, 2, 3, 21, 32, 48, q, None, None) == A              # d_logits off a 16-byte boundary
    assert L.vitx_op_dense_labels(p, 128, 1, 2, 3, 21, 32, 48, q, q + 1, None) == A                 # d_score off a 4-byte boundary
    assert host(p, 24, 1, 2, 3, 21, 32, 48, q) == 0                              # ld = K rounded up to 4 is enough
    # vitx_op_dense: refused before any device call
    z = lambda *a: L.vitx_op_dense(*a, None)
    assert z(1, None, p, p, p, 1, 2, 3, 21, 64, 32, 48, q, None) == A and z(2, p, p, p, p, 1, 2, 3, 21, 64, 32, 48, q, None) == A
    assert z(1, p, p, p, p, 1, 2, 3, 21, 0, 32, 48, q, None) == A and z(1, p, p, p, p, 1, 2, 3, 0, 64, 32, 48, q, None) == A
    assert z(1, p + 4, p, p, p, 1, 2, 3, 21, 64, 32, 48, q, None) == A
    assert z(1, p, p, p, p, 1, 2, 3, 21, 96, 32, 48, q, None) == U and z(1, p, p, p, p, 1, 2, 3, 257, 64, 32, 48, q, None) == U
    assert z(1, p, p, p, p, 1, 2, 3, 21, 64, 1, 48, q, None) == U
    assert z(1, p, p, p, p, 65535, 64, 64, 21, 64, 64, 64, q, None) == U and b"byte window" in L.vitx_last_error()      # 268 million operand rows
