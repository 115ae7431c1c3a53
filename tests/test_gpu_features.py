"""Image embeddings and token features (vitx_feat_enable / vitx_feat_read / vitx_op_features, include/vitx.h).

F = the f32 final LayerNorm of the residual stream, before its rounding to the operand type.  Checked
  - op level: rounded to bf16 / fp16 it IS vitx_op_layernorm's output, bit for bit; against float64 under exact_data.ln_bound; the pooled
    mean and the L2 scale under the contract's bounds (tests/feature_data.py); whole buffers inside NaN canaries; strides;
  - end to end: against float64 from the context's own residual-stream trace, the logits recomputed from the returned class embedding,
    against the oracle, for bits (features on / off, batch, streams, LayerNorm fusion, graph cache), for other models and operand modes,
    for its errors, and through the CLI and the C++ header."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as X
import feature_data as FD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = 3, 5
U24 = 2.0 ** -24


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ op level
class _Op:
    """One vitx_op_features launch on x [n_img][N][D] with NaN rows around the input and NaN canaries around every output."""
    PAD = 8          # NaN rows before and after the addressed rows of X
    GUARD = 1024     # NaN floats before and after every output

    def __init__(self, torch, binding, x, w, b, cls=True, mean=True, tokens=True, l2=False, gap=0, eps=X.LN_EPS):
        n_img, N, D = x.shape
        self.n_img, self.N, self.D, self.gap = n_img, N, D, gap
        nan = float("nan")
        xbuf = torch.full(((n_img * N + 2 * self.PAD), D), nan, dtype=torch.float32, device="cuda")
        xbuf[self.PAD:self.PAD + n_img * N] = _dev(torch, x.reshape(n_img * N, D))
        dw, db = _dev(torch, w), _dev(torch, b)
        sizes = {"cls": D if cls else 0, "mean": D if mean else 0, "tokens": (N - 1) * D if tokens else 0}
        self.stride = sum(sizes.values()) + gap                  # the packed per-image layout of the engine (+ an untouched gap)
        self.buf = torch.full((2 * self.GUARD + n_img * self.stride,), nan, dtype=torch.float32, device="cuda")
        self.off, o = {}, self.GUARD
        for k in ("cls", "mean", "tokens"):
            self.off[k] = o if sizes[k] else None
            o += sizes[k]
        self.sizes = sizes
        ptr = lambda k: self.buf.data_ptr() + 4 * self.off[k] if self.off[k] is not None else 0
        binding.op_features(xbuf.data_ptr() + 4 * self.PAD * D, D, N * D, dw.data_ptr(), db.data_ptr(), ptr("cls"), ptr("mean"), ptr("tokens"), self.stride,
                            n_img, N, D, eps, l2)
        torch.cuda.synchronize()
        self.host = self.buf.cpu().numpy()

    def get(self, k):
        n, s = self.n_img, self.sizes[k]
        v = np.stack([self.host[self.off[k] + i * self.stride:self.off[k] + i * self.stride + s] for i in range(n)])
        return v.reshape(n, self.N - 1, self.D) if k == "tokens" else v

    def check_untouched(self):
        """The guards before and after, and the gap behind every image's payload, still hold NaN; the payload is finite."""
        h, G = self.host, self.GUARD
        assert np.isnan(h[:G]).all() and np.isnan(h[-G:]).all()
        body = h[G:-G].reshape(self.n_img, self.stride)
        pay = self.stride - self.gap
        assert np.isfinite(body[:, :pay]).all()
        if self.gap:
            assert np.isnan(body[:, pay:]).all()


def _layernorm_bits(torch, binding, rows, w, b, dt):
    """vitx_op_layernorm of [M][D] rows -> int16 bits of the operand type."""
    M, D = rows.shape
    tdt = torch.float16 if dt == binding.F16 else torch.bfloat16
    y = torch.zeros((M, D), dtype=tdt, device="cuda")
    dx, dw, db = _dev(torch, rows), _dev(torch, w), _dev(torch, b)
    binding.check(binding.lib().vitx_op_layernorm(dt, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), y.data_ptr(), M, D, X.LN_EPS, None), "vitx_op_layernorm")
    torch.cuda.synchronize()
    return y.cpu().view(torch.int16).numpy()


@pytest.mark.parametrize("D", X.LN_WIDTHS)
def test_op_features_rounded_are_the_layernorm_kernels_bits_and_within_the_f64_bound(binding, torch_gpu, D):
    """Every instantiated width, N in {2, 17, 65, 197, 577, 785}, hostile and random rows.
    1. The f32 class and token outputs, rounded to nearest even by torch, equal vitx_op_layernorm's bf16 and fp16 outputs bit for bit.
    2. They are within exact_data.ln_bound (ulp_out = 2^-23) of the float64 LayerNorm.
    3. The pooled mean is within the fixed-order-sum bound of the float64 mean of the launch's own token output."""
    torch = torch_gpu
    w, b = X.ln_params(D)
    for N in FD.OP_TOKENS:
        n_img = 8 if N <= 65 else 3
        for kind, x in (("hostile", FD.mixed_images(D, n_img, N, seed=N)), ("random", FD.random_images(D, n_img, N, seed=N))):
            op = _Op(torch, binding, x, w, b)
            op.check_untouched()
            cls, mean, tok = op.get("cls"), op.get("mean"), op.get("tokens")
            f = np.concatenate([cls[:, None, :], tok], axis=1)                    # [n_img][N][D] in the rows' order
            assert np.isfinite(f).all()
            for dt, tdt in ((binding.BF16, torch.bfloat16), (binding.F16, torch.float16)):
                want = _layernorm_bits(torch, binding, x.reshape(n_img * N, D), w, b, dt)
                got = torch.from_numpy(f.reshape(n_img * N, D)).to(tdt).view(torch.int16).numpy()
                assert np.array_equal(got, want), (kind, N, dt, int((got != want).sum()))
            y64, bound = FD.features64(x, w, b)
            ratio = float((np.abs(f - y64) / bound).max())
            print(f"D {D} N {N} {kind}: max |F - F64| / ln_bound = {ratio:.3f}")
            assert ratio <= 1.0, (kind, N, ratio)
            m64, mb = FD.mean_bound(tok)
            mr = float((np.abs(mean - m64) / np.maximum(mb, 1e-300)).max())
            print(f"D {D} N {N} {kind}: max |mean - mean64| / bound = {mr:.3f}")
            assert (np.abs(mean - m64) <= mb).all(), (kind, N, mr)


@pytest.mark.parametrize("D,N", [(128, 17), (192, 197), (768, 197), (1024, 65), (1152, 65), (2048, 17)])
def test_op_features_l2(binding, torch_gpu, D, N):
    """VITX_FEAT_L2: the returned class and mean vectors have float64 norm within 4 * 2^-24 * sqrt(D) of 1 and equal v / ||v|| of the
    un-normalised output of a second launch within 8 * 2^-24 per element; the tokens are the same bits with and without it; w = b = 0 gives
    zeros, not NaN."""
    torch = torch_gpu
    w, b = X.ln_params(D)
    for x in (FD.mixed_images(D, 4, N, seed=3), FD.random_images(D, 4, N, seed=3)):
        raw = _Op(torch, binding, x, w, b, l2=False)
        nrm = _Op(torch, binding, x, w, b, l2=True)
        nrm.check_untouched()
        assert np.array_equal(_bits(raw.get("tokens")), _bits(nrm.get("tokens")))
        for k in ("cls", "mean"):
            v = raw.get(k).astype(np.float64)
            u = nrm.get(k).astype(np.float64)
            assert np.abs(np.linalg.norm(u, axis=1) - 1.0).max() <= 4 * U24 * np.sqrt(D), k
            assert np.abs(u - v / np.linalg.norm(v, axis=1, keepdims=True)).max() <= 8 * U24, k
    z = _Op(torch, binding, FD.random_images(D, 2, N, seed=4), np.zeros(D, np.float32), np.zeros(D, np.float32), l2=True)
    z.check_untouched()
    assert not z.get("cls").any() and not z.get("mean").any() and not z.get("tokens").any()


@pytest.mark.parametrize("D,N", [(64, 17), (768, 197), (1024, 65), (1280, 17)])
def test_op_features_whole_buffer_null_outputs_gaps_and_strides(binding, torch_gpu, D, N):
    """Outputs passed as NULL write nothing and change no other output's bits; an out_img_stride larger than the payload leaves the gaps
    untouched; NaN rows around X are never read (every output stays finite, _Op.check_untouched); the class embedding computed from a
    compact [n][1][D] input (the class-rows-only last layer's shape) is the same bits as from the full tensor."""
    torch = torch_gpu
    w, b = X.ln_params(D)
    x = FD.mixed_images(D, 5, N, seed=9)
    full = _Op(torch, binding, x, w, b)
    full.check_untouched()
    for sel in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0)):
        op = _Op(torch, binding, x, w, b, cls=bool(sel[0]), mean=bool(sel[1]), tokens=bool(sel[2]), gap=4 * (1 + sum(sel)))
        op.check_untouched()
        for k, on in zip(("cls", "mean", "tokens"), sel):
            if on:
                assert np.array_equal(_bits(op.get(k)), _bits(full.get(k))), (sel, k)
    compact = _Op(torch, binding, x[:, :1].copy(), w, b, cls=True, mean=False, tokens=False)
    compact.check_untouched()
    assert np.array_equal(_bits(compact.get("cls")), _bits(full.get("cls")))
    # images far apart in memory (img_stride > N * D) and rows far apart (row_stride > D)
    wide = torch.full((5, N, 2, D + 64), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :, 0, :D] = _dev(torch, x)
    out = torch.full((5, N, D), float("nan"), dtype=torch.float32, device="cuda")
    dw, db = _dev(torch, w), _dev(torch, b)
    binding.op_features(wide.data_ptr(), 2 * (D + 64), N * 2 * (D + 64), dw.data_ptr(), db.data_ptr(), out.data_ptr(), 0, out.data_ptr() + 4 * D, N * D, 5, N, D, X.LN_EPS)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[:, 0]), _bits(full.get("cls"))) and np.array_equal(_bits(got[:, 1:]), _bits(full.get("tokens")))


def test_op_features_argument_checks(binding, torch_gpu):
    torch = torch_gpu
    L = binding.lib()
    x = torch.zeros((4 * 17 * 128,), dtype=torch.float32, device="cuda")
    o = torch.zeros((4 * 17 * 128,), dtype=torch.float32, device="cuda")
    p, q = x.data_ptr(), o.data_ptr()
    assert L.vitx_op_features(p, 128, 17 * 128, p, p, None, None, None, 128, 4, 17, 128, 1e-6, 0, None) == ERR_ARG           # nothing to write
    assert L.vitx_op_features(None, 128, 17 * 128, p, p, q, None, None, 128, 4, 17, 128, 1e-6, 0, None) == ERR_ARG
    assert L.vitx_op_features(p, 128, 128, p, p, None, q, None, 128, 4, 1, 128, 1e-6, 0, None) == ERR_ARG                    # N == 1 with mean
    assert L.vitx_op_features(p, 128, 128, p, p, None, None, q, 128, 4, 1, 128, 1e-6, 0, None) == ERR_ARG                    # N == 1 with tokens
    assert L.vitx_op_features(p, 100, 1700, p, p, q, None, None, 100, 4, 17, 100, 1e-6, 0, None) == ERR_UNSUPPORTED          # no instantiation
    assert L.vitx_op_features(p + 4, 128, 17 * 128, p, p, q, None, None, 128, 4, 17, 128, 1e-6, 0, None) == ERR_ARG          # alignment
    assert L.vitx_op_features(p, 128, 17 * 128, p, p, q, None, None, 130, 4, 17, 128, 1e-6, 0, None) == ERR_ARG              # stride
    assert L.vitx_op_features(p, 128, 128, p, p, q, None, None, 128, 4, 1, 128, 1e-6, 0, None) == 0                          # N == 1, class rows only
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end: helpers
def _synthetic(pkg, name, **kw):
    return pkg.synth.cached_synthetic(name, head_scale=4.0, **kw)


def _images(pkg, n, size, seed):
    return pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, size, seed=seed))


def _forward_dev(torch, ctx, imgs):
    d = _dev(torch, imgs)
    n = imgs.shape[0]
    C = ctx.model.num_classes
    p = torch.empty((n, C), dtype=torch.float32, device="cuda"); lg = torch.empty((n, C), dtype=torch.float32, device="cuda")
    ctx.forward_device(d.data_ptr(), n, p.data_ptr(), lg.data_ptr(), 0)
    ctx.synchronize()
    return p.cpu().numpy(), lg.cpu().numpy()


def _norm_params(model):
    idx = {name: i for i, (name, *_rest) in enumerate(model.tensors())}
    vec = lambda name: model.tensor_f32(idx[name]).reshape(-1)
    return idx, vec("norm.weight"), vec("norm.bias")


def _check_against_trace(feats, trace, ids, layers, w, b, eps, where=""):
    """Every feature of the traced images against float64 LayerNorm / mean of the context's OWN traced X_l, under the op-level bounds.
    feats[l][kind][image id]; trace [L + 1][len(ids)][N][D]."""
    worst = 0.0
    for l in layers:
        x = trace[l + 1]                                                    # X_l = stage l + 1
        y64, bound = FD.features64(x, w, b, eps)
        f = feats[l]
        if "cls" in f:
            r = np.abs(f["cls"][ids] - y64[:, 0]) / bound[:, 0]
            worst = max(worst, float(r.max()))
            assert r.max() <= 1.0, (where, l, "cls", float(r.max()))
        if "tokens" in f:
            r = np.abs(f["tokens"][ids] - y64[:, 1:]) / bound[:, 1:]
            worst = max(worst, float(r.max()))
            assert r.max() <= 1.0, (where, l, "tokens", float(r.max()))
            if "mean" in f:
                m64, mb = FD.mean_bound(f["tokens"][ids])
                assert (np.abs(f["mean"][ids] - m64) <= mb).all(), (where, l, "mean")
        elif "mean" in f:                                                   # no token output to take the mean of: the f64 mean of F64, both bounds added
            m64 = y64[:, 1:].mean(axis=1)
            mb = bound[:, 1:].mean(axis=1) + U24 * ((x.shape[1] - 1) * np.abs(y64[:, 1:]).mean(axis=1) + 2 * np.abs(m64))
            assert (np.abs(f["mean"][ids] - m64) <= mb).all(), (where, l, "mean")
    return worst


def _round_operand(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.float16 if dtype == 0 else torch.bfloat16).float().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ wiring at the benchmarked size
@pytest.mark.parametrize("dtype", [0, 1])
def test_features_of_vit_base_at_batch_256_match_the_contexts_own_trace_and_logits(pkg, binding, torch_gpu, dtype):
    """ViT-B/16, batch 256 on two sub-batch streams, F16 and BF16; class, mean and token features of layers {0, L/2, L-1}; the images on
    either side of every sub-batch boundary and at both ends.  Every feature equals float64 LayerNorm / mean of the context's own traced
    X_l under the op-level bounds, and the logits recomputed in float64 from the returned last-layer class embedding and the head weights
    (rounded to the operand type as the context uploads them) match the forward's within (h + D 2^-24) S_c + 1e-6, S_c = sum|w F| + |bias|:
    h = the half-ulp of the one rounding of the head GEMM's operand (2^-8 bf16, 2^-11 fp16), D 2^-24 = an f32 accumulation of D products."""
    from conftest import boundary_rows
    torch = torch_gpu
    path = _synthetic(pkg, "vit_base_patch16_224")
    ids = boundary_rows(binding, path, 256, dtype)
    model = binding.Model(path)
    hp = model.hparams
    L, D = hp.num_hidden_layers, hp.hidden_size
    layers = [0, L // 2, L - 1]
    imgs = _images(pkg, 256, 224, seed=2025)
    ctx = binding.Context(model, device=0, max_batch=256, dtype=dtype)
    assert len(ctx.split(256)) == 2
    ctx.trace_enable(ids)
    ctx.feat_enable(cls=True, mean=True, tokens=True, layers=layers)
    probs, logits = _forward_dev(torch, ctx, imgs)
    trace = ctx.trace_read()
    feats = ctx.feat_read(256)
    assert sorted(feats) == layers and feats[0]["tokens"].shape == (256, 196, D)
    for l in layers:
        for k in ("cls", "mean", "tokens"):
            assert np.isfinite(feats[l][k]).all()
    idx, w, b = _norm_params(model)
    worst = _check_against_trace(feats, trace, ids, layers, w, b, hp.eps, "vit_base")
    print(f"dtype {dtype}: max |F - F64(trace)| / ln_bound = {worst:.3f}")
    Wh = _round_operand(torch, model.tensor_f32(idx["head.weight"]).reshape(hp.num_classes, D), dtype)
    bh = model.tensor_f32(idx["head.bias"]).reshape(-1).astype(np.float64)
    F = feats[L - 1]["cls"].astype(np.float64)                               # all 256 images
    want = F @ Wh.T + bh
    S = np.abs(F) @ np.abs(Wh).T + np.abs(bh)
    h = 2.0 ** -11 if dtype == 0 else 2.0 ** -8
    r = np.abs(logits - want) / ((h + D * U24) * S + 1e-6)
    print(f"dtype {dtype}: max |logit - logit64(F_cls)| / bound = {float(r.max()):.3f}")
    assert r.max() <= 1.0, float(r.max())
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ against the oracle
# 1 - cos against the oracle's embedding, measured on an MI355X (the worst of the 6 checked images; the test prints it).  The assertion is 2 x that.
ORACLE_COS = {0: {"cls": 3.244e-07, "mean": 3.772e-09},        # F16 against oracle.REF
              1: {"cls": 1.469e-05, "mean": 2.364e-07}}        # BF16 against oracle.GPU_BF16


@pytest.mark.parametrize("dtype", [0, 1])
def test_last_layer_features_of_vit_base_against_the_oracle(pkg, binding, oracle, torch_gpu, dtype):
    """vit_base_patch16_224, head_scale 4, batch 256.  Oracle: OracleModel.forward(dump) then oracle.layernorm with the final norm -- for F16
    with the reference's rounding points (oracle.REF), for BF16 with the bf16 ones (oracle.GPU_BF16).
    F16: the two ratios tests/test_gpu_parity_r02.py holds X_l to (max error <= 2.5e-2 x RMS, RMS error <= 2e-3 x RMS) on the last layer's
    class + token rows: the norm rescales rows to unit variance and norm.weight of the synthetic files is 1 +- 0.02, so the band carries over.
    BF16: that file's band for the bf16 stream against the bf16 oracle (RMS error <= 1.5e-2 x RMS; it sets no bound on the maximum).
    1 - cos of the class and mean embeddings against the oracle's, worst image: asserted <= 2 x the value measured on an MI355X
    (ORACLE_COS: F16 cls 3.2e-7, mean 3.8e-9; BF16 cls 1.5e-5, mean 2.4e-7; the same run measured the last-layer rows at max 3.2e-3 / RMS 4.4e-4
    of the RMS for F16 and RMS 3.0e-3 for BF16) -- the inputs are seeded and the kernels deterministic; the factor leaves room for a legitimate change of an upstream
    GEMM's accumulation order, which moves the figure inside the operand-rounding band."""
    from conftest import boundary_rows
    torch = torch_gpu
    path = _synthetic(pkg, "vit_base_patch16_224")
    ids = boundary_rows(binding, path, 256, dtype)
    model = binding.Model(path)
    hp = model.hparams
    L, D = hp.num_hidden_layers, hp.hidden_size
    imgs = _images(pkg, 256, 224, seed=2025)
    ctx = binding.Context(model, device=0, max_batch=256, dtype=dtype)
    ctx.feat_enable(cls=True, mean=True, tokens=True)
    _forward_dev(torch, ctx, imgs)
    f = ctx.feat_read(256)[L - 1]
    ctx.close(); model.close()
    om = oracle.OracleModel(path)
    _, _, xd = om.forward(imgs[ids], oracle.REF if dtype == 0 else oracle.GPU_BF16, dump=True)
    N = xd.shape[1] // len(ids)
    ref = oracle.layernorm(xd[L], om.tensor("norm.weight").reshape(-1), om.tensor("norm.bias").reshape(-1), hp.eps).reshape(len(ids), N, D).astype(np.float64)
    got = np.concatenate([f["cls"][ids][:, None, :], f["tokens"][ids]], axis=1).astype(np.float64)
    rms = float(np.sqrt((ref ** 2).mean()))
    e_max, e_rms = float(np.abs(got - ref).max()) / rms, float(np.sqrt(((got - ref) ** 2).mean())) / rms
    print(f"dtype {dtype}: last-layer F vs oracle: max error {e_max:.3e} x RMS, RMS error {e_rms:.3e} x RMS")
    cos = lambda a, c: (a * c).sum(axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(c, axis=1))
    d_cls = float((1.0 - cos(f["cls"][ids].astype(np.float64), ref[:, 0])).max())
    d_mean = float((1.0 - cos(f["mean"][ids].astype(np.float64), ref[:, 1:].mean(axis=1))).max())
    print(f"dtype {dtype}: 1 - cos vs oracle, worst of {len(ids)} images: cls {d_cls:.3e}, mean {d_mean:.3e}")
    if dtype == 0:
        assert e_max <= 2.5e-2 and e_rms <= 2e-3, (e_max, e_rms)
    else:
        assert e_rms <= 1.5e-2, e_rms
    assert d_cls <= 2 * ORACLE_COS[dtype]["cls"] and d_mean <= 2 * ORACLE_COS[dtype]["mean"], (d_cls, d_mean)


# ------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("n", [1, 5, 256])
def test_probabilities_and_logits_bits_with_features_on(pkg, binding, torch_gpu, dtype, n):
    """1. Class embedding of the last layer only (+ anything of earlier layers): probabilities and logits are the bits of features off.
    2. Mean or tokens of the last layer: they are the bits of a last_layer_all_rows = 1 context with features off.
    6. The class embedding of a last_layer_all_rows = 1 context is row 0 of the every-row path reached through mean / tokens."""
    torch = torch_gpu
    path = _synthetic(pkg, "vit_tiny_patch16_224")
    model = binding.Model(path)
    imgs = _images(pkg, n, 224, seed=5)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype)
    allr = binding.Context(model, device=0, max_batch=n, dtype=dtype, last_layer_all_rows=1)
    p0, l0 = _forward_dev(torch, ctx, imgs)
    pa, la = _forward_dev(torch, allr, imgs)
    ctx.feat_enable(cls=True)
    p1, l1 = _forward_dev(torch, ctx, imgs)
    assert np.array_equal(_bits(p1), _bits(p0)) and np.array_equal(_bits(l1), _bits(l0))
    ctx.feat_enable(cls=True, mean=True, tokens=True, layers=[0, 6])          # intermediate layers never change the forward
    p1, l1 = _forward_dev(torch, ctx, imgs)
    assert np.array_equal(_bits(p1), _bits(p0)) and np.array_equal(_bits(l1), _bits(l0))
    allr.feat_enable(cls=True)
    pc, lc = _forward_dev(torch, allr, imgs)
    cls_allrows = allr.feat_read(n)[11]["cls"].copy()
    assert np.array_equal(_bits(pc), _bits(pa)) and np.array_equal(_bits(lc), _bits(la))
    for kw in ({"mean": True}, {"tokens": True}, {"cls": False, "mean": True}):
        ctx.feat_enable(**kw)
        p2, l2 = _forward_dev(torch, ctx, imgs)
        assert np.array_equal(_bits(p2), _bits(pa)) and np.array_equal(_bits(l2), _bits(la)), kw
        f = ctx.feat_read(n)[11]
        if "cls" in f:
            assert np.array_equal(_bits(f["cls"]), _bits(cls_allrows)), kw
    ctx.feat_disable()
    p3, l3 = _forward_dev(torch, ctx, imgs)
    assert np.array_equal(_bits(p3), _bits(p0)) and np.array_equal(_bits(l3), _bits(l0))
    ctx.close(); allr.close(); model.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_feature_bits_of_an_image_do_not_depend_on_batch_position_or_streams(pkg, binding, torch_gpu, dtype):
    """3. An image's features are identical at batch 1, 2, 17 and 256, at any position in the batch, and with one and two streams."""
    from conftest import boundary_rows
    torch = torch_gpu
    path = _synthetic(pkg, "vit_tiny_patch16_224")
    ids = boundary_rows(binding, path, 256, dtype)
    model = binding.Model(path)
    imgs = _images(pkg, 256, 224, seed=8)
    layers = [0, 6, 11]
    flat = lambda f, i: np.concatenate([f[l][k][i].reshape(-1) for l in layers for k in ("cls", "mean", "tokens")])
    ctx = binding.Context(model, device=0, max_batch=256, dtype=dtype)
    assert len(ctx.split(256)) == 2
    ctx.feat_enable(cls=True, mean=True, tokens=True, layers=layers)
    _forward_dev(torch, ctx, imgs)
    big = ctx.feat_read(256)
    want = {i: flat(big, i).copy() for i in ids}
    one = binding.Context(model, device=0, max_batch=256, dtype=dtype, streams=1)
    one.feat_enable(cls=True, mean=True, tokens=True, layers=layers)
    _forward_dev(torch, one, imgs)
    f1 = one.feat_read(256)
    for i in ids:
        assert np.array_equal(_bits(flat(f1, i)), _bits(want[i])), ("streams=1", i)
    for i in ids:
        _forward_dev(torch, ctx, imgs[i:i + 1])
        assert np.array_equal(_bits(flat(ctx.feat_read(1), 0)), _bits(want[i])), ("batch 1", i)
    i = ids[len(ids) // 2]
    for n, pos in ((2, 1), (17, 0), (17, 9), (17, 16)):                      # the image at another position of a smaller batch
        batch = imgs[:n].copy(); batch[pos] = imgs[i]
        _forward_dev(torch, ctx, batch)
        assert np.array_equal(_bits(flat(ctx.feat_read(n), pos)), _bits(want[i])), (n, pos)
    ctx.close(); one.close(); model.close()


def test_feature_bits_with_layernorm_fusion_off_and_with_the_graph_option(pkg, binding, torch_gpu):
    """4. no_ln_fusion = 1 gives the same features (ViT-B at 128 images: the shape whose residual GEMMs fuse the LayerNorm).
    5. A graph = 1 context gives the same features: the cache is bypassed while they are on and replays again once they are off."""
    torch = torch_gpu
    path = _synthetic(pkg, "vit_base_patch16_224")
    model = binding.Model(path)
    imgs = _images(pkg, 128, 224, seed=12)
    got = []
    for opts in ({}, {"no_ln_fusion": 1}):
        ctx = binding.Context(model, device=0, max_batch=128, dtype=binding.BF16, **opts)
        ctx.feat_enable(cls=True, mean=True, tokens=True, layers=[3, 11])
        _forward_dev(torch, ctx, imgs)
        got.append(ctx.feat_read(128))
        if not opts:
            assert ctx.ln_fusion_active() == 1
        ctx.close()
    for l in (3, 11):
        for k in ("cls", "mean", "tokens"):
            assert np.array_equal(_bits(got[0][l][k]), _bits(got[1][l][k])), (l, k)
    model.close()

    path = _synthetic(pkg, "vit_tiny_patch16_224")
    model = binding.Model(path)
    imgs = _images(pkg, 4, 224, seed=10)
    ref = binding.Context(model, device=0, max_batch=4, dtype=binding.F16, graph=0)
    p_ref = ref.forward(imgs)
    ref.feat_enable(cls=True, layers=[5, 11])
    ref.forward(imgs)
    f_ref = ref.feat_read()
    ctx = binding.Context(model, device=0, max_batch=4, dtype=binding.F16, graph=1)
    for _ in range(2):
        assert np.array_equal(_bits(ctx.forward(imgs)), _bits(p_ref))
    assert ctx.graph_launches() == 1
    ctx.feat_enable(cls=True, layers=[5, 11])
    for _ in range(2):
        assert np.array_equal(_bits(ctx.forward(imgs)), _bits(p_ref))
        f = ctx.feat_read()
        assert all(np.array_equal(_bits(f[l]["cls"]), _bits(f_ref[l]["cls"])) for l in (5, 11))
    assert ctx.graph_launches() == 1
    ctx.feat_disable()
    assert np.array_equal(_bits(ctx.forward(imgs)), _bits(p_ref)) and ctx.graph_launches() == 2
    ctx.close(); ref.close(); model.close()


# Relative L2 distance of the class embedding, class-rows-only tail against the every-row last layer (the reference's graph), worst of 64
# images of vit_base_patch16_224; measured on an MI355X (the test prints it).  The assertion is 2 x that.
TAIL_REL_L2 = {0: 7.439e-05, 1: 2.628e-04}


@pytest.mark.parametrize("dtype", [0, 1])
def test_class_embedding_of_the_class_rows_only_tail_against_the_whole_graph(pkg, binding, torch_gpu, dtype):
    """Not exact, by the header's own statement for last_layer_all_rows: the tail's GEMMs run other tile shapes on other rows.  ViT-B at
    batch 64; measured 7.4e-5 (F16) and 2.6e-4 (BF16), beside the 3.0e-4 / 1.1e-3 the probabilities move by."""
    torch = torch_gpu
    path = _synthetic(pkg, "vit_base_patch16_224")
    model = binding.Model(path)
    imgs = _images(pkg, 64, 224, seed=2025)
    e = []
    for all_rows in (0, 1):
        ctx = binding.Context(model, device=0, max_batch=64, dtype=dtype, last_layer_all_rows=all_rows)
        ctx.feat_enable(cls=True)
        _forward_dev(torch, ctx, imgs)
        e.append(ctx.feat_read(64)[11]["cls"].astype(np.float64))
        ctx.close()
    model.close()
    rel = float((np.linalg.norm(e[0] - e[1], axis=1) / np.linalg.norm(e[1], axis=1)).max())
    print(f"dtype {dtype}: class embedding, tail vs every row: worst relative L2 distance {rel:.3e}")
    assert rel <= 2 * TAIL_REL_L2[dtype], rel


# ------------------------------------------------------------------------------------------------ other models and operand modes
@pytest.mark.parametrize("name,dtype,n,quant", [("vit_micro_patch16_64", 0, 9, 0), ("vit_micro_patch16_64", 1, 9, 0), ("vit_mini_hd72_patch14_112", 1, 5, 0),
                                                ("vit_micro_patch8_224", 0, 3, 0), ("vit_tiny_patch16_224", 1, 5, 2), ("vit_small_patch16_224", 2, 6, 0)])
def test_features_of_other_models_match_their_own_trace(pkg, binding, torch_gpu, tmp_path, name, dtype, n, quant):
    """D = 128 (flat statistics, N = 17), D = 1152, N = 785, a q4_0 file, an MXFP8 context: every layer, all three kinds, every image."""
    torch = torch_gpu
    path = _synthetic(pkg, name)
    if quant:
        q = str(tmp_path / "q.gguf")
        binding.quantize_file(path, q, quant)
        path = q
    model = binding.Model(path)
    hp = model.hparams
    L = hp.num_hidden_layers
    imgs = _images(pkg, n, hp.img_size, seed=31)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype)
    ids = list(range(n))
    ctx.trace_enable(ids)
    ctx.feat_enable(cls=True, mean=True, tokens=True, layers=range(L))
    ctx.forward(imgs)
    trace, feats = ctx.trace_read(), ctx.feat_read(n)
    _, w, b = _norm_params(model)
    worst = _check_against_trace(feats, trace, ids, list(range(L)), w, b, hp.eps, name)
    print(f"{name} dtype {dtype}: max |F - F64(trace)| / ln_bound = {worst:.3f}")
    # the same context with the trace off and the class embedding only: the class-rows-only tail runs the kernel on the compact class rows
    ctx.trace_enable([])
    ctx.feat_enable(cls=True, l2=True)
    ctx.forward(imgs)
    c = ctx.feat_read(n)[L - 1]["cls"].astype(np.float64)
    assert np.abs(np.linalg.norm(c, axis=1) - 1.0).max() <= 4 * U24 * np.sqrt(hp.hidden_size)
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ errors
def test_feature_errors(pkg, binding, torch_gpu):
    L = binding.lib()
    path = pkg.synth.cached_synthetic("vit_micro_patch16_64")
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=4, dtype=binding.F16)
    h = ctx._h
    assert L.vitx_feat_enable(h, binding.FEAT_CLS, 1 << 2) == ERR_ARG               # the model has 2 layers
    assert L.vitx_feat_enable(h, 16, 0) == ERR_ARG                                  # unknown flag
    assert L.vitx_feat_enable(h, binding.FEAT_L2, 0) == ERR_ARG                     # the modifier alone
    assert L.vitx_feat_floats(h) == 0 and L.vitx_feat_device(h) is None
    ctx.feat_enable(cls=True, mean=True, tokens=True, layers=[1])
    fpi = 128 * (1 + 1 + 16)
    assert L.vitx_feat_floats(h) == fpi and L.vitx_feat_device(h)
    buf = np.empty(4 * fpi, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.vitx_feat_read(h, fp, buf.size) == ERR_ARG                             # before any forward with features on
    imgs = _images(pkg, 3, 64, seed=1)
    ctx.forward(imgs)
    assert L.vitx_feat_read(h, fp, 3 * fpi - 1) == ERR_ARG                          # too small
    assert L.vitx_feat_read(h, fp, 3 * fpi) == 0 and L.vitx_feat_images(h) == 3
    with pytest.raises(ValueError):
        ctx.feat_read(4)
    f = ctx.feat_read()
    assert f[1]["tokens"].shape == (3, 16, 128) and np.array_equal(buf[:fpi][:128], f[1]["cls"][0])
    ptr, n_f = ctx.feat_device()
    assert ptr and n_f == fpi
    ctx.feat_enable(cls=True)                                                       # layer mask 0 = the last layer; re-enabling forgets the last forward
    assert L.vitx_feat_floats(h) == 128 and L.vitx_feat_read(h, fp, buf.size) == ERR_ARG
    ctx.feat_disable()                                                              # frees; a later forward succeeds
    assert L.vitx_feat_floats(h) == 0 and L.vitx_feat_device(h) is None and L.vitx_feat_read(h, fp, buf.size) == ERR_ARG
    p = ctx.forward(imgs)
    assert np.isfinite(p).all()
    # maps and features together: both still come out right
    ctx.attn_enable([0, 1], rollout=True)
    ctx.forward(imgs)
    cls0, roll0 = ctx.attn_read()
    ctx.attn_disable()
    ctx.feat_enable(cls=True, mean=True, layers=[0, 1])
    ctx.forward(imgs)
    f0 = ctx.feat_read()
    ctx.attn_enable([0, 1], rollout=True)
    p_both = ctx.forward(imgs)
    cls1, roll1 = ctx.attn_read()
    f1 = ctx.feat_read()
    assert np.array_equal(_bits(cls1), _bits(cls0)) and np.array_equal(_bits(roll1), _bits(roll0))
    assert all(np.array_equal(_bits(f1[l][k]), _bits(f0[l][k])) for l in (0, 1) for k in ("cls", "mean"))
    assert np.isfinite(p_both).all()
    ctx.close(); model.close()

    st = binding.Model(pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0))
    sctx = binding.Context(st, device=0, max_batch=1, dtype=binding.F16)
    assert L.vitx_feat_enable(sctx._h, binding.FEAT_CLS, 0) == ERR_UNSUPPORTED
    assert L.vitx_feat_enable(sctx._h, 0, 0) == 0                                   # off is always accepted
    sctx.close(); st.close()


def test_features_take_one_pass(pkg, binding, torch_gpu):
    """A forward of more images than one pass of the kernels takes is refused with features on, before anything runs."""
    torch = torch_gpu
    L = binding.lib()
    model = binding.Model(_synthetic(pkg, "vit_base_patch16_224"))
    ctx = binding.Context(model, device=0, max_batch=2300, dtype=binding.F16, streams=1)
    limit = ctx.split(2300)[0]
    assert limit < 2300
    ctx.feat_enable(cls=True)
    n = limit + 1
    x = torch.zeros((n, 224, 224, 3), dtype=torch.float32, device="cuda")            # sized for the call: memory-safe even if the check were gone
    p = torch.zeros((n, model.num_classes), dtype=torch.float32, device="cuda")
    assert L.vitx_forward_device(ctx._h, x.data_ptr(), n, p.data_ptr(), None, None) == ERR_ARG
    assert L.vitx_feat_images(ctx._h) == 0
    ctx.close(); model.close()


def test_profile_reports_the_feature_launches(pkg, binding, torch_gpu):
    """Profiling reports one launch per selected layer and sub-batch under the class `features`, with its algorithmic bytes; none while off."""
    torch = torch_gpu
    model = binding.Model(_synthetic(pkg, "vit_tiny_patch16_224"))
    n, N, D = 32, 197, 192
    imgs = _images(pkg, n, 224, seed=2)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=binding.BF16)
    ctx.profile_enable(True)
    _forward_dev(torch, ctx, imgs)
    assert "features" not in [p["name"] for p in ctx.profile_read()]
    ctx.feat_enable(cls=True, tokens=True, layers=[4, 11])
    _forward_dev(torch, ctx, imgs)
    pr = {p["name"]: p for p in ctx.profile_read()}
    ctx.profile_enable(False)
    parts = len(ctx.split(n))
    assert pr["features"]["launches"] == 2 * parts
    assert pr["features"]["bytes"] == 2 * (n * N * D * 4 + n * N * D * 4)            # every row read once, class + token rows written
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ interfaces
@pytest.mark.parametrize("kind,l2", [("cls", False), ("mean", True), ("tokens", False)])
def test_cli_embed_writes_the_rows_feat_read_returns(pkg, binding, torch_gpu, tmp_path, kind, l2):
    path = _synthetic(pkg, "vit_tiny_patch16_224")
    u8 = pkg.synth.synthetic_images_u8(3, 224, seed=11)
    out = tmp_path / "emb.npy"
    cli = [sys.executable, os.path.join(ROOT, "vit_cli.py"), "-m", path, "--embed", str(out), "--embed-kind", kind] + (["--embed-l2"] if l2 else [])

    def ppm(p, img):
        p.write_bytes(b"P6\n224 224\n255\n" + np.ascontiguousarray(img, np.uint8).tobytes())

    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=binding.F16)
    ctx.feat_enable(cls=kind == "cls", mean=kind == "mean", tokens=kind == "tokens", l2=l2)
    x = np.stack([binding.preprocess(u, 224) for u in u8])
    # one image (-i): one row, the classification lines unchanged
    ppm(tmp_path / "img.ppm", u8[0])
    r = subprocess.run(cli + ["-i", str(tmp_path / "img.ppm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count(" > ") == 5
    ctx.forward(x[:1])
    want = ctx.feat_read(1)[11][kind]
    got = np.load(out)
    assert got.shape == (1,) + want.shape[1:] and np.array_equal(_bits(got), _bits(want))
    # a directory: one row per image in walk order + the list of names
    lab = model.label(3)                                                     # one label directory: the walk order is the sorted file names
    (tmp_path / "val" / lab).mkdir(parents=True)
    for i in range(3):
        ppm(tmp_path / "val" / lab / f"im{i}.ppm", u8[i])
    r = subprocess.run(cli + ["--dir", str(tmp_path / "val"), "--batch", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "top-1 accuracy:" in r.stdout
    ctx.forward(x)
    want = ctx.feat_read(3)[11][kind]
    got = np.load(out)
    assert np.array_equal(_bits(got), _bits(want))
    listed = open(str(out) + ".txt").read().split("\n")[:-1]
    assert [os.path.basename(p) for p in listed] == ["im0.ppm", "im1.ppm", "im2.ppm"]
    ctx.close(); model.close()


def test_cpp_example_embed_main_prints_cosine_similarities(pkg, binding, torch_gpu, tmp_path):
    """examples/embed_main.cpp built with g++ against vit.cpp_amd/vit.h + libvitx.so (vit_embed_batch): cosine 1.000000 for an image against
    itself, a value strictly inside (-1, 1) for two different assets."""
    from PIL import Image
    pkgdir = os.path.join(ROOT, "vit.cpp_amd")
    exe = str(tmp_path / "embed_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "examples", "embed_main.cpp"), "-I" + pkgdir, "-L" + pkgdir, "-lvitx", "-L/opt/rocm/lib",
                        "-Wl,-rpath," + pkgdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assets = os.path.join(ROOT, "tests", "golden", "assets")
    files = sorted(f for f in os.listdir(assets) if f.lower().endswith((".jpg", ".jpeg", ".png")))
    assert len(files) >= 2
    a, b = os.path.join(assets, files[0]), os.path.join(assets, files[1])
    path = _synthetic(pkg, "vit_tiny_patch16_224")

    def cosine(p, q):
        r = subprocess.run([exe, path, p, q], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("cosine similarity")]
        assert len(line) == 1, r.stdout
        return line[0].split()[-1]

    assert cosine(a, a) == "1.000000"
    v = float(cosine(a, b))
    assert -1.0 < v < 1.0, v


def test_a_refused_enable_leaves_the_features_on(pkg, binding, torch_gpu):
    """A vitx_feat_enable that is refused for its arguments (unknown flags) leaves the features as they were enabled: the next forward gives the same bits."""
    L = binding.lib()
    model = binding.Model(_synthetic(pkg, "vit_micro_patch16_64"))
    imgs = _images(pkg, 9, 64, seed=3)
    ctx = binding.Context(model, device=0, max_batch=9, dtype=binding.BF16)
    last = model.hparams.num_hidden_layers - 1
    ctx.feat_enable(cls=True, mean=True, tokens=True, l2=True, layers=[0, last])
    _forward_dev(torch_gpu, ctx, imgs)
    first = ctx.feat_read(9)
    fpi = L.vitx_feat_floats(ctx._h)
    assert L.vitx_feat_enable(ctx._h, 0x100 | binding.FEAT_CLS, 0) == binding.ERR_ARG
    _forward_dev(torch_gpu, ctx, imgs)
    assert L.vitx_feat_images(ctx._h) == 9 and L.vitx_feat_floats(ctx._h) == fpi
    again = ctx.feat_read(9)
    for l in (0, last):
        for k in ("cls", "mean", "tokens"):
            assert np.array_equal(_bits(again[l][k]), _bits(first[l][k])), (l, k)
    ctx.close(); model.close()
