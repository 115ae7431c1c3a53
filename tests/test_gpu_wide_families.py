"""Every model family through the wide-batch path: the wide fixtures of tests/wide_data.py (D 512, 3 layers) at a batch whose two sub-batches
run the persistent 256 x 256 GEMMs with norm2 / the next norm1 fused into proj / fc2, and the row blocks a fused launch leaves behind repaired in
the prologue of the GEMM that consumes them (GemmArgs::fix) -- in front of the erf- and QuickGELU fc1 epilogues, the plain fc1 of a gated MLP, the
two-plane qkv epilogue with rope.hip behind it, with 5 prefix rows or none, eps 1e-5 and 1e-12, a pre-norm, the pooled heads.

Per fixture and operand type four contexts of one model: (1) no_ln_fusion, the anchor; (2) the default; (3) ln_test 1, every fifth tile of every
fusing launch forced to fall back; (4) a three-image context that runs the boundary images one by one on the ring tiles.  The logits of 1, 2 and 3
are equal bit for bit over the whole batch, those of 4 equal their rows of it; the profile's `layernorm` launch counts are the ones
tests/wide_data.py derives from forward.cpp, so the fused path is known to have run; and the traced residual stream and the probabilities of the
boundary images lie inside the gates of the family's float64 restatement and outside those of every listed mutant
(tests/test_cpu_wide_data.py: each mutant is at least two gates from the restatement).

Measured on an MI355X, figure / gate of the fusing context against the restatement (worst of probabilities, trace stages and, siglip_map, 1 - cos and
length of e), bf16 | f16 (parity mode) | f16 with f16_fast_attention:
    vit_erf 0.10 | 0.16      clip 0.14 | 0.27      dinov2_reg 0.07 | 0.40      siglip_map 0.94 (1 - cos) | 0.67      dinov3_rope 0.34 | 0.36 | 0.89
    glu_g 0.29 | 0.43        glu_hplus 0.47 | 0.46 | 0.73                     glu_odd 0.28 | 0.45
`layernorm` launches per forward, stand-alone context -> fusing context: vit_erf, dinov3_rope, glu_hplus 14 -> 6; clip 16 -> 8; dinov2_reg, glu_g
12 -> 2; siglip_map 14 -> 4; glu_odd 12 -> 12.  Fix-up tiles of three forced forwards: 624 (class-token heads: 8 fusing launches per forward, at
least 612) and 780 (pooled heads: 10, at least 765); 416 in one forward with real time-outs; 0 on every context that was not forced.
With the consumer GEMM's fix-up prologue normalising with a literal 1e-6 instead of the model's eps (a scratch build), the forced context of vit_erf,
clip (both operand types) and dinov3_rope differs from the stand-alone one on 2400 .. 2700 of 6503 images (1518 of 3614); dinov2_reg (eps 1e-6) passes."""
import numpy as np
import pytest

import prefix_data as PD
import ref64 as R64
import wide_data as WD

pytestmark = pytest.mark.gpu

MODES = {"bf16": (1, {}), "f16": (0, {}), "f16_fast": (0, {"f16_fast_attention": 1})}      # f16: the parity mode (q, k, v in two planes)
CASES = [(k, m) for k in WD.FIXTURES for m in ("bf16", "f16")] + [("dinov3_rope", "f16_fast"), ("glu_hplus", "f16_fast")]
TIMEOUTS = ("glu_hplus", "bf16")            # ln_test 3 (real 50 us time-outs of the peers): once, it does not depend on the family
C = 10
_REF = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ref(pkg, key, dtype, name=None):
    """The restatement of the boundary images, once per (fixture, operand rounding, mutant); dtype None: unrounded."""
    k = (key, dtype, name)
    if k not in _REF:
        fx = WD.FIXTURES[key]
        n, s1 = WD.batch_for(fx.tokens)
        imgs = WD.images(fx.tokens)[WD.boundary_ids(n, s1)]
        t = PD.file_tensors(pkg, WD.fixture_file(pkg, key))
        _REF[k] = WD.forward64(key, t, imgs, dtype, **(fx.mutants(0)[name] if name else {}))
    return _REF[k]


def _run(torch, ctx, d_imgs, n):
    probs = torch.empty((n, C), device="cuda"); logits = torch.empty((n, C), device="cuda")
    ctx.forward_device(d_imgs.data_ptr(), n, probs.data_ptr(), logits.data_ptr(), 0)
    ctx.synchronize()
    return probs, logits


def _profile(torch, ctx, d_imgs, n):
    ctx.profile_enable(True)
    _, logits = _run(torch, ctx, d_imgs, n)
    prof = {e["name"]: e for e in ctx.profile_read()}
    ctx.profile_enable(False)
    return prof, logits


@pytest.mark.parametrize("key,mode", CASES)
def test_wide_batch_of_every_family(pkg, binding, torch_gpu, key, mode):
    torch = torch_gpu
    dtype, extra = MODES[mode]
    fx = WD.FIXTURES[key]
    N = fx.tokens
    n, s1 = WD.batch_for(N)
    ids = WD.boundary_ids(n, s1)
    imgs = WD.images(N)
    counts, forced_min = WD.launches(key), WD.forced_tiles(key, N)
    where = f"wide {key} {mode}"
    model = binding.Model(WD.fixture_file(pkg, key))
    opts = dict(streams=2, split_first=s1, **extra)
    ctxs = {"plain": binding.Context(model, 0, n, dtype, no_ln_fusion=1, **opts), "fused": binding.Context(model, 0, n, dtype, **opts),
            "forced": binding.Context(model, 0, n, dtype, ln_test=binding.LN_TEST_KEY | 1, **opts)}
    small = binding.Context(model, 0, 3, dtype, **opts)
    for label, ctx in ctxs.items():
        assert (ctx.tokens, ctx.prefix) == (N, fx.prefix) and ctx.split(n) == [s1, n - s1] and ctx.boundary_rows(n) == ids
        assert ctx.ln_fusion_active() == (0 if label == "plain" else 1), label
    d_imgs = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()

    # ---- the same bits on every path, three forwards each
    out = {}
    for label, ctx in ctxs.items():
        runs = [_run(torch, ctx, d_imgs, n) for _ in range(3)]
        for p, l in runs[1:]:
            assert torch.equal(l, runs[0][1]) and torch.equal(p, runs[0][0]), f"{where}: repeated forwards of the {label} context differ"
        out[label] = runs[0]
    assert bool(torch.isfinite(out["plain"][1]).all())
    for label in ("fused", "forced"):
        diff = (out[label][1] != out["plain"][1]).any(dim=1)
        assert torch.equal(out[label][1], out["plain"][1]) and torch.equal(out[label][0], out["plain"][0]), \
            f"{where}: the {label} context differs from the stand-alone LayerNorms on {int(diff.sum())} of {n} images, first {int(diff.nonzero()[0]) if bool(diff.any()) else -1}"
    fb = {label: ctx.ln_fallbacks() for label, ctx in ctxs.items()}
    print(f"{where}: batch {n} = {s1} + {n - s1}; fix-up tiles in 3 forwards: plain {fb['plain']}, fused {fb['fused']}, forced {fb['forced']} (at least {3 * forced_min})")
    assert fb["plain"] == 0
    if fx.fusable:
        assert forced_min > 0 and fb["forced"] >= 3 * forced_min
    else:
        assert fb["fused"] == 0 and fb["forced"] == 0
    if (key, mode) == TIMEOUTS:
        ctx = binding.Context(model, 0, n, dtype, ln_test=binding.LN_TEST_KEY | 3, **opts)
        p, l = _run(torch, ctx, d_imgs, n)
        fb3 = ctx.ln_fallbacks()
        ctx.close()
        print(f"{where}: real time-outs: {fb3} fix-up tiles (at least {forced_min})")
        assert torch.equal(l, out["plain"][1]) and torch.equal(p, out["plain"][0]) and fb3 >= forced_min
    logits = out["plain"][1].cpu().numpy(); probs = out["plain"][0].cpu().numpy()

    # ---- a boundary image alone, on the ring tiles, is its row of the wide batch
    assert small.split(1) == [1]
    for i in ids:
        p1, l1 = small.forward(imgs[i:i + 1], want_logits=True)
        assert np.array_equal(_bits(l1), _bits(logits[i:i + 1])) and np.array_equal(_bits(p1), _bits(probs[i:i + 1])), f"{where}: image {i} alone differs from its row of the batch"

    # ---- the launches: the fused path really ran (profiling serialises the sub-batches; which launches fuse does not change)
    prof = {label: _profile(torch, ctxs[label], d_imgs, n) for label in ("plain", "fused")}
    for label, (pr, l) in prof.items():
        assert torch.equal(l, out["plain"][1]), f"{where}: the profiled {label} forward differs"
        assert ("attention_cls" in pr) == counts["cls_tail"], (label, sorted(pr))
    ln_plain, ln_fused = prof["plain"][0]["layernorm"]["launches"], prof["fused"][0]["layernorm"]["launches"]
    print(f"{where}: layernorm launches per forward: stand-alone context {ln_plain} (expected {counts['standalone']}), fusing context {ln_fused} "
          f"(expected {counts['layernorm']}: {counts['fused']} LayerNorms ride in GEMMs)")
    assert ln_plain == counts["standalone"] and ln_fused == counts["layernorm"]
    if not fx.fusable:
        assert ln_plain == ln_fused
    if fx.glu:
        rows = (WD.L - 1) * n * N + (n if counts["cls_tail"] else n * N)
        for label in prof:          # one launch per layer and sub-batch, on the real rows (tests/test_gpu_swiglu.py)
            sw = prof[label][0]["swiglu"]
            assert sw["launches"] == 2 * WD.L and sw["bytes"] == rows * 3 * fx.glu * 2, (label, sw)

    # ---- the pooled embedding / the cls + mean head's class feature: the same bits with and without fusion
    e = None
    if fx.pool or fx.map:
        feats = {}
        for label in ("plain", "fused"):
            ctxs[label].feat_enable(cls=True)
            _, l = _run(torch, ctxs[label], d_imgs, n)
            assert torch.equal(l, out["plain"][1]), f"{where}: features changed the {label} forward"
            feats[label] = ctxs[label].feat_read(n)[WD.L - 1]["cls"].copy()
            ctxs[label].feat_disable()
        assert np.isfinite(feats["plain"]).all() and np.array_equal(_bits(feats["fused"]), _bits(feats["plain"])), f"{where}: VITX_FEAT_CLS differs between the fusing and the stand-alone context"
        e = feats["fused"][ids]

    # ---- the high-precision anchor: the fusing context's trace and probabilities of the boundary images against the float64 restatement
    ref = _ref(pkg, key, dtype)
    d = float(np.abs(probs[ids] - ref["probs"]).max())          # the untraced forward (class rows only in the last layer, where the model keeps that)
    print(f"{where}: untraced forward: max|dprob| / gate {d / R64.PROB_TOL[dtype]:.3f}")
    assert d <= R64.PROB_TOL[dtype]
    ctx = ctxs["fused"]
    ctx.trace_enable(ids)
    p, _ = _run(torch, ctx, d_imgs, n)
    x = ctx.trace_read()
    ctx.trace_enable([])
    assert x.shape == (WD.L + 1, len(ids), N, WD.D)
    got = dict(trace=x, probs=p.cpu().numpy()[ids], e=e)
    ok, ratios = WD.inside(key, got, ref, dtype, exact=_ref(pkg, key, None) if fx.map else None)
    print(f"{where}: figure / gate against the restatement: worst {max(ratios.values()):.3f}  " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert ok, (where, ratios)
    for name in fx.mutants(dtype):
        far, parts = WD.distance(key, got, _ref(pkg, key, dtype, name), dtype)
        print(f"{where}: mutant {name}: worst figure / gate {far:.2f}")
        assert far > 1.0, (where, name, parts)
    for c in list(ctxs.values()) + [small]:
        c.close()
    model.close()
