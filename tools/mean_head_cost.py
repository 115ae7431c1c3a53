"""What the mean-pool head costs: ViT-B/16, batch 256 in ONE sub-batch (streams = 1), 196 patch rows, bf16.  Interleaved rounds of
  - the raw-mean head's two launches (VITX_POOL_MEAN_NORM: pool_mean.hip), the `head_pool` class of a profiled forward of an order-1 file;
  - the feature pass with the mean-only head operand (VITX_POOL_MEAN), the same class of an order-0 file (it also writes the operand);
  - vitx_op_features with d_mean alone on rows of the same shape ([batch][197][768], first = 1), ten launches between device events;
  - a device copy of the bytes they read (batch x 196 x 768 f32; it also writes them), ten copies between device events,
and one long image: the same two profile classes of contexts of 1024 x 1024 pixels (4096 patch rows), batch 1.  A launch of either kernel takes one
token count, so a long image BESIDE short ones does not occur in an image context; the line shows what one long image costs with one workgroup per
image (the feature pass) and with one per 64-row chunk (the part launch).

    python tools/mean_head_cost.py [--rounds 7] [--batch 256]

Prints one line per measurement with min / median / max over the rounds, and a JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    pkg = _pkg.load()
    from vitcpp_amd import binding
    n = a.batch
    names = {"raw mean + norm (2 launches)": binding.POOL_MEAN_NORM, "features pass, mean-only operand": binding.POOL_MEAN}
    models = {k: binding.Model(pkg.synth.cached_synthetic(a.model, head_scale=4.0, head_pool=v)) for k, v in names.items()}
    hp = models[next(iter(models))].hparams
    rows, D, S, C = (hp.img_size // hp.patch_size) ** 2, hp.hidden_size, hp.img_size, hp.num_classes
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def head_pool_us(ctx, imgs, probs, k):
        ctx.forward_device(imgs.data_ptr(), k, probs.data_ptr(), 0, 0)
        ctx.profile_enable(True)
        ctx.forward_device(imgs.data_ptr(), k, probs.data_ptr(), 0, 0)
        torch.cuda.synchronize()
        p = [e for e in ctx.profile_read() if e["name"] == "head_pool"][0]
        ctx.profile_enable(False)
        return (p["total_ms"] - p["launches"] * ctx.profile_bracket_us() * 1e-3) * 1e3

    def between_events(fn, reps=10):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def report(times):
        for k, v in times.items():
            print(f"{k:44s} min {min(v):8.1f}  median {np.median(v):8.1f}  max {max(v):8.1f} us   rounds: {' '.join(f'{t:.1f}' for t in v)}")
        return {k: dict(min=min(v), median=float(np.median(v)), max=max(v)) for k, v in times.items()}

    ctxs = {k: binding.Context(m, device=0, max_batch=n, dtype=binding.BF16, streams=1) for k, m in models.items()}
    imgs = torch.from_numpy(pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, S))).cuda()
    probs = torch.empty((n, C), dtype=torch.float32, device="cuda")
    x, dst = torch.randn((n, rows + 1, D), device="cuda"), torch.empty((n, rows, D), device="cuda")
    w, b, mean = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda"), torch.empty((n, D), device="cuda")
    op, cp = "vitx_op_features, d_mean alone", "device copy of the same bytes"
    times = {k: [] for k in list(ctxs) + [op, cp]}
    for r in range(a.rounds + 1):                 # round 0 warms everything up
        got = {k: head_pool_us(c, imgs, probs, n) for k, c in ctxs.items()}
        got[op] = between_events(lambda: binding.op_features(x.data_ptr(), D, (rows + 1) * D, w.data_ptr(), b.data_ptr(), 0, mean.data_ptr(), 0, D, n, rows + 1, D, 1e-6))
        got[cp] = between_events(lambda: dst.copy_(x[:, 1:]))
        if r:
            for k, v in got.items():
                times[k].append(v)
    res = report(times)
    del ctxs, imgs, x, dst
    # one long image: 4096 patch rows
    big = {k + f", one image of {(1024 // hp.patch_size) ** 2} patch rows": binding.Context(m, device=0, max_batch=1, dtype=binding.BF16, img_size=1024) for k, m in models.items()}
    img1 = torch.randn((1, 1024, 1024, 3), device="cuda")
    long_times = {k: [] for k in big}
    for r in range(a.rounds + 1):
        for k, c in big.items():
            v = head_pool_us(c, img1, probs, 1)
            if r:
                long_times[k].append(v)
    res_long = report(long_times)
    print(json.dumps({"model": a.model, "batch": n, "dtype": "bf16", "patch_rows": rows, "us": res, "long_image_us": res_long}))


if __name__ == "__main__":
    main()
