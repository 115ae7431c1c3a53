"""What register tokens and the cls + mean head cost: a synthetic ViT-B/14-224 with 4 register tokens and the pooled head (261 tokens)
against the same file's twin without registers and with the class-token head (257 tokens), batch 256, bf16, forwards interleaved.

    python tools/registers_cost.py [--rounds 5] [--steps 10] [--model vit_base_patch14_224] [--batch 256]

Prints one line per model (median over rounds of the mean ms per forward), the twin also with last_layer_all_rows = 1 (what a pooled head
implies), the `head_pool` class of one profiled forward of the pooled model, and a JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vit_base_patch14_224")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    import torch
    pkg = _pkg.load()
    from vitcpp_amd import binding
    n = a.batch
    settings = {"R=0 cls head": (dict(), dict()), "R=0 cls head, every row of the last layer": (dict(), dict(last_layer_all_rows=1)),
                "R=4 cls+mean head": (dict(registers=4, head_pool=1), dict())}
    models, ctxs = {}, {}
    for k, (fkw, ckw) in settings.items():
        models[k] = binding.Model(pkg.synth.cached_synthetic(a.model, head_scale=4.0, **fkw))
        ctxs[k] = binding.Context(models[k], device=0, max_batch=n, dtype=binding.BF16, **ckw)
    m0 = next(iter(models.values()))
    imgs = torch.from_numpy(pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, m0.img_size))).cuda()
    probs = torch.empty((n, m0.num_classes), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in settings}
    for r in range(a.rounds + 1):                 # round 0 warms every context up
        for k, ctx in ctxs.items():
            for _ in range(2):
                ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st)
            e0.record(stream)
            for _ in range(a.steps):
                ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st)
            e1.record(stream); e1.synchronize()
            if r > 0:
                times[k].append(e0.elapsed_time(e1) / a.steps)
    res = {k: float(np.median(v)) for k, v in times.items()}
    base = res["R=0 cls head"]
    for k, v in res.items():
        print(f"{k:44s} {ctxs[k].tokens} tokens {v:8.3f} ms/forward  ({(v / base - 1) * 100:+.1f} %)  rounds: {' '.join(f'{t:.3f}' for t in times[k])}")
    ctx = ctxs["R=4 cls+mean head"]
    bracket = ctx.profile_bracket_us()
    ctx.profile_enable(True)
    ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st)
    torch.cuda.synchronize()
    prof = {e["name"]: e for e in ctx.profile_read()}
    ctx.profile_enable(False)
    p = prof["head_pool"]
    ms = p["total_ms"] - p["launches"] * bracket * 1e-3
    print(f"head_pool kernel: {p['launches']} launches  {ms:7.3f} ms  {p['bytes'] / 1e6:8.1f} MB  {p['bytes'] / ms * 1e-6:7.0f} GB/s"
          f"  ({p['bytes'] / ms * 1e-6 / 6000 * 100:.0f} % of a 6.0 TB/s streaming kernel)")
    print("profile of that forward: " + "  ".join(f"{k} {v['total_ms'] - v['launches'] * bracket * 1e-3:.3f}" for k, v in prof.items()))
    print(json.dumps({"model": a.model, "batch": n, "dtype": "bf16", "ms_per_forward": res, "head_pool_kernel": dict(launches=p["launches"], ms=ms, bytes=p["bytes"]),
                      "event_bracket_us": bracket}))


if __name__ == "__main__":
    main()
