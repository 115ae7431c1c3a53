"""What the embeddings and token features cost: ViT-B/16, batch 256, bf16; forwards interleaved with features off / the class embedding /
class + mean (last layer) / the token features of the last layer / of four layers.

    python tools/feat_cost.py [--rounds 5] [--steps 10] [--model vit_base_patch16_224] [--batch 256]

Prints one line per setting (median over rounds of the mean ms per forward), for the settings with features the `features` class of one
profiled forward (launches, ms, achieved GB/s from the profile's algorithmic bytes), and a JSON line."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    import torch
    pkg = _pkg.load()
    from vitcpp_amd import binding
    model = binding.Model(pkg.synth.cached_synthetic(a.model, head_scale=4.0))
    n, L = a.batch, model.hparams.num_hidden_layers
    ctx = binding.Context(model, device=0, max_batch=n, dtype=binding.BF16)
    imgs = torch.from_numpy(pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, model.img_size))).cuda()
    probs = torch.empty((n, model.num_classes), dtype=torch.float32, device="cuda")
    four = sorted({L // 4 - 1, L // 2 - 1, 3 * L // 4 - 1, L - 1} & set(range(L)))
    settings = {"off": None, "cls": dict(cls=True), "cls+mean": dict(cls=True, mean=True), "tokens": dict(cls=False, tokens=True),
                f"tokens x {len(four)} layers": dict(cls=False, tokens=True, layers=four)}
    times = {k: [] for k in settings}
    stream = torch.cuda.Stream()                  # forwards and timing events on one explicit stream
    st = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def enable(kw):
        ctx.feat_disable() if kw is None else ctx.feat_enable(**kw)

    for r in range(a.rounds + 1):                 # round 0 warms every setting up
        for name, kw in settings.items():
            enable(kw)
            for _ in range(2):
                ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st)
            e0.record(stream)
            for _ in range(a.steps):
                ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st)
            e1.record(stream); e1.synchronize()
            if r > 0:
                times[name].append(e0.elapsed_time(e1) / a.steps)
    res = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in res.items():
        print(f"{k:20s} {v:8.3f} ms/forward  ({(v / res['off'] - 1) * 100:+.1f} %)  rounds: {' '.join(f'{t:.3f}' for t in times[k])}")
    # the kernel itself: one profiled forward per setting (sub-batches back to back on one stream, every launch bracketed by events)
    bracket = ctx.profile_bracket_us()
    prof = {}
    for name, kw in settings.items():
        if kw is None:
            continue
        enable(kw)
        ctx.profile_enable(True)
        ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st)
        torch.cuda.synchronize()
        p = [e for e in ctx.profile_read() if e["name"] == "features"][0]
        ctx.profile_enable(False)
        ms = p["total_ms"] - p["launches"] * bracket * 1e-3
        prof[name] = dict(launches=p["launches"], ms=ms, bytes=p["bytes"], gbps=p["bytes"] / ms * 1e-6)
        print(f"features kernel, {name:20s} {p['launches']} launches  {ms:7.3f} ms  {p['bytes'] / 1e6:8.1f} MB  {prof[name]['gbps']:7.0f} GB/s"
              f"  ({prof[name]['gbps'] / 6000 * 100:.0f} % of a 6.0 TB/s streaming kernel)")
    ctx.feat_disable()
    print(json.dumps({"model": a.model, "batch": n, "dtype": "bf16", "ms_per_forward": res, "features_kernel": prof, "event_bracket_us": bracket}))


if __name__ == "__main__":
    main()
