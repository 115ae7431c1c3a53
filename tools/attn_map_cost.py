"""What the attention maps cost: ViT-B, batch 256, bf16; forwards interleaved with maps off / every layer's class-token map / rollout.

    python tools/attn_map_cost.py [--rounds 5] [--steps 10] [--model vit_base_patch16_224] [--batch 256]

Prints one line per setting (median over rounds of the mean ms per forward) and a JSON line."""
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
    n = a.batch
    ctx = binding.Context(model, device=0, max_batch=n, dtype=binding.BF16)
    imgs = torch.from_numpy(pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, model.img_size))).cuda()
    probs = torch.empty((n, model.num_classes), dtype=torch.float32, device="cuda")
    settings = {"off": ([], False), "cls_all_layers": (None, False), "rollout": ([], True)}
    times = {k: [] for k in settings}
    stream = torch.cuda.Stream()                  # forwards and timing events on one explicit stream
    st = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(a.rounds + 1):                 # round 0 warms every setting up
        for name, (layers, roll) in settings.items():
            ctx.attn_enable(layers, rollout=roll)
            for _ in range(2):
                ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st)
            e0.record(stream)
            for _ in range(a.steps):
                ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st)
            e1.record(stream); e1.synchronize()
            if r > 0:
                times[name].append(e0.elapsed_time(e1) / a.steps)
    ctx.attn_disable()
    res = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in res.items():
        print(f"{k:16s} {v:8.3f} ms/forward  ({(v / res['off'] - 1) * 100:+.1f} %)  rounds: {' '.join(f'{t:.3f}' for t in times[k])}")
    print(json.dumps({"model": a.model, "batch": n, "dtype": "bf16", "ms_per_forward": res}))


if __name__ == "__main__":
    main()
