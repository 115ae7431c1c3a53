"""What the MXFP8 operand mode buys: BF16 and MXFP8 forwards interleaved on one device, whole graph (last_layer_all_rows = 1) and the
library default, at ViT-B/16 batch 256 and ViT-L/16-384 batch 128; per-class kernel time of each mode (vitx_profile_read); both
matrix-pipe probes; and max |dp| / top-1 agreement of MXFP8 against BF16 on the same seeded batch.

    python tools/mxfp8_cost.py [--rounds 5] [--steps 10] [--out profiles/mxfp8_cost.txt]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _pkg  # noqa: E402

CASES = [("vit_base_patch16_224", 256), ("vit_large_patch16_384", 128)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = _pkg.load()
    from vitcpp_amd import binding
    lines, record = [], {"cases": []}
    for name, n in CASES:
        model = binding.Model(pkg.synth.cached_synthetic(name, head_scale=4.0))
        imgs_h = pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, model.img_size))
        imgs = torch.from_numpy(imgs_h).cuda()
        probs = torch.empty((n, model.num_classes), dtype=torch.float32, device="cuda")
        ctxs = {}
        for dt_name, dt in (("bf16", binding.BF16), ("mxfp8", binding.MXFP8)):
            for mode, opts in (("whole_graph", {"last_layer_all_rows": 1}), ("default", {})):
                ctxs[(dt_name, mode)] = binding.Context(model, device=0, max_batch=n, dtype=dt, **opts)
        times = {k: [] for k in ctxs}
        stream = torch.cuda.Stream(); st = stream.cuda_stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(a.rounds + 1):             # round 0 warms every context up
            for k, ctx in ctxs.items():
                for _ in range(2):
                    ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st)
                e0.record(stream)
                for _ in range(a.steps):
                    ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st)
                e1.record(stream); e1.synchronize()
                if r > 0:
                    times[k].append(e0.elapsed_time(e1) / a.steps)
        res = {f"{k[0]}/{k[1]}": float(np.median(v)) for k, v in times.items()}
        lines.append(f"== {name} batch {n} (median of {a.rounds} interleaved rounds of {a.steps} forwards)")
        for (dt_name, mode), v in times.items():
            ms = float(np.median(v))
            lines.append(f"  {dt_name:6s} {mode:12s} {ms:8.3f} ms/forward  {n / ms * 1e3:9.1f} images/s   rounds: {' '.join(f'{t:.3f}' for t in v)}")
        for mode in ("whole_graph", "default"):
            lines.append(f"  MXFP8 / BF16 ({mode}): {res['mxfp8/' + mode] / res['bf16/' + mode]:.3f} of the time")
        # per-class kernel time, one profiled forward per mode (whole graph)
        prof = {}
        for dt_name in ("bf16", "mxfp8"):
            ctx = ctxs[(dt_name, "whole_graph")]
            ctx.profile_enable(True)
            ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st); torch.cuda.synchronize()
            ctx.profile_read()
            ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, st)
            prof[dt_name] = ctx.profile_read()
            ctx.profile_enable(False)
        lines.append("  per class (one profiled whole-graph forward, raw event intervals): class  bf16 ms  mxfp8 ms  mxfp8 TF/s")
        names = [e["name"] for e in prof["bf16"]] + [e["name"] for e in prof["mxfp8"] if e["name"] not in [x["name"] for x in prof["bf16"]]]
        for cname in names:
            b = next((e for e in prof["bf16"] if e["name"] == cname), None); m = next((e for e in prof["mxfp8"] if e["name"] == cname), None)
            tf = (m["flops"] / (m["total_ms"] * 1e-3) / 1e12) if m and m["total_ms"] > 0 and m["flops"] > 0 else 0.0
            lines.append(f"    {cname:18s} {b['total_ms'] if b else 0:8.3f} {m['total_ms'] if m else 0:9.3f} {tf:10.1f}")
        # accuracy on the same seeded batch (host copies)
        p_bf = ctxs[("bf16", "default")].forward(imgs_h); p_mx = ctxs[("mxfp8", "default")].forward(imgs_h)
        dp = float(np.abs(p_mx - p_bf).max()); top1 = float((p_mx.argmax(1) == p_bf.argmax(1)).mean())
        lines.append(f"  MXFP8 vs BF16 (default, {n} images): max|dp| = {dp:.3e}, top-1 agreement {top1:.4f}")
        record["cases"].append({"model": name, "batch": n, "ms_per_forward": res, "max_dp": dp, "top1_agree": top1,
                                "profile": {k: [{x: e[x] for x in ("name", "launches", "total_ms", "flops")} for e in v] for k, v in prof.items()}})
        del ctxs
    tb, _ = binding.probe_mfma(0, binding.BF16, 2, 150.0)
    tm, mhz = binding.probe_mfma(0, binding.MXFP8, 2, 150.0)
    lines.append(f"== matrix-pipe probes (random operands): bf16 {tb:.0f} TF/s, MXFP8 {tm:.0f} TF/s ({mhz:.0f} MHz)")
    record["probe_tflops"] = {"bf16": tb, "mxfp8": tm}
    text = "\n".join(lines)
    print(text)
    print(json.dumps(record))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
