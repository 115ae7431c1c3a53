"""Device time of the model-preprocessing kernel (vitx_preprocess_ex_device with Pillow's bilinear and bicubic: shortest edge 224, centre crop
224) beside the reference's preprocess kernel (vitx_preprocess_u8_device, bicubic: preprocess_kernel<true>) on the same sources and the same
224 x 224 output, batch 64, the three launches interleaved.

    python tools/preprocess_cost.py [--rounds 7] [--batch 64] [--out profiles/preprocess_cost.txt]

Sources: 500 x 375 (a web photo), 4032 x 3024 (a phone photo), 224 x 224 (already at size: both passes are the identity).  Per source every kernel is
warmed up, then timed with device events over a window of at least 0.2 s of back-to-back launches, `rounds` times in alternation; the record
holds the median, the minimum and the maximum of the rounds.  The two kernels do different work -- the antialiased one reads scale^2 times as
many taps -- so this is a price list, not a race."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_cost.txt"))
    a = ap.parse_args()
    import torch
    _pkg.load()
    from vitcpp_amd import binding as B
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_cost.py measures on the GPU: none is visible")
    n, S = a.batch, 224
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines, record = [f"batch {n}, output {S} x {S} f32 HWC, {a.rounds} interleaved rounds, device events; ms per launch of {n} images: median [min .. max]"], []
    imagenet = dict(mean255=(123.675, 116.28, 103.53), std255=(58.395, 57.12, 57.375))
    for nx, ny in ((500, 375), (4032, 3024), (224, 224)):
        src = torch.randint(0, 256, (n, ny, nx, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(nx))
        out = torch.empty((n, S, S, 3), dtype=torch.float32, device="cuda")
        pps = {k: B.Preproc.make(B.PP_SHORTEST_EDGE, S, 0, f, crop=S, **imagenet) for k, f in (("pil_bicubic", B.PP_PIL_BICUBIC), ("pil_bilinear", B.PP_PIL_BILINEAR))}
        runs = {k: (lambda pp=pp: B.preprocess_ex_device(pp, src.data_ptr(), n, nx, ny, out.data_ptr(), st)) for k, pp in pps.items()}
        runs["reference_bicubic"] = lambda: B.preprocess_device(src.data_ptr(), n, nx, ny, S, out.data_ptr(), B.BICUBIC, st)
        steps, times = {}, {k: [] for k in runs}
        for k, run in runs.items():                      # warm-up, and the launches a 0.2 s window holds
            run(); run()
            e0.record(stream); run(); e1.record(stream); e1.synchronize()
            steps[k] = int(min(max(200.0 / max(e0.elapsed_time(e1), 1e-3), 3), 2000))
        for _ in range(a.rounds):
            for k, run in runs.items():
                e0.record(stream)
                for _ in range(steps[k]):
                    run()
                e1.record(stream); e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / steps[k])
        base = float(np.median(times["reference_bicubic"]))
        in_mb, out_mb = n * nx * ny * 3 / 1e6, n * S * S * 12 / 1e6
        lines.append(f"source {nx} x {ny} ({in_mb:.1f} MB of u8 in, {out_mb:.1f} MB of f32 out):")
        for k, v in times.items():
            med = float(np.median(v))
            lines.append(f"  {k:18s} {med:9.4f} [{min(v):.4f} .. {max(v):.4f}]  {med / n * 1e3:8.2f} us/image  {n / med * 1e3:10.0f} images/s  "
                         f"{med / base:6.2f} x reference  ({steps[k]} launches per window)")
            record.append(dict(source=[nx, ny], kernel=k, ms_median=med, ms_min=min(v), ms_max=max(v), launches_per_window=steps[k]))
        del src, out
    lines.append(json.dumps(dict(batch=n, out=S, rounds=a.rounds, device=torch.cuda.get_device_name(0), results=record)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
