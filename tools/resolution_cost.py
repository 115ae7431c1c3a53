"""What a forward costs at another image size than the file's: ViT-B/16 bf16 from the 224^2 file at 160 .. 512, the batch chosen for roughly
constant token rows (256 x 197), contexts of ONE loaded model (shared weights), settings interleaved in one process.

    python tools/resolution_cost.py [--rounds 5] [--steps 10] [--model vit_base_patch16_224] [--sizes 160,224,256,320,384,448,512]

Per size: ms/forward (median over rounds of the mean), images/s, TFLOP/s by synth.gflop_per_image at that size, the attention classes of
one profiled forward (vitx_profile_read), the resample kernel's duration (vitx_op_pos_embed_resample, median of 9 timed launches) and the
context-creation time with the option and without it (an ordinary context on the file vitx_model_resize_file writes for that size); both
creations attach to weights that are already on the device.  A JSON line at the end."""
import argparse
import dataclasses
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vit_base_patch16_224")
    ap.add_argument("--sizes", default="160,224,256,320,384,448,512")
    ap.add_argument("--rows", type=int, default=256 * 197)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    import torch
    pkg = _pkg.load()
    from vitcpp_amd import binding
    src = pkg.synth.cached_synthetic(a.model, head_scale=4.0)
    model = binding.Model(src)
    hp = pkg.synth.hparams_for(a.model)
    P, D, S0 = hp.patch_size, hp.hidden_size, hp.img_size
    sizes = [int(s) for s in a.sizes.split(",")]
    keeper = binding.Context(model, device=0, max_batch=1, dtype=binding.BF16)          # holds the weights: every context below attaches to them
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tmp = tempfile.mkdtemp(prefix="resolution_cost")
    runs = {}
    for S in sizes:
        N = (S // P) ** 2 + 1
        n = max(1, round(a.rows / N))
        r = dict(S=S, N=N, n=n)
        # creation without the option: an ordinary context on the resized file, its weights already uploaded by a keeper of that file
        dst = os.path.join(tmp, f"{S}.gguf")
        binding.resize_file(src, dst, S, binding.POS_BICUBIC)
        m2 = binding.Model(dst)
        k2 = binding.Context(m2, device=0, max_batch=1, dtype=binding.BF16)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        c2 = binding.Context(m2, device=0, max_batch=n, dtype=binding.BF16)
        r["create_file_ms"] = (time.perf_counter() - t0) * 1e3
        assert c2.shares_weights()
        c2.close(); k2.close(); m2.close(); os.remove(dst)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ctx = binding.Context(model, device=0, max_batch=n, dtype=binding.BF16, img_size=S)
        r["create_option_ms"] = (time.perf_counter() - t0) * 1e3
        assert ctx.shares_weights() and ctx.tokens == N
        r["ctx"] = ctx
        r["imgs"] = torch.from_numpy(pkg.synth.normalize_u8(pkg.synth.synthetic_images_u8(n, S))).cuda()
        r["probs"] = torch.empty((n, model.num_classes), dtype=torch.float32, device="cuda")
        # the resample kernel on its own, on a table of this model's shape
        g0, g1 = S0 // P, S // P
        d_in = torch.randn((1 + g0 * g0, D), dtype=torch.float32, device="cuda") * 0.02
        d_out = torch.empty((1 + g1 * g1, D), dtype=torch.float32, device="cuda")
        ks = []
        for i in range(10):
            e0.record(stream)
            binding.op_pos_embed_resample(d_in.data_ptr(), g0, D, g1, binding.POS_BICUBIC, d_out.data_ptr(), st)
            e1.record(stream); e1.synchronize()
            if i:
                ks.append(e0.elapsed_time(e1) * 1e3)
        r["resample_us"] = float(np.median(ks))
        r["times"] = []
        runs[S] = r
    for rnd in range(a.rounds + 1):                 # round 0 warms every size up
        for S, r in runs.items():
            c, n = r["ctx"], r["n"]
            for _ in range(2):
                c.forward_device(r["imgs"].data_ptr(), n, r["probs"].data_ptr(), 0, st)
            e0.record(stream)
            for _ in range(a.steps):
                c.forward_device(r["imgs"].data_ptr(), n, r["probs"].data_ptr(), 0, st)
            e1.record(stream); e1.synchronize()
            if rnd > 0:
                r["times"].append(e0.elapsed_time(e1) / a.steps)
    out = []
    for S, r in runs.items():
        c, n = r["ctx"], r["n"]
        ms = float(np.median(r["times"]))
        gf = pkg.synth.gflop_per_image(dataclasses.replace(hp, img_size=S))
        c.profile_enable(True)
        c.forward_device(r["imgs"].data_ptr(), n, r["probs"].data_ptr(), 0, st)
        torch.cuda.synchronize()
        attn = {e["name"]: (e["launches"], round(e["total_ms"], 3)) for e in c.profile_read() if e["name"].startswith("attention")}
        c.profile_enable(False)
        rec = dict(img_size=S, tokens=r["N"], batch=n, split=c.split(n), ms_per_forward=ms, images_per_s=n / ms * 1e3, gflop_per_image=gf, tflops=n * gf / ms,
                   attention=attn, resample_kernel_us=r["resample_us"], create_with_option_ms=r["create_option_ms"], create_on_resized_file_ms=r["create_file_ms"])
        out.append(rec)
        print(f"img {S:4d}  tokens {r['N']:5d}  batch {n:4d}  {ms:8.3f} ms/forward  {rec['images_per_s']:8.0f} img/s  {gf:7.2f} GFLOP/img  {rec['tflops']:6.1f} TFLOP/s  "
              f"attention {attn}  resample {r['resample_us']:6.1f} us  create {r['create_option_ms']:7.1f} ms (option) / {r['create_file_ms']:7.1f} ms (resized file)  "
              f"rounds: {' '.join(f'{t:.3f}' for t in r['times'])}")
    print(json.dumps({"model": a.model, "dtype": "bf16", "rows_target": a.rows, "sizes": out}))


if __name__ == "__main__":
    main()
