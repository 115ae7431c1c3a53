"""Cost of the gate of a gated MLP (include/vitx.h "gated MLP"), interleaved in ONE process (separate runs are not comparable):
    python tools/swiglu_cost.py [--rounds R] [--iters I] [--steps S] [--batch B] [--layers L] [--out profiles/swiglu_cost.txt]
  1. per launch, DINOv2 ViT-g/14 shapes at batch B (D 1536, F 4096, N = 257 tokens): vitx_op_swiglu on bf16 and on fp16, each next to a
     device-to-device copy that MOVES THE SAME BYTES in the same rounds -- the pass reads 2 rows F elements and writes rows F, a copy of 1.5 rows F
     elements reads and writes as much.  Rounds of I launches, kernel after kernel, R times; median, min and max, achieved GB/s, and the ratio to
     the copy.  No threshold: the ratio is recorded.
  2. the whole forward at batch B of a ViT-g/14-shaped synthetic file with L layers (default 4: the share of a layer's kernels does not depend on
     the depth, the patch embedding and the head are a fixed 1-2 %) and the `swiglu` class of its per-kernel profile: the upper bound on what
     folding the gate into fc1's epilogue could return."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256); ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swiglu_cost.txt"))
a = ap.parse_args()
L = B.lib()
s = torch.cuda.current_stream().cuda_stream
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


D, H, F, P, S = 1536, 24, 4096, 14, 224
n = a.batch
N = (S // P) ** 2 + 1
rows = n * N
say(f"# tools/swiglu_cost.py --batch {n} --rounds {a.rounds} --iters {a.iters} --steps {a.steps} --layers {a.layers}   ({torch.cuda.get_device_name(0)})")

# 1. the kernel on its own, beside a copy that moves the same bytes
gen = torch.Generator(device="cuda").manual_seed(1)
ops, keep = {}, []
moved = 3 * rows * F * 2                                              # bytes read + written by one launch
for form, dt, tdt in (("bf16", B.BF16, torch.bfloat16), ("f16", B.F16, torch.float16)):
    src = torch.randn((rows, 2 * F), device="cuda", generator=gen).to(tdt)
    dst = torch.empty((rows, F), dtype=tdt, device="cuda")
    c_src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"); c_dst = torch.empty_like(c_src)
    keep.append((src, dst, c_src, c_dst))
    ops[f"swiglu_{form}"] = (lambda dt=dt, src=src, dst=dst: L.vitx_op_swiglu(dt, src.data_ptr(), 2 * F, dst.data_ptr(), F, rows, F, s))
    ops[f"copy_{form}"] = (lambda c_src=c_src, c_dst=c_dst: (c_dst.copy_(c_src), 0)[1])
ts = {k: [] for k in ops}
for k, f in ops.items():
    for _ in range(3): B.check(f(), k)
torch.cuda.synchronize()
for _ in range(a.rounds):
    for k, f in ops.items():
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters): f()
        e1.record(); torch.cuda.synchronize()
        ts[k].append(e0.elapsed_time(e1) / a.iters * 1e3)
for form in ("bf16", "f16"):
    for k in (f"swiglu_{form}", f"copy_{form}"):
        m, lo, hi = med(ts[k])
        say(f"{k:12s} rows={rows} F={F}: {moved / 1e6:7.1f} MB read + written: median {m:7.1f} us  min {lo:7.1f}  max {hi:7.1f}  ({moved / m / 1e3:7.1f} GB/s)")
    r, c = med(ts[f"swiglu_{form}"])[0], med(ts[f"copy_{form}"])[0]
    say(f"swiglu_{form} / copy_{form} = x{r / c:.3f}  ({'at' if r <= 1.05 * c else 'BELOW'} copy speed; recorded, not gated)")
del keep, ops
torch.cuda.empty_cache()

# 2. the forward of a ViT-g/14-shaped file with the gated MLP, and the gate's share of it
cache = os.environ.get("VITX_CACHE", "/tmp/vitx_cache"); os.makedirs(cache, exist_ok=True)
path = os.path.join(cache, f"swiglu_cost-vit_g14-L{a.layers}-F{F}.gguf")
hp = pkg.ggml_file.HParams(D, a.layers, H, 10, P, S, 1)
if not os.path.exists(path):
    pkg.ggml_file.write_model(path, hp, pkg.synth.make_weights(hp, head_scale=4.0, glu=F), ftype=1)
say(f"# forward: D {D}, {H} heads, F {F}, {N} tokens, {a.layers} layers, batch {n}: {pkg.synth.gflop_per_image(hp, glu=F):.1f} GFLOP per image")
imgs = torch.randn((n, S, S, 3), device="cuda")
st = torch.cuda.Stream(); ss = st.cuda_stream
for dname, dt, opt in (("bf16", B.BF16, {}), ("f16 parity", B.F16, {})):
    m = B.Model(path)
    c = B.Context(m, 0, n, dt, last_layer_all_rows=1, **opt)
    probs = torch.empty((n, hp.num_classes), device="cuda")
    for _ in range(3): c.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
    torch.cuda.synchronize()
    t_f = []
    for _ in range(a.rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps): c.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
        torch.cuda.synchronize(); t_f.append((time.perf_counter() - t0) / a.steps * 1e3)
    m_, lo, hi = med(t_f)
    say(f"forward ViT-g/14-shaped, {a.layers} layers, b{n} {dname:10s}: median {m_:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({n / m_ * 1e3:.0f} img/s)")
    c.profile_enable(True)
    c.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
    prof = {e["name"]: e for e in c.profile_read()}
    c.profile_enable(False)
    bracket = c.profile_bracket_us()
    total = sum(v["total_ms"] * 1e3 - v["launches"] * bracket for v in prof.values())
    for name in ("gemm_fc1_gelu", "swiglu", "gemm_fc2_resid"):
        e = prof[name]
        t_us = e["total_ms"] * 1e3 - e["launches"] * bracket
        say(f"profile {dname:10s} class {name:14s}: {e['launches']:3d} launches, {t_us:8.1f} us of {total:9.1f} us of kernels ({100 * t_us / total:5.2f} %), {e['bytes'] / t_us / 1e3:7.1f} GB/s "
            f"(event brackets of {bracket:.1f} us subtracted; sub-batches run back to back while profiling)")
    c.close(); m.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
