"""Cost of rotary position embeddings (include/vitx.h "rotary position embeddings"), interleaved in ONE process (separate runs are not comparable):
    python tools/rope_cost.py [--rounds R] [--iters I] [--steps S] [--batch B] [--out profiles/rope_cost.txt]
  1. per launch, ViT-B/16 shapes at batch B (N = 1 + 4 registers + 196 patches): vitx_op_rope on bf16, on one fp16 plane and on the parity mode's two
     fp16 planes, each next to a device-to-device copy of THE SAME BYTES in the same rounds -- an in-place pass reads and writes what a copy reads and
     writes (q and k of the patch rows; the table is a few hundred KB and is not counted).  Rounds of I launches, kernel after kernel, R times;
     median, min and max, achieved GB/s, and the ratio to the copy.  No threshold: the ratio is recorded.
  2. the whole forward at batch B of a file with `rope` against the same file without it, interleaved, and the `rope` class of the per-kernel profile."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B
import rope_data as RD

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batch", type=int, default=256); ap.add_argument("--model", default="vit_base_patch16_224"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rope_cost.txt"))
a = ap.parse_args()
L = B.lib()
s = torch.cuda.current_stream().cuda_stream
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


hp = pkg.synth.hparams_for(a.model)
D, H, n = hp.hidden_size, hp.num_attention_heads, a.batch
g = hp.img_size // hp.patch_size
T = 1 + RD.REGISTERS
N = g * g + T
hd = D // H
say(f"# tools/rope_cost.py --model {a.model} --batch {n} --rounds {a.rounds} --iters {a.iters} --steps {a.steps}   ({torch.cuda.get_device_name(0)})")

# 1. the kernel on its own, beside a copy of the same bytes
cos64, sin64 = RD.table64(RD.THETA, hd, g, g)
cos = torch.from_numpy(cos64.astype(np.float32)).cuda(); sin = torch.from_numpy(sin64.astype(np.float32)).cuda()
rows = n * N
gen = torch.Generator(device="cuda").manual_seed(1)
ops, moved, keep = {}, {}, []
for form, dt, tdt, planes in (("bf16", B.BF16, torch.bfloat16, 1), ("f16", B.F16, torch.float16, 1), ("f16_planes", B.F16, torch.float16, 2)):
    qkv = (torch.randn((planes, rows, 3 * D), device="cuda", generator=gen) * 0.5).to(tdt)
    nbytes = planes * n * (N - T) * 2 * D * 2                       # q and k of the patch rows, every plane: read once, written once
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    keep.append((qkv, src, dst))
    ops[f"rope_{form}"] = (lambda dt=dt, qkv=qkv, planes=planes: L.vitx_op_rope(dt, qkv.data_ptr(), rows * 3 * D if planes == 2 else 0, cos.data_ptr(), sin.data_ptr(), n, N, T, D, H, s))
    ops[f"copy_{form}"] = (lambda src=src, dst=dst: (dst.copy_(src), 0)[1])
    moved[form] = nbytes
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
for form, nbytes in moved.items():
    for k in (f"rope_{form}", f"copy_{form}"):
        m, lo, hi = med(ts[k])
        say(f"{k:16s} n={n} N={N} T={T} D={D} H={H}: {nbytes / 1e6:6.1f} MB read + as many written: median {m:7.1f} us  min {lo:7.1f}  max {hi:7.1f}  ({2 * nbytes / m / 1e3:7.1f} GB/s)")
    r, c = med(ts[f"rope_{form}"])[0], med(ts[f"copy_{form}"])[0]
    say(f"rope_{form} / copy_{form} = x{r / c:.3f}  ({'at' if r <= 1.05 * c else 'BELOW'} copy speed; recorded, not gated)")

# 2. the forward: a file with `rope` beside the same file without it
cache = os.environ.get("VITX_CACHE", "/tmp/vitx_cache"); os.makedirs(cache, exist_ok=True)
paths = {}
for rope in (False, True):
    paths[rope] = os.path.join(cache, f"rope_cost-{a.model}-r{int(rope)}.gguf")
    if not os.path.exists(paths[rope]):
        hp_, t = RD.fixture_tensors(pkg, a.model, qk_scale=1.0, rope=rope)
        pkg.ggml_file.write_model(paths[rope], hp_, t, ftype=1)
imgs = torch.randn((n, hp.img_size, hp.img_size, 3), device="cuda")
st = torch.cuda.Stream(); ss = st.cuda_stream
for dname, dt, opt in (("bf16", B.BF16, {}), ("f16 parity", B.F16, {}), ("f16 fast", B.F16, dict(f16_fast_attention=1))):
    runs = []
    for name, rope in (("without rope", False), ("with rope", True)):
        m = B.Model(paths[rope])
        c = B.Context(m, 0, n, dt, last_layer_all_rows=1, **opt)
        runs.append(dict(name=name, m=m, c=c, ts=[], probs=torch.empty((n, hp.num_classes), device="cuda")))
    for r in runs:
        for _ in range(3): r["c"].forward_device(imgs.data_ptr(), n, r["probs"].data_ptr(), 0, ss)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for r in runs:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps): r["c"].forward_device(imgs.data_ptr(), n, r["probs"].data_ptr(), 0, ss)
            torch.cuda.synchronize(); r["ts"].append((time.perf_counter() - t0) / a.steps * 1e3)
    base = med(runs[0]["ts"])[0]
    for r in runs:
        m_, lo, hi = med(r["ts"])
        say(f"forward {a.model} + {RD.REGISTERS} registers b{n} {dname:10s} {r['name']:12s}: median {m_:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({n / m_ * 1e3:.0f} img/s)  x{m_ / base:.4f}")
    c = runs[1]["c"]
    c.profile_enable(True)
    c.forward_device(imgs.data_ptr(), n, runs[1]["probs"].data_ptr(), 0, ss)
    prof = {e["name"]: e for e in c.profile_read()}
    c.profile_enable(False)
    bracket = c.profile_bracket_us()
    e = prof["rope"]
    t_us = e["total_ms"] * 1e3 - e["launches"] * bracket
    total = sum(v["total_ms"] * 1e3 - v["launches"] * bracket for v in prof.values())
    say(f"profile {dname:10s} class rope: {e['launches']:3d} launches, {t_us:7.1f} us of {total:8.1f} us of kernels ({100 * t_us / total:.2f} %), {e['bytes'] / t_us / 1e3:7.1f} GB/s "
        f"(event brackets of {bracket:.1f} us subtracted; sub-batches run back to back while profiling)")
    assert "rope" not in {e["name"] for e in (runs[0]["c"].profile_enable(True), runs[0]["c"].forward_device(imgs.data_ptr(), n, runs[0]["probs"].data_ptr(), 0, ss), runs[0]["c"].profile_read())[2]}
    for r in runs:
        r["c"].close(); r["m"].close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
