"""Cost of zero-shot classification (include/vitx.h "zero-shot classification"), interleaved in ONE process (separate runs are not comparable):
    python tools/zeroshot_cost.py [--rounds R] [--iters I] [--steps S] [--batch B] [--classes 1000 21843] [--out profiles/zeroshot_cost.txt]
ViT-B/16 224^2 with a CLIP-style 512-wide bias-free projection as its head, batch B, bf16, one bank of K classes per run:
  1. per launch, from the per-kernel profile of a bank-on forward: the class "zeroshot" (zs_embed, the bank GEMM, zs_score of every sub-batch)
     beside the class "gemm_head" + "softmax" of the same forward;
  2. vitx_op_zeroshot on its own at n = B (the three launches back to back) beside vitx_op_gemm at the bank GEMM's shape: the two small
     kernels are the difference;
  3. the whole forward with the bank on and off, alternating, R rounds of S steps: median, min and max of each, and the slowdown.
No gate rests on these figures."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batch", type=int, default=256); ap.add_argument("--model", default="vit_base_patch16_224"); ap.add_argument("--width", type=int, default=512)
ap.add_argument("--classes", type=int, nargs="+", default=[1000, 21843]); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zeroshot_cost.txt"))
a = ap.parse_args()
L = B.lib()
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def up(v, m):
    return (v + m - 1) // m * m


hp = pkg.synth.hparams_for(a.model)
n, E, D = a.batch, a.width, hp.hidden_size
say(f"# tools/zeroshot_cost.py --model {a.model} --width {E} --batch {n} --rounds {a.rounds} --iters {a.iters} --steps {a.steps}   ({torch.cuda.get_device_name(0)})")

# the model file: ViT-B with a [E][D] bias-free projection as its head (what convert.py writes for a CLIP vision tower)
hp.num_classes = E
w = pkg.synth.make_weights(hp, head_scale=8.0)
w["head.bias"] = np.zeros_like(w["head.bias"])
cache = os.environ.get("VITX_CACHE", "/tmp/vitx_cache"); os.makedirs(cache, exist_ok=True)
path = os.path.join(cache, f"zs_cost-{a.model}-e{E}.gguf")
if not os.path.exists(path):
    pkg.ggml_file.write_model(path, hp, w, ftype=1)
model = B.Model(path)
ctx = B.Context(model, 0, n, B.BF16)
imgs = torch.randn((n, hp.img_size, hp.img_size, 3), device="cuda")
probs = torch.empty((n, E), device="cuda")
st = torch.cuda.Stream(); ss = st.cuda_stream
s0 = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(1)
bracket = ctx.profile_bracket_us()

for K in a.classes:
    bank = rng.standard_normal((K, E)); bank = (bank / np.linalg.norm(bank, axis=1, keepdims=True)).astype(np.float32)
    say(f"## K = {K} classes of width {E}: the bank is {up(K, 128) * E * 2 / 1e6:.2f} MB in bf16")
    # 1. the per-kernel profile of a bank-on forward
    ctx.zeroshot_set(bank, B.ZS_SOFTMAX, 100.0, 0.0)
    for _ in range(3): ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
    ctx.profile_enable(True)
    ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
    prof = {e["name"]: e for e in ctx.profile_read()}
    ctx.profile_enable(False)
    for k in ("zeroshot", "gemm_head", "softmax"):
        e = prof[k]
        say(f"profile class {k:10s}: {e['launches']:2d} launches, {e['total_ms'] * 1e3 - e['launches'] * bracket:7.1f} us in all (event brackets of {bracket:.1f} us subtracted; "
            f"{len(ctx.split(n))} sub-batches back to back while profiling)")
    # 2. the launches on their own, n = B in one piece
    kp, npad = up(K, 128), up(n, 256)
    z = torch.randn((n, E), device="cuda")
    d_bank = torch.zeros((kp, E), device="cuda", dtype=torch.bfloat16); d_bank[:K] = torch.from_numpy(bank).cuda().to(torch.bfloat16)
    d_a = torch.zeros((npad, E), device="cuda", dtype=torch.bfloat16); d_acc = torch.zeros((npad + 1, kp), device="cuda")
    d_p = torch.empty((n, K), device="cuda"); d_l = torch.empty((n, K), device="cuda")
    gw = torch.zeros((up(K, 128), E), device="cuda", dtype=torch.bfloat16); gb = torch.zeros(up(K, 128), device="cuda"); go = torch.zeros((npad, up(K, 64)), device="cuda")
    ops = {"op_zeroshot (3 launches)": lambda: L.vitx_op_zeroshot(B.BF16, z.data_ptr(), E, d_bank.data_ptr(), d_a.data_ptr(), d_acc.data_ptr(), d_p.data_ptr(), d_l.data_ptr(), n, K, E, 0, 100.0, 0.0, s0),
           "op_gemm at the bank's shape": lambda: L.vitx_op_gemm(B.BF16, 3, d_a.data_ptr(), gw.data_ptr(), gb.data_ptr(), go.data_ptr(), npad, up(K, 64), E, s0)}
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
    for k in ops:
        m, lo, hi = med(ts[k])
        say(f"{k:28s} n={n} K={K} E={E}: median {m:7.1f} us  min {lo:7.1f}  max {hi:7.1f}  (back to back on one stream, launch gaps included)")
    # 3. the forward, bank on and off alternating
    tf = {"off": [], "on": []}
    for _ in range(a.rounds):
        for mode in ("off", "on"):
            ctx.zeroshot_set(bank if mode == "on" else None, B.ZS_SOFTMAX, 100.0, 0.0)
            ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps): ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
            torch.cuda.synchronize(); tf[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
    base = med(tf["off"])[0]
    for mode in ("off", "on"):
        m, lo, hi = med(tf[mode])
        say(f"forward {a.model} b{n} bf16 bank {mode:3s}: median {m:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({n / m * 1e3:.0f} img/s)  x{m / base:.4f}")
    ctx.zeroshot_set(None)
ctx.close(); model.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
