"""Cost of the attention-pooling (MAP) head of a model without a class token (include/vitx.h), interleaved in ONE process (separate runs are
not comparable):
    python tools/map_head_cost.py [--rounds R] [--iters I] [--steps S] [--batch B] [--out profiles/map_head_cost.txt]
  1. per launch, ViT-B/16 shapes at batch B: vitx_op_attention_pool; vitx_op_gemm at the shape of the K/V projection the fold makes unnecessary
     (M = B * 196, N = 2 D, K = D), both operand types; vitx_op_features_ex computing the mean over the same rows (the existing one-pass kernel
     over the same bytes).  Rounds of I launches, kernel after kernel, R times; median, min and max.
  2. the whole pooled tail from the per-kernel profile of a forward (classes head_pool and gemm_cls_tail: the pooling kernel, the H value
     projections, proj, fc1, fc2, the final rounding; its LayerNorm is one launch of class layernorm).
  3. the whole forward at batch B of a MAP file beside a class-token file of the same dimensions created with last_layer_all_rows = 1.
Condition the feature is held to: the pooling kernel is faster than the K/V GEMM it replaces."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batch", type=int, default=256); ap.add_argument("--model", default="vit_base_patch16_224"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_head_cost.txt"))
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
N = (hp.img_size // hp.patch_size) ** 2
say(f"# tools/map_head_cost.py --model {a.model} --batch {n} --rounds {a.rounds} --iters {a.iters} --steps {a.steps}   ({torch.cuda.get_device_name(0)})")

# 1. the kernels on their own
g = torch.Generator(device="cuda").manual_seed(1)
X = torch.randn((n * N, D), device="cuda", generator=g)
lw = 1 + 0.1 * torch.randn(D, device="cuda", generator=g); lb = 0.1 * torch.randn(D, device="cuda", generator=g)
u = torch.randn((H, D), device="cuda", generator=g) * (2.0 / D ** 0.5)
M_out = torch.zeros((n, H, D), device="cuda"); mean_out = torch.zeros((n, D), device="cuda")
Mrows = n * N
assert Mrows % 128 == 0
ops = {"attention_pool": lambda: L.vitx_op_attention_pool(X.data_ptr(), D, N * D, lw.data_ptr(), lb.data_ptr(), 1e-6, u.data_ptr(), M_out.data_ptr(), None, n, N, D, H, s),
       "features_mean": lambda: L.vitx_op_features_ex(X.data_ptr(), D, N * D, lw.data_ptr(), lb.data_ptr(), None, mean_out.data_ptr(), None, D, n, N, 0, D, 1e-6, 0, None, 0, s)}
keep = []
for dname, dt, tdt in (("bf16", B.BF16, torch.bfloat16), ("f16", B.F16, torch.float16)):
    A = (torch.randn((Mrows, D), device="cuda", generator=g) * 0.5).to(tdt)
    W = (torch.randn((2 * D, D), device="cuda", generator=g) * 0.05).to(tdt)
    bias = torch.randn(2 * D, device="cuda", generator=g) * 0.1
    out = torch.zeros((Mrows, 2 * D), device="cuda", dtype=tdt)
    keep.append((A, W, bias, out))
    ops[f"gemm_kv_{dname}"] = (lambda dt=dt, A=A, W=W, bias=bias, out=out: L.vitx_op_gemm(dt, 0, A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), Mrows, 2 * D, D, s))
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
x_bytes = Mrows * D * 4
for k in ops:
    m, lo, hi = med(ts[k])
    extra = f"({x_bytes / m / 1e6:6.2f} TB/s of X)" if not k.startswith("gemm") else f"({2.0 * Mrows * 2 * D * D / m / 1e6:6.1f} TF/s)"
    say(f"{k:16s} n={n} N={N} D={D} H={H}: median {m:7.1f} us  min {lo:7.1f}  max {hi:7.1f}  {extra}")
pool = med(ts["attention_pool"])[0]
for dname in ("bf16", "f16"):
    gk = med(ts[f"gemm_kv_{dname}"])[0]
    say(f"condition ({dname}): attention_pool {pool:.1f} us {'<' if pool < gk else '>='} K/V GEMM {gk:.1f} us  -> {'holds' if pool < gk else 'FAILS: the fold has bought nothing'}  (x{pool / gk:.3f})")
say(f"attention_pool / features_mean = x{pool / med(ts['features_mean'])[0]:.3f}  (recorded, not gated)")

# 2. + 3. the forward: a MAP file beside a class-token file of the same dimensions
import map_data as MD
w = pkg.synth.make_weights(hp, head_scale=8.0)
cache = os.environ.get("VITX_CACHE", "/tmp/vitx_cache"); os.makedirs(cache, exist_ok=True)
p_cls = os.path.join(cache, f"map_cost-{a.model}-cls.gguf"); p_map = os.path.join(cache, f"map_cost-{a.model}-map.gguf")
if not os.path.exists(p_cls):
    pkg.ggml_file.write_model(p_cls, hp, w, ftype=1)
if not os.path.exists(p_map):
    t = {}
    for k, v in w.items():
        if k == "cls_token": continue
        if k == "pos_embed": v = np.ascontiguousarray(v[:, 1:])
        if k == "head.weight": t.update(MD.pool_tensors(D))
        t[k] = v
    pkg.ggml_file.write_model(p_map, hp, t, ftype=1)
imgs = torch.randn((n, hp.img_size, hp.img_size, 3), device="cuda")
st = torch.cuda.Stream(); ss = st.cuda_stream
for dname, dt in (("bf16", B.BF16), ("f16", B.F16)):
    runs = []
    for name, path, opt in (("class token, all rows", p_cls, dict(last_layer_all_rows=1)), ("MAP head", p_map, {})):
        m = B.Model(path)
        c = B.Context(m, 0, n, dt, **opt)
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
        say(f"forward {a.model} b{n} {dname} {r['name']:22s}: median {m_:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({n / m_ * 1e3:.0f} img/s)  x{m_ / base:.4f}")
    c = runs[1]["c"]
    c.profile_enable(True)
    c.forward_device(imgs.data_ptr(), n, runs[1]["probs"].data_ptr(), 0, ss)
    prof = {e["name"]: e for e in c.profile_read()}
    c.profile_enable(False)
    bracket = c.profile_bracket_us()
    tail = 0.0
    for k in ("head_pool", "gemm_cls_tail"):
        e = prof.get(k)
        if e:
            t_us = e["total_ms"] * 1e3 - e["launches"] * bracket
            tail += t_us
            say(f"pooled tail {dname} class {k:14s}: {e['launches']:3d} launches, {t_us:7.1f} us (event brackets of {bracket:.1f} us subtracted; sub-batches run back to back while profiling)")
    say(f"pooled tail {dname}: {tail:7.1f} us of the profiled forward + one LayerNorm launch per sub-batch")
    for r in runs:
        r["c"].close(); r["m"].close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
