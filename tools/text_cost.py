"""Cost of the text tower (include/vitx.h "the text tower"), interleaved in ONE process (separate runs are not comparable):
    python tools/text_cost.py [--rounds R] [--iters I] [--steps S] [--out profiles/text_cost.txt]
  1. per launch, unmasked, both operand types, at (n 1024, T 77, D 512, H 8) and (n 1024, T 64, D 768, H 12): vitx_op_attention_text against
     vitx_op_attention_generic (the kernel it is modelled on) and vitx_op_attention (the dispatcher's choice); the causal launch of the new kernel
     beside them.  R alternating rounds of I launches; median, min and max.
  2. the whole vitx_text_embed_device at n = 1000 on synthetic towers of the two shapes (CLIP ViT-B/32's text tower: D 512, 12 layers, 8 heads,
     T 77, vocabulary 49408, causal, QuickGELU; SigLIP-B's: D 768, 12 layers, 12 heads, T 64, vocabulary 32000).
Nothing is gated on these numbers: they are recorded as measured."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--prompts", type=int, default=1000); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_cost.txt"))
a = ap.parse_args()
L = B.lib()
s = torch.cuda.current_stream().cuda_stream
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


say(f"# tools/text_cost.py --rounds {a.rounds} --iters {a.iters} --steps {a.steps} --prompts {a.prompts}   ({torch.cuda.get_device_name(0)})")
SHAPES = (("clip_b32", 1024, 77, 512, 8), ("siglip_b", 1024, 64, 768, 12))

# 1. the attention kernels on their own
g = torch.Generator(device="cuda").manual_seed(1)
for name, n, T, D, H in SHAPES:
    for dname, dt, tdt in (("bf16", B.BF16, torch.bfloat16), ("f16", B.F16, torch.float16)):
        qkv = (torch.randn((n * T, 3 * D), device="cuda", generator=g) * 0.8).to(tdt)
        out = torch.zeros((n * T, D), device="cuda", dtype=tdt)
        ops = {"text": lambda: L.vitx_op_attention_text(dt, qkv.data_ptr(), out.data_ptr(), n, T, D, H, 0, s),
               "generic": lambda: L.vitx_op_attention_generic(dt, qkv.data_ptr(), out.data_ptr(), n, T, D, H, s),
               "dispatcher": lambda: L.vitx_op_attention(dt, qkv.data_ptr(), out.data_ptr(), n, T, D, H, s),
               "text causal": lambda: L.vitx_op_attention_text(dt, qkv.data_ptr(), out.data_ptr(), n, T, D, H, 1, s)}
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
        base = med(ts["generic"])[0]
        for k in ops:
            m, lo, hi = med(ts[k])
            say(f"attention {name} n={n} T={T} D={D} H={H} {dname} {k:12s}: median {m:7.1f} us  min {lo:7.1f}  max {hi:7.1f}  x{m / base:.3f} of generic")


# 2. the whole text forward
def synthetic_tower(path, V, T, D, L_, H, E, causal, act, eps, eos):
    rng = np.random.default_rng(D)
    r = lambda *shape: (rng.standard_normal(shape, dtype=np.float32) * np.float32(0.02))
    t = {"arch": np.array([act, eps, causal, eos + 1], np.float32), "token_embed.weight": r(V, D), "pos_embed": r(T, D)}
    for i in range(L_):
        p = f"blocks.{i}."
        for nm, shape in (("norm1", None), ("attn.qkv", (3 * D, D)), ("attn.proj", (D, D)), ("norm2", None), ("mlp.fc1", (4 * D, D)), ("mlp.fc2", (D, 4 * D))):
            t[p + nm + ".weight"] = np.ones(D, np.float32) if shape is None else r(*shape)
            t[p + nm + ".bias"] = np.zeros(D if shape is None else shape[0], np.float32)
    t["norm.weight"] = np.ones(D, np.float32); t["norm.bias"] = np.zeros(D, np.float32)
    t["head.weight"] = r(E, D); t["head.bias"] = np.zeros(E, np.float32)
    pkg.ggml_file.write_model(path, pkg.ggml_file.HParams(D, L_, H, E, 0, T, 1), t, id2label={}, ftype=1)


cache = os.environ.get("VITX_CACHE", "/tmp/vitx_cache"); os.makedirs(cache, exist_ok=True)
TOWERS = (("clip_b32", 49408, 77, 512, 12, 8, 512, 1, 2, 1e-5, 49407), ("siglip_b", 32000, 64, 768, 12, 12, 768, 0, 0, 1e-6, -1))
n = a.prompts
st = torch.cuda.Stream(); ss = st.cuda_stream
for name, V, T, D, L_, H, E, causal, act, eps, eos in TOWERS:
    path = os.path.join(cache, f"text_cost-{name}.gguf")
    if not os.path.exists(path):
        synthetic_tower(path, V, T, D, L_, H, E, causal, act, eps, eos)
    ids = np.random.default_rng(2).integers(1, V - 1, (n, T)).astype(np.int32)
    if eos >= 0:
        ids[np.arange(n), np.random.default_rng(3).integers(4, T, n)] = eos
    m = B.Model(path)
    runs = [dict(dname=dname, c=B.TextContext(m, n, dt), ts=[], out=torch.empty((n, E), device="cuda")) for dname, dt in (("bf16", B.BF16), ("f16", B.F16))]
    for r in runs:
        for _ in range(2): r["c"].embed_device(ids, r["out"].data_ptr(), stream=ss)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for r in runs:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps): r["c"].embed_device(ids, r["out"].data_ptr(), stream=ss)
            torch.cuda.synchronize(); r["ts"].append((time.perf_counter() - t0) / a.steps * 1e3)
    for r in runs:
        m_, lo, hi = med(r["ts"])
        say(f"text forward {name} n={n} T={T} D={D} L={L_} {r['dname']}: median {m_:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({n / m_ * 1e3:.0f} prompts/s, host id check and upload included)")
        r["c"].close()
    m.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
