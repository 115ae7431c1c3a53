"""Cost of the MLP activations (vitx_activation: tanh-GELU, erf-GELU, QuickGELU), interleaved in ONE process (separate runs are not comparable):
    python tools/act_cost.py [--rounds R] [--iters I] [--steps S] [--batch B]
  1. the fc1 GEMM with each activation's epilogue (vitx_op_gemm epi 1 / 6 / 7) at the forward's shapes, both operand types: rounds of I launches,
     activation after activation, R times; median, min and max of the per-launch time;
  2. the whole ViT-B/16 forward at batch B of a tanh file against the same weights written with `arch` = erf / QuickGELU, both operand types."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batch", type=int, default=256); ap.add_argument("--model", default="vit_base_patch16_224")
a = ap.parse_args()
L = B.lib()
ACTS = (("tanh", 1, 0), ("erf", 6, 1), ("quick", 7, 2))          # name, fc1 epilogue, vitx_activation
s = torch.cuda.current_stream().cuda_stream


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


# 1. fc1: M = the rows of 128 images (one stream), and of the two sub-batches of a 256-image forward (103 + 153 images), padded to 256
N, K = 3072, 768
for dname, dt, tdt in (("bf16", B.BF16, torch.bfloat16), ("f16", B.F16, torch.float16)):
    for M in (25344, 20480, 30208):
        g = torch.Generator(device="cuda").manual_seed(1)
        A = (torch.randn((M, K), device="cuda", generator=g) * 0.5).to(tdt)
        W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(tdt)
        bias = torch.randn(N, device="cuda", generator=g) * 0.1
        out = torch.zeros((M, N), device="cuda", dtype=tdt)
        ts = {n: [] for n, _, _ in ACTS}
        for n, epi, _ in ACTS:
            for _ in range(3): B.check(L.vitx_op_gemm(dt, epi, A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, s))
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for n, epi, _ in ACTS:
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters): L.vitx_op_gemm(dt, epi, A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, s)
                e1.record(); torch.cuda.synchronize()
                ts[n].append(e0.elapsed_time(e1) / a.iters * 1e3)
        base = med(ts["tanh"])[0]
        for n, _, _ in ACTS:
            m, lo, hi = med(ts[n])
            print(f"fc1 {dname} M={M} N={N} K={K} {n:5s}: median {m:7.1f} us  min {lo:7.1f}  max {hi:7.1f}  ({2.0 * M * N * K / m / 1e6:6.1f} TF/s)  x{m / base:.4f} of tanh", flush=True)

# 2. the whole forward: one file per activation, the same weights
hp = pkg.synth.hparams_for(a.model)
w = pkg.synth.make_weights(hp, head_scale=8.0)
cache = os.environ.get("VITX_CACHE", "/tmp/vitx_cache"); os.makedirs(cache, exist_ok=True)
imgs = torch.randn((a.batch, hp.img_size, hp.img_size, 3), device="cuda")
st = torch.cuda.Stream(); ss = st.cuda_stream
for dname, dt in (("bf16", B.BF16), ("f16", B.F16)):
    runs = []
    for n, _, act in ACTS:
        path = os.path.join(cache, f"act_cost-{a.model}-{n}.gguf")
        if not os.path.exists(path):
            t = dict(w) if act == 0 else {"arch": np.array([act, 1e-6, 0, 0], np.float32), **w}
            pkg.ggml_file.write_model(path, hp, t, ftype=1)
        m = B.Model(path); assert m.activation == act
        c = B.Context(m, 0, a.batch, dt)
        runs.append(dict(name=n, m=m, c=c, ts=[], probs=torch.empty((a.batch, hp.num_classes), device="cuda")))
    for r in runs:
        for _ in range(3): r["c"].forward_device(imgs.data_ptr(), a.batch, r["probs"].data_ptr(), 0, ss)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for r in runs:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps): r["c"].forward_device(imgs.data_ptr(), a.batch, r["probs"].data_ptr(), 0, ss)
            torch.cuda.synchronize(); r["ts"].append((time.perf_counter() - t0) / a.steps * 1e3)
    base = med(runs[0]["ts"])[0]
    for r in runs:
        m_, lo, hi = med(r["ts"])
        print(f"forward {a.model} b{a.batch} {dname} {r['name']:5s}: median {m_:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({a.batch / m_ * 1e3:.0f} img/s)  x{m_ / base:.4f} of tanh", flush=True)
    for r in runs:
        r["c"].close(); r["m"].close()
