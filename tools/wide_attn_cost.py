"""Cost of the LDS-staged attention of head dims 72 .. 128 (attention_wide.hip), interleaved rounds in ONE process on one GPU, on the pattern of
tools/pack_staged_cost.py:
    python tools/wide_attn_cost.py [--rounds R] [--out profiles/wide_attn_cost.txt]
1. The kernel alone, bf16 and F16, at SO400M's (64 x 729 tokens, D 1152, H 16: head dim 72), ViT-H/14's (256 x 257, D 1280, H 16: head dim 80) and
bigG/14's (64 x 257, D 1664, H 16: head dim 104) shapes and one line at head dim 128 (64 x 257, D 2048, H 16): vitx_op_attention_wide against vitx_op_attention_generic on the same buffer, output bits
compared at the timed sizes; algorithmic bytes and FLOPs per launch from the shapes.  The CONDITION per line: faster than the generic kernel with
min .. max ranges that do not overlap; a line that misses it says so.  Not measured (the record says so itself): other N, head dims 88, 96, 112, 120, HBM-cold inputs, packs at
these head dims (they keep attention_packed_kernel).
Then the forward of an SO400M-shaped synthetic file -- D 1152, 27 layers, 16 heads of 72, `mlp` width 4304 (run as 4352), patch 14, 378^2 (SO400M's own
384^2 gives the same 27 x 27 grid; a file's image size is a multiple of its patch), class token + linear head instead of the attention-pooling head --
batch 64, bf16 and F16: a first number, nothing exists to compare it with (--skip-forward leaves it out)."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--resources", help="the compiler's remarks for the kernel, ENTERED BY HAND: re-read them after any change to the kernel or its flags",
                default="head dim 72 / 80 / 104 / 128: 70 / 70 / 84 / 96 VGPRs, 36880 / 40960 / 53264 / 65536 bytes of static LDS, no scratch; 4 / 4 / 3 / 2 workgroups per CU, bound by LDS")
ap.add_argument("--skip-forward", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_attn_cost.txt"))
a = ap.parse_args()
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


say(f"# tools/wide_attn_cost.py --rounds {a.rounds} --iters {a.iters}   ({torch.cuda.get_device_name(0)})")
say(f"attention_wide_kernel, copied BY HAND (--resources) from hipcc -Rpass-analysis=kernel-resource-usage for gfx950, not read by this tool: {a.resources}")
L = B.lib()
met = True
for dtype, tname, tdt in ((B.BF16, "bf16", torch.bfloat16), (B.F16, "F16", torch.float16)):
    for label, n, N, D, H in (("SO400M 64 x 729", 64, 729, 1152, 16), ("ViT-H/14 256 x 257", 256, 257, 1280, 16), ("bigG/14 64 x 257", 64, 257, 1664, 16), ("head dim 128, 64 x 257", 64, 257, 2048, 16)):
        qkv = (torch.randn((n * N, 3 * D), device="cuda") * 0.5).to(tdt)
        outs = [torch.zeros((n * N, D), dtype=tdt, device="cuda") for _ in range(2)]
        runs = [dict(name="wide", ts=[], f=lambda: B.op_attention_wide(dtype, qkv.data_ptr(), outs[0].data_ptr(), n, N, D, H)),
                dict(name="generic", ts=[], f=lambda: B.check(L.vitx_op_attention_generic(dtype, qkv.data_ptr(), outs[1].data_ptr(), n, N, D, H, None)))]
        for r in runs:
            for _ in range(3): r["f"]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):                                   # interleaved: every run a.iters times between two events on the null stream, run after run
            for r in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(torch.cuda.default_stream())
                for _ in range(a.iters): r["f"]()
                e1.record(torch.cuda.default_stream()); torch.cuda.synchronize()
                r["ts"].append(e0.elapsed_time(e1) / a.iters)
        differ = int((outs[0].view(torch.int16) != outs[1].view(torch.int16)).sum())
        w, g = med(runs[0]["ts"]), med(runs[1]["ts"])
        ok = w[2] < g[1]
        met = met and ok and differ == 0
        say(f"attention {tname} {label} (head dim {D // H}): algorithmic {n * N * 4 * D * 2 / 1e6:.1f} MB (qkv read once, out written), {4 * n * N * N * D / 1e9:.2f} GFLOP (Q.K^T once and P.V) per launch")
        say(f"  wide   : median {w[0] * 1e3:.1f} us [{w[1] * 1e3:.1f} .. {w[2] * 1e3:.1f}] per launch   {g[0] / w[0]:.2f} x the generic kernel's rate, ranges "
            f"{'do not overlap: condition met' if ok else 'OVERLAP or slower: CONDITION NOT MET'}; " + ("bits equal to generic" if differ == 0 else f"{differ} ELEMENTS DIFFER from generic"))
        say(f"  generic: median {g[0] * 1e3:.1f} us [{g[1] * 1e3:.1f} .. {g[2] * 1e3:.1f}] per launch")
        del qkv, outs
say("condition (faster than the generic kernel, ranges apart, equal bits) on every line: " + ("met" if met else "NOT MET"))
if not a.skip_forward:
    D, Lyr, H, F, P, S, n = 1152, 27, 16, 4304, 14, 378, 64
    path = os.path.join(os.environ.get("VITX_CACHE", "/tmp/vitx_cache"), "so400m_shaped_synth.gguf")
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        hp = pkg.ggml_file.HParams(D, Lyr, H, 1000, P, S, 1)
        t = pkg.synth.make_weights(hp)
        for i in range(Lyr):                                        # the 4 D wide MLP cut to F rows / columns
            q = f"blocks.{i}.mlp."
            t[q + "fc1.weight"], t[q + "fc1.bias"], t[q + "fc2.weight"] = t[q + "fc1.weight"][:F].copy(), t[q + "fc1.bias"][:F].copy(), t[q + "fc2.weight"][:, :F].copy()
        pkg.ggml_file.write_model(path, hp, {"mlp": np.array([F, 0, 0, 0], np.float32), **t})
    model = B.Model(path)
    imgs = torch.randn((n, S, S, 3), device="cuda")
    probs = torch.empty((n, 1000), device="cuda")
    side = torch.cuda.Stream()
    for dtype, tname in ((B.BF16, "bf16"), (B.F16, "F16")):
        ctx = B.Context(model, device=0, max_batch=n, dtype=dtype)
        for _ in range(2): ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, side.cuda_stream)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            for _ in range(3): ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, side.cuda_stream)
            e1.record(side); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 3)
        m = med(ts)
        say(f"forward, SO400M-shaped synthetic file (D {D}, {Lyr} layers, {H} heads of {D // H}, mlp {F} -> {(F + 63) // 64 * 64}, {S}^2 = {1 + (S // P) ** 2} tokens, class-token head), batch {n}, {tname}: "
            f"median {m[0]:.2f} ms [{m[1]:.2f} .. {m[2]:.2f}]   ({n / m[0] * 1e3:.0f} img/s); finite probabilities: {bool(torch.isfinite(probs).all())}")
        ctx.close()
    model.close()
say("NOT MEASURED: other N, head dims 88, 96, 112, 120, HBM-cold inputs, packs at these head dims (they keep attention_packed_kernel), the attention-pooling head at SO400M's size; "
    "hand-entered records (float64 errors, the bench.py regression check) live in profiles/wide_attn_notes.txt, which this tool does not write.")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
