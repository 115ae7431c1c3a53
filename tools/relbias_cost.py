"""Cost of the relative position bias inside the attention (attention_bias.hip), interleaved rounds in ONE process on one GPU, on the pattern of
tools/pack_staged_cost.py:
    python tools/relbias_cost.py [--rounds R] [--iters I] [--out profiles/relbias_cost.txt]
The kernel (vitx_op_attention_bias, random tables in +-2) against vitx_op_attention -- the tuned dispatcher, what a context of the same shape would run
if the term did not exist -- and vitx_op_attention_generic, whose arithmetic it shares, on the same qkv: ViT-B/16 at 224^2 (256 x 12 heads x 197
tokens, grid 14) and ViT-L/16 at 384^2 (64 x 16 heads x 577 tokens, grid 24), bf16 and F16.  Algorithmic bytes and FLOPs per launch from the shapes.
Nothing here is a gate.  Not measured: other grids, HBM-cold tables, a whole forward (no BEiT-sized fixture is timed)."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relbias_cost.txt"))
a = ap.parse_args()
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


say(f"# tools/relbias_cost.py --rounds {a.rounds} --iters {a.iters}   ({torch.cuda.get_device_name(0)})")
L = B.lib()
for dtype, tname, tdt in ((B.BF16, "bf16", torch.bfloat16), (B.F16, "F16", torch.float16)):
    for label, n, H, g in (("ViT-B/16 256 x 197", 256, 12, 14), ("ViT-L/16 64 x 577", 64, 16, 24)):
        N, D = g * g + 1, 64 * H
        qkv = (torch.randn((n * N, 3 * D), device="cuda") * 0.5).to(tdt)
        table = torch.rand((H, (2 * g - 1) ** 2 + 3), device="cuda") * 4 - 2
        outs = [torch.zeros((n * N, D), dtype=tdt, device="cuda") for _ in range(3)]
        runs = [dict(name="bias", ts=[], f=lambda: B.attention_bias(dtype, qkv.data_ptr(), table.data_ptr(), outs[0].data_ptr(), n, g, g, D, H)),
                dict(name="dispatcher", ts=[], f=lambda: B.check(L.vitx_op_attention(dtype, qkv.data_ptr(), outs[1].data_ptr(), n, N, D, H, None))),
                dict(name="generic", ts=[], f=lambda: B.check(L.vitx_op_attention_generic(dtype, qkv.data_ptr(), outs[2].data_ptr(), n, N, D, H, None)))]
        for r in runs:
            for _ in range(3): r["f"]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):                       # interleaved: every run a.iters times between two events on the null stream, run after run
            for r in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters): r["f"]()
                e1.record(); torch.cuda.synchronize()
                r["ts"].append(e0.elapsed_time(e1) / a.iters)
        say(f"attention {tname} {label}: algorithmic {n * N * 4 * D * 2 / 1e6:.1f} MB (qkv read once, out written; the tables: {table.numel() * 4 / 1e3:.1f} KB), "
            f"{4 * n * N * N * D / 1e9:.2f} GFLOP (Q.K^T once and P.V) per launch")
        b = med(runs[0]["ts"])
        for r in runs:
            m, lo, hi = med(r["ts"])
            note = "" if r is runs[0] else f"   bias / {r['name']} = {b[0] / m:.2f}, ranges {'do not overlap' if b[1] > hi or b[2] < lo else 'OVERLAP'} (reported, not gated)"
            say(f"attention {tname} {label:18s} {r['name']:10s}: median {m * 1e3:.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}] per launch{note}")
        del qkv, outs
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
