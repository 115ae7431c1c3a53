"""Cost of the windowed attention with a decomposed relative position term (attention_window.hip), interleaved rounds in ONE process on one GPU, in the
manner of tools/relbias_cost.py:
    python tools/window_cost.py [--rounds R] [--iters I] [--images N] [--out profiles/window_cost.txt]
At the Segment-Anything ViT-B shape (grid 64 x 64, D 768, 12 heads, random tables in +-0.5):
  * a windowed layer (ws 14: 25 windows per image, the edge ones padded) against vitx_op_attention_generic on the same amount of work posed as 25 N
    images of 196 tokens (no position term, no pads: what the arithmetic costs without the windows and the term);
  * a global layer (one 64 x 64 window) against vitx_op_attention, the tuned dispatcher, at 4096 tokens.
Nothing here is a gate.  Not measured: other grids, HBM-cold tables, a whole encoder (no file of Segment-Anything's size is timed)."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=10); ap.add_argument("--images", type=int, default=4)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_cost.txt"))
a = ap.parse_args()
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


say(f"# tools/window_cost.py --rounds {a.rounds} --iters {a.iters} --images {a.images}   ({torch.cuda.get_device_name(0)})")
L, g, ws, H, n = B.lib(), 64, 14, 12, a.images
D, G = 64 * H, g * g
for dtype, tname, tdt in ((B.BF16, "bf16", torch.bfloat16), (B.F16, "F16", torch.float16)):
    qkv = (torch.randn((n * G, 3 * D), device="cuda") * 0.5).to(tdt)
    qkvw = (torch.randn((25 * n * ws * ws, 3 * D), device="cuda") * 0.5).to(tdt)
    tabs = {w: [(torch.rand((2 * w - 1, 64), device="cuda") - 0.5).to(tdt) for _ in range(2)] for w in (ws, g)}
    bias = torch.rand(3 * D, device="cuda") - 0.5
    outs = [torch.zeros((max(n * G, len(qkvw)), D), dtype=tdt, device="cuda") for _ in range(4)]
    win = lambda w, o: B.attention_window(dtype, qkv.data_ptr(), tabs[w][0].data_ptr(), tabs[w][1].data_ptr(), bias.data_ptr(), o.data_ptr(), n, g, w, D, H)
    pairs = [("windowed ws 14", [dict(name="window", ts=[], f=lambda: win(ws, outs[0])),
                                 dict(name=f"generic {25 * n} x 196", ts=[], f=lambda: B.check(L.vitx_op_attention_generic(dtype, qkvw.data_ptr(), outs[1].data_ptr(), 25 * n, ws * ws, D, H, None)))]),
             ("global 64 x 64", [dict(name="window", ts=[], f=lambda: win(g, outs[2])),
                                 dict(name="dispatcher N 4096", ts=[], f=lambda: B.check(L.vitx_op_attention(dtype, qkv.data_ptr(), outs[3].data_ptr(), n, G, D, H, None)))])]
    for label, runs in pairs:
        for r in runs:
            for _ in range(2): r["f"]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):                       # interleaved: every run a.iters times between two events on the null stream, run after run
            for r in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters): r["f"]()
                e1.record(); torch.cuda.synchronize()
                r["ts"].append(e0.elapsed_time(e1) / a.iters)
        base = sorted(runs[0]["ts"])
        for r in runs:
            ts = sorted(r["ts"])
            note = "" if r is runs[0] else f"   window / this = {base[len(base) // 2] / ts[len(ts) // 2]:.2f}, ranges {'do not overlap' if base[0] > ts[-1] or base[-1] < ts[0] else 'OVERLAP'} (reported, not gated)"
            say(f"attention {tname} {n} x {g} x {g}, {H} heads, {label:15s} {r['name']:18s}: median {ts[len(ts) // 2] * 1e3:.1f} us [{ts[0] * 1e3:.1f} .. {ts[-1] * 1e3:.1f}] per launch{note}")
    del qkv, qkvw, outs
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
