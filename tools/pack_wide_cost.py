"""Cost of the staged packed attention kernel of head dims 72 .. 128 (attention_packed_wide.hip), interleaved rounds in ONE process on one GPU, on the
pattern of tools/pack_staged_cost.py:
    python tools/pack_wide_cost.py [--rounds R] [--iters I] [--skip-forward] [--out profiles/pack_wide_cost.txt]
  1. the kernel alone, bf16 and F16: 64 x 729 at D 1152 / H 16 (SO400M, head dim 72), 256 x 257 at D 1280 / H 16 (ViT-H/14, head dim 80) and the seeded
     mixed pack of tools/pack_cost.py (256 images, 29 shapes) at D 1152 / H 16.  AUTO (the new kernel) and GENERIC (attention_packed_kernel: what the
     parent commit ran here) on the same tables through vitx_op_attention_packed_tables_ex, beside vitx_op_attention_wide (the fixed-shape twin) on the
     uniform packs; output bits AUTO against GENERIC at the timed sizes; algorithmic bytes and FLOPs per launch from the shapes.
  2. the packed forward of the SO400M-shaped synthetic file of tools/wide_attn_cost.py (class-token head), a uniform pack of 64 x 378^2, bf16: a default
     (AUTO) and a GENERIC context in alternating rounds.
Condition: AUTO faster than GENERIC on every line with min .. max ranges apart, and equal bits.  AUTO against the wide kernel is reported, not gated: the
head-dim-64 packed kernel is 1.02 .. 1.04 x its fixed-shape twin's time in profiles/pack_cost.txt (the search of the work list).
Not measured: other head dims, HBM-cold tables, the attention-pooling head at SO400M's size, packs of very short images."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--resources", help="the compiler's remarks for the kernel, ENTERED BY HAND: re-read them after any change to the kernel or its flags",
                default="head dim 72 / 80: 70 / 70 VGPRs, 36880 / 40960 bytes of static LDS, no scratch; 4 / 4 workgroups per CU, bound by LDS")
ap.add_argument("--skip-forward", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_wide_cost.txt"))
a = ap.parse_args()
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def rounds(runs, iters, stream=None):
    """Interleaved: every run `iters` times between two events on `stream` (None: the null stream), run after run, a.rounds times; r["ts"] in ms per call."""
    stream = stream or torch.cuda.default_stream()
    for r in runs:
        for _ in range(3): r["f"]()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for r in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(iters): r["f"]()
            e1.record(stream); torch.cuda.synchronize()
            r["ts"].append(e0.elapsed_time(e1) / iters)


def line(name, ts, scale, unit, note=""):
    m, lo, hi = med(ts)
    say(f"  {name:8s}: median {m * scale:.1f} {unit} [{lo * scale:.1f} .. {hi * scale:.1f}]{note}")


say(f"# tools/pack_wide_cost.py --rounds {a.rounds} --iters {a.iters} --steps {a.steps}   ({torch.cuda.get_device_name(0)})")
say(f"attention_packed_wide_kernel, copied BY HAND (--resources) from hipcc -Rpass-analysis=kernel-resource-usage for gfx950, not read by this tool: {a.resources}")
rng = np.random.default_rng(7)                                                      # pack_cost.py's mixed pack
shapes = [B.rect_shape(int(rng.integers(320, 1281)), int(rng.integers(320, 1281)), 16, 224, 448) for _ in range(256)]
mixed = [1 + (h // 16) * (w // 16) for w, h in shapes]
say(f"mixed pack: 256 images, {len(set(shapes))} distinct shapes, {min(mixed)} .. {max(mixed)} tokens, sum N = {sum(mixed)}, sum N^2 = {sum(t * t for t in mixed)}")
L = B.lib()
met = True
for dtype, tname, tdt in ((B.BF16, "bf16", torch.bfloat16), (B.F16, "F16", torch.float16)):
    for label, counts, D, H, uniform in (("SO400M 64 x 729", [729] * 64, 1152, 16, True), ("ViT-H/14 256 x 257", [257] * 256, 1280, 16, True), ("mixed 256", mixed, 1152, 16, False)):
        row0 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        qb0 = np.concatenate([[0], np.cumsum([(c + 63) // 64 for c in counts])]).astype(np.int32)
        d_row0, d_qb0, rows, qblocks, n = torch.from_numpy(row0).cuda(), torch.from_numpy(qb0).cuda(), int(row0[-1]), int(qb0[-1]), len(counts)
        qkv = (torch.randn((rows, 3 * D), device="cuda") * 0.5).to(tdt)
        outs = [torch.zeros((rows, D), dtype=tdt, device="cuda") for _ in range(3)]
        tab = lambda kern, o: B.check(L.vitx_op_attention_packed_tables_ex(dtype, kern, qkv.data_ptr(), o.data_ptr(), d_row0.data_ptr(), d_qb0.data_ptr(), n, qblocks, D, H))
        runs = [dict(name="auto", ts=[], f=lambda: tab(B.PACK_ATTN_AUTO, outs[0])), dict(name="generic", ts=[], f=lambda: tab(B.PACK_ATTN_GENERIC, outs[1]))]
        if uniform:
            runs.append(dict(name="wide", ts=[], f=lambda: B.op_attention_wide(dtype, qkv.data_ptr(), outs[2].data_ptr(), n, counts[0], D, H)))
        rounds(runs, a.iters)
        differ = int((outs[0].view(torch.int16) != outs[1].view(torch.int16)).sum())
        w, g = med(runs[0]["ts"]), med(runs[1]["ts"])
        ok = w[2] < g[1] and differ == 0
        met = met and ok
        say(f"attention {tname} {label} (head dim {D // H}): algorithmic {rows * 4 * D * 2 / 1e6:.1f} MB (qkv read once, out written), {4 * sum(c * c for c in counts) * D / 1e9:.2f} GFLOP (Q.K^T once and P.V) per launch")
        line("auto", runs[0]["ts"], 1e3, "us", f" per launch   {g[0] / w[0]:.2f} x the generic kernel's rate, ranges {'do not overlap' if w[2] < g[1] else 'OVERLAP or slower: CONDITION NOT MET'}; "
             + ("bits equal to generic" if differ == 0 else f"{differ} ELEMENTS DIFFER from generic"))
        line("generic", runs[1]["ts"], 1e3, "us", " per launch")
        if uniform:
            line("wide", runs[2]["ts"], 1e3, "us", f" per launch   auto / wide = {w[0] / med(runs[2]['ts'])[0]:.3f} (reported, not gated)")
        del qkv, outs
say("condition (faster than the generic packed kernel, ranges apart, equal bits) on every attention line: " + ("met" if met else "NOT MET"))
if not a.skip_forward:
    D, Lyr, H, F, P, S, n = 1152, 27, 16, 4304, 14, 378, 64
    path = os.path.join(os.environ.get("VITX_CACHE", "/tmp/vitx_cache"), "so400m_shaped_synth.gguf")       # tools/wide_attn_cost.py's file
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        hp = pkg.ggml_file.HParams(D, Lyr, H, 1000, P, S, 1)
        t = pkg.synth.make_weights(hp)
        for i in range(Lyr):                                        # the 4 D wide MLP cut to F rows / columns
            q = f"blocks.{i}.mlp."
            t[q + "fc1.weight"], t[q + "fc1.bias"], t[q + "fc2.weight"] = t[q + "fc1.weight"][:F].copy(), t[q + "fc1.bias"][:F].copy(), t[q + "fc2.weight"][:, :F].copy()
        pkg.ggml_file.write_model(path, hp, {"mlp": np.array([F, 0, 0, 0], np.float32), **t})
    model = B.Model(path)
    ntok, sh = n * (1 + (S // P) ** 2), np.asarray([(S, S)] * n, np.int32)
    pixels = torch.randn((n * S * S * 3,), device="cuda")
    probs = [torch.empty((n, 1000), device="cuda") for _ in range(2)]
    side = torch.cuda.Stream()
    ctxs = [(name, B.PackContext(model, 0, max_tokens=ntok, max_images=n, dtype=B.BF16, attn_kernel=k)) for name, k in (("AUTO", B.PACK_ATTN_AUTO), ("GENERIC", B.PACK_ATTN_GENERIC))]
    runs = [dict(name=name, ts=[], f=(lambda c=c, p=p: c.forward_device(pixels.data_ptr(), sh, p.data_ptr(), 0, side.cuda_stream))) for (name, c), p in zip(ctxs, probs)]
    rounds(runs, a.steps, side)
    w, g = med(runs[0]["ts"]), med(runs[1]["ts"])
    say(f"packed forward, SO400M-shaped synthetic file (D {D}, {Lyr} layers, {H} heads of {D // H}, mlp {F}, class-token head), uniform pack {n} x {S}^2 ({ntok} tokens), bf16; "
        f"contexts report attn_kernel {[c.attn_kernel for _, c in ctxs]}; probabilities equal bit for bit: {bool(torch.equal(probs[0].view(torch.int32), probs[1].view(torch.int32)))}")
    line("AUTO", runs[0]["ts"], 1.0, "ms", f"   ({n / w[0] * 1e3:.0f} img/s)   {g[0] / w[0]:.3f} x the GENERIC context's rate, ranges {'do not overlap' if w[2] < g[1] else 'OVERLAP or slower: EXPECTATION NOT MET'}")
    line("GENERIC", runs[1]["ts"], 1.0, "ms", f"   ({n / g[0] * 1e3:.0f} img/s)")
    for _, c in ctxs:
        c.close()
    model.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
