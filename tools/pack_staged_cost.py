"""Cost of the staged packed attention kernel (attention_packed_staged.hip), interleaved rounds in ONE process on one GPU, on the pattern of tools/pack_cost.py:
    python tools/pack_staged_cost.py [--rounds R] [--steps S] [--images N] [--parent-lib PATH] [--out profiles/pack_staged_cost.txt]
  1. the kernel alone, bf16 and F16, D 768, H 12, on the packs of pack_cost.py (256 x 197, 64 x 577, the seeded mixed pack): the staged kernel and the
     packed generic kernel on the same tables (vitx_op_attention_packed_tables_ex), beside vitx_op_attention (the tuned dispatcher) on the uniform packs;
     output bits staged against generic at the timed sizes; algorithmic bytes and FLOPs per launch from the shapes.
  2. the forward of the mixed pack and of the uniform N x 224^2 pack, ViT-B/16, bf16: PackContext(attn_kernel=STAGED) and (attn_kernel=GENERIC) in alternating
     rounds and, with --parent-lib (a libvitx.so built from the parent commit), that library's packed context in the same rounds: the baseline of the gain.
Nothing here is a gate.  Not measured: other H and D, HBM-cold tables, packs of very short images (300 x 2 runs in a test, not as a workload)."""
import argparse, importlib.util, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--steps", type=int, default=10); ap.add_argument("--images", type=int, default=256)
ap.add_argument("--model", default="vit_base_patch16_224"); ap.add_argument("--skip-forward", action="store_true"); ap.add_argument("--parent-lib", default="")
ap.add_argument("--resources", help="the compiler's remark for the kernel, ENTERED BY HAND: re-read it after any change to the kernel or its flags", default="62 (F16) / 63 (bf16) VGPRs, 32768 bytes of static LDS, no scratch; 5 workgroups (20 waves) per CU, bound by LDS")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_staged_cost.txt"))
a = ap.parse_args()
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(ts, unit="ms", scale=1.0):
    m, lo, hi = med(ts)
    return f"median {m * scale:.3f} {unit} [{lo * scale:.3f} .. {hi * scale:.3f}]"


def rounds(runs, iters, stream=None):
    """Interleaved: every run `iters` times between two events on `stream` (None: the null stream), run after run, a.rounds times; r["ts"] in ms per call."""
    stream = stream or torch.cuda.default_stream()
    torch.cuda.synchronize()
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


say(f"# tools/pack_staged_cost.py --model {a.model} --images {a.images} --rounds {a.rounds} --steps {a.steps}   ({torch.cuda.get_device_name(0)})")
say(f"attention_packed_staged_kernel, copied BY HAND (--resources) from hipcc -Rpass-analysis=kernel-resource-usage for gfx950, not read by this tool: {a.resources}")
D, H, P = 768, 12, 16
rng = np.random.default_rng(7)                                                      # pack_cost.py's mixed pack
sources = [(int(rng.integers(320, 1281)), int(rng.integers(320, 1281))) for _ in range(a.images)]
shapes = [B.rect_shape(nx, ny, P, 224, 448)[::-1] for nx, ny in sources]            # (h, w)
tokens = [1 + (h // P) * (w // P) for h, w in shapes]
say(f"mixed pack: {a.images} images, {len(set(shapes))} distinct shapes, {min(tokens)} .. {max(tokens)} tokens, sum N = {sum(tokens)}, sum N^2 = {sum(t * t for t in tokens)}")

# ---- 1. the kernel alone
L = B.lib()
for dtype, tname, tdt in ((B.BF16, "bf16", torch.bfloat16), (B.F16, "F16", torch.float16)):
    for label, counts, uniform in (("256 x 197", [197] * 256, True), ("64 x 577", [577] * 64, True), (f"mixed {a.images}", tokens, False)):
        row0 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        qb0 = np.concatenate([[0], np.cumsum([(c + 63) // 64 for c in counts])]).astype(np.int32)
        d_row0, d_qb0, rows, qblocks, n = torch.from_numpy(row0).cuda(), torch.from_numpy(qb0).cuda(), int(row0[-1]), int(qb0[-1]), len(counts)
        qkv = (torch.randn((rows, 3 * D), device="cuda") * 0.5).to(tdt)
        outs = [torch.zeros((rows, D), dtype=tdt, device="cuda") for _ in range(3)]
        tab = lambda kern, o: B.check(L.vitx_op_attention_packed_tables_ex(dtype, kern, qkv.data_ptr(), o.data_ptr(), d_row0.data_ptr(), d_qb0.data_ptr(), n, qblocks, D, H))
        runs = [dict(name="staged", ts=[], f=lambda: tab(B.PACK_ATTN_STAGED, outs[0])), dict(name="generic", ts=[], f=lambda: tab(B.PACK_ATTN_GENERIC, outs[1]))]
        if uniform:
            runs.append(dict(name="dispatcher", ts=[], f=lambda: B.check(L.vitx_op_attention(dtype, qkv.data_ptr(), outs[2].data_ptr(), n, counts[0], D, H, None))))
        rounds(runs, 20)
        n2 = sum(c * c for c in counts)
        say(f"attention {tname} {label}: algorithmic {rows * 4 * D * 2 / 1e6:.1f} MB (qkv read once, out written), {4 * n2 * D / 1e9:.2f} GFLOP (Q.K^T once and P.V) per launch")
        differ = int((outs[0].view(torch.int16) != outs[1].view(torch.int16)).sum())
        for r in runs:
            note = ""
            if r["name"] == "staged":
                s, g = med(r["ts"]), med(runs[1]["ts"])
                note = f"   {g[0] / s[0]:.2f} x the generic kernel's rate, ranges {'do not overlap' if s[2] < g[1] else 'OVERLAP'}; " + \
                       ("bits equal to generic" if differ == 0 else f"{differ} ELEMENTS DIFFER from generic")
            if r["name"] == "dispatcher":
                note = f"   staged / dispatcher = {med(runs[0]['ts'])[0] / med(r['ts'])[0]:.2f} (reported, not gated)"
            say(f"attention {tname} {label:10s} {r['name']:10s}: {fmt(r['ts'], 'us', 1e3)} per launch{note}")
        del qkv, outs


def write_record():
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if a.skip_forward:
    write_record()
    sys.exit(0)

# ---- 2. forwards: this library's two kernels and the parent commit's library in the same rounds
libs = [("this tree", B)]
if a.parent_lib:
    spec = importlib.util.spec_from_file_location("vitcpp_amd.binding_parent", os.path.join(_pkg.PKG_DIR, "binding.py"))
    BP = importlib.util.module_from_spec(spec); sys.modules[spec.name] = BP; spec.loader.exec_module(BP)
    BP.LIB_PATH = os.path.abspath(a.parent_lib)
    libs.append(("parent commit", BP))
hp = pkg.synth.hparams_for(a.model)
path = pkg.synth.cached_synthetic(a.model, head_scale=8.0)
models = {name: b.Model(path) for name, b in libs}
C, S = hp.num_classes, hp.img_size
order = sorted(range(a.images), key=lambda i: shapes[i])
sh_arr = np.asarray([shapes[i] for i in order], np.int32)
uni = np.asarray([(S, S)] * a.images, np.int32)
probs = torch.empty((a.images, C), device="cuda")
side = torch.cuda.Stream()
for label, sh, ntok in ((f"{a.images} mixed-shape images", sh_arr, sum(tokens)), (f"uniform pack {a.images} x {S}^2", uni, a.images * (1 + (S // P) ** 2))):
    pixels = torch.randn((int(sum(int(h) * int(w) * 3 for h, w in sh)),), device="cuda")
    ctxs = [("STAGED", B.PackContext(models["this tree"], 0, max_tokens=ntok, max_images=a.images, dtype=B.BF16, attn_kernel=B.PACK_ATTN_STAGED)),
            ("GENERIC", B.PackContext(models["this tree"], 0, max_tokens=ntok, max_images=a.images, dtype=B.BF16, attn_kernel=B.PACK_ATTN_GENERIC))]
    if a.parent_lib:
        ctxs.append(("parent commit's library", BP.PackContext(models["parent commit"], 0, max_tokens=ntok, max_images=a.images, dtype=BP.BF16)))
    runs = [dict(name=name, ts=[], f=(lambda c=c: c.forward_device(pixels.data_ptr(), sh, probs.data_ptr(), 0, side.cuda_stream))) for name, c in ctxs]
    rounds(runs, a.steps, side)
    say(f"forward {a.model} bf16, {label} ({ntok} tokens):")
    base = runs[-1]
    for r in runs:
        note = ""
        if a.parent_lib and r is not base:
            m, b = med(r["ts"]), med(base["ts"])
            note = f"   {b[0] / m[0]:.3f} x the parent's rate" + ("" if r["name"] == "STAGED" else f"; median {'inside' if b[1] <= m[0] <= b[2] else 'OUTSIDE'} the parent's min .. max")
        say(f"  {r['name']:24s}: {fmt(r['ts'])}   ({a.images / med(r['ts'])[0] * 1e3:.0f} img/s){note}")
    for _, c in ctxs:
        c.close()
    del pixels
for m in models.values():
    m.close()
write_record()
