"""Cost of rectangular contexts (include/vitx.h "rectangular contexts"), interleaved in ONE process (separate runs are not comparable):
    python tools/rect_cost.py [--parent path/to/the/parent/commit's/libvitx.so] [--rounds R] [--steps S] [--batch B] [--out profiles/rect_cost.txt]
  1. the SQUARE forward against the parent commit: ViT-B/16, 224^2, batch B, bf16, whole forward, the builds alternating for R rounds of S forwards
     (the parent's library is loaded twice, so its own round-to-round and copy-to-copy spread is measured in the same run), and the patch_embed class of
     the per-kernel profile per launch.  The condition: this build's median is not above the parent's by more than the parent's own spread.
  2. pp_pil_kernel against the parent: profiles/preprocess_cost.txt's 500 x 375 case (batch 64, shortest edge 224, crop 224, Pillow bicubic), alternating.
  3. for the record, not gated: a 224 x 448 context (393 tokens) beside a 320 x 320 one (401 tokens), this build only.
Without --parent, 1 and 2 time this build alone."""
import argparse, importlib.util, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; pkg = _pkg.load()

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None); ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batch", type=int, default=256); ap.add_argument("--model", default="vit_base_patch16_224")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rect_cost.txt"))
a = ap.parse_args()
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def load_binding(tag, lib):
    """A copy of the binding module of its own on `lib` (tools/ab_libs.py)."""
    os.environ["VITX_LIB"] = os.path.abspath(lib)
    spec = importlib.util.spec_from_file_location(f"{pkg.__name__}.binding_{tag}", os.path.join(ROOT, "vit.cpp_amd", "binding.py"))
    B = importlib.util.module_from_spec(spec); spec.loader.exec_module(B)
    return B


new_lib = os.path.join(ROOT, "vit.cpp_amd", "libvitx.so")
builds = ([("parent_a", a.parent), ("parent_b", a.parent)] if a.parent else []) + [("new", new_lib)]
bind = {name: load_binding(name, lib) for name, lib in builds}
os.environ.pop("VITX_LIB", None)
B = bind["new"]
n = a.batch
hp = pkg.synth.hparams_for(a.model)
path = pkg.synth.cached_synthetic(a.model, head_scale=8.0)
say(f"# tools/rect_cost.py --model {a.model} --batch {n} --rounds {a.rounds} --steps {a.steps} parent={'given' if a.parent else 'none'}   ({torch.cuda.get_device_name(0)})")
st = torch.cuda.Stream(); ss = st.cuda_stream


def time_forwards(runs, imgs_of):
    for r in runs:
        for _ in range(3): r["c"].forward_device(imgs_of(r).data_ptr(), n, r["probs"].data_ptr(), 0, ss)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for r in runs:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps): r["c"].forward_device(imgs_of(r).data_ptr(), n, r["probs"].data_ptr(), 0, ss)
            torch.cuda.synchronize(); r["ts"].append((time.perf_counter() - t0) / a.steps * 1e3)


def patch_class(runs, imgs_of):
    """The patch_embed class of the per-kernel profile, us per launch: one profiled forward per build and round, build after build; r["pe"] = (median, min, max, launches)."""
    per = {r["name"]: [] for r in runs}
    for _ in range(a.rounds):
        for r in runs:
            c = r["c"]
            c.profile_enable(True); c.forward_device(imgs_of(r).data_ptr(), n, r["probs"].data_ptr(), 0, ss); torch.cuda.synchronize()
            prof = {e["name"]: e for e in c.profile_read()}; c.profile_enable(False)
            e = prof["patch_embed"]
            per[r["name"]].append((e["total_ms"] * 1e3 - e["launches"] * c.profile_bracket_us()) / e["launches"]); r["pe_launches"] = e["launches"]
    for r in runs:
        r["pe"] = med(per[r["name"]])


# 1. the square forward, build after build
imgs = torch.randn((n, hp.img_size, hp.img_size, 3), device="cuda")
runs = []
for name, _ in builds:
    m = bind[name].Model(path)
    runs.append(dict(name=name, m=m, c=bind[name].Context(m, 0, n, bind[name].BF16), ts=[], probs=torch.empty((n, hp.num_classes), device="cuda")))
time_forwards(runs, lambda r: imgs)
patch_class(runs, lambda r: imgs)
for r in runs:
    m_, lo, hi = med(r["ts"])
    same = "" if r is runs[0] else ("  probabilities bit-identical to " + runs[0]["name"] if torch.equal(r["probs"], runs[0]["probs"]) else "  PROBABILITIES DIFFER from " + runs[0]["name"])
    say(f"forward {a.model} b{n} bf16 {r['name']:9s}: median {m_:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({n / m_ * 1e3:.0f} img/s)   patch_embed {r['pe'][0]:.1f} us per launch [{r['pe'][1]:.1f} .. {r['pe'][2]:.1f}] ({r['pe_launches']} launches){same}")
if a.parent:
    pa, pb, nw = (med(r["ts"]) for r in runs)
    parent = min(pa[0], pb[0])
    spread = max(pa[2], pb[2]) - min(pa[1], pb[1])
    say(f"new median - parent median = {nw[0] - parent:+.3f} ms; the parent's own spread in this run (both copies, min to max) {spread:.3f} ms: "
        f"{'INSIDE' if nw[0] - parent <= spread else 'OUTSIDE'} the condition")
    pe = [r["pe"] for r in runs]
    pe_parent, pe_spread = min(pe[0][0], pe[1][0]), max(pe[0][2], pe[1][2]) - min(pe[0][1], pe[1][1])
    say(f"patch_embed per launch: new median - parent median = {pe[2][0] - pe_parent:+.1f} us; the parent's own spread {pe_spread:.1f} us: "
        f"{'INSIDE' if pe[2][0] - pe_parent <= pe_spread else 'OUTSIDE'} the condition")
for r in runs:
    r["c"].close(); r["m"].close()

# 2. pp_pil_kernel on the 500 x 375 case of profiles/preprocess_cost.txt
nb, S, nx, ny = 64, 224, 500, 375
src = torch.randint(0, 256, (nb, ny, nx, 3), dtype=torch.uint8, device="cuda")
out = torch.empty((nb, S, S, 3), dtype=torch.float32, device="cuda")
imagenet = dict(mean255=tuple(float(v) for v in pkg.synth.IMAGENET_MEAN), std255=tuple(float(v) for v in pkg.synth.IMAGENET_STD))
s0 = torch.cuda.current_stream().cuda_stream
pruns = [dict(name=name, B=bind[name], pp=bind[name].Preproc.make(bind[name].PP_SHORTEST_EDGE, S, 0, bind[name].PP_PIL_BICUBIC, crop=S, **imagenet), ts=[]) for name, _ in builds]
iters = 200
for r in pruns:
    for _ in range(5): r["B"].preprocess_ex_device(r["pp"], src.data_ptr(), nb, nx, ny, out.data_ptr(), s0)
torch.cuda.synchronize()
for _ in range(a.rounds):
    for r in pruns:
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters): r["B"].preprocess_ex_device(r["pp"], src.data_ptr(), nb, nx, ny, out.data_ptr(), s0)
        e1.record(); torch.cuda.synchronize()
        r["ts"].append(e0.elapsed_time(e1) / iters)
for r in pruns:
    m_, lo, hi = med(r["ts"])
    say(f"pp_pil_kernel bicubic {nx} x {ny} -> {S}^2 b{nb} {r['name']:9s}: median {m_:.4f} ms  min {lo:.4f}  max {hi:.4f}")
if a.parent:
    pa, pb, nw = (med(r["ts"]) for r in pruns)
    parent = min(pa[0], pb[0])
    spread = max(pa[2], pb[2]) - min(pa[1], pb[1])
    say(f"new median - parent median = {nw[0] - parent:+.4f} ms; the parent's own spread {spread:.4f} ms: {'INSIDE' if nw[0] - parent <= spread else 'OUTSIDE'} the condition")
# ... and the rectangular window of the same source (288 x 224, vitx_rect_shape), this build
w, h = B.rect_shape(nx, ny, hp.patch_size, S)
out_r = torch.empty((nb, h, w, 3), dtype=torch.float32, device="cuda")
ts = []
for _ in range(a.rounds):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): B.preprocess_rect_device(pruns[-1]["pp"], src.data_ptr(), nb, nx, ny, w, h, out_r.data_ptr(), s0)
    e1.record(); torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1) / iters)
m_, lo, hi = med(ts)
say(f"pp_pil_kernel bicubic {nx} x {ny} -> {w} x {h} (rect) b{nb} new: median {m_:.4f} ms  min {lo:.4f}  max {hi:.4f}")

# 3. for the record: 224 x 448 (393 tokens) beside 320 x 320 (401 tokens)
m = B.Model(path)
runs = []
for name, kw, shape in (("320 x 320", dict(img_size=320), (320, 320)), ("224 x 448", dict(img_shape=(224, 448)), (224, 448))):
    c = B.Context(m, 0, n, B.BF16, **kw)
    runs.append(dict(name=name, c=c, ts=[], probs=torch.empty((n, hp.num_classes), device="cuda"), imgs=torch.randn((n, shape[0], shape[1], 3), device="cuda"), tokens=c.tokens))
time_forwards(runs, lambda r: r["imgs"])
patch_class(runs, lambda r: r["imgs"])
for r in runs:
    m_, lo, hi = med(r["ts"])
    say(f"forward {a.model} b{n} bf16 context {r['name']} ({r['tokens']} tokens): median {m_:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({n / m_ * 1e3:.0f} img/s, "
        f"{m_ / r['tokens'] / n * 1e6:.2f} ns per token)   patch_embed {r['pe'][0]:.1f} us per launch")
    r["c"].close()
m.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
