"""Cost of the depth head (include/vitx.h "depth estimation"), interleaved in ONE process (separate runs are not comparable):
    python tools/depth_cost.py [--parent path/to/the/parent/commit's/libvitx.so] [--rounds R] [--iters I] [--steps S] [--batch B] [--out profiles/depth_cost.txt]
ViT-B/14-shaped, batch B, bf16, K = 256 bins, upsample 4, depth maps at the image's own size, a head with a class half over one layer and over four,
raw rows:
  1. depth_fine per launch (one sub-batch: the larger of the forward's two), beside a device-to-device copy that moves the same algorithmic bytes -- the
     logits read once and the fine plane written once -- so a copy of half their sum, read and written; depth_resize per launch;
  2. the other stages per launch: the raw operand rows of one layer (vitx_op_depth_rows), the patch GEMM and the class GEMM (vitx_op_gemm at their shapes);
  3. the whole forward with the head set against the SAME shape of context with last_layer_all_rows = 1 and no head (the head makes the last layer
     compute every row: that part is not the head's own cost), alternating, R rounds of S steps: median, min and max of each;
  4. the same at 518 x 518 (1369 patches);
  5. with --parent: the forward WITHOUT a depth head against the parent commit's library (loaded twice, so its own spread is measured in the same run),
     224 x 224, the builds alternating; the condition: this build's median lies inside the parent's min .. max range, and the probabilities are bit-identical.
Not measured: f16, upsample 1 and 2, SID bins (the kernels do not see the difference), non-integer output scales.  No gate rests on these figures."""
import argparse, importlib.util, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _pkg; pkg = _pkg.load()

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batch", type=int, default=256); ap.add_argument("--model", default="vit_base_patch14_224")
ap.add_argument("--sizes", type=int, nargs="+", default=[224, 518])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_cost.txt"))
a = ap.parse_args()
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def up(v, m):
    return (v + m - 1) // m * m


def load_binding(tag, lib):
    """A copy of the binding module of its own on `lib` (tools/ab_libs.py)."""
    os.environ["VITX_LIB"] = os.path.abspath(lib)
    spec = importlib.util.spec_from_file_location(f"{pkg.__name__}.binding_{tag}", os.path.join(ROOT, "vit.cpp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    mod.lib()
    return mod


new_lib = os.path.join(ROOT, "vit.cpp_amd", "libvitx.so")
builds = ([("parent_a", a.parent), ("parent_b", a.parent)] if a.parent else []) + [("new", new_lib)]
bind = {name: load_binding(name, lib) for name, lib in builds}
os.environ.pop("VITX_LIB", None)
B = bind["new"]
L = B.lib()


def timed(ops, iters):
    """{name: [us per call of every round]}: the ops alternate inside every round"""
    ts = {k: [] for k in ops}
    for f in ops.values():
        for _ in range(3): f()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, f in ops.items():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters): f()
            e1.record(); torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / iters * 1e3)
    return ts


hp = pkg.synth.hparams_for(a.model)
n, D, Lh, P = a.batch, hp.hidden_size, hp.num_hidden_layers, hp.patch_size
K, u = 256, 4
say(f"# tools/depth_cost.py --model {a.model} --batch {n} --sizes {' '.join(map(str, a.sizes))} --rounds {a.rounds} --iters {a.iters} --steps {a.steps} parent={'given' if a.parent else 'none'}   ({torch.cuda.get_device_name(0)})")
path = pkg.synth.cached_synthetic(a.model, head_scale=8.0)
model = B.Model(path)
s0 = torch.cuda.current_stream().cuda_stream
st = torch.cuda.Stream(); ss = st.cuda_stream
rng = np.random.default_rng(1)
cf = B.C.c_float

for S in a.sizes:
    g = S // P
    Np, f = g * g, u * g
    kw = {} if S == hp.img_size else {"img_shape": (S, S)}
    ctx = B.Context(model, 0, n, B.BF16, last_layer_all_rows=1, **kw)
    cut = ctx.split(n)
    nl = max(cut)
    steps = a.steps if S <= 256 else max(2, a.steps // 3)
    imgs = torch.randn((n, S, S, 3), device="cuda")
    probs = torch.empty((n, hp.num_classes), device="cuda")
    say(f"## {S} x {S}: grid {g} x {g}, {Np} patches, fine plane {f} x {f}, depth maps {S} x {S}; the forward runs as sub-batches of {cut}; per-launch figures are for {nl} images")
    for m in (1, 4):
        Dc, Kpad, rows = m * D, up(K, 128), nl * Np
        M, Mc = up(rows, 256), up(nl, 256)
        layers = [Lh - 1] if m == 1 else [2, 5, 8, 11]
        wp = (rng.standard_normal((K, Dc)) * 0.05).astype(np.float32); wc = (rng.standard_normal((K, Dc)) * 0.05).astype(np.float32)
        bias = rng.standard_normal(K).astype(np.float32); bins = B.depth_bins(K, 0.001, 10.0, "UD")
        say(f"### K = {K} bins over {m} layer(s) {layers}, class half, raw rows, upsample {u}: Dc = {Dc}, K_pad = {Kpad}")
        # 1 + 2. the stages of one launch
        lg = torch.randn((M, Kpad), device="cuda"); off = torch.randn((nl, Kpad), device="cuda"); d_bins = torch.from_numpy(bins).cuda()
        fine = torch.empty((nl, f, f), device="cuda"); out = torch.empty((nl, S, S), device="cuda")
        alg = rows * Kpad * 4 + nl * f * f * 4
        src = torch.empty(alg // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        alg_r = nl * (f * f + S * S) * 4
        x = torch.randn((rows, D), device="cuda"); y = torch.empty((rows, D), dtype=torch.bfloat16, device="cuda")
        d_a = torch.zeros((M, Dc), dtype=torch.bfloat16, device="cuda"); d_w = torch.zeros((Kpad, Dc), dtype=torch.bfloat16, device="cuda")
        d_ac = torch.zeros((Mc, Dc), dtype=torch.bfloat16, device="cuda")
        d_b = torch.zeros(Kpad, device="cuda"); d_o = torch.empty((M, Kpad), device="cuda"); d_oc = torch.empty((Mc, Kpad), device="cuda")
        ops = {"depth_fine": lambda: L.vitx_op_depth_fine(lg.data_ptr(), Kpad, off.data_ptr(), d_bins.data_ptr(), nl, g, g, K, u, fine.data_ptr(), s0),
               "device-to-device copy": lambda: dst.copy_(src),
               "depth_resize": lambda: L.vitx_op_depth_resize(fine.data_ptr(), nl, f, f, S, S, cf(0.001), cf(10.0), out.data_ptr(), s0),
               "raw operand rows, one layer": lambda: L.vitx_op_depth_rows(B.BF16, x.data_ptr(), D, y.data_ptr(), D, rows, D, s0),
               "patch GEMM (op_gemm)": lambda: L.vitx_op_gemm(B.BF16, 3, d_a.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), d_o.data_ptr(), M, Kpad, Dc, s0),
               "class GEMM (op_gemm)": lambda: L.vitx_op_gemm(B.BF16, 3, d_ac.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), d_oc.data_ptr(), Mc, Kpad, Dc, s0)}
        ts = timed(ops, a.iters)
        res = {}
        for name in ops:
            res[name] = med(ts[name])
            mm, lo, hi = res[name]
            extra = ""
            if name == "depth_fine": extra = f"  {alg / 1e6:.1f} MB algorithmic ({rows * Kpad * 4 / 1e6:.1f} logits + {nl * f * f * 4 / 1e6:.1f} fine): {alg / mm / 1e6:.3f} TB/s"
            if "copy" in name: extra = f"  {alg / 1e6:.1f} MB read + written: {alg / mm / 1e6:.3f} TB/s"
            if name == "depth_resize": extra = f"  {alg_r / 1e6:.1f} MB algorithmic: {alg_r / mm / 1e6:.3f} TB/s"
            say(f"{name:28s}: median {mm:8.1f} us  min {lo:8.1f}  max {hi:8.1f}{extra}")
        say(f"depth_fine / copy = {res['depth_fine'][0] / res['device-to-device copy'][0]:.1f}x   (back to back on one stream, launch gaps included)")
        del lg, off, fine, out, src, dst, x, y, d_a, d_w, d_ac, d_o, d_oc
        # 3. the forward, head on and off alternating
        tf = {"off": [], "on": []}
        for _ in range(a.rounds):
            for mode in ("off", "on"):
                if mode == "on": ctx.depth_set(wp, wc, bias, bins, layers, u, 0.001, 10.0)
                else: ctx.depth_set(None)
                if mode == "on": scratch_on = ctx.depth_scratch_bytes()
                ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(steps): ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
                torch.cuda.synchronize(); tf[mode].append((time.perf_counter() - t0) / steps * 1e3)
        ctx.depth_set(None)
        base = med(tf["off"])[0]
        say(f"operand rows + logit scratch over the {len(cut)} slices: {scratch_on / 1e6:.1f} MB; fine planes {n * f * f * 4 / 1e6:.1f} MB; depth maps {n * S * S * 4 / 1e6:.1f} MB")
        for mode in ("off", "on"):
            mm, lo, hi = med(tf[mode])
            say(f"forward {a.model} {S}^2 b{n} bf16 all rows, head {mode:3s}: median {mm:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({n / mm * 1e3:.0f} img/s)  x{mm / base:.4f}")
    ctx.close()
    del imgs, probs
model.close()

# 5. the forward without a depth head against the parent commit
if a.parent:
    S = hp.img_size
    imgs = torch.randn((n, S, S, 3), device="cuda")
    runs = []
    for name, _ in builds:
        m_ = bind[name].Model(path)
        runs.append(dict(name=name, m=m_, c=bind[name].Context(m_, 0, n, bind[name].BF16), ts=[], probs=torch.empty((n, hp.num_classes), device="cuda")))
    for r in runs:
        for _ in range(3): r["c"].forward_device(imgs.data_ptr(), n, r["probs"].data_ptr(), 0, ss)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for r in runs:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps): r["c"].forward_device(imgs.data_ptr(), n, r["probs"].data_ptr(), 0, ss)
            torch.cuda.synchronize(); r["ts"].append((time.perf_counter() - t0) / a.steps * 1e3)
    say(f"## no depth head, against the parent commit: {a.model} {S}^2 b{n} bf16 (the context's default tail), the builds alternating")
    for r in runs:
        mm, lo, hi = med(r["ts"])
        same = "" if r is runs[0] else ("  probabilities bit-identical to " + runs[0]["name"] if torch.equal(r["probs"], runs[0]["probs"]) else "  PROBABILITIES DIFFER from " + runs[0]["name"])
        say(f"forward {r['name']:9s}: median {mm:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({n / mm * 1e3:.0f} img/s){same}")
    pa, pb, nw = (med(r["ts"]) for r in runs)
    lo, hi = min(pa[1], pb[1]), max(pa[2], pb[2])
    say(f"new median {nw[0]:.3f} ms; the parent's own range in this run (both copies, min to max) {lo:.3f} .. {hi:.3f} ms: {'INSIDE' if nw[0] <= hi else 'ABOVE'} the range")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fo:
    fo.write("\n".join(lines) + "\n")
