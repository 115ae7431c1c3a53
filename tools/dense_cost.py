"""Cost of the dense head (include/vitx.h "dense prediction"), interleaved in ONE process (separate runs are not comparable):
    python tools/dense_cost.py [--rounds R] [--iters I] [--steps S] [--batch B] [--out profiles/dense_cost.txt]
ViT-B/16, batch B, bf16, label maps at the image's own size, for heads of K = 150 (ADE20K) and K = 21 (VOC) classes over one layer and over four:
  1. the label kernel per launch (one sub-batch: the larger of the forward's two), beside a device-to-device copy that moves the same algorithmic
     bytes -- the logits read once and the labels written once -- so a copy of half their sum, read and written;
  2. the three stages per launch: the operand rows (the stand-alone LayerNorm of the sub-batch's patch rows, once per selected layer; timed through
     vitx_op_layernorm, which writes the same rows compactly), the GEMM (vitx_op_gemm at its shape), the label kernel;
  3. the whole forward with the head set against the SAME shape of context with last_layer_all_rows = 1 and no head (the head makes the last layer
     compute every row: that part is not the head's own cost), alternating, R rounds of S steps: median, min and max of each;
  4. the same at 448 x 448 (the context --img-fit 448 makes for a square picture; 784 patches).
No gate rests on these figures."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batch", type=int, default=256); ap.add_argument("--model", default="vit_base_patch16_224")
ap.add_argument("--sizes", type=int, nargs="+", default=[224, 448])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_cost.txt"))
a = ap.parse_args()
L = B.lib()
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def up(v, m):
    return (v + m - 1) // m * m


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
say(f"# tools/dense_cost.py --model {a.model} --batch {n} --sizes {' '.join(map(str, a.sizes))} --rounds {a.rounds} --iters {a.iters} --steps {a.steps}   ({torch.cuda.get_device_name(0)})")
model = B.Model(pkg.synth.cached_synthetic(a.model, head_scale=8.0))
s0 = torch.cuda.current_stream().cuda_stream
st = torch.cuda.Stream(); ss = st.cuda_stream
rng = np.random.default_rng(1)

for S in a.sizes:
    g = S // P
    Np = g * g
    heads = [(150, 1), (150, 4), (21, 1)] if S == a.sizes[0] else [(150, 1)]
    kw = {} if S == hp.img_size else {"img_shape": (S, S)}
    ctx = B.Context(model, 0, n, B.BF16, last_layer_all_rows=1, **kw)
    cut = ctx.split(n)
    nl = max(cut)
    imgs = torch.randn((n, S, S, 3), device="cuda")
    probs = torch.empty((n, hp.num_classes), device="cuda")
    say(f"## {S} x {S}: grid {g} x {g}, {Np} patches, label maps {S} x {S}; the forward runs as sub-batches of {cut}; per-launch figures are for {nl} images")
    for K, m in heads:
        Dc, Kpad, rows = m * D, up(K, 128), nl * Np
        M = up(rows, 256)
        layers = list(range(Lh - m, Lh))
        W = (rng.standard_normal((K, Dc)) * 0.05).astype(np.float32); bias = rng.standard_normal(K).astype(np.float32)
        say(f"### K = {K} classes over {m} layer(s) {layers}: Dc = {Dc}, K_pad = {Kpad}")
        # 1 + 2. the stages of one launch
        lg = torch.randn((M, Kpad), device="cuda")
        lab = torch.empty((nl, S, S), dtype=torch.uint8, device="cuda")
        alg = rows * Kpad * 4 + nl * S * S
        src = torch.empty(alg // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        x = torch.randn((rows, D), device="cuda"); lw = torch.ones(D, device="cuda"); lb = torch.zeros(D, device="cuda")
        y = torch.empty((rows, D), dtype=torch.bfloat16, device="cuda")
        d_a = torch.zeros((M, Dc), dtype=torch.bfloat16, device="cuda"); d_w = torch.zeros((Kpad, Dc), dtype=torch.bfloat16, device="cuda")
        d_b = torch.zeros(Kpad, device="cuda"); d_o = torch.empty((M, Kpad), device="cuda")
        ops = {"label kernel": lambda: L.vitx_op_dense_labels(lg.data_ptr(), Kpad, nl, g, g, K, S, S, lab.data_ptr(), None, s0),
               "device-to-device copy": lambda: dst.copy_(src),
               "operand rows, one layer": lambda: L.vitx_op_layernorm(B.BF16, x.data_ptr(), lw.data_ptr(), lb.data_ptr(), y.data_ptr(), rows, D, 1e-6, s0),
               "GEMM (op_gemm)": lambda: L.vitx_op_gemm(B.BF16, 3, d_a.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), d_o.data_ptr(), M, Kpad, Dc, s0)}
        ts = timed(ops, a.iters)
        res = {}
        for name in ops:
            res[name] = med(ts[name])
            mm, lo, hi = res[name]
            extra = ""
            if name == "label kernel": extra = f"  {alg / 1e6:.1f} MB algorithmic ({rows * Kpad * 4 / 1e6:.1f} logits + {nl * S * S / 1e6:.1f} labels): {alg / mm / 1e6:.3f} TB/s"
            if "copy" in name: extra = f"  {alg / 1e6:.1f} MB read + written: {alg / mm / 1e6:.3f} TB/s"
            say(f"{name:26s}: median {mm:8.1f} us  min {lo:8.1f}  max {hi:8.1f}{extra}")
        say(f"label kernel / copy = {res['label kernel'][0] / res['device-to-device copy'][0]:.1f}x   (back to back on one stream, launch gaps included)")
        del lg, lab, src, dst, x, y, d_a, d_w, d_o
        # 3. the forward, head on and off alternating
        tf = {"off": [], "on": []}
        for _ in range(a.rounds):
            for mode in ("off", "on"):
                if mode == "on": ctx.dense_set(W, bias, layers)
                else: ctx.dense_set(None)
                scratch = ctx.dense_scratch_bytes()
                if mode == "on": scratch_on = scratch
                ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(a.steps): ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
                torch.cuda.synchronize(); tf[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
        ctx.dense_set(None)
        base = med(tf["off"])[0]
        say(f"operand rows + logit scratch over the {len(cut)} slices: {scratch_on / 1e6:.1f} MB; labels {n * S * S / 1e6:.1f} MB")
        for mode in ("off", "on"):
            mm, lo, hi = med(tf[mode])
            say(f"forward {a.model} {S}^2 b{n} bf16 all rows, head {mode:3s}: median {mm:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({n / mm * 1e3:.0f} img/s)  x{mm / base:.4f}")
    ctx.close()
    del imgs, probs
model.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
