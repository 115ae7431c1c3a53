"""Cost of nearest neighbours in a gallery (include/vitx.h "nearest neighbours in a gallery"), interleaved in ONE process (separate runs are not comparable):
    python tools/nn_cost.py [--rounds R] [--iters I] [--steps S] [--batch B] [--rows 10000 1000000] [--k 20] [--out profiles/nn_cost.txt]
ViT-B/16 224^2, batch B, bf16, source VITX_NN_EMBED (E = 768), one gallery of G rows per run:
  1. the whole forward with the gallery on and off, alternating, R rounds of S steps: median, min and max of each, and the slowdown;
  2. per chunk of Gc = 32768 rows at n = B: the chunk GEMM (vitx_op_gemm at its shape), the selection launch in steady state (a state that has seen a
     whole gallery: few scores beat the threshold) and as the first chunk (every list fills up), beside a device-to-device copy of the same score bytes;
  3. vitx_op_nn over the largest gallery at three chunk sizes: the sweep behind the shipped Gc.
No gate rests on these figures."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batch", type=int, default=256); ap.add_argument("--model", default="vit_base_patch16_224"); ap.add_argument("--k", type=int, default=20)
ap.add_argument("--rows", type=int, nargs="+", default=[10000, 1000000]); ap.add_argument("--chunks", type=int, nargs="+", default=[8192, 32768, 131072])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_cost.txt"))
a = ap.parse_args()
L = B.lib()
lines = []
GC = 32768


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
n, k, E = a.batch, a.k, hp.hidden_size
say(f"# tools/nn_cost.py --model {a.model} --batch {n} --k {k} --rows {' '.join(map(str, a.rows))} --rounds {a.rounds} --iters {a.iters} --steps {a.steps}   ({torch.cuda.get_device_name(0)})")
model = B.Model(pkg.synth.cached_synthetic(a.model, head_scale=8.0))
ctx = B.Context(model, 0, n, B.BF16)
imgs = torch.randn((n, hp.img_size, hp.img_size, 3), device="cuda")
probs = torch.empty((n, hp.num_classes), device="cuda")
st = torch.cuda.Stream(); ss = st.cuda_stream
s0 = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(1)
block = rng.standard_normal((65536, E)); block = (block / np.linalg.norm(block, axis=1, keepdims=True)).astype(np.float32)
npad = up(n, 256)

for G in a.rows:
    gal = np.ascontiguousarray(np.tile(block, (up(G, 65536) // 65536, 1))[:G])       # unit rows; beyond 65536 rows the block repeats (the index breaks the ties)
    say(f"## G = {G} rows of width {E}: the gallery is {up(G, 128) * E * 2 / 1e6:.1f} MB in bf16, {-(-G // GC)} chunks of {GC} rows")
    # 1. the forward, gallery on and off alternating
    tf = {"off": [], "on": []}
    for _ in range(a.rounds):
        for mode in ("off", "on"):
            ctx.nn_set(gal if mode == "on" else None, k, B.NN_EMBED)
            scratch = ctx.nn_scratch_bytes() or 0
            if mode == "on": scratch_on = scratch
            ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps): ctx.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)
            torch.cuda.synchronize(); tf[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
    ctx.nn_set(None)
    base = med(tf["off"])[0]
    say(f"score scratch + running state over the {len(ctx.split(n))} slices: {scratch_on / 1e6:.1f} MB (the same at every G)")
    for mode in ("off", "on"):
        m, lo, hi = med(tf[mode])
        say(f"forward {a.model} b{n} bf16 gallery {mode:3s}: median {m:.3f} ms  min {lo:.3f}  max {hi:.3f}  ({n / m * 1e3:.0f} img/s)  x{m / base:.4f}")
    del gal

# 2. one chunk at n = B
scores = torch.from_numpy((rng.standard_normal((n, 65536)) * 0.036).astype(np.float32)).cuda()       # cosines of random unit rows of width 768: sigma = 768^-1/2
chunk = scores[:, :GC].contiguous(); other = torch.empty_like(chunk)
state = torch.zeros(B.op_nn_state_bytes(n, k) // 8, dtype=torch.int64, device="cuda")
for c0 in range(0, 65536, GC):                                                                        # a state that has seen 65536 scores per query
    B.op_nn_select(scores.data_ptr() + 4 * c0, 65536, n, GC, c0, state.data_ptr(), k, c0 == 0, s0)
fresh = torch.zeros_like(state)
d_a = torch.zeros((npad, E), device="cuda", dtype=torch.bfloat16); gw = torch.zeros((GC, E), device="cuda", dtype=torch.bfloat16)
gb = torch.zeros(GC, device="cuda"); go = torch.zeros((npad, GC), device="cuda")
pairs = torch.empty((n, k, 2), device="cuda")
ops = {"chunk GEMM (op_gemm)": lambda: L.vitx_op_gemm(B.BF16, 3, d_a.data_ptr(), gw.data_ptr(), gb.data_ptr(), go.data_ptr(), npad, GC, E, s0),
       "selection, steady state": lambda: L.vitx_op_nn_select(chunk.data_ptr(), GC, n, GC, 65536, state.data_ptr(), k, 0, s0),
       "selection, first chunk": lambda: L.vitx_op_nn_select(chunk.data_ptr(), GC, n, GC, 0, fresh.data_ptr(), k, 1, s0),
       "device-to-device copy": lambda: other.copy_(chunk),
       "final merge (op_nn_finish)": lambda: L.vitx_op_nn_finish(state.data_ptr(), n, k, None, 0, 0.0, pairs.data_ptr(), None, s0)}
ts = timed(ops, a.iters)
mb = n * GC * 4 / 1e6
say(f"## one chunk: n = {n} queries x Gc = {GC} gallery rows, E = {E}, k = {k}; the scores of a chunk are {mb:.1f} MB")
for name in ops:
    m, lo, hi = med(ts[name])
    extra = f"  {mb / m:.2f} TB/s of scores read" if name.startswith("selection") else (f"  {2 * mb / m:.2f} TB/s read + written" if "copy" in name else "")
    say(f"{name:28s}: median {m:7.1f} us  min {lo:7.1f}  max {hi:7.1f}{extra}  (back to back on one stream, launch gaps included)")

# 3. the chunk-size sweep: vitx_op_nn over the largest gallery
G = max(a.rows)
d_gal = torch.from_numpy(block).cuda().to(torch.bfloat16).repeat(up(G, 65536) // 65536 + 1, 1)[:up(G, 128)].contiguous()
z = torch.randn((n, E), device="cuda")
st_op = torch.zeros(B.op_nn_state_bytes(n, k) // 8, dtype=torch.int64, device="cuda")
ops = {}
accs = {}
for c in a.chunks:
    accs[c] = torch.zeros((npad + 1, c), device="cuda")
    ops[f"op_nn G={G} chunk={c}"] = (lambda c=c: B.op_nn(B.BF16, z.data_ptr(), E, False, n, d_gal.data_ptr(), G, E, k, c, d_a.data_ptr(), accs[c].data_ptr(), st_op.data_ptr(), pairs.data_ptr(), s0))
ts = timed(ops, max(1, a.iters // 10))
say(f"## the chunk size: vitx_op_nn at n = {n}, G = {G}, E = {E}, k = {k} (the operand rows, every chunk's GEMM and selection, the final merge)")
for name in ops:
    m, lo, hi = med(ts[name])
    c = int(name.rsplit("=", 1)[1])
    say(f"{name:32s}: median {m / 1e3:8.3f} ms  min {lo / 1e3:8.3f}  max {hi / 1e3:8.3f}  ({-(-G // c)} chunks, score scratch {npad * c * 4 / 1e6:.1f} MB per slice)")
ctx.close(); model.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
