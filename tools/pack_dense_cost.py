"""Cost of the dense head on packed batches (include/vitx.h "packed batches", the dense head), interleaved rounds in ONE process on one GPU (separate
runs are not comparable):
    python tools/pack_dense_cost.py [--rounds R] [--iters I] [--steps S] [--images N] [--out profiles/pack_dense_cost.txt]
  (a) the label launch alone: a uniform pack of ViT-B/16 shape, 153 images of 224^2 (grid 14 x 14), K = 150 and K = 21, through
      vitx_op_dense_labels_packed_tables beside vitx_op_dense_labels (the fixed-shape kernel, the yardstick: 371.6 / 74.3 us in profiles/dense_cost.txt) on
      the SAME logits in the same rounds; their outputs are compared bit for bit.  The difference is the work-list search and the table row.
  (b) the forward of the mixed pack of tools/pack_cost.py (the same seeded shapes), ViT-B/16, bf16: one packed forward without and with a K = 150 head
      (label maps at the images' own shapes), beside one rectangular context per distinct shape with the same head, bucket after bucket.
Nothing here is a gate.  Not measured: score maps, kept logits, heads over four layers, output shapes other than the images' own (vitx_pack_dense_out),
packs with one very large output beside many small ones, HBM-cold tables."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--images", type=int, default=256); ap.add_argument("--model", default="vit_base_patch16_224"); ap.add_argument("--skip-forward", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_dense_cost.txt"))
a = ap.parse_args()
lines = []
NOT_MEASURED = ("## not measured: score maps, kept logits, heads over four layers, output shapes other than the images' own (vitx_pack_dense_out), packs with one very "
                "large output beside many small ones, HBM-cold tables")


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(ts, unit="ms", scale=1.0):
    m, lo, hi = med(ts)
    return f"median {m * scale:9.3f} {unit}  min {lo * scale:9.3f}  max {hi * scale:9.3f}"


def rounds(runs, iters):
    """Interleaved: every run `iters` times between two events, run after run, a.rounds times; r["ts"] in ms per call."""
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


def write_record():
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


say(f"# tools/pack_dense_cost.py --model {a.model} --images {a.images} --rounds {a.rounds} --iters {a.iters} --steps {a.steps}   ({torch.cuda.get_device_name(0)})")
stream = torch.cuda.Stream(); ss = stream.cuda_stream
P = 16

# ---- (a) the label launch alone
n, gh, gw, oh, ow = 153, 14, 14, 224, 224
say(f"## (a) label launch alone: uniform pack, {n} images, grid {gh} x {gw} -> {oh} x {ow}; {a.rounds} interleaved rounds of {a.iters} launches back to back on one stream")
for K in (150, 21):
    ld = (K + 127) // 128 * 128
    lg = torch.randn((n * gh * gw, ld), device="cuda")
    lab = [torch.zeros((n * oh * ow,), dtype=torch.uint8, device="cuda") for _ in range(2)]
    tab, tiles, cells = B.dense_pack_tables([(gh, gw)] * n, [(oh, ow)] * n, np.arange(n) * gh * gw)
    d_tab = torch.from_numpy(tab).cuda()
    runs = [dict(name="fixed-shape kernel", ts=[], f=lambda: B.op_dense_labels(lg.data_ptr(), ld, n, gh, gw, K, oh, ow, lab[0].data_ptr(), 0, ss)),
            dict(name="packed kernel", ts=[], f=lambda: B.op_dense_labels_packed_tables(lg.data_ptr(), ld, d_tab.data_ptr(), n, tiles, cells, K, lab[1].data_ptr(), 0, ss))]
    rounds(runs, a.iters)
    differ = int((lab[0] != lab[1]).sum())
    for r in runs:
        say(f"K = {K:3d}  {r['name']:18s}: {fmt(r['ts'], 'us', 1e3)}")
    f_, p_ = med(runs[0]["ts"]), med(runs[1]["ts"])
    say(f"K = {K:3d}  packed / fixed = {p_[0] / f_[0]:.4f} (medians; the fixed-shape kernel's own spread: {(f_[2] - f_[1]) / f_[0] * 100:.1f} %, the packed kernel's: {(p_[2] - p_[1]) / p_[0] * 100:.1f} %)   "
        f"{tiles} workgroups each   labels {'equal bit for bit' if differ == 0 else f'{differ} BYTES DIFFER'}")
    del lg, lab

if a.skip_forward:
    write_record()
    sys.exit(0)

# ---- (b) the forward of the mixed pack with and without a head
rng = np.random.default_rng(7)
sources = [(int(rng.integers(320, 1281)), int(rng.integers(320, 1281))) for _ in range(a.images)]
shapes = sorted(B.rect_shape(nx, ny, P, 224, 448)[::-1] for nx, ny in sources)        # (h, w), sorted: one patch-embedding launch per distinct shape
tokens = [1 + (h // P) * (w // P) for h, w in shapes]
distinct = sorted(set(shapes))
pixels_out = sum(h * w for h, w in shapes)
hp = pkg.synth.hparams_for(a.model)
model = B.Model(pkg.synth.cached_synthetic(a.model, head_scale=8.0))
C, D, K = hp.num_classes, hp.hidden_size, 150
hw = np.random.default_rng(1)
W, b = (hw.standard_normal((K, D)) * 0.05).astype(np.float32), hw.standard_normal(K).astype(np.float32)
pixels = torch.randn((sum(h * w * 3 for h, w in shapes),), device="cuda")
probs = torch.empty((a.images, C), device="cuda")
sh_arr = np.asarray(shapes, np.int32)
say(f"## (b) forward {a.model} bf16, {a.images} mixed-shape images: {len(distinct)} distinct shapes, {sum(tokens)} tokens, {pixels_out / 1e6:.2f} M output pixels; head K = {K} over the last layer")


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


anchor = B.Context(model, 0, 1, B.BF16)                                           # holds the image contexts' weight set: the deltas below are scratch
plain = B.PackContext(model, 0, max_tokens=sum(tokens), max_images=a.images, dtype=B.BF16)
headed = B.PackContext(model, 0, max_tokens=sum(tokens), max_images=a.images, dtype=B.BF16)
headed.dense_set(W, b, None, max_pixels=pixels_out)
for c in (plain, headed):
    c.forward_device(pixels.data_ptr(), sh_arr, probs.data_ptr(), 0, ss)
torch.cuda.synchronize()
before = free_bytes()
buckets, at = [], 0
for shp in distinct:
    k = shapes.count(shp)
    c = B.Context(model, 0, k, B.BF16, img_shape=shp)
    c.dense_set(W, b, None)
    buckets.append((c, k, at)); at += k * shp[0] * shp[1] * 3
bucket_bytes = before - free_bytes()


def run_buckets():
    img0 = 0
    for c, k, off in buckets:
        c.forward_device(pixels.data_ptr() + off * 4, k, probs.data_ptr() + img0 * C * 4, 0, ss); img0 += k


runs = [dict(name="packed, no head", ts=[], f=lambda: plain.forward_device(pixels.data_ptr(), sh_arr, probs.data_ptr(), 0, ss)),
        dict(name="packed, head", ts=[], f=lambda: headed.forward_device(pixels.data_ptr(), sh_arr, probs.data_ptr(), 0, ss)),
        dict(name="buckets, head", ts=[], f=run_buckets)]
rounds(runs, a.steps)
base = med(runs[0]["ts"])[0]
say(f"  one packed forward, no head                     : {fmt(runs[0]['ts'])}   x1.0000   scratch {plain.scratch_bytes / 2 ** 20:.0f} MiB   {plain.launches[0]} launches")
say(f"  one packed forward, head                        : {fmt(runs[1]['ts'])}   x{med(runs[1]['ts'])[0] / base:.4f}   scratch {headed.scratch_bytes / 2 ** 20:.0f} MiB   {headed.launches[0]} launches")
say(f"  {len(distinct):3d} rectangular contexts with the head, in turn : {fmt(runs[2]['ts'])}   x{med(runs[2]['ts'])[0] / base:.4f}   scratch {bucket_bytes / 2 ** 20:.0f} MiB")
for c, _, _ in buckets:
    c.close()
plain.close(); headed.close(); anchor.close(); model.close()
say(NOT_MEASURED)
write_record()
