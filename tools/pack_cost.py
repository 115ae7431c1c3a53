"""Cost of packed batches (include/vitx.h "packed batches"), interleaved rounds in ONE process on one GPU (separate runs are not comparable):
    python tools/pack_cost.py [--rounds R] [--steps S] [--images N] [--out profiles/pack_cost.txt]
  1. the attention kernel alone, bf16 and F16, D 768, H 12: two uniform packs of ViT-B shape (256 x 197 and 64 x 577 tokens) through
     vitx_op_attention_packed_tables, beside vitx_op_attention_generic (the same arithmetic) and vitx_op_attention (the dispatcher's tuned choice) in the
     same rounds; and a mixed pack of N shapes drawn from vitx_rect_shape at short side 224, patch 16, over a seeded list of source sizes, for which
     there is no single-launch yardstick: us per launch and the rate per unit of sum N_i^2 relative to the 256 x 197 pack.
  2. the forward of that mixed pack, ViT-B/16, bf16, three ways: one packed forward; one rectangular context per distinct shape, bucket after bucket;
     every image stretched to the largest shape's context.  Milliseconds, scratch bytes, launches per forward.
  3. the forward of a uniform pack, N x 224^2: a packed context beside Context(last_layer_all_rows=1, no_ln_fusion=1) and the default context.
Nothing here is a gate.  Not measured: head dims other than 64, `glu` and RoPE files, HBM-cold tables (every timed call finds its tables cached)."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--steps", type=int, default=10); ap.add_argument("--images", type=int, default=256)
ap.add_argument("--model", default="vit_base_patch16_224"); ap.add_argument("--skip-forward", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_cost.txt"))
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


def rounds(runs, iters):
    """Interleaved: every run `iters` times between two events, run after run, a.rounds times; r["ts"] in ms per call."""
    torch.cuda.synchronize()          # the operands were made on torch's own stream
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


say(f"# tools/pack_cost.py --model {a.model} --images {a.images} --rounds {a.rounds} --steps {a.steps}   ({torch.cuda.get_device_name(0)})")
stream = torch.cuda.Stream(); ss = stream.cuda_stream
D, H, P = 768, 12, 16

# the mixed pack: aspect-preserving shapes of seeded source sizes (photographs between 2:1 and 1:2)
rng = np.random.default_rng(7)
sources = [(int(rng.integers(320, 1281)), int(rng.integers(320, 1281))) for _ in range(a.images)]
shapes = [B.rect_shape(nx, ny, P, 224, 448)[::-1] for nx, ny in sources]            # (h, w)
tokens = [1 + (h // P) * (w // P) for h, w in shapes]
distinct = sorted(set(shapes))
say(f"mixed pack: {a.images} images, short side 224, patch {P}: {len(distinct)} distinct shapes, {min(tokens)} .. {max(tokens)} tokens, sum N = {sum(tokens)}, sum N^2 = {sum(t * t for t in tokens)}")


def tables(counts):
    row0 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    qb0 = np.concatenate([[0], np.cumsum([(c + 63) // 64 for c in counts])]).astype(np.int32)
    return torch.from_numpy(row0).cuda(), torch.from_numpy(qb0).cuda(), int(row0[-1]), int(qb0[-1])


# ---- 1. the attention kernel alone
for dtype, tname, tdt in ((B.BF16, "bf16", torch.bfloat16), (B.F16, "F16", torch.float16)):
    per_n2 = {}
    for label, counts, uniform in (("256 x 197", [197] * 256, True), ("64 x 577", [577] * 64, True), (f"mixed {a.images}", tokens, False)):
        d_row0, d_qb0, rows, qblocks = tables(counts)
        qkv = (torch.randn((rows, 3 * D), device="cuda") * 0.5).to(tdt)
        outs = [torch.zeros((rows, D), dtype=tdt, device="cuda") for _ in range(3)]
        n = len(counts)
        runs = [dict(name="packed", ts=[], f=lambda: B.check(B.lib().vitx_op_attention_packed_tables(dtype, qkv.data_ptr(), outs[0].data_ptr(), d_row0.data_ptr(), d_qb0.data_ptr(), n, qblocks, D, H, ss)))]
        if uniform:
            runs.append(dict(name="generic", ts=[], f=lambda: B.check(B.lib().vitx_op_attention_generic(dtype, qkv.data_ptr(), outs[1].data_ptr(), n, counts[0], D, H, ss))))
            runs.append(dict(name="dispatcher", ts=[], f=lambda: B.check(B.lib().vitx_op_attention(dtype, qkv.data_ptr(), outs[2].data_ptr(), n, counts[0], D, H, ss))))
        rounds(runs, 20)
        n2 = sum(c * c for c in counts)
        per_n2[label] = med(runs[0]["ts"])[0] / n2
        for r in runs:
            same = ""
            if r["name"] == "generic":
                differ = int((outs[0].view(torch.int16) != outs[1].view(torch.int16)).sum())
                same = "   bits equal to packed" if differ == 0 else f"   {differ} ELEMENTS DIFFER from packed ({int(torch.isnan(outs[0].float()).sum())} / {int(torch.isnan(outs[1].float()).sum())} NaN)"
            say(f"attention {tname} {label:10s} {r['name']:10s}: {fmt(r['ts'], 'us', 1e3)} per launch{same}")
        if not uniform:
            say(f"attention {tname} {label}: time per unit of sum N_i^2 = {per_n2[label] / per_n2['256 x 197']:.3f} x that of the 256 x 197 pack, {per_n2[label] / per_n2['64 x 577']:.3f} x that of the 64 x 577 pack")
        del qkv, outs

def write_record():
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if a.skip_forward:
    write_record()
    sys.exit(0)

# ---- 2. the forward of the mixed pack, three ways
hp = pkg.synth.hparams_for(a.model)
path = pkg.synth.cached_synthetic(a.model, head_scale=8.0)
model = B.Model(path)
C = hp.num_classes
order = sorted(range(a.images), key=lambda i: shapes[i])                          # sorted by shape: one patch-embedding launch per distinct shape
sh_sorted = [shapes[i] for i in order]
pixels = torch.randn((sum(h * w * 3 for h, w in sh_sorted),), device="cuda")
probs = torch.empty((a.images, C), device="cuda")


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


anchor = B.Context(model, 0, 1, B.BF16)                                           # holds the image contexts' weight set: the deltas below are scratch
pack = B.PackContext(model, 0, max_tokens=sum(tokens), max_images=a.images, dtype=B.BF16)
sh_arr = np.asarray(sh_sorted, np.int32)
pack.forward_device(pixels.data_ptr(), sh_arr, probs.data_ptr(), 0, ss); torch.cuda.synchronize()
pack_launches, pack_pe = pack.launches
before = free_bytes()
buckets, at = [], 0
for shp in distinct:
    k = sh_sorted.count(shp)
    c = B.Context(model, 0, k, B.BF16, img_shape=shp)
    buckets.append((c, k, at)); at += k * shp[0] * shp[1] * 3
bucket_bytes = before - free_bytes()
big = max(distinct, key=lambda s: s[0] * s[1])
before = free_bytes()
stretched = B.Context(model, 0, a.images, B.BF16, img_shape=big)
stretched_bytes = before - free_bytes()
big_imgs = torch.randn((a.images, big[0], big[1], 3), device="cuda")


def run_buckets():
    img0 = 0
    for c, k, off in buckets:
        c.forward_device(pixels.data_ptr() + off * 4, k, probs.data_ptr() + img0 * C * 4, 0, ss); img0 += k


def launches_of(ctxs_and_calls):
    total = 0
    for c, call in ctxs_and_calls:
        c.profile_enable(True); call(); torch.cuda.synchronize()
        total += sum(e["launches"] for e in c.profile_read()); c.profile_enable(False)
    return total


runs = [dict(name="packed", ts=[], f=lambda: pack.forward_device(pixels.data_ptr(), sh_arr, probs.data_ptr(), 0, ss)),
        dict(name="buckets", ts=[], f=run_buckets),
        dict(name="stretched", ts=[], f=lambda: stretched.forward_device(big_imgs.data_ptr(), a.images, probs.data_ptr(), 0, ss))]
rounds(runs, a.steps)
bl = launches_of([(c, (lambda c=c, k=k, off=off: c.forward_device(pixels.data_ptr() + off * 4, k, probs.data_ptr(), 0, ss))) for c, k, off in buckets])
sl = launches_of([(stretched, lambda: stretched.forward_device(big_imgs.data_ptr(), a.images, probs.data_ptr(), 0, ss))])
say(f"forward {a.model} bf16, {a.images} mixed-shape images ({sum(tokens)} tokens):")
say(f"  one packed forward (sorted by shape)         : {fmt(runs[0]['ts'])}   scratch {pack.scratch_bytes / 2 ** 20:.0f} MiB   {pack_launches} launches ({pack_pe} patch embeddings)")
say(f"  {len(distinct)} rectangular contexts, bucket after bucket : {fmt(runs[1]['ts'])}   scratch {bucket_bytes / 2 ** 20:.0f} MiB   {bl} launches")
say(f"  every image stretched to {big[0]} x {big[1]} ({a.images * (1 + (big[0] // P) * (big[1] // P))} tokens): {fmt(runs[2]['ts'])}   scratch {stretched_bytes / 2 ** 20:.0f} MiB   {sl} launches")
unsorted_arr = np.asarray(shapes, np.int32)
pack.forward_device(pixels.data_ptr(), unsorted_arr, probs.data_ptr(), 0, ss); torch.cuda.synchronize()      # (pixel sizes only: the order of the floats does not matter to the clock)
say(f"  the same pack unsorted: {pack.launches[0]} launches ({pack.launches[1]} patch embeddings)")
for c, _, _ in buckets:
    c.close()
stretched.close(); pack.close(); del big_imgs, pixels

# ---- 3. the forward of a uniform pack
S = hp.img_size
n = a.images
imgs = torch.randn((n, S, S, 3), device="cuda")
N = 1 + (S // P) ** 2
pack = B.PackContext(model, 0, max_tokens=n * N, max_images=n, dtype=B.BF16)
plain = B.Context(model, 0, n, B.BF16, last_layer_all_rows=1, no_ln_fusion=1)
default = B.Context(model, 0, n, B.BF16)
uni = np.asarray([(S, S)] * n, np.int32)
runs = [dict(name="packed context", ts=[], f=lambda: pack.forward_device(imgs.data_ptr(), uni, probs.data_ptr(), 0, ss)),
        dict(name="Context(last_layer_all_rows=1, no_ln_fusion=1)", ts=[], f=lambda: plain.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss)),
        dict(name="Context() default", ts=[], f=lambda: default.forward_device(imgs.data_ptr(), n, probs.data_ptr(), 0, ss))]
rounds(runs, a.steps)
say(f"forward {a.model} bf16, uniform pack {n} x {S}^2 ({n * N} tokens):")
for r in runs:
    say(f"  {r['name']:48s}: {fmt(r['ts'])}   ({n / med(r['ts'])[0] * 1e3:.0f} img/s)")
pack.close(); plain.close(); default.close(); anchor.close(); model.close()
write_record()
