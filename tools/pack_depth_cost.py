"""Cost of the depth head on packed batches (include/vitx.h "packed batches", the depth head), interleaved rounds in ONE process on one GPU (separate
runs are not comparable):
    python tools/pack_depth_cost.py [--rounds R] [--iters I] [--steps S] [--images N] [--parent-lib libvitx_parent.so] [--out profiles/pack_depth_cost.txt]
  (a) the two launches alone: a uniform pack of ViT-B/16 shape, 153 images of 224^2 (grid 14 x 14), K = 256 bins, u = 4 (fine 56 x 56, map 224 x 224),
      through vitx_op_depth_fine_packed_tables / vitx_op_depth_resize_packed_tables beside vitx_op_depth_fine / vitx_op_depth_resize (the fixed-shape
      kernels, the yardstick) on the SAME logits in the same rounds; their outputs are compared bit for bit.  The difference is the work-list search
      and the table row.
  (b) with --parent-lib (the library of the parent commit, built apart and loaded beside this tree's): the fixed-shape kernels of both libraries on the
      same logits in the same rounds -- their bodies moved into csrc/depth_tile.h -- and their outputs compared bit for bit.
  (c) the forward of the mixed pack of tools/pack_cost.py (the same seeded shapes), ViT-B/16, bf16: one packed forward without and with a K = 256,
      u = 4 head with a class half (maps at the images' own shapes), with --parent-lib the parent library's packed forward without a head in the
      same rounds, and a second head-less context of this tree made after the parent's (what two contexts of ONE library differ by).
Nothing here is a gate: every ratio stands beside the round-to-round spread ((max - min) / median) of its yardstick.  Not measured: kept logits and
fine planes read back, heads over four layers, VITX_DEPTH_NORM, u = 1 and 2, output shapes other than the images' own (vitx_pack_depth_out), packs
with one very large output beside many small ones, one rectangular context per shape with the same head, HBM-cold tables."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--images", type=int, default=256); ap.add_argument("--model", default="vit_base_patch16_224"); ap.add_argument("--skip-forward", action="store_true")
ap.add_argument("--parent-lib", default=None, help="libvitx.so of the parent commit: sections (b) and the parent's forward in (c)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_depth_cost.txt"))
a = ap.parse_args()
lines = []
NOT_MEASURED = ("## not measured: kept logits and fine planes read back, heads over four layers, VITX_DEPTH_NORM, u = 1 and 2, output shapes other than the images' own "
                "(vitx_pack_depth_out), packs with one very large output beside many small ones, one rectangular context per shape with the same head, HBM-cold tables")


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def spread(ts):
    m, lo, hi = med(ts)
    return (hi - lo) / m * 100


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


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: status {rc}")


parent = None
if a.parent_lib:
    parent = C.CDLL(os.path.abspath(a.parent_lib))
    vp, ip, cf = C.c_void_p, C.c_int, C.c_float
    parent.vitx_op_depth_fine.argtypes = [vp, C.c_long, vp, vp, ip, ip, ip, ip, ip, vp, vp]
    parent.vitx_op_depth_resize.argtypes = [vp, ip, ip, ip, ip, ip, cf, cf, vp, vp]
    parent.vitx_model_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    parent.vitx_pack_create.argtypes = [vp, ip, ip, ip, ip, vp, C.POINTER(vp)]
    parent.vitx_pack_forward_device.argtypes = [vp, vp, C.POINTER(C.c_int32), ip, vp, vp, vp]
    parent.vitx_pack_free.argtypes = [vp]; parent.vitx_model_free.argtypes = [vp]

say(f"# tools/pack_depth_cost.py --model {a.model} --images {a.images} --rounds {a.rounds} --iters {a.iters} --steps {a.steps}"
    f"{' --parent-lib <the parent commit>' if parent else ''}   ({torch.cuda.get_device_name(0)})")
stream = torch.cuda.Stream(); ss = stream.cuda_stream
P = 16

# ---- (a), (b) the two launches alone
n, gh, gw, u, K = 153, 14, 14, 4, 256
fh, fw, oh, ow = u * gh, u * gw, 224, 224
lo, hi = 0.001, 10.0
ld = (K + 127) // 128 * 128
say(f"## (a) fine and resize launches alone: uniform pack, {n} images, grid {gh} x {gw} -> fine {fh} x {fw} -> {oh} x {ow}, K = {K}, offsets per image; {a.rounds} interleaved "
    f"rounds of {a.iters} launches back to back on one stream")
lg = torch.randn((n * gh * gw, ld), device="cuda")
off = torch.randn((n, ld), device="cuda") * 0.25
bins = torch.linspace(0.5, 10.0, K, device="cuda")
fine = [torch.zeros((n * fh * fw,), device="cuda") for _ in range(3)]
out = [torch.zeros((n * oh * ow,), device="cuda") for _ in range(3)]
tab, ftiles, otiles, cells = B.depth_pack_tables([(gh, gw)] * n, [(oh, ow)] * n, np.arange(n) * gh * gw, np.arange(n), u)
d_tab = torch.from_numpy(tab).cuda()
B.op_depth_fine(lg.data_ptr(), ld, off.data_ptr(), bins.data_ptr(), n, gh, gw, K, u, fine[0].data_ptr(), ss)      # the resize runs read fine[0]
torch.cuda.synchronize()
runs = [dict(name="fine, fixed-shape kernel", ts=[], f=lambda: B.op_depth_fine(lg.data_ptr(), ld, off.data_ptr(), bins.data_ptr(), n, gh, gw, K, u, fine[0].data_ptr(), ss)),
        dict(name="fine, packed kernel", ts=[], f=lambda: B.op_depth_fine_packed_tables(lg.data_ptr(), ld, off.data_ptr(), ld, bins.data_ptr(), d_tab.data_ptr(), n, ftiles, cells, K, fine[1].data_ptr(), ss)),
        dict(name="resize, fixed-shape kernel", ts=[], f=lambda: B.op_depth_resize(fine[0].data_ptr(), n, fh, fw, oh, ow, lo, hi, out[0].data_ptr(), ss)),
        dict(name="resize, packed kernel", ts=[], f=lambda: B.op_depth_resize_packed_tables(fine[0].data_ptr(), d_tab.data_ptr(), n, otiles, lo, hi, out[1].data_ptr(), ss))]
if parent:
    runs += [dict(name="fine, parent's fixed-shape", ts=[], f=lambda: ok(parent.vitx_op_depth_fine(lg.data_ptr(), ld, off.data_ptr(), bins.data_ptr(), n, gh, gw, K, u, fine[2].data_ptr(), ss), "parent fine")),
             dict(name="resize, parent's fixed-shape", ts=[], f=lambda: ok(parent.vitx_op_depth_resize(fine[0].data_ptr(), n, fh, fw, oh, ow, lo, hi, out[2].data_ptr(), ss), "parent resize"))]
rounds(runs, a.iters)
same = lambda x, y: "equal bit for bit" if bool((x.view(torch.int32) == y.view(torch.int32)).all()) else f"{int((x.view(torch.int32) != y.view(torch.int32)).sum())} FLOATS DIFFER"
for r in runs[:4]:
    say(f"  {r['name']:28s}: {fmt(r['ts'], 'us', 1e3)}")
for what, f_, p_, x, y, wgs in (("fine", runs[0], runs[1], fine[0], fine[1], ftiles), ("resize", runs[2], runs[3], out[0], out[1], otiles)):
    say(f"  {what}: packed / fixed = {med(p_['ts'])[0] / med(f_['ts'])[0]:.4f} (medians; the fixed-shape kernel's own spread: {spread(f_['ts']):.1f} %, the packed kernel's: "
        f"{spread(p_['ts']):.1f} %)   {wgs} workgroups each   outputs {same(x, y)}")
if parent:
    say(f"## (b) the fixed-shape kernels of this tree (bodies in csrc/depth_tile.h) against the parent commit's library, the same rounds and logits")
    for r in runs[4:]:
        say(f"  {r['name']:28s}: {fmt(r['ts'], 'us', 1e3)}")
    for what, t_, p_, x, y in (("fine", runs[0], runs[4], fine[0], fine[2]), ("resize", runs[2], runs[5], out[0], out[2])):
        say(f"  {what}: this tree / parent = {med(t_['ts'])[0] / med(p_['ts'])[0]:.4f} (medians; the parent kernel's own spread: {spread(p_['ts']):.1f} %, this tree's: "
            f"{spread(t_['ts']):.1f} %)   outputs {same(x, y)}")
del lg, fine, out

if a.skip_forward:
    write_record()
    sys.exit(0)

# ---- (c) the forward of the mixed pack with and without a head
rng = np.random.default_rng(7)
sources = [(int(rng.integers(320, 1281)), int(rng.integers(320, 1281))) for _ in range(a.images)]
shapes = sorted(B.rect_shape(nx, ny, P, 224, 448)[::-1] for nx, ny in sources)        # (h, w), sorted: one patch-embedding launch per distinct shape
tokens = [1 + (h // P) * (w // P) for h, w in shapes]
distinct = sorted(set(shapes))
pixels_out = sum(h * w for h, w in shapes)
hp = pkg.synth.hparams_for(a.model)
path = pkg.synth.cached_synthetic(a.model, head_scale=8.0)
model = B.Model(path)
Cn, D = hp.num_classes, hp.hidden_size
hw = np.random.default_rng(1)
wp, wc = (hw.standard_normal((K, D)) * 0.05).astype(np.float32), (hw.standard_normal((K, D)) * 0.05).astype(np.float32)
bias, hbins = hw.standard_normal(K).astype(np.float32), np.linspace(0.5, 10.0, K).astype(np.float32)
pixels = torch.randn((sum(h * w * 3 for h, w in shapes),), device="cuda")
probs = torch.empty((a.images, Cn), device="cuda")
sh_arr = np.ascontiguousarray(np.asarray(shapes, np.int32))
say(f"## (c) forward {a.model} bf16, {a.images} mixed-shape images: {len(distinct)} distinct shapes, {sum(tokens)} tokens, {pixels_out / 1e6:.2f} M output pixels; head K = {K}, u = {u}, "
    f"raw rows of the last layer, with a class half")
plain = B.PackContext(model, 0, max_tokens=sum(tokens), max_images=a.images, dtype=B.BF16)
headed = B.PackContext(model, 0, max_tokens=sum(tokens), max_images=a.images, dtype=B.BF16)
headed.depth_set(wp, wc, bias, hbins, None, u, lo, hi, max_pixels=pixels_out)
runs = [dict(name="packed, no head", ts=[], f=lambda: plain.forward_device(pixels.data_ptr(), sh_arr, probs.data_ptr(), 0, ss)),
        dict(name="packed, head", ts=[], f=lambda: headed.forward_device(pixels.data_ptr(), sh_arr, probs.data_ptr(), 0, ss))]
pm = pp = None
if parent:
    pm, pp = C.c_void_p(), C.c_void_p()
    ok(parent.vitx_model_load(path.encode(), C.byref(pm)), "parent vitx_model_load")
    ok(parent.vitx_pack_create(pm, 0, sum(tokens), a.images, B.BF16, None, C.byref(pp)), "parent vitx_pack_create")
    i32p = C.POINTER(C.c_int32)
    runs.append(dict(name="parent, no head", ts=[], f=lambda: ok(parent.vitx_pack_forward_device(pp, pixels.data_ptr(), sh_arr.ctypes.data_as(i32p), a.images, probs.data_ptr(), None, ss),
                                                                 "parent vitx_pack_forward_device")))
# a second context of this tree without a head, made AFTER the parent's: two contexts of one library differ by where their scratch lies, and that
# difference is the scale the parent's ratio has to be read against
plain2 = B.PackContext(model, 0, max_tokens=sum(tokens), max_images=a.images, dtype=B.BF16)
runs.append(dict(name="packed, no head, second context", ts=[], f=lambda: plain2.forward_device(pixels.data_ptr(), sh_arr, probs.data_ptr(), 0, ss)))
rounds(runs, a.steps)
base = med(runs[0]["ts"])[0]
say(f"  one packed forward, no head                     : {fmt(runs[0]['ts'])}   x1.0000   spread {spread(runs[0]['ts']):.2f} %   scratch {plain.scratch_bytes / 2 ** 20:.0f} MiB   {plain.launches[0]} launches")
say(f"  one packed forward, head                        : {fmt(runs[1]['ts'])}   x{med(runs[1]['ts'])[0] / base:.4f}   spread {spread(runs[1]['ts']):.2f} %   scratch {headed.scratch_bytes / 2 ** 20:.0f} MiB   "
    f"{headed.launches[0]} launches")
if parent:
    pb = med(runs[2]["ts"])[0]
    say(f"  the parent commit's packed forward, no head     : {fmt(runs[2]['ts'])}   spread {spread(runs[2]['ts']):.2f} %")
    say(f"  no head: this tree / parent = {base / pb:.4f} (medians; the parent's own spread {spread(runs[2]['ts']):.2f} %)")
    parent.vitx_pack_free(pp); parent.vitx_model_free(pm)
b2 = med(runs[-1]["ts"])[0]
say(f"  a second context of this tree, no head          : {fmt(runs[-1]['ts'])}   spread {spread(runs[-1]['ts']):.2f} %   second / first context of this tree = {b2 / base:.4f}")
plain2.close()
plain.close(); headed.close(); model.close()
say(NOT_MEASURED)
write_record()
