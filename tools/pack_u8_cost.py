"""Cost of feeding packed batches from u8 originals (include/vitx.h "packed batches", u8 sources), interleaved rounds in ONE process on one GPU
(separate runs are not comparable):
    python tools/pack_u8_cost.py [--rounds R] [--steps S] [--images N] [--parent path/to/the/parent/commit's/libvitx.so] [--bench-log FILE]
                                 [--out profiles/pack_u8_cost.txt]
The workload is tools/pack_cost.py's: N seeded source sizes between 2:1 and 1:2, their aspect-preserving shapes at short side 224, patch 16, sorted
by shape; the u8 originals are random bytes of each source's aspect ratio with the long side at about 500, and once at about 2000.
  1. the preprocessing alone: vitx_op_preprocess_pack (ONE launch; the entry point also uploads its tables and synchronises, and that is inside the
     clock) beside the N vitx_preprocess_rect_device launches it replaces, on the same sources, with the outputs compared bit for bit.  The N launches
     are enqueued from Python, one ctypes call each, between two events: where the kernels are shorter than a call, the gaps between them are inside
     that clock too -- the figure is what a caller of the C ABI from Python pays for N launches, not the sum of N kernel times;
  2. the forward fed from device memory, ViT-B/16 bf16: vitx_pack_u8_sources + vitx_pack_forward_device beside the N launches + the f32-fed forward;
  3. end to end from host memory, wall time (long side 500 only): forward_u8 beside the host preprocessing of pack_images + forward_flat;
  4. with --parent, the way tools/ab_libs.py loads a second build (its own copy of the binding module, VITX_LIB): the fixed-shape pp_pil_kernel
     (vitx_preprocess_rect_device, 64 x 500 x 375 -> 288 x 224) and the f32-fed packed forward without heads, this build beside the parent's in the
     same rounds, outputs compared bit for bit;
  5. with --bench-log, the record of a bench.py alternation made beside this run: a file of lines "<tree> <bench.py's JSON line>", in run order, is
     restated as one line per run with the two ranges.
Nothing here is a gate.  Not measured: the 2000-pixel originals from host memory (the host reference alone takes seconds per pack), HBM-cold
sources (every timed call reads what the last one read), other filters than bicubic."""
import argparse, importlib.util, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--steps", type=int, default=5); ap.add_argument("--images", type=int, default=256)
ap.add_argument("--model", default="vit_base_patch16_224"); ap.add_argument("--parent", default=""); ap.add_argument("--bench-log", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_u8_cost.txt"))
a = ap.parse_args()
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def fmt(ts, unit="ms", scale=1.0):
    ts = sorted(ts)
    return f"median {ts[len(ts) // 2] * scale:.3f} {unit} [{ts[0] * scale:.3f} .. {ts[-1] * scale:.3f}]"


def rounds(runs, iters, stream=None, wall=False):
    """Interleaved: every run `iters` times, run after run, a.rounds times; r["ts"] in ms per call -- between two events on `stream`, or wall time."""
    torch.cuda.synchronize()
    for r in runs:
        r["f"]()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for r in runs:
            if wall:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(iters): r["f"]()
                torch.cuda.synchronize(); r["ts"].append((time.perf_counter() - t0) / iters * 1e3)
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(iters): r["f"]()
                e1.record(stream); torch.cuda.synchronize()
                r["ts"].append(e0.elapsed_time(e1) / iters)


say(f"# tools/pack_u8_cost.py --model {a.model} --images {a.images} --rounds {a.rounds} --steps {a.steps}{' --parent <the parent commit build>' if a.parent else ''}"
    f"{' --bench-log <the alternation log>' if a.bench_log else ''}   ({torch.cuda.get_device_name(0)})")
stream = torch.cuda.Stream(); ss = stream.cuda_stream
null = torch.cuda.default_stream()
P = 16
rng = np.random.default_rng(7)
sources = [(int(rng.integers(320, 1281)), int(rng.integers(320, 1281))) for _ in range(a.images)]          # tools/pack_cost.py's list: (nx, ny)
order = sorted(range(a.images), key=lambda i: B.rect_shape(*sources[i], P, 224, 448)[::-1])
sources = [sources[i] for i in order]
shapes = np.asarray([B.rect_shape(nx, ny, P, 224, 448)[::-1] for nx, ny in sources], np.int32)             # (h, w)
tokens = int(sum(1 + (h // P) * (w // P) for h, w in shapes))
mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
pp = B.Preproc.make(resize_a=224, resize_b=224, filter=B.PP_PIL_BICUBIC, mean255=mean, std255=std)
say(f"pack: {a.images} images, {len({tuple(s) for s in shapes.tolist()})} distinct shapes, {tokens} tokens, {int((shapes[:, 0] * shapes[:, 1]).sum())} output pixels")

hp = pkg.synth.hparams_for(a.model)
model = B.Model(pkg.synth.cached_synthetic(a.model, head_scale=8.0))
C = hp.num_classes
out_floats = int((shapes[:, 0].astype(np.int64) * shapes[:, 1]).sum()) * 3
dst0 = np.concatenate([[0], np.cumsum(shapes[:, 0].astype(np.int64) * shapes[:, 1] * 3)])

for long_side in (500, 2000):
    srcs = np.asarray([(max(1, round(ny * long_side / max(nx, ny))), max(1, round(nx * long_side / max(nx, ny)))) for nx, ny in sources], np.int32)      # (ny, nx)
    src0, tile0, lds = B.pack_u8_check(model, pp, srcs, shapes)
    nbytes = int(src0[-1])
    d_src = torch.randint(0, 256, ((nbytes + 3) // 4 * 4,), dtype=torch.uint8, device="cuda")
    d_one, d_n = (torch.zeros(out_floats, dtype=torch.float32, device="cuda") for _ in range(2))
    say(f"## originals with the long side at {long_side}: {nbytes / 2 ** 20:.1f} MiB of u8 sources, {int(tile0[-1])} tiles, {lds} bytes of LDS per workgroup")

    def n_launches(st, out=d_n):
        for i, ((ny, nx), (h, w)) in enumerate(zip(srcs.tolist(), shapes.tolist())):
            B.preprocess_rect_device(pp, d_src.data_ptr() + int(src0[i]), 1, nx, ny, w, h, out.data_ptr() + 4 * int(dst0[i]), st)
    # 1. the preprocessing alone (the op runs on the null stream: so do its rivals here)
    runs = [dict(name="one packed launch (+ its table upload and synchronise)", ts=[], f=lambda: B.preprocess_pack(pp, d_src.data_ptr(), srcs, shapes, d_one.data_ptr())),
            dict(name=f"{a.images} vitx_preprocess_rect_device launches (from Python)", ts=[], f=lambda: n_launches(0))]
    rounds(runs, a.steps, stream=null)
    same = bool(torch.equal(d_one.view(torch.int32), d_n.view(torch.int32)))
    for r in runs:
        say(f"preprocess {long_side}: {r['name']:56s}: {fmt(r['ts'])}")
    say(f"preprocess {long_side}: outputs {'bit-identical' if same else 'DIFFER'}")

    # 2. the forward fed from device memory
    pack = B.PackContext(model, 0, max_tokens=tokens, max_images=a.images, dtype=B.BF16)
    pack.u8_set(pp, max_src_bytes=nbytes)
    probs_u8, probs_f32 = (torch.empty((a.images, C), device="cuda") for _ in range(2))

    def fed_u8():
        pack.u8_sources(srcs); pack.forward_device(d_src.data_ptr(), shapes, probs_u8.data_ptr(), 0, ss)

    def fed_f32():
        n_launches(ss); pack.forward_device(d_n.data_ptr(), shapes, probs_f32.data_ptr(), 0, ss)
    runs = [dict(name="u8 sources: one preprocessing launch + forward", ts=[], f=fed_u8), dict(name=f"{a.images} launches (from Python) + f32-fed forward", ts=[], f=fed_f32)]
    rounds(runs, a.steps, stream=stream)
    fed_u8(); torch.cuda.synchronize(); lu = pack.launches[0]
    pack.forward_device(d_n.data_ptr(), shapes, probs_f32.data_ptr(), 0, ss); torch.cuda.synchronize(); lf = pack.launches[0]
    for r in runs:
        say(f"forward {a.model} bf16 from device memory {long_side}: {r['name']:56s}: {fmt(r['ts'])}")
    say(f"forward {long_side}: launches {lu} (u8-fed) against {lf} + {a.images}; probabilities {'bit-identical' if torch.equal(probs_u8, probs_f32) else 'DIFFER'}")

    # 3. end to end from host memory, wall time
    if long_side == 500:
        host = d_src.cpu().numpy()
        imgs = [host[int(src0[i]):int(src0[i + 1])].reshape(ny, nx, 3) for i, (ny, nx) in enumerate(srcs.tolist())]
        res = {}

        def from_u8():
            res["u8"] = pack.forward_u8(imgs, shapes)[0]

        def from_host():
            flat = np.concatenate([B.preprocess_rect(im, pp, int(w), int(h)).ravel() for im, (h, w) in zip(imgs, shapes)])       # what pack_images does, at the pack's shapes
            res["host"] = pack.forward_flat(flat, shapes)[0]
        runs = [dict(name="forward_u8 (3 bytes per source pixel up, one launch)", ts=[], f=from_u8), dict(name="pack_images' host resize + forward_flat (12 bytes per output pixel up)", ts=[], f=from_host)]
        rounds(runs, 1, wall=True)
        for r in runs:
            say(f"end to end from host memory {long_side}, wall: {r['name']:70s}: {fmt(r['ts'])}")
        say(f"end to end {long_side}: probabilities {'bit-identical' if np.array_equal(res['u8'].view(np.uint32), res['host'].view(np.uint32)) else 'DIFFER'}")
        del host, imgs
    pack.close()
    del d_src, d_one, d_n

# 4. the unchanged paths beside the parent commit's build
if a.parent:
    os.environ["VITX_LIB"] = os.path.abspath(a.parent)
    spec = importlib.util.spec_from_file_location(f"{pkg.__name__}.binding_parent", os.path.join(ROOT, "vit.cpp_amd", "binding.py"))
    Bp = importlib.util.module_from_spec(spec); spec.loader.exec_module(Bp)
    assert not hasattr(Bp.lib(), "vitx_pack_u8_set"), "--parent names a build that has the u8 sources"
    builds = (("this build", B, model), ("parent", Bp, Bp.Model(model.path)))
    n, nx, ny, ow, oh = 64, 500, 375, 288, 224
    src = torch.randint(0, 256, (n, ny, nx, 3), dtype=torch.uint8, device="cuda")
    outs = [torch.zeros((n, oh, ow, 3), device="cuda") for _ in builds]
    runs = [dict(name=name, ts=[], f=(lambda L=L, o=o: L.preprocess_rect_device(L.Preproc.make(resize_a=224, resize_b=224, filter=L.PP_PIL_BICUBIC, mean255=mean, std255=std),
                                                                                 src.data_ptr(), n, nx, ny, ow, oh, o.data_ptr(), ss))) for (name, L, _), o in zip(builds, outs)]
    rounds(runs, 20, stream=stream)
    for r in runs:
        say(f"pp_pil_kernel {n} x {nx} x {ny} -> {ow} x {oh}: {r['name']:12s}: {fmt(r['ts'], 'us', 1e3)} per launch")
    say(f"pp_pil_kernel: outputs {'bit-identical' if torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)) else 'DIFFER'}")
    pixels = torch.randn((out_floats,), device="cuda")
    packs = [L.PackContext(m, 0, max_tokens=tokens, max_images=a.images, dtype=L.BF16) for _, L, m in builds]
    probs = [torch.empty((a.images, C), device="cuda") for _ in builds]
    runs = [dict(name=name, ts=[], f=(lambda p=p, o=o: p.forward_device(pixels.data_ptr(), shapes, o.data_ptr(), 0, ss))) for (name, _, _), p, o in zip(builds, packs, probs)]
    rounds(runs, a.steps, stream=stream)
    for r, p in zip(runs, packs):
        say(f"packed forward {a.model} bf16, f32-fed, no heads: {r['name']:12s}: {fmt(r['ts'])}   {p.launches[0]} launches, scratch {p.scratch_bytes} bytes")
    say(f"packed forward: probabilities {'bit-identical' if torch.equal(probs[0], probs[1]) else 'DIFFER'}")
    for p in packs:
        p.close()

# 5. the benchmark's headline, this tree alternated with the parent's
if a.bench_log:
    import json
    vals = {}
    say("## bench.py --gpus 1, this tree alternated with the parent commit's tree in one visit, in run order")
    with open(a.bench_log) as f:
        for ln in f:
            who, js = ln.split(None, 1)
            d = json.loads(js)
            vals.setdefault(who, []).append(float(d["value"]))
            say(f"bench {who:6s}: {d['value']:.1f} images/sec, {d['ms_per_step']:.4f} ms per step")
    if "this" in vals and "parent" in vals:
        lo, hi = min(vals["parent"]), max(vals["parent"])
        inside = sum(lo <= v <= hi for v in vals["this"])
        say(f"bench: parent {lo:.1f} .. {hi:.1f}, this tree {min(vals['this']):.1f} .. {max(vals['this']):.1f}: {inside} of {len(vals['this'])} runs of this tree inside the parent's spread, "
            f"{sum(v < lo for v in vals['this'])} below it, {sum(v > hi for v in vals['this'])} above it; means {sum(vals['this']) / len(vals['this']) / (sum(vals['parent']) / len(vals['parent'])) - 1:+.2%}")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
