"""Cost of attention maps on packed batches (include/vitx.h "packed batches", attention maps), bf16, ViT-B shapes, one GPU.
  (a) each packed map launch against its fixed-shape kernel on the SAME QKV: a uniform pack of 64 images of 197 tokens, D 768, H 12.  The packed kernels
      are reached through the synchronous test entry points (vitx_op_*_packed take no stream), so their time is KERNEL time from a trace, taken in a
      run of its own:
          rocprofv3 --kernel-trace --output-format csv -d TRACE -- python tools/pack_attn_cost.py --kernels --manifest TRACE/manifest.json [--parent-lib P.so]
      runs 7 interleaved rounds -- fixed, packed (and, with --parent-lib, the parent commit's fixed-shape kernel, section (c)) `iters` launches each,
      kernel after kernel -- compares the outputs bit for bit and writes the order of its launches to the manifest; the report run below reads the
      trace's dispatch rows of the map kernels in start order and assigns them by that order.
  (b) the forward of the mixed pack of tools/pack_cost.py (the same seeded shapes, sorted by shape): maps off, the last layer's class maps, rollout; scratch
      and launches; beside one rectangular context per distinct shape, bucket after bucket, with the same outputs on.  Device events, interleaved rounds.
  (c) what this change does not alter, against the parent commit's library (--parent-lib, loaded beside this tree's): the four fixed-shape map kernels
      (in the trace run, outputs compared bit for bit), the packed forward without maps in the rounds of (b) (probabilities compared bit for bit), and
      bench.py alternated three times, whose lines the caller collects into --bench-log ("this <json line>" / "parent <json line>", the parent's run with
      VITX_LIB and --allow-overrides).
      python tools/pack_attn_cost.py --trace TRACE --manifest TRACE/manifest.json [--parent-lib P.so] [--bench-log LOG] [--out profiles/pack_attn_cost.txt]
Nothing here is a gate: every ratio stands beside the min .. max of its yardstick.  Not measured: F16, head dims other than 64, `rope` and register
files, packs with one 1024-token image beside many small ones (the launch then carries NT = 16 register tiles for every image), class maps of all
twelve layers, HBM-cold tables, vitx_pack_attn_read."""
import argparse, csv, ctypes as C, glob, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=10); ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--images", type=int, default=256); ap.add_argument("--model", default="vit_base_patch16_224")
ap.add_argument("--kernels", action="store_true", help="the trace run of (a): launch the kernels, write --manifest, report nothing")
ap.add_argument("--manifest", default=None); ap.add_argument("--trace", default=None, help="the directory rocprofv3 wrote the trace run's CSV into")
ap.add_argument("--parent-lib", default=None, help="libvitx.so of the parent commit: section (c)")
ap.add_argument("--bench-log", default=None); ap.add_argument("--skip-forward", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_attn_cost.txt"))
a = ap.parse_args()
lines = []
D, H, P, N_UNI, N_IMG = 768, 12, 16, 197, 64
KERNELS = ("class map", "factor", "step", "row")
MAP_KERNEL_WORDS = ("attn_cls_map", "attn_head_mean", "attn_rollout_step", "attn_rollout_row")


def say(x):
    print(x, flush=True); lines.append(x)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(ts, unit="ms", scale=1.0):
    m, lo, hi = med(ts)
    return f"median {m * scale:9.3f} {unit} [{lo * scale:9.3f} .. {hi * scale:9.3f}]"


def against(m, parent_ts):
    """Where this tree's median time lies against the parent's own min .. max."""
    lo, hi = min(parent_ts), max(parent_ts)
    return "inside the parent's own min .. max" if lo <= m <= hi else ("below the parent's min (faster)" if m < lo else "**ABOVE the parent's max (slower)**")


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: status {rc}")


def load_parent():
    if not a.parent_lib:
        return None
    L = C.CDLL(os.path.abspath(a.parent_lib))
    vp, ip = C.c_void_p, C.c_int
    L.vitx_op_attention_map.argtypes = [ip, vp, C.c_long, vp, vp, ip, ip, ip, ip, vp]
    L.vitx_op_rollout_factor.argtypes = [ip, vp, C.c_long, vp, ip, ip, ip, ip, vp]
    L.vitx_op_rollout_step.argtypes = [vp, vp, ip, ip, vp]
    L.vitx_op_rollout_row.argtypes = [vp, C.c_long, vp, vp, C.c_long, ip, ip, ip, vp]
    L.vitx_model_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.vitx_pack_create.argtypes = [vp, ip, ip, ip, ip, vp, C.POINTER(vp)]
    L.vitx_pack_forward_device.argtypes = [vp, vp, C.POINTER(C.c_int32), ip, vp, vp, vp]
    L.vitx_pack_free.argtypes = [vp]; L.vitx_model_free.argtypes = [vp]
    return L


parent = load_parent()

# ================================================================================================ the trace run of (a) and (c)
if a.kernels:
    n, N = N_IMG, N_UNI
    row0 = (np.arange(n + 1) * N).astype(np.int32)
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv = (torch.randn((n * N, 3 * D), device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    libs = ["fixed", "packed"] + (["parent"] if parent else [])
    cls = {k: z(n, H * N) for k in libs}; fac = {k: z(n, N * N) for k in libs}; row = {k: z(n, N) for k in libs}
    r_in = z(n, N * N); B.op_rollout_factor(B.BF16, qkv.data_ptr(), r_in.data_ptr(), n, N, D, H)       # the step's right operand and the row's r (one launch, in the manifest)
    step0 = r_in.clone(); step = {k: z(n, N * N) for k in libs}
    q, dt = qkv.data_ptr(), B.BF16
    calls = {
        ("class map", "fixed"): lambda: B.op_attention_map(dt, q, cls["fixed"].data_ptr(), 0, n, N, D, H),
        ("class map", "packed"): lambda: B.op_attention_map_packed(dt, q, cls["packed"].data_ptr(), 0, row0, D, H),
        ("factor", "fixed"): lambda: B.op_rollout_factor(dt, q, fac["fixed"].data_ptr(), n, N, D, H),
        ("factor", "packed"): lambda: B.op_attention_map_packed(dt, q, 0, fac["packed"].data_ptr(), row0, D, H, half_identity=True),
        ("step", "fixed"): lambda: B.op_rollout_step(step["fixed"].data_ptr(), r_in.data_ptr(), n, N),
        ("step", "packed"): lambda: B.op_rollout_step_packed(step["packed"].data_ptr(), r_in.data_ptr(), row0),
        ("row", "fixed"): lambda: B.op_rollout_row(cls["fixed"].data_ptr(), H * N, r_in.data_ptr(), row["fixed"].data_ptr(), N, n, N, H),
        ("row", "packed"): lambda: B.op_rollout_row_packed(cls["packed"].data_ptr(), r_in.data_ptr(), row["packed"].data_ptr(), row0, H),
    }
    if parent:
        calls.update({
            ("class map", "parent"): lambda: ok(parent.vitx_op_attention_map(dt, q, 0, cls["parent"].data_ptr(), None, n, N, D, H, None), "parent class map"),
            ("factor", "parent"): lambda: ok(parent.vitx_op_rollout_factor(dt, q, 0, fac["parent"].data_ptr(), n, N, D, H, None), "parent factor"),
            ("step", "parent"): lambda: ok(parent.vitx_op_rollout_step(step["parent"].data_ptr(), r_in.data_ptr(), n, N, None), "parent step"),
            ("row", "parent"): lambda: ok(parent.vitx_op_rollout_row(cls["parent"].data_ptr(), H * N, r_in.data_ptr(), row["parent"].data_ptr(), N, n, N, H, None), "parent row"),
        })
    order = [["setup", "setup", -1]]

    def launch(kern, lib, rnd):
        if kern == "step":                               # in place: every launch starts from the same left operand (a device copy, not a map kernel)
            step[lib].copy_(step0)
        calls[(kern, lib)](); order.append([kern, lib, rnd])

    for kern in KERNELS:                                 # warm-up (round -1), then the class maps exist for the row launches
        for lib in libs:
            for _ in range(2): launch(kern, lib, -1)
    torch.cuda.synchronize()
    for rnd in range(a.rounds):
        turn = libs[rnd % len(libs):] + libs[:rnd % len(libs)]          # whose launches come first rotates from round to round
        for kern in KERNELS:
            for lib in turn:
                for _ in range(a.iters): launch(kern, lib, rnd)
        torch.cuda.synchronize()
    eq = lambda x, y: bool((x.view(torch.int32) == y.view(torch.int32)).all())
    same = {kern: {lib: eq(buf["fixed"], buf[lib]) for lib in libs[1:]} for kern, buf in (("class map", cls), ("factor", fac), ("step", step), ("row", row))}
    with open(a.manifest, "w") as f:
        json.dump(dict(order=order, same=same, n=n, N=N, rounds=a.rounds, iters=a.iters), f)
    print(f"{len(order)} map-kernel launches; outputs equal to the fixed-shape kernel's: {same}")
    sys.exit(0)


def write_record():
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


say(f"# tools/pack_attn_cost.py --model {a.model} --images {a.images} --rounds {a.rounds} --iters {a.iters} --steps {a.steps}"
    f"{' --parent-lib <the parent commit>' if parent else ''}   ({torch.cuda.get_device_name(0)})")

# ================================================================================================ (a), (c): the kernels, from the trace
if a.trace and a.manifest:
    man = json.load(open(a.manifest))
    rows = []
    for path in glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if any(w in r["Kernel_Name"] for w in MAP_KERNEL_WORDS):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    order = man["order"]
    if len(rows) != len(order):
        say(f"## (a) NOT REPORTED: the trace holds {len(rows)} dispatches of the map kernels, the manifest {len(order)} launches")
    else:
        per = {}
        for (t0, t1, name), (kern, lib, rnd) in zip(rows, order):
            if rnd >= 0:
                assert ("packed" in name) == (lib == "packed"), (name, kern, lib)
                per.setdefault((kern, lib), {}).setdefault(rnd, []).append((t1 - t0) * 1e-3)
        ts = {k: [float(np.mean(v[r])) for r in sorted(v)] for k, v in per.items()}        # us per launch, one figure per round
        say(f"## (a) each packed map launch against its fixed-shape kernel, the same QKV: uniform pack, {man['n']} images of {man['N']} tokens, D {D}, H {H}, bf16; kernel time "
            f"from a kernel trace, {man['rounds']} interleaved rounds of {man['iters']} launches (the order of the libraries rotates), a round's figure = the mean of its launches")
        for kern in KERNELS:
            f_, p_ = ts[(kern, "fixed")], ts[(kern, "packed")]
            ratio = med(p_)[0] / med(f_)[0]
            inside = med(f_)[1] <= med(p_)[0] <= med(f_)[2] or med(p_)[1] <= med(f_)[0] <= med(p_)[2]
            verdict = "inside the spread of either kernel" if inside else f"**OUTSIDE the spread of both kernels: packed / fixed = {ratio:.4f}**"
            say(f"  {kern:9s} fixed : {fmt(f_, 'us')}")
            say(f"  {kern:9s} packed: {fmt(p_, 'us')}   packed / fixed = {ratio:.4f} (medians)   {verdict}   outputs "
                f"{'equal bit for bit' if man['same'][kern]['packed'] else 'DIFFER'}")
        if any((k, "parent") in ts for k in KERNELS):
            say("## (c) the fixed-shape map kernels of this tree (bodies in csrc/attention_map_tile.h) against the parent commit's library, the same rounds and operands")
            for kern in KERNELS:
                f_, p_ = ts[(kern, "fixed")], ts[(kern, "parent")]
                ratio = med(f_)[0] / med(p_)[0]
                say(f"  {kern:9s} parent: {fmt(p_, 'us')}   this tree / parent = {ratio:.4f} (medians)   {against(med(f_)[0], p_)}   outputs "
                    f"{'equal bit for bit' if man['same'][kern]['parent'] else 'DIFFER'}")
else:
    say("## (a) NOT MEASURED in this run: no --trace / --manifest of a kernel-trace run was given")

if a.skip_forward:
    write_record()
    sys.exit(0)

# ================================================================================================ (b), (c): the forward of the mixed pack
stream = torch.cuda.Stream(); ss = stream.cuda_stream


def rounds(runs, iters):
    """Interleaved: every run `iters` times between two events, run after run, a.rounds times; r["ts"] in ms per call."""
    torch.cuda.synchronize()
    for r in runs:
        for _ in range(2): r["f"]()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for r in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(iters): r["f"]()
            e1.record(stream); torch.cuda.synchronize()
            r["ts"].append(e0.elapsed_time(e1) / iters)


rng = np.random.default_rng(7)
sources = [(int(rng.integers(320, 1281)), int(rng.integers(320, 1281))) for _ in range(a.images)]
shapes = sorted(B.rect_shape(nx, ny, P, 224, 448)[::-1] for nx, ny in sources)        # (h, w), sorted: one patch-embedding launch per distinct shape
tokens = [1 + (h // P) * (w // P) for h, w in shapes]
distinct = sorted(set(shapes))
sq = sum(t * t for t in tokens)
hp = pkg.synth.hparams_for(a.model)
path = pkg.synth.cached_synthetic(a.model, head_scale=8.0)
model = B.Model(path)
Cn, L = hp.num_classes, hp.num_hidden_layers
pixels = torch.randn((sum(h * w * 3 for h, w in shapes),), device="cuda")
probs = {k: torch.zeros((a.images, Cn), device="cuda") for k in ("off", "last", "rollout", "parent", "buckets")}
sh_arr = np.ascontiguousarray(np.asarray(shapes, np.int32))
say(f"## (b) forward {a.model} bf16, {a.images} mixed-shape images sorted by shape: {len(distinct)} distinct shapes, {min(tokens)} .. {max(tokens)} tokens, sum N = {sum(tokens)}, "
    f"sum N^2 = {sq}; {a.rounds} interleaved rounds of {a.steps} forwards (device events)")


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


anchor = B.Context(model, 0, 1, B.BF16)                                               # holds the image contexts' weight set: the deltas below are scratch
packs = {k: B.PackContext(model, 0, max_tokens=sum(tokens), max_images=a.images, dtype=B.BF16) for k in ("off", "last", "rollout")}
packs["last"].attn_enable([L - 1])
packs["rollout"].attn_enable([], rollout=True, max_sq_tokens=sq)
runs = [dict(name=k, ts=[], f=(lambda k=k: packs[k].forward_device(pixels.data_ptr(), sh_arr, probs[k].data_ptr(), 0, ss))) for k in ("off", "last", "rollout")]
bucket_bytes = {}
buckets = {}
for mode in ("last", "rollout"):
    before = free_bytes()
    buckets[mode], at = [], 0
    for shp in distinct:
        k = shapes.count(shp)
        c = B.Context(model, 0, k, B.BF16, img_shape=shp)
        c.attn_enable([L - 1] if mode == "last" else [], rollout=mode == "rollout")
        buckets[mode].append((c, k, at)); at += k * shp[0] * shp[1] * 3
    bucket_bytes[mode] = before - free_bytes()


def run_buckets(mode):
    img0 = 0
    for c, k, off in buckets[mode]:
        c.forward_device(pixels.data_ptr() + off * 4, k, probs["buckets"].data_ptr() + img0 * Cn * 4, 0, ss); img0 += k


runs += [dict(name=f"buckets {m}", ts=[], f=(lambda m=m: run_buckets(m))) for m in ("last", "rollout")]
pm = pp = None
if parent:
    pm, pp = C.c_void_p(), C.c_void_p()
    ok(parent.vitx_model_load(path.encode(), C.byref(pm)), "parent vitx_model_load")
    ok(parent.vitx_pack_create(pm, 0, sum(tokens), a.images, B.BF16, None, C.byref(pp)), "parent vitx_pack_create")
    i32p = C.POINTER(C.c_int32)
    runs.append(dict(name="parent", ts=[], f=lambda: ok(parent.vitx_pack_forward_device(pp, pixels.data_ptr(), sh_arr.ctypes.data_as(i32p), a.images, probs["parent"].data_ptr(), None, ss),
                                                        "parent vitx_pack_forward_device")))
rounds(runs, a.steps)
by = {r["name"]: r["ts"] for r in runs}
base = med(by["off"])[0]
eqp = lambda x, y: "equal bit for bit" if bool((probs[x].view(torch.int32) == probs[y].view(torch.int32)).all()) else "DIFFER"
for k, what in (("off", "maps off"), ("last", "the last layer's class maps"), ("rollout", "rollout")):
    say(f"  one packed forward, {what:28s}: {fmt(by[k])}   x{med(by[k])[0] / base:.4f}   scratch {packs[k].scratch_bytes / 2 ** 20:7.0f} MiB   {packs[k].launches[0]} launches"
        + ("" if k == "off" else f"   probabilities {eqp(k, 'off')} to maps off"))
for m in ("last", "rollout"):
    t = by[f"buckets {m}"]
    say(f"  {len(distinct)} rectangular contexts, {('the last layer class maps' if m == 'last' else 'rollout'):26s}: {fmt(t)}   x{med(t)[0] / med(by[m])[0]:.4f} of the packed forward with the same "
        f"outputs   scratch {bucket_bytes[m] / 2 ** 20:7.0f} MiB")
if parent:
    t = by["parent"]
    say(f"## (c) the packed forward without maps against the parent commit's library, the same rounds: parent {fmt(t)}   this tree / parent = {base / med(t)[0]:.4f} (medians)   "
        f"{against(base, t)}   probabilities {eqp('off', 'parent')}")
    parent.vitx_pack_free(pp); parent.vitx_model_free(pm)
for mode in buckets:
    for c, _, _ in buckets[mode]:
        c.close()
for p_ in packs.values():
    p_.close()
anchor.close(); model.close()

if a.bench_log and os.path.exists(a.bench_log):
    vals = {"this": [], "parent": []}
    for ln in open(a.bench_log):
        who, _, js = ln.partition(" ")
        if who in vals and js.strip().startswith("{"):
            vals[who].append(float(json.loads(js)["value"]))
    if vals["this"] and vals["parent"]:
        lo, hi = min(vals["parent"]), max(vals["parent"])
        m = sorted(vals["this"])[len(vals["this"]) // 2]
        say(f"## (c) bench.py --gpus 1, alternated {len(vals['this'])} times (images/s): this tree {vals['this']}, the parent commit's library {vals['parent']}   "
            f"{'this tree median inside the parent own min .. max' if lo <= m <= hi else ('this tree median ABOVE the parent max' if m > hi else '**this tree median BELOW the parent min**')}")
say("## not measured: F16, head dims other than 64, `rope` and register files, a pack with one 1024-token image beside many small ones, class maps of all twelve layers, "
    "HBM-cold tables, vitx_pack_attn_read")
write_record()
