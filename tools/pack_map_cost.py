"""Cost of the packed attention-pooling launches (csrc/attention_pool_packed.hip) beside the fixed-shape kernel (csrc/attention_pool.hip) on the same
rows, interleaved in ONE process (separate runs are not comparable):
    python tools/pack_map_cost.py [--rounds R] [--iters I] [--out profiles/pack_map_cost.txt]
Per case (n images x N rows, D 768, H 12): vitx_op_attention_pool_packed_tables (both launches, Mp in bf16 and in f16) and vitx_op_attention_pool (f32 M),
R rounds of I launches, the order rotating between rounds; min .. max per kernel.  Then the mixed pack of tools/pack_cost.py's kind (one 4000-row image
beside 200 of 196 rows) against a uniform pack of the same row count: time per row, to show there is no imbalance tail."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_map_cost.txt"))
a = ap.parse_args()
L = B.lib()
lines = []


def say(x):
    print(x, flush=True); lines.append(x)


def timed(ops):
    ts = {k: [] for k in ops}
    names = list(ops)
    for k in names:
        for _ in range(3): B.check(ops[k](), k)
    torch.cuda.synchronize()
    for r in range(a.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters): ops[k]()
            e1.record(); torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / a.iters * 1e3)
    return ts


D, H = 768, 12
g = torch.Generator(device="cuda").manual_seed(1)
lw = 1 + 0.1 * torch.randn(D, device="cuda", generator=g); lb = 0.1 * torch.randn(D, device="cuda", generator=g)
u = torch.randn((H, D), device="cuda", generator=g) * (2.0 / D ** 0.5)
say(f"# tools/pack_map_cost.py --rounds {a.rounds} --iters {a.iters}   ({torch.cuda.get_device_name(0)}); D {D} H {H}; us per call, min .. max over the rounds")


def packed_op(X, rows, dt, out):
    R, chunk0 = B.pack_pool_chunks(rows)
    n = len(rows)
    tab = torch.from_numpy(np.concatenate([np.concatenate([[0], np.cumsum(rows)]), chunk0]).astype(np.int32)).cuda()
    part = torch.zeros((int(chunk0[-1]), H, D + 2), device="cuda")
    keep.append((tab, part))
    return lambda: L.vitx_op_attention_pool_packed_tables(X.data_ptr(), tab.data_ptr(), tab.data_ptr() + 4 * (n + 1), n, int(chunk0[-1]), lw.data_ptr(), lb.data_ptr(), 1e-6,
                                                          u.data_ptr(), part.data_ptr(), None, out.data_ptr(), dt, D, H)


keep = []
for n, N in ((256, 196), (64, 576)):
    X = torch.randn((n * N, D), device="cuda", generator=g)
    M = torch.zeros((n, H, D), device="cuda")
    ops = {"fixed": lambda X=X, M=M, n=n, N=N: L.vitx_op_attention_pool(X.data_ptr(), D, N * D, lw.data_ptr(), lb.data_ptr(), 1e-6, u.data_ptr(), M.data_ptr(), None, n, N, D, H, None)}
    for dname, dt, tdt in (("bf16", B.BF16, torch.bfloat16), ("f16", B.F16, torch.float16)):
        ops[f"packed {dname}"] = packed_op(X, [N] * n, dt, torch.zeros((n, H, D), device="cuda", dtype=tdt))
    ts = timed(ops)
    for k in ops:
        say(f"{n:4d} x {N:4d} rows  {k:12s}: {min(ts[k]):7.1f} .. {max(ts[k]):7.1f}")
    for dname in ("bf16", "f16"):
        p, f = ts[f"packed {dname}"], ts["fixed"]
        verdict = "faster, outside both spreads" if max(p) < min(f) else "**NOT faster outside both spreads**"
        say(f"{n:4d} x {N:4d} rows  packed {dname} / fixed = x{min(p) / min(f):.3f} (min / min): {verdict}; the K/V GEMM's 99 us (profiles/map_head_cost.txt, 256 x 196): "
            + ("met" if max(p) < 99.0 else "**not met**" if N == 196 else "another shape"))
rows_mixed = [4000] + [196] * 200
total = sum(rows_mixed)
X = torch.randn((total, D), device="cuda", generator=g)
out = torch.zeros((len(rows_mixed), H, D), device="cuda", dtype=torch.bfloat16)
uni = [196] * (total // 196)
ops = {"mixed": packed_op(X, rows_mixed, B.BF16, out), "uniform": packed_op(X, uni, B.BF16, out)}
ts = timed(ops)
for k, rows in (("mixed", rows_mixed), ("uniform", uni)):
    say(f"pack of {len(rows)} images, {sum(rows)} rows ({k}): {min(ts[k]):7.1f} .. {max(ts[k]):7.1f}  = {min(ts[k]) * 1e3 / sum(rows):.2f} ns per row")
say("The forward of such a pack against one image context per shape is not available: image contexts of attention-pooling files stay at the file's own shape.")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
