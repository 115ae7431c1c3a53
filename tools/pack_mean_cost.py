"""Cost of the packed cls + mean launches (csrc/features_packed.hip) beside the class-row gather and the image context's feature kernel on the same rows,
interleaved in ONE process (separate runs are not comparable):
    python tools/pack_mean_cost.py [--rounds R] [--iters I] [--out profiles/pack_mean_cost.txt]
Per pack (D 768, T = 1, bf16 operand): vitx_op_feat_pool_packed_tables (both launches: operand z and the f32 mean) against vitx_op_text_pool on the class rows
(launch_pool_rows' kernel text) + vitx_op_features (one call per run of images of one row count; one workgroup per image), R rounds of I launches, the
order rotating between rounds; min .. max per side.  Packs: uniform 256 x 197 rows, and one 4001-row image beside 200 of 197 rows with a uniform pack of
about the same rows.  The expectation recorded, met or not: the skewed pack costs no more per row than the uniform one beyond the spread of the rounds."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _pkg; pkg = _pkg.load()
from vitcpp_amd import binding as B

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_mean_cost.txt"))
a = ap.parse_args()
L = B.lib()
lines, keep = [], []
D, T = 768, 1


def say(x):
    print(x, flush=True); lines.append(x)


def timed(ops):
    ts = {k: [] for k in ops}
    names = list(ops)
    for k in names:
        for _ in range(3): ops[k]()
    torch.cuda.synchronize()
    for r in range(a.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters): ops[k]()
            e1.record(); torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / a.iters * 1e3)
    return ts


g = torch.Generator(device="cuda").manual_seed(1)
lw = 1 + 0.1 * torch.randn(D, device="cuda", generator=g); lb = 0.1 * torch.randn(D, device="cuda", generator=g)
say(f"# tools/pack_mean_cost.py --rounds {a.rounds} --iters {a.iters}   ({torch.cuda.get_device_name(0)}); D {D} T {T} bf16; us per call, min .. max over the rounds")


def sides(X, rows):
    """The two sides on a pack of images of `rows` rows each: the packed launches, and the class-row gather + the feature kernel per run of one row count."""
    n, row0 = len(rows), np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    R, _, pc0 = B.pack_mean_chunks(row0, T)
    m_pad = -(-n // 256) * 256
    d_row0, d_pc0 = torch.from_numpy(row0).cuda(), torch.from_numpy(pc0).cuda()
    d_cls_rows = torch.from_numpy((row0[:-1] - np.arange(n)).astype(np.int32)).cuda()        # vitx_op_text_pool with T = 1 reads row i + pooled[i] = row0[i]
    part = torch.zeros((int(pc0[-1]), D), device="cuda"); mean = torch.zeros((n, D), device="cuda"); mean2 = torch.zeros((n, D), device="cuda")
    z = torch.zeros((m_pad, 2 * D), device="cuda", dtype=torch.bfloat16); zc = torch.zeros((m_pad, D), device="cuda", dtype=torch.bfloat16)
    keep.append((d_row0, d_pc0, d_cls_rows, part, mean, mean2, z, zc))
    runs, i = [], 0                                                                          # (first image, images, rows per image) of every run
    while i < n:
        j = i
        while j < n and rows[j] == rows[i]: j += 1
        runs.append((i, j - i, rows[i])); i = j

    def packed():
        B.check(L.vitx_op_feat_pool_packed_tables(B.BF16, X.data_ptr(), d_row0.data_ptr(), d_pc0.data_ptr(), n, int(pc0[-1]), T, D, lw.data_ptr(), lb.data_ptr(), 1e-6, part.data_ptr(),
                                                  None, mean.data_ptr(), z.data_ptr(), m_pad, 0), "packed")

    def fixed():
        B.check(L.vitx_op_text_pool(B.BF16, X.data_ptr(), d_cls_rows.data_ptr(), lw.data_ptr(), lb.data_ptr(), zc.data_ptr(), n, 1, D, 1e-6, None), "text_pool")
        for i0, k, N in runs:
            B.check(L.vitx_op_features(X.data_ptr() + int(row0[i0]) * D * 4, D, N * D, lw.data_ptr(), lb.data_ptr(), None, mean2.data_ptr() + i0 * D * 4, None, D, k, N, D, 1e-6, 0, None), "features")
    return {"packed (2 launches)": packed, f"gather + features ({1 + len(runs)} launches)": fixed}


per_row = {}
for label, rows in (("uniform 256 x 197", [197] * 256), ("skewed 4001 + 200 x 197", [4001] + [197] * 200), ("uniform 220 x 197", [197] * 220)):
    X = torch.randn((sum(rows), D), device="cuda", generator=g)
    ts = timed(sides(X, rows))
    for k, v in ts.items():
        say(f"{label:24s} {sum(rows):6d} rows  {k:34s}: {min(v):7.1f} .. {max(v):7.1f}  = {min(v) * 1e3 / sum(rows):.2f} ns per row")
    per_row[label] = [t * 1e3 / sum(rows) for t in ts["packed (2 launches)"]]
sk, un = per_row["skewed 4001 + 200 x 197"], per_row["uniform 220 x 197"]
say(f"expectation (the skewed pack costs no more per row than the uniform one beyond the spread of the rounds): skewed {min(sk):.2f} .. {max(sk):.2f}, uniform "
    f"{min(un):.2f} .. {max(un):.2f} ns per row: " + ("met" if min(sk) <= max(un) else "**NOT met**"))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
