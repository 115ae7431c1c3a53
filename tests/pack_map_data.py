"""Cases and gates of tests/test_gpu_pack_map.py and tests/test_cpu_pack_map.py: the attention-pooling head on packed batches (include/vitx.h
"packed batches", pool_head)."""
import numpy as np

import map_data as MD
import prefix_data as PD
import ref64 as R64

# ---- the op: packs of row counts around the kernel's edges (a 16-row step, the chunk of R rows), by name; R comes from pack_pool_chunks at run time.
# Every count of {1, 15, 16, 17, R - 1, R, R + 1, 2 R + 5} once; (D, H) each once.
OP_CASES = [((1, "R", 17), 128, 2), ((15, "R+1", 16), 768, 12), (("R-1", 1, 16, 15), 768, 13), ((17, "2R+5", "R"), 1152, 16)]

def rows_of(names, R):
    return [n if isinstance(n, int) else {"R-1": R - 1, "R": R, "R+1": R + 1, "2R+5": 2 * R + 5}[n] for n in names]

# ---- end to end: the MICRO attention-pooling fixture (patch 14, 56 x 56: 16 rows), one pack of the file's own shape, a wider one and a taller one of
# 33 x 4 = 132 rows (above the chunk of 128)
E2E_SHAPES = [(56, 56), (56, 112), (462, 56)]
E2E_SEED = 31

def e2e_images():
    rng = np.random.default_rng(E2E_SEED)
    return [(rng.integers(-64, 64, (h, w, 3)) / 16.0).astype(np.float32) for h, w in E2E_SHAPES]      # prefix_data.exact_images' pixels

def restatement(pkg, binding, img, dtype, **mutant):
    """ref64.forward64 of one image (the position table from the engine's host resampler); dtype None: no operand rounding."""
    rnd = {0: PD.f16_round, 1: PD.bf16_round}
    t = PD.file_tensors(pkg, MD.fixture_file(pkg))
    kw = {} if dtype is None else dict(wround=rnd[dtype], uround=rnd[dtype])
    return R64.forward64(t, img[None], 2, binding=binding, **kw, **mutant)

# The restatement's own operand-rounding noise on the three images, 1 - cos(e rounded, e unrounded), by operand type: the figures of
#     PYTHONPATH=tests:. python tests/pack_map_data.py
# (CPU only).  The gate of a shape is 2 x the larger of this and map_data's constants (map_data.cos_gate's margin); the own-shape image keeps
# map_data.cos_gate as it stands.
COS_NOISE = {0: (9.94e-08, 7.33e-08, 3.75e-08), 1: (1.05e-05, 1.77e-05, 8.84e-06)}

def cos_gate(dtype, k):
    return MD.cos_gate(dtype) if k == 0 else max(MD.cos_gate(dtype), 2 * COS_NOISE[dtype][k])

if __name__ == "__main__":
    import _pkg
    pkg = _pkg.load()
    from vitcpp_amd import binding
    for dt in (0, 1):
        out = []
        for img in e2e_images():
            out.append(float(MD.one_minus_cos(restatement(pkg, binding, img, dt)["e"], restatement(pkg, binding, img, None)["e"]).max()))
        print(dt, tuple(float(f"{v:.3g}") for v in out))
