"""The attention-pooling head on packed batches on the MI355X (include/vitx.h "packed batches", pool_head): the packed pooling kernel against
float64 and beside the fixed-shape kernel, its leaks, drops and position independence, the forward of a pack end to end against ref64.forward64, and
creation."""
import ctypes as C

import numpy as np
import pytest

import map_data as MD
import pack_map_data as KD
import prefix_data as PD
import rect_data as XD
import ref64 as R64
from ref64 import PROB_TOL
from test_gpu_map_head import _bits, _check_pool, _dev, _pool_inputs

pytestmark = pytest.mark.gpu
SENT = -12345.5

def _check(M, F, u, where):
    """_check_pool on one image's M [H][D]; the packed op has no probability output, so the reference's own stand in for it."""
    return _check_pool(M[None], MD.pool64(F[None].astype(np.float64), u.astype(np.float64))[1], F[None], u, where)

def _pack_rows(rows, d, h, seed, gap=3):
    """The rows of a pack end to end (each image drawn as _pool_inputs draws one), `gap` rows of 1e30 then NaN behind the last; w, b, u."""
    x, w, b, u = _pool_inputs(1, sum(rows), d, h, seed, gap)
    return x[0], w, b, u, np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)

def _run_packed(binding, torch, x, w, b, u, row0, extra=1):
    n, (h, d) = len(row0) - 1, u.shape
    dx, dw, db, du = (_dev(torch, a) for a in (x, w, b, u))
    M = torch.full((n + extra, h, d), SENT, dtype=torch.float32, device="cuda")
    binding.op_attention_pool_packed(dx.data_ptr(), row0, dw.data_ptr(), db.data_ptr(), 1e-6, du.data_ptr(), M.data_ptr(), d, h)
    M = M.cpu().numpy()
    assert (M[n:] == SENT).all(), "rows of d_M past n were written"
    rows = int(row0[-1])
    F = torch.zeros((rows, d), dtype=torch.float32, device="cuda")       # from the feature kernel: the LayerNorm's own error stays outside the bound
    binding.op_features_ex(dx.data_ptr(), d, rows * d, dw.data_ptr(), db.data_ptr(), 0, 0, F.data_ptr(), rows * d, 1, rows, 0, d, 1e-6)
    return M[:n], F.cpu().numpy()

@pytest.mark.parametrize("names,d,h", KD.OP_CASES)
def test_op_against_float64_beside_the_fixed_kernel(binding, torch_gpu, names, d, h):
    torch = torch_gpu
    R, _ = binding.pack_pool_chunks([1])
    rows = KD.rows_of(names, R)
    x, w, b, u, row0 = _pack_rows(rows, d, h, seed=d + h)
    M, F = _run_packed(binding, torch, x, w, b, u, row0)
    dx, dw, db, du = (_dev(torch, a) for a in (x, w, b, u))
    for i, N in enumerate(rows):
        Fi = F[row0[i]:row0[i + 1]]
        _check(M[i], Fi, u, f"packed, image {i}: N {N} D {d} H {h}")
        old = torch.zeros((1, h, d), dtype=torch.float32, device="cuda")
        binding.op_attention_pool(dx.data_ptr() + int(row0[i]) * d * 4, d, N * d, dw.data_ptr(), db.data_ptr(), 1e-6, du.data_ptr(), old.data_ptr(), 0, 1, N, d, h)
        _check(old.cpu().numpy()[0], Fi, u, f"fixed-shape kernel, image {i}: N {N} D {d} H {h}")

def test_position_neighbours_and_what_lies_behind(binding, torch_gpu):
    """One image's M has the same bits alone, first, last, and between a NaN and a 1e30 neighbour; NaN rows lie directly behind the pack's last row."""
    torch = torch_gpu
    R, _ = binding.pack_pool_chunks([1])
    d, h, N = 768, 12, R + 21
    x, w, b, u, _ = _pack_rows([N], d, h, seed=5, gap=0)
    other = _pack_rows([40], d, h, seed=6, gap=0)[0]
    nan = np.full((2, d), np.nan, np.float32)
    run = lambda parts: _run_packed(binding, torch, np.concatenate(parts + [nan]), w, b, u, np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32))[0]
    alone = run([x])[0]
    assert np.isfinite(alone).all()
    for where, parts, i in (("first", [x, other], 0), ("last", [other, x], 1), ("between NaN and 1e30", [np.full((17, d), np.nan, np.float32), x, np.full((R, d), 1e30, np.float32)], 1)):
        assert np.array_equal(_bits(run(parts)[i]), _bits(alone)), where

@pytest.mark.parametrize("where", ["step-edge", "chunk-edge"])
def test_a_row_that_alone_carries_a_head(binding, torch_gpu, where):
    """Row t_hot alone carries head H - 1's score, so M_{H-1} = F[t_hot]; heads 0 and H - 1 get opposite u before, so a kernel that read the wrong head's
    column fails the float64 check."""
    torch = torch_gpu
    R, _ = binding.pack_pool_chunks([1])
    d, h, rows = 128, 4, [20, R + 30, 9]
    t_hot = {"step-edge": 16, "chunk-edge": R}[where]
    x, w, b, u, row0 = _pack_rows(rows, d, h, seed=60 + t_hot)
    u[h - 1] = -u[0]
    M, F = _run_packed(binding, torch, x, w, b, u, row0)
    want, _, tol = _check(M[1], F[row0[1]:row0[2]], u, f"opposite heads, {where}")
    assert (np.abs(M[1, 0] - want[0, h - 1]) / tol[0, 0]).max() > 10, "head 0's M must not pass as head H - 1's"
    f = F[row0[1] + t_hot].astype(np.float64)
    u[h - 1] = (40.0 * f / (f @ f)).astype(np.float32)
    M, _ = _run_packed(binding, torch, x, w, b, u, row0)
    tols = [_check(M[i], F[row0[i]:row0[i + 1]], u, f"hot row {t_hot}, image {i}")[2] for i in range(3)]
    assert (np.abs(M[1, h - 1] - F[row0[1] + t_hot]) <= tols[1][0, h - 1]).all(), "M of the one-hot head is not the hot row"

@pytest.mark.parametrize("dtype", [0, 1])
def test_pack_end_to_end(pkg, binding, torch_gpu, dtype):
    imgs = KD.e2e_images()
    model = binding.Model(MD.fixture_file(pkg))
    tokens = sum((h // 14) * (w // 14) for h, w in KD.E2E_SHAPES)
    pack = binding.PackContext(model, device=0, max_tokens=tokens, max_images=3, dtype=dtype, pool_head=True)
    pack.feat_enable(cls=True)
    p, lg = pack.forward(imgs)
    e = pack.feat_read()[0]
    lens = []
    for k, img in enumerate(imgs):
        ref, exact = KD.restatement(pkg, binding, img, dtype), KD.restatement(pkg, binding, img, None)
        cos, gate = float(MD.one_minus_cos(e[k:k + 1], exact["e"]).max()), KD.cos_gate(dtype, k)
        flat = float(MD.one_minus_cos(e[k:k + 1], KD.restatement(pkg, binding, img, None, flat=True)["e"]).max())
        dp = float(np.abs(p[k] - ref["probs"][0]).max())
        print(f"dtype {dtype} image {k} {img.shape[:2]}: 1 - cos(e) {cos:.3e} (gate {gate:.3e}), flat-softmax mutant {flat:.3e}, max|dprob| {dp:.3e}")
        assert cos <= gate and flat > gate
        assert p[k].argmax() == ref["probs"][0].argmax() and dp <= PROB_TOL[dtype]
        lens.append(MD.mean_length(e[k:k + 1], exact["e"]))
        p1, lg1 = pack.forward([img])
        assert np.array_equal(_bits(p1[0]), _bits(p[k])) and np.array_equal(_bits(lg1[0]), _bits(lg[k])) and np.array_equal(_bits(pack.feat_read()[0][0]), _bits(e[k])), k
    assert tuple(pack.launches) == (1 + 7 * 2 + 2 + 9, 1), "one image, tables cached: the patch embedding, 7 per layer, H + 9 for the pooled tail and the head"
    print(f"dtype {dtype}: |e| / |e_restatement| - 1 per image {lens}")
    pack.close()
    # the file's own shape under map_data's gates as they stand, applied as tests/test_gpu_map_head.py applies them: its 17 images as one pack, the
    # worst 1 - cos and the MEAN length over the images
    own = PD.exact_images(17, 56, seed=1)
    pack = binding.PackContext(model, device=0, max_tokens=17 * 16, max_images=17, dtype=dtype, pool_head=True)
    pack.feat_enable(cls=True)
    pack.forward(list(own))
    e17 = pack.feat_read()[0]
    exact = R64.forward64(PD.file_tensors(pkg, MD.fixture_file(pkg)), own, 2)["e"]
    cos, ml = float(MD.one_minus_cos(e17, exact).max()), MD.mean_length(e17, exact)
    print(f"dtype {dtype}: 17 own-shape images: 1 - cos(e) worst {cos:.3e} (gate {MD.cos_gate(dtype):.3e}), mean length {ml:+.3e} (gate {MD.len_gate(dtype):.3e})")
    assert cos <= MD.cos_gate(dtype) and abs(ml) <= MD.len_gate(dtype)
    pack.close(); model.close()

def test_creation(pkg, binding, torch_gpu):
    def code(fn):
        with pytest.raises(binding.VitxError) as ei:
            fn()
        return ei.value.code, str(ei.value)
    cls_model, map_model = binding.Model(XD.fixture_file(pkg, "p16")), binding.Model(MD.fixture_file(pkg))
    mk = lambda m, **kw: binding.PackContext(m, device=0, max_tokens=64, max_images=2, dtype=binding.BF16, **kw)
    assert code(lambda: mk(cls_model, pool_head=1))[0] == binding.ERR_ARG
    assert code(lambda: mk(map_model, pool_head=2))[0] == binding.ERR_ARG
    pack = mk(map_model, pool_head=1)
    for fn in (lambda: pack.attn_enable([0]), lambda: pack.dense_set(np.zeros((3, 128), np.float32)),
               lambda: pack.depth_set(np.zeros((3, 128), np.float32), bins=np.arange(1, 4, dtype=np.float32))):
        c, text = code(fn)
        assert c == binding.ERR_UNSUPPORTED and "attention-pooling" in text
    pack.close(); map_model.close()
    # a class-token pack does not notice the option: an options struct of zeros and the binding's default give the same bytes and bits
    img = XD.images(1, 16, 48)[0]
    a = mk(cls_model)
    h = C.c_void_p()
    opt = binding.PackOptions()
    binding.check(binding.lib().vitx_pack_create(cls_model._h, 0, 64, 2, binding.BF16, C.byref(opt), C.byref(h)), "vitx_pack_create")
    assert binding.lib().vitx_pack_scratch_bytes(h) == a.scratch_bytes
    b = mk(cls_model, pool_head=0)
    assert np.array_equal(_bits(a.forward([img])[0]), _bits(b.forward([img])[0])) and a.scratch_bytes == b.scratch_bytes
    binding.lib().vitx_pack_free(h)
    a.close(); b.close(); cls_model.close()
