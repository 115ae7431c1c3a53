"""Nearest neighbours in a gallery on the MI355X (include/vitx.h "nearest neighbours in a gallery"): the selection kernel bit for bit on given score
matrices under every cut into chunks, the whole op bit for bit on exact data and under the operand types' bound on ordinary data, the vote against
float64 on the engine's own scores, the forward end to end on a CLIP-class, a SigLIP-class and a DINOv2-class micro file, the invariants (batch,
position, cut, bank and gallery together, gallery replaced, off), the profile, the graph cache, and every error.  The restatement is tests/nn_data.py,
pinned to the host's vitx_topk in tests/test_cpu_nn.py."""
import ctypes as C

import numpy as np
import pytest

import nn_data as NN
import prefix_data as PD
import zs_data as Z

pytestmark = pytest.mark.gpu

SENT = -12345.5
TDT = {0: "float16", 1: "bfloat16"}
BIG = 2 ** 31 - 2000
CHUNK = 32768                    # the context's chunk (vitx.h: Gc)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _up(v, m):
    return (v + m - 1) // m * m


def _state(binding, torch, n, k):
    """A running-state buffer full of ones bits: the first launch must initialise it, not read it."""
    return torch.full((binding.op_nn_state_bytes(n, k) // 8,), -1, dtype=torch.int64, device="cuda")


def _pairs(torch, n, k):
    return torch.full((n + 1, k, 2), SENT, dtype=torch.float32, device="cuda")


def _read_pairs(torch, d_pairs, n):
    torch.cuda.synchronize()
    p = d_pairs.cpu().numpy()
    assert (p[n:] == SENT).all(), "the sentinel row behind the n real rows was written"
    return np.ascontiguousarray(p[:n, :, 1]).view(np.int32), np.ascontiguousarray(p[:n, :, 0]).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the selection kernel on given scores
def _feed(binding, torch, d_s, ld, n, cols, step, base, k, d_state, d_pairs):
    """Columns 0 .. cols of d_s [n][ld] in chunks of `step` columns (each chunk its own pointer into the rows), then the final merge."""
    for c0 in range(0, cols, step):
        binding.op_nn_select(d_s.data_ptr() + 4 * c0, ld, n, min(step, cols - c0), base + c0, d_state.data_ptr(), k, c0 == 0)
    binding.op_nn_finish(d_state.data_ptr(), n, k, d_pairs.data_ptr())
    return _read_pairs(torch, d_pairs, n)


@pytest.mark.parametrize("kind", NN.KINDS)
def test_selection_bit_for_bit_under_every_cut(binding, torch_gpu, kind):
    """Every score row is followed by a gap of NaN (ld > cols): a NaN read from there would be selected in the hostile rows' place or change a row of
    equals.  A chunk that does not start at column 0 starts off a 16-byte boundary for most c0 (the per-element path); ld alternates between a
    multiple of 4 (16-byte groups from column 0) and an odd value.  Every case runs twice on the same buffers: the same bits."""
    torch = torch_gpu
    case = 0
    for n in (1, 3, 5):
        for cols in (None, 64, 127, 128, 129, 1000):
            for k in (1, 2, 63, 64):
                c = cols or k
                if k > c:
                    continue
                s = NN.score_rows(kind, n, c, seed=n * 10000 + c)
                want_idx, want_bits = NN.select(s, k)
                if kind == "equal":
                    assert np.array_equal(want_idx, np.tile(np.arange(k), (n, 1)))
                for step in (c, 1, 3, 64, 128, 333):
                    if step > c and step != 333:
                        continue
                    case += 1
                    base = BIG if case & 1 else 0
                    ld = _up(c, 4) + 4 if case & 2 else c + 3
                    buf = np.full((n, ld), np.nan, np.float32); buf[:, :c] = s
                    d_s = torch.from_numpy(buf).cuda()
                    d_state, d_pairs = _state(binding, torch, n, k), _pairs(torch, n, k)
                    idx, bits = _feed(binding, torch, d_s, ld, n, c, step, base, k, d_state, d_pairs)
                    tag = (kind, n, c, k, step, base, ld)
                    assert np.array_equal(idx.astype(np.int64), want_idx.astype(np.int64) + base), tag
                    assert np.array_equal(bits, want_bits), tag
                    assert all(len(set(r)) == k for r in idx), tag
                    idx2, bits2 = _feed(binding, torch, d_s, ld, n, c, step, base, k, d_state, d_pairs)
                    assert np.array_equal(idx2, idx) and np.array_equal(bits2, bits), tag
    assert case > 300


# ------------------------------------------------------------------------------------------------ 2. the op on exact data
def _run_op(binding, torch, z, t, dtype, k, chunk, z_is_operand, z_stride=None, poison=True):
    """vitx_op_nn on z [n][E] (f32, or -- z_is_operand -- values exact in the operand type) and the gallery t [G][E] (exact in the operand type).  The gap
    between z's rows holds NaN; the operand scratch, the whole score scratch (pad rows, pad columns, the bias row) and the state start as NaN, +-inf and
    ones bits.  Returns idx [n][k], score bits [n][k], the operand rows a [n_pad][E] as f32."""
    n, E = z.shape
    G = t.shape[0]
    g_pad, n_pad = _up(G, 128), _up(n, 256)
    zs = z_stride or E
    tdt = getattr(torch, TDT[dtype])
    zb = np.full((n, zs), np.nan, np.float32); zb[:, :E] = z
    d_z = torch.from_numpy(zb).cuda()
    if z_is_operand:
        d_z = d_z.to(tdt)
        assert np.array_equal(d_z.float().cpu().numpy()[:, :E], z), "z must be exact in the operand type"
    tb = np.zeros((g_pad, E), np.float32); tb[:G] = t
    d_t = torch.from_numpy(tb).cuda().to(tdt)
    assert np.array_equal(d_t.float().cpu().numpy(), tb), "the gallery must be exact in the operand type"
    pat = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")], device="cuda")
    if poison:
        d_a = pat.repeat(n_pad * E // 4).reshape(n_pad, E).to(tdt)
        d_acc = pat.repeat((n_pad + 1) * chunk // 4).reshape(n_pad + 1, chunk).clone()
    else:
        d_a = torch.zeros((n_pad, E), dtype=tdt, device="cuda")
        d_acc = torch.zeros((n_pad + 1, chunk), dtype=torch.float32, device="cuda")
    before = d_acc.cpu().numpy().copy()
    d_state, d_pairs = _state(binding, torch, n, k), _pairs(torch, n, k)
    binding.op_nn(dtype, d_z.data_ptr(), zs, z_is_operand, n, d_t.data_ptr(), G, E, k, chunk, d_a.data_ptr(), d_acc.data_ptr(), d_state.data_ptr(), d_pairs.data_ptr())
    idx, bits = _read_pairs(torch, d_pairs, n)
    a, acc = d_a.float().cpu().numpy(), d_acc.cpu().numpy()
    assert not a[n:].any(), "the operand pad rows must be written as zeros"
    assert not acc[n_pad].any(), "the bias row must be zeros"
    assert np.array_equal(_bits(acc[n:n_pad]), _bits(before[n:n_pad])), "pad rows of the score scratch were written"
    last = G - (G - 1) // chunk * chunk               # real columns of the last chunk: everything behind them is as the last full chunk (or the poison) left it
    if G <= chunk:
        assert np.array_equal(_bits(acc[:n, last:]), _bits(before[:n, last:])), "pad columns of the score scratch were written"
    return idx, bits, a


@pytest.mark.parametrize("z_is_operand", [0, 1], ids=["f32", "operand"])
@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
def test_op_bit_for_bit_on_exact_data(binding, torch_gpu, dtype, z_is_operand):
    for n in (1, 3, 129):
        for k in (1, 5, 64):
            for G in (k, 127, 128, 129, 385):
                if k > G:
                    continue
                z, t, a = NN.exact_case(n, G, seed=n * 1000 + G)
                exact, most = NN.exact_conditions(a, t)
                assert exact and most < 2 ** 24                        # every partial sum: an integer / 64 below 2^24
                assert np.array_equal(Z.device_operand(z, dtype), a)
                s = (a.astype(np.float64) @ t.astype(np.float64).T).astype(np.float32)
                want_idx, want_bits = NN.select(s, k)
                for chunk in (128, 256):
                    idx, bits, a_dev = _run_op(binding, torch_gpu, z, t, dtype, k, chunk, z_is_operand, z_stride=80)
                    tag = (n, k, G, chunk)
                    assert np.array_equal(_bits(a_dev[:n]), _bits(a)), (tag, "operand rows")
                    assert np.array_equal(idx, want_idx), tag
                    assert np.array_equal(bits, want_bits), tag
                    assert np.isfinite(bits.view(np.float32)).all() and idx.min() >= 0 and idx.max() < G, tag     # no pad row, no pad column, no poison


# ------------------------------------------------------------------------------------------------ 3. the op on ordinary data
@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("E", [64, 192])
def test_op_on_ordinary_data_under_the_bound(binding, torch_gpu, E, dtype):
    n, G, k, chunk = 37, 1000, 20, 256
    rng = np.random.default_rng(E + dtype)
    z = rng.standard_normal((n, E)).astype(np.float32)
    t = Z.ROUND[dtype](Z.unit_rows(rng.standard_normal((G, E))))
    idx, bits, a_dev = _run_op(binding, torch_gpu, z, t, dtype, k, chunk, 0)
    a = Z.device_operand(z, dtype)
    assert np.array_equal(_bits(a_dev[:n]), _bits(a))
    score = bits.view(np.float32)
    s64 = a.astype(np.float64) @ t.astype(np.float64).T
    bound = Z.COS_BOUND[dtype](E)
    rows = np.arange(n)[:, None]
    err = float(np.abs(score - s64[rows, idx]).max())
    ky = (NN.rank(score).astype(np.uint64) << np.uint64(32)) | (~idx.view(np.uint32)).astype(np.uint64)
    left = s64.copy(); left[rows, idx] = -np.inf
    over = float((left.max(1) - score[:, -1]).max())
    print(f"E {E} dtype {dtype}: max |score - float64| {err:.3e} (bound {bound:.3e}); best row left out minus the k-th score {over:.3e} (allowed {2 * bound:.3e})")
    assert err <= bound
    assert (ky[:, :-1] > ky[:, 1:]).all(), "the list is not sorted by the (score, index) key"
    assert all(len(set(r)) == k for r in idx) and idx.min() >= 0 and idx.max() < G
    assert over <= 2 * bound


# ------------------------------------------------------------------------------------------------ 4. the vote
@pytest.mark.parametrize("T", [0.07, 1.0])
@pytest.mark.parametrize("n_labels", [1, 2, 1000])
def test_vote(binding, torch_gpu, n_labels, T):
    """Scores within 2 of each other at T = 0.07 (|q| <= 28.6), within 30 at T = 1: |score_j - score_0| / T <= 32.  The tolerance: expf's argument
    carries (|q| + 2) 2^-23 from the subtraction and the division, the k serial adds k 2^-24: 7.9e-6 at |q| <= 32 and k <= 64."""
    torch = torch_gpu
    n, G = 4, 300
    rng = np.random.default_rng(n_labels)
    s = (rng.random((n, G)) * (2.0 if T < 1 else 30.0) - 1.0).astype(np.float32)
    s[1, :70] = s[1, 0]                                   # ties among the best of one row
    labels = rng.integers(0, n_labels, G).astype(np.int32)
    d_s, d_lab = torch.from_numpy(s).cuda(), torch.from_numpy(labels).cuda()
    for k in (1, 20, 64):
        d_state, d_pairs = _state(binding, torch, n, k), _pairs(torch, n, k)
        d_vote = torch.full((n + 1, n_labels), SENT, dtype=torch.float32, device="cuda")
        binding.op_nn_select(d_s.data_ptr(), G, n, G, 0, d_state.data_ptr(), k, True)
        binding.op_nn_finish(d_state.data_ptr(), n, k, d_pairs.data_ptr(), d_lab.data_ptr(), n_labels, T, d_vote.data_ptr())
        idx, bits = _read_pairs(torch, d_pairs, n)
        want_idx, want_bits = NN.select(s, k)
        assert np.array_equal(idx, want_idx) and np.array_equal(bits, want_bits)
        v = d_vote.cpu().numpy()
        assert (v[n:] == SENT).all()
        v = v[:n]
        score = bits.view(np.float32)
        assert np.abs((score - score[:, :1]) / np.float32(T)).max() <= 32
        want = NN.vote64(score, idx, labels, n_labels, T)
        hit = want > 0
        assert ((v == 0) == ~hit).all(), "classes without a neighbour must be exactly 0 (and only those)"
        rel = float(np.abs(v[hit] / want[hit] - 1).max())
        tot = float(np.abs(v.astype(np.float64).sum(1) - 1).max())
        print(f"n_labels {n_labels} T {T} k {k}: max relative error {rel:.3e}, max |row sum - 1| {tot:.3e}")
        assert rel <= 1e-5 and tot <= 1e-6
        if k == 1:
            onehot = np.zeros((n, n_labels), np.float32); onehot[np.arange(n), labels[idx[:, 0]]] = 1
            assert np.array_equal(_bits(v), _bits(onehot))


# ------------------------------------------------------------------------------------------------ 5. end to end
NAME = "vit_micro_patch14_56"
N_GALLERY, N_LABELS, K = 40, 5, 5
CASES = [("clip", "logits"), ("clip", "embed"), ("siglip", "embed"), ("dinov2", "embed")]


def _model_file(pkg, family):
    """clip / siglip: the micro files of zs_data; dinov2: the register + cls-mean-head micro file of tests/test_gpu_registers.py (arch_data's own
    DINOv2 fixture has the pooled head but no registers)."""
    if family == "dinov2":
        return pkg.synth.cached_synthetic(NAME, head_scale=4.0, registers=4, head_pool=1)
    return Z.model_file(pkg, family)


def _gallery_images():
    return PD.exact_images(N_GALLERY, 56, seed=7)


def _forward_z(binding, ctx, source, imgs):
    """One forward: (z = the source embedding of that very forward as the op takes it, is_operand, probs, logits).  NN_LOGITS: the logits.  NN_EMBED:
    RNE of the last layer's VITX_FEAT_CLS (| VITX_FEAT_MEAN for the cls + mean head), which the header pins to the head operand bit for bit."""
    if source == binding.NN_LOGITS:
        p, lg = ctx.forward(imgs, want_logits=True)
        return lg, 0, p, lg
    pooled = ctx.model.head_pool == binding.POOL_CLS_MEAN
    ctx.feat_enable(cls=True, mean=pooled)
    p, lg = ctx.forward(imgs, want_logits=True)
    f = ctx.feat_read(imgs.shape[0])[ctx.model.hparams.num_hidden_layers - 1]
    ctx.feat_disable()
    z = np.concatenate([f["cls"], f["mean"]], axis=1) if pooled else f["cls"]
    return binding.round_operand(z, ctx.dtype), 1, p, lg


def _op_on(binding, torch, z, is_operand, gallery, dtype, k, chunk=CHUNK):
    t = Z.ROUND[dtype](gallery)
    return _run_op(binding, torch, np.ascontiguousarray(z, np.float32), t, dtype, k, chunk, is_operand, poison=False)[:2]


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("family,src", CASES)
def test_forward_end_to_end(pkg, binding, torch_gpu, family, src, dtype):
    """The result of a forward with a gallery set equals, bit for bit, vitx_op_nn applied to the z of the same forward, and the vote the float64 vote of
    the engine's own scores.  Self-retrieval at rank 0 is NOT asserted: the micro models map their images to nearly one embedding (mutual cosines
    >= 0.9997 for the CLIP-class file, zs_data.bank), so no margin above COS_BOUND between an image and every other one has been established."""
    source = binding.NN_LOGITS if src == "logits" else binding.NN_EMBED
    model = binding.Model(_model_file(pkg, family))
    ctx = binding.Context(model, device=0, max_batch=Z.N_IMAGES, dtype=dtype)
    assert len(ctx.split(Z.N_IMAGES)) == 2
    D, C_ = model.hparams.hidden_size, model.num_classes
    E = ctx.nn_width(source)
    assert E == (C_ if src == "logits" else (2 * D if family == "dinov2" else D))
    gallery = binding.nn_gallery(ctx, _gallery_images(), source)
    assert gallery.shape == (N_GALLERY, E) and np.abs(np.linalg.norm(gallery.astype(np.float64), axis=1) - 1).max() < 1e-6
    labels = (np.arange(N_GALLERY) % N_LABELS).astype(np.int32)
    ctx.nn_set(gallery, K, source, labels, N_LABELS, 0.07)
    L = binding.lib()
    assert (L.vitx_nn_rows(ctx._h), L.vitx_nn_k(ctx._h), L.vitx_nn_labels(ctx._h), L.vitx_nn_images(ctx._h)) == (N_GALLERY, K, N_LABELS, 0)
    imgs = Z.images()
    n = imgs.shape[0]
    z, is_op, _, _ = _forward_z(binding, ctx, source, imgs)
    idx, score, vote = ctx.nn_read(n)
    want_idx, want_bits = _op_on(binding, torch_gpu, z, is_op, gallery, dtype, K)
    assert np.array_equal(idx, want_idx) and np.array_equal(_bits(score), want_bits)
    want_vote = NN.vote64(score, idx, labels, N_LABELS, 0.07)
    hit = want_vote > 0
    assert ((vote == 0) == ~hit).all() and np.abs(vote[hit] / want_vote[hit] - 1).max() <= 1e-5
    # the device buffer is what read returns: [capacity][k] {score, index}
    ptr, k_dev = ctx.nn_device()
    dev = np.empty((n, K, 2), np.float32)
    assert C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(dev.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), dev.nbytes, 2) == 0
    assert k_dev == K and np.array_equal(_bits(dev[:, :, 0]), _bits(score)) and np.array_equal(np.ascontiguousarray(dev[:, :, 1]).view(np.int32), idx)
    if (family, src) == ("clip", "logits"):
        # a gallery of more than one chunk through the forward: the same bits as the op at a chunk of 256 rows
        big = Z.unit_rows(np.random.default_rng(11).standard_normal((CHUNK + 8, E)))
        ctx.nn_set(big, 20, source)
        z, is_op, _, _ = _forward_z(binding, ctx, source, imgs)
        idx, score, vote = ctx.nn_read(n)
        want_idx, want_bits = _op_on(binding, torch_gpu, z, is_op, big, dtype, 20, chunk=256)
        assert vote is None and np.array_equal(idx, want_idx) and np.array_equal(_bits(score), want_bits)
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 6. invariants and plumbing
def test_invariants(pkg, binding, torch_gpu):
    L = binding.lib()
    imgs = Z.images()
    n = Z.N_IMAGES
    model = binding.Model(Z.model_file(pkg, "clip"))
    ctx = binding.Context(model, device=0, max_batch=n, dtype=1)
    cut = ctx.split(n)
    assert len(cut) == 2
    src = binding.NN_EMBED
    E = ctx.nn_width(src)
    gallery = binding.nn_gallery(ctx, _gallery_images(), src)
    labels = (np.arange(N_GALLERY) % N_LABELS).astype(np.int32)
    assert ctx.nn_device() == (0, 0) and ctx.nn_scratch_bytes() == 0
    plain = ctx.forward(imgs, want_logits=True)

    def run(x):
        p, lg = ctx.forward(x, want_logits=True)
        return ctx.nn_read(x.shape[0]) + (p, lg)

    ctx.nn_set(gallery, K, src, labels, N_LABELS, 0.07)
    idx, score, vote, p, lg = run(imgs)
    assert np.array_equal(_bits(p), _bits(plain[0])) and np.array_equal(_bits(lg), _bits(plain[1]))       # the forward's own outputs keep their bits
    # batch 1 at both ends and on both sides of the cut; a batch of 7 with the image in position 3
    for i in sorted({0, cut[0] - 1, cut[0], n - 1}):
        i1, s1, v1, _, _ = run(imgs[i:i + 1])
        assert np.array_equal(i1, idx[i:i + 1]) and np.array_equal(_bits(s1), _bits(score[i:i + 1])) and np.array_equal(_bits(v1), _bits(vote[i:i + 1])), i
        others = [j for j in range(n) if j != i][:6]
        order = others[:3] + [i] + others[3:]
        i7, s7, v7, _, _ = run(imgs[order])
        assert np.array_equal(i7[3], idx[i]) and np.array_equal(_bits(s7[3]), _bits(score[i])) and np.array_equal(_bits(v7[3]), _bits(vote[i])), i
    # off: the buffers are gone, the forward's bits stay; on again: the same result
    ctx.nn_set(None)
    assert ctx.nn_device() == (0, 0) and ctx.nn_scratch_bytes() == 0 and L.vitx_nn_rows(ctx._h) == 0 and L.vitx_nn_images(ctx._h) == 0
    off = ctx.forward(imgs, want_logits=True)
    assert np.array_equal(_bits(off[0]), _bits(plain[0])) and np.array_equal(_bits(off[1]), _bits(plain[1]))
    with pytest.raises(binding.VitxError) as ei:
        ctx.nn_read()
    assert ei.value.code == binding.ERR_ARG
    ctx.nn_set(gallery, K, src, labels, N_LABELS, 0.07)
    again = run(imgs)
    assert np.array_equal(again[0], idx) and np.array_equal(_bits(again[1]), _bits(score)) and np.array_equal(_bits(again[2]), _bits(vote))
    assert np.array_equal(_bits(again[3]), _bits(plain[0])) and np.array_equal(_bits(again[4]), _bits(plain[1]))
    # a bank and a gallery together: each equals its solo result
    bank = Z.unit_rows(np.random.default_rng(3).standard_normal((24, Z.CLIP_E)))
    ctx.zeroshot_set(bank, Z.SOFTMAX, 100.0, 0.0)
    both = run(imgs)
    zp_both = ctx.zeroshot_read(n)
    ctx.nn_set(None)
    ctx.forward(imgs)
    zp_solo = ctx.zeroshot_read(n)
    ctx.zeroshot_set(None)
    assert np.array_equal(_bits(zp_both), _bits(zp_solo))
    assert np.array_equal(both[0], idx) and np.array_equal(_bits(both[1]), _bits(score)) and np.array_equal(_bits(both[2]), _bits(vote))
    assert np.array_equal(_bits(both[3]), _bits(plain[0]))
    # the gallery replaced: another G, k and source, no labels -- and the scratch does not depend on G
    g200 = Z.unit_rows(np.random.default_rng(4).standard_normal((200, Z.CLIP_E)))
    g5000 = Z.unit_rows(np.random.default_rng(5).standard_normal((5000, Z.CLIP_E)))
    ctx.nn_set(g200, 9, binding.NN_LOGITS)
    b200 = ctx.nn_scratch_bytes()
    i2, s2, v2, _, _ = run(imgs)
    assert i2.shape == (n, 9) and v2 is None and i2.max() < 200 and (L.vitx_nn_rows(ctx._h), L.vitx_nn_k(ctx._h), L.vitx_nn_labels(ctx._h)) == (200, 9, 0)
    w_idx, w_bits = _op_on(binding, torch_gpu, plain[1], 0, g200, 1, 9)
    assert np.array_equal(i2, w_idx) and np.array_equal(_bits(s2), w_bits)
    ctx.nn_set(g5000, 9, binding.NN_LOGITS)
    assert ctx.nn_scratch_bytes() == b200 > 0 and L.vitx_nn_images(ctx._h) == 0
    i5, _, _, _, _ = run(imgs)
    assert i5.max() >= 200
    # the profile: one operand launch, two per chunk, one final merge, per sub-batch; nothing while off
    ctx.nn_set(gallery, K, src, labels, N_LABELS, 0.07)
    ctx.profile_enable(True)
    ctx.forward(imgs)
    pr = {e["name"]: e for e in ctx.profile_read()}
    assert pr["nn"]["launches"] == (2 * 1 + 1 + 1) * len(cut)
    ctx.nn_set(Z.unit_rows(np.random.default_rng(6).standard_normal((CHUNK + 1, E))), K, src)
    ctx.forward(imgs)
    pr = {e["name"]: e for e in ctx.profile_read()}
    assert pr["nn"]["launches"] == (2 * 2 + 1 + 1) * len(cut)
    ctx.nn_set(None)
    ctx.forward(imgs)
    assert "nn" not in [e["name"] for e in ctx.profile_read()]
    ctx.profile_enable(False)
    ctx.close()
    # one stream: the same bits as two
    ctx1 = binding.Context(model, device=0, max_batch=n, dtype=1, streams=1)
    assert len(ctx1.split(n)) == 1
    ctx1.nn_set(gallery, K, src, labels, N_LABELS, 0.07)
    ctx1.forward(imgs)
    i1s, s1s, v1s = ctx1.nn_read(n)
    assert np.array_equal(i1s, idx) and np.array_equal(_bits(s1s), _bits(score)) and np.array_equal(_bits(v1s), _bits(vote))
    ctx1.close(); model.close()


def test_graph_cache_is_bypassed_while_a_gallery_is_set(pkg, binding, torch_gpu):
    imgs = Z.images()[:5]
    model = binding.Model(Z.model_file(pkg, "clip"))
    ctx = binding.Context(model, device=0, max_batch=5, dtype=1, graph=1)
    ctx.nn_set(Z.unit_rows(np.random.default_rng(8).standard_normal((50, Z.CLIP_E))), 3, binding.NN_LOGITS)
    outs = [ctx.forward(imgs) for _ in range(4)]
    assert ctx.graph_launches() == 0
    idx, score, _ = ctx.nn_read(5)
    ctx.nn_set(None)
    again = [ctx.forward(imgs) for _ in range(4)]
    assert ctx.graph_launches() >= 1
    for o in outs + again:
        assert np.array_equal(_bits(o), _bits(outs[0]))
    assert np.isfinite(score).all() and idx.min() >= 0 and idx.max() < 50
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors(pkg, binding, torch_gpu):
    L = binding.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    model = binding.Model(Z.model_file(pkg, "siglip"))
    ctx = binding.Context(model, device=0, max_batch=4, dtype=1)
    h = ctx._h
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    S = binding.NN_EMBED
    E = ctx.nn_width(S)
    G = 12
    t = Z.unit_rows(np.random.default_rng(1).standard_normal((G, E)))
    lab = (np.arange(G) % 3).astype(np.int32)
    tp, lp = t.ctypes.data_as(fp), lab.ctypes.data_as(ip)
    assert ctx.nn_width(7) == 0 and ctx.nn_width(binding.NN_LOGITS) == model.num_classes
    assert L.vitx_nn_set(h, None, 3, E, 1, S, None, 0, 0.07) == A                    # NULL gallery with G > 0
    assert L.vitx_nn_set(h, tp, G, E, 0, S, None, 0, 0.07) == A                      # k < 1
    assert L.vitx_nn_set(h, tp, G, E, G + 1, S, None, 0, 0.07) == A                  # k > G
    assert L.vitx_nn_set(h, tp, 0, E, 1, S, None, 0, 0.07) == A
    assert L.vitx_nn_set(h, tp, G, 64, 1, S, None, 0, 0.07) == A                     # not the source's width (128)
    assert L.vitx_nn_set(h, tp, G, E, 1, 2, None, 0, 0.07) == A and L.vitx_nn_set(h, tp, G, E, 1, -1, None, 0, 0.07) == A      # unknown source
    for bad in (np.nan, np.inf):
        tb = t.copy(); tb[G - 1, E - 1] = bad
        assert L.vitx_nn_set(h, tb.ctypes.data_as(fp), G, E, 1, S, None, 0, 0.07) == A
        assert "[%d][%d]" % (G - 1, E - 1) in L.vitx_last_error().decode()
    for bad in (-1, 3):
        lb = lab.copy(); lb[5] = bad
        assert L.vitx_nn_set(h, tp, G, E, 1, S, lb.ctypes.data_as(ip), 3, 0.07) == A
    assert L.vitx_nn_set(h, tp, G, E, 1, S, lp, 0, 0.07) == A                        # labels with n_labels < 1
    for bad in (0.0, -0.07, float("inf"), float("nan")):
        assert L.vitx_nn_set(h, tp, G, E, 1, S, lp, 3, bad) == A                     # labels with a temperature that is not finite and positive
    t65 = Z.unit_rows(np.random.default_rng(2).standard_normal((70, E)))
    assert L.vitx_nn_set(h, t65.ctypes.data_as(fp), 70, E, 65, S, None, 0, 0.07) == U     # k > 64
    assert L.vitx_nn_set(h, tp, 2 ** 31 - 128, E, 1, S, None, 0, 0.07) == U               # refused before the gallery is read
    assert L.vitx_nn_rows(h) == 0 and L.vitx_nn_device(h) is None and L.vitx_nn_scratch_bytes(h) == 0       # nothing above left a gallery behind
    idx = np.empty((4, 2), np.int32); sc = np.empty((4, 2), np.float32); vt = np.empty((4, 3), np.float32)
    assert L.vitx_nn_read(h, idx.ctypes.data_as(ip), sc.ctypes.data_as(fp), None) == A          # off
    ctx.nn_set(t, 2, S)
    assert L.vitx_nn_read(h, idx.ctypes.data_as(ip), sc.ctypes.data_as(fp), None) == A          # before any forward with the gallery set
    ctx.forward(Z.images()[:3])
    assert L.vitx_nn_images(h) == 3
    assert L.vitx_nn_read(h, None, sc.ctypes.data_as(fp), None) == A and L.vitx_nn_read(h, idx.ctypes.data_as(ip), None, None) == A
    assert L.vitx_nn_read(h, idx.ctypes.data_as(ip), sc.ctypes.data_as(fp), vt.ctypes.data_as(fp)) == A     # a vote without labels
    assert L.vitx_nn_read(h, idx.ctypes.data_as(ip), sc.ctypes.data_as(fp), None) == 0
    ctx.close(); model.close()
    # a width that is not a multiple of 64: arch_data's CLIP-class file has 10 "classes"
    import arch_data as AD
    m10 = binding.Model(AD.fixture_file(pkg, "clip"))
    c10 = binding.Context(m10, device=0, max_batch=2, dtype=1)
    with pytest.raises(binding.VitxError) as ei:
        c10.nn_set(Z.unit_rows(np.random.default_rng(1).standard_normal((3, 10))), 1, binding.NN_LOGITS)
    assert ei.value.code == U and "multiple of 64" in str(ei.value)
    c10.close(); m10.close()
    # a ViTSTR context
    st = binding.Model(pkg.synth.cached_synthetic("vitstr_tiny_patch16_224", head_scale=4.0))
    cs = binding.Context(st, device=0, max_batch=1, dtype=0)
    with pytest.raises(binding.VitxError) as ei:
        cs.nn_set(Z.unit_rows(np.random.default_rng(1).standard_normal((3, cs.nn_width(binding.NN_EMBED)))), 1, binding.NN_EMBED)
    assert ei.value.code == U and "ViTSTR" in str(ei.value)
    cs.close(); st.close()


def test_nearest_neighbours_take_one_pass(pkg, binding, torch_gpu):
    """A forward of more images than one pass of the kernels takes is refused while a gallery is set, before anything runs."""
    torch = torch_gpu
    L = binding.lib()
    name = "vit_micro_patch8_224"                        # 785 tokens: the F16 parity mode's window holds 3339 images
    model = binding.Model(Z.clip_file(pkg, name=name))
    big = 3400
    ctx = binding.Context(model, device=0, max_batch=big, dtype=binding.F16, streams=1)
    limit = ctx.split(big)[0]
    assert limit < big
    ctx.nn_set(Z.unit_rows(np.random.default_rng(2).standard_normal((5, Z.CLIP_E))), 2, binding.NN_LOGITS)
    n = limit + 1
    x = torch.zeros((n, 224, 224, 3), dtype=torch.float32, device="cuda")            # sized for the call: memory-safe even if the check were gone
    p = torch.zeros((n, model.num_classes), dtype=torch.float32, device="cuda")
    assert L.vitx_forward_device(ctx._h, x.data_ptr(), n, p.data_ptr(), None, None) == binding.ERR_ARG
    assert "one pass" in L.vitx_last_error().decode() and L.vitx_nn_images(ctx._h) == 0
    ctx.close(); model.close()


def test_a_refused_set_leaves_the_gallery_in_place(pkg, binding, torch_gpu):
    """A vitx_nn_set that is refused for its arguments (a NaN in the gallery) leaves the gallery that was set: the next forward gives the same bits."""
    L = binding.lib()
    imgs = Z.images()[:5]
    model = binding.Model(Z.model_file(pkg, "clip"))
    ctx = binding.Context(model, device=0, max_batch=5, dtype=1)
    g = Z.unit_rows(np.random.default_rng(8).standard_normal((50, Z.CLIP_E)))
    labels = np.arange(50, dtype=np.int32) % 4
    ctx.nn_set(g, 3, binding.NN_LOGITS, labels, 4)
    ctx.forward(imgs)
    idx, score, vote = ctx.nn_read(5)
    bad = g.copy(); bad[7, 1] = np.nan
    with pytest.raises(binding.VitxError) as ei:
        ctx.nn_set(bad, 3, binding.NN_LOGITS, labels, 4)
    assert ei.value.code == binding.ERR_ARG
    ctx.forward(imgs)
    assert L.vitx_nn_images(ctx._h) == 5 and L.vitx_nn_rows(ctx._h) == 50
    idx2, score2, vote2 = ctx.nn_read(5)
    assert np.array_equal(idx2, idx) and np.array_equal(_bits(score2), _bits(score)) and np.array_equal(_bits(vote2), _bits(vote))
    ctx.close(); model.close()
