"""Attention maps on packed contexts, on the GPU (include/vitx.h "packed batches"): the four packed map kernels against the fixed-shape entry points
on every image alone, bit for bit (one body, csrc/attention_map_tile.h: no tolerance); position and neighbours; a uniform pack against the
fixed-shape launch; end to end against a rectangular context and against packs of one image; what maps leave alone; refusals; stream order; the CLI.

Every output buffer carries sentinel floats behind its last image (and between the two matrix arenas) that must keep their bits."""
import os

import numpy as np
import pytest

import pack_attn_data as AD
import pack_data as KD
import rect_data as XD
import test_gpu_stream_order as SO

pytestmark = pytest.mark.gpu

SENT = -12345.5
TAIL = 70
L = 2                      # layers of the micro fixtures


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _tdt(torch, dtype):
    return torch.float16 if dtype == 0 else torch.bfloat16


def _qkv(torch, dtype, rows, Dm, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn((rows, 3 * Dm), device="cuda", generator=g) * 0.8).to(_tdt(torch, dtype))


def _sent(torch, floats):
    return torch.full((floats + TAIL,), SENT, dtype=torch.float32, device="cuda")


def _same(torch, got, want, what):
    g, w = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} floats differ, the first at {int(bad[0])}: got {float(got.flatten()[int(bad[0])])!r}, "
                             f"expected {float(want.flatten()[int(bad[0])])!r}")


class Packed:
    """Every output of the packed entry points on one pack of three QKV buffers (three layers' worth): the class maps of the last, the head mean and
    the factor of the first, the chain A2 <- A2 . A1, A3 <- A3 . A2, and the row with and without r.  Arenas: [a | TAIL | r | TAIL] in one tensor."""

    def __init__(self, binding, torch, dtype, tokens, Dm, H, qkvs):
        self.row0 = AD.row0_of_tokens(tokens)
        self.sq0 = AD.tables(self.row0)[1]
        rows, sq = int(self.row0[-1]), int(self.sq0[-1])
        q1, q2, q3 = qkvs
        B = binding
        self.cls, self.mean, self.a3 = _sent(torch, rows * H), _sent(torch, sq), _sent(torch, sq)
        self.arena = _sent(torch, 2 * sq + TAIL)
        self.a1, self.a2 = self.arena[:sq], self.arena[sq + TAIL:2 * sq + TAIL]
        self.row, self.row_w = _sent(torch, rows), _sent(torch, rows)
        B.op_attention_map_packed(dtype, q3.data_ptr(), self.cls.data_ptr(), 0, self.row0, Dm, H)
        B.op_attention_map_packed(dtype, q1.data_ptr(), 0, self.mean.data_ptr(), self.row0, Dm, H)
        B.op_attention_map_packed(dtype, q1.data_ptr(), 0, self.a1.data_ptr(), self.row0, Dm, H, half_identity=True)
        B.op_attention_map_packed(dtype, q2.data_ptr(), 0, self.a2.data_ptr(), self.row0, Dm, H, half_identity=True)
        B.op_attention_map_packed(dtype, q3.data_ptr(), 0, self.a3.data_ptr(), self.row0, Dm, H, half_identity=True)
        self.factor = self.a1.clone()
        B.op_rollout_step_packed(self.a2.data_ptr(), self.a1.data_ptr(), self.row0)
        self.step1 = self.a2.clone()
        B.op_rollout_step_packed(self.a3.data_ptr(), self.a2.data_ptr(), self.row0)
        B.op_rollout_row_packed(self.cls.data_ptr(), self.a2.data_ptr(), self.row.data_ptr(), self.row0, H)
        B.op_rollout_row_packed(self.cls.data_ptr(), 0, self.row_w.data_ptr(), self.row0, H)
        torch.cuda.synchronize()
        self.H, self.sq, self.rows = H, sq, rows

    def image(self, i):
        """{name: the floats of image i}"""
        r0, r1, s0, s1, H = int(self.row0[i]), int(self.row0[i + 1]), int(self.sq0[i]), int(self.sq0[i + 1]), self.H
        return {"class maps": self.cls[r0 * H:r1 * H], "head mean": self.mean[s0:s1], "factor": self.factor[s0:s1], "step 1": self.step1[s0:s1],
                "step 2": self.a3[s0:s1], "row": self.row[r0:r1], "row without r": self.row_w[r0:r1]}

    def sentinels_intact(self, torch):
        sq, rows, H = self.sq, self.rows, self.H
        for name, t in (("class maps", self.cls[rows * H:]), ("head mean", self.mean[sq:]), ("step 2", self.a3[sq:]), ("between the arenas", self.arena[sq:sq + TAIL]),
                        ("behind the arenas", self.arena[2 * sq + TAIL:]), ("row", self.row[rows:]), ("row without r", self.row_w[rows:])):
            assert bool((t == SENT).all()), f"the sentinel floats {name} were written"


def _fixed(binding, torch, dtype, n, N, Dm, H, qkvs):
    """The same outputs by the fixed-shape entry points on n images of N tokens (qkvs: [n * N][3 D] each), as {name: [n][...] floats}."""
    B = binding
    q1, q2, q3 = (q.contiguous() for q in qkvs)
    f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    cls, mean, a1, a2, a3, row, row_w = f(n, H * N), f(n, N * N), f(n, N * N), f(n, N * N), f(n, N * N), f(n, N), f(n, N)
    B.op_attention_map(dtype, q3.data_ptr(), cls.data_ptr(), 0, n, N, Dm, H)
    B.op_attention_map(dtype, q1.data_ptr(), 0, mean.data_ptr(), n, N, Dm, H)
    B.op_rollout_factor(dtype, q1.data_ptr(), a1.data_ptr(), n, N, Dm, H)
    B.op_rollout_factor(dtype, q2.data_ptr(), a2.data_ptr(), n, N, Dm, H)
    B.op_rollout_factor(dtype, q3.data_ptr(), a3.data_ptr(), n, N, Dm, H)
    factor = a1.clone()
    B.op_rollout_step(a2.data_ptr(), a1.data_ptr(), n, N)
    step1 = a2.clone()
    B.op_rollout_step(a3.data_ptr(), a2.data_ptr(), n, N)
    B.op_rollout_row(cls.data_ptr(), H * N, a2.data_ptr(), row.data_ptr(), N, n, N, H)
    B.op_rollout_row(cls.data_ptr(), H * N, 0, row_w.data_ptr(), N, n, N, H)
    torch.cuda.synchronize()
    return {"class maps": cls, "head mean": mean, "factor": factor, "step 1": step1, "step 2": a3, "row": row, "row without r": row_w}


# ------------------------------------------------------------------------------------------------ 1. one packed launch against the fixed-shape ops
@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("Dm,H", AD.SHAPES, ids=[f"hd{d // h}" for d, h in AD.SHAPES])
def test_one_packed_launch_is_the_fixed_shape_op_per_image(binding, torch_gpu, Dm, H, dtype):
    """pack_attn_data.TOKENS in one pack.  Class maps, head mean, factor, two chained steps, the row with and without r: each image's floats are those
    of the fixed-shape entry point on that image alone (n_img = 1), bit for bit."""
    torch = torch_gpu
    rows = sum(AD.TOKENS)
    qkvs = [_qkv(torch, dtype, rows, Dm, seed=Dm + H + 10 * k + dtype) for k in range(3)]
    pk = Packed(binding, torch, dtype, AD.TOKENS, Dm, H, qkvs)
    pk.sentinels_intact(torch)
    for i, N in enumerate(AD.TOKENS):
        r0, r1 = int(pk.row0[i]), int(pk.row0[i + 1])
        want = _fixed(binding, torch, dtype, 1, N, Dm, H, [q[r0:r1] for q in qkvs])
        for name, got in pk.image(i).items():
            _same(torch, got, want[name][0], f"image {i} (N {N}): {name}")
            assert bool(torch.isfinite(got).all()), (i, name)


# ------------------------------------------------------------------------------------------------ 2. neighbours and position
@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
def test_position_and_neighbours_do_not_reach_an_image(binding, torch_gpu, dtype):
    """One image of 65 tokens (two key tiles, five row blocks, the last of one row) first, in the middle and last, beside different neighbours (the
    widest gives the launch NT = 1, 4 or 16); then the neighbours' QKV rows become NaN and 1e30.  Its seven outputs keep their bits throughout."""
    torch = torch_gpu
    Dm, H, N = 128, 4, 65
    own = [_qkv(torch, dtype, N, Dm, seed=40 + k) for k in range(3)]
    want = _fixed(binding, torch, dtype, 1, N, Dm, H, own)
    for where, before, after in (("first", (), (17, 1)), ("middle", (257, 15), (1, 64)), ("last", (16, 1024, 2), ())):
        tokens = tuple(before) + (N,) + tuple(after)
        at, i = sum(before), len(before)
        for poison in (None, float("nan"), 1e30):
            qkvs = []
            for k in range(3):
                q = _qkv(torch, dtype, sum(tokens), Dm, seed=50 + k)
                if poison is not None:
                    q[:] = poison
                q[at:at + N] = own[k]
                qkvs.append(q)
            pk = Packed(binding, torch, dtype, tokens, Dm, H, qkvs)
            pk.sentinels_intact(torch)
            for name, got in pk.image(i).items():
                _same(torch, got, want[name][0], f"{where}, neighbours {poison}: {name}")


# ------------------------------------------------------------------------------------------------ 3. a uniform pack is the fixed-shape launch
@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("N", [197, 50])
def test_uniform_pack_is_the_fixed_shape_launch(binding, torch_gpu, N, dtype):
    """n = 3 images of one token count: every output of the packed launches is the fixed-shape launch's over the 3 images, whole buffers, bit for bit."""
    torch = torch_gpu
    Dm, H, n = 192, 4, 3
    qkvs = [_qkv(torch, dtype, n * N, Dm, seed=60 + k + N) for k in range(3)]
    pk = Packed(binding, torch, dtype, (N,) * n, Dm, H, qkvs)
    pk.sentinels_intact(torch)
    want = _fixed(binding, torch, dtype, n, N, Dm, H, qkvs)
    for i in range(n):
        for name, got in pk.image(i).items():
            _same(torch, got, want[name][i], f"image {i}: {name}")


# ------------------------------------------------------------------------------------------------ 4. end to end
E2E = ("p16h4", "p14r4h4", "p14ropeh4")


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", E2E)
def test_uniform_pack_maps_are_the_rect_contexts(pkg, binding, torch_gpu, kind, dtype):
    """5 images of one shape at head dim 32 (both paths run the generic attention and hold the same q, k): the class maps of both layers and the rollout
    row of the packed context are those of a rectangular context's attn_read, bit for bit."""
    model = binding.Model(KD.variant_file(pkg, kind))
    shape = KD.UNIFORM_SHAPE[model.hparams.patch_size]
    n = 5
    imgs = XD.images(n, *shape)
    ctx = binding.Context(model, device=0, max_batch=n, dtype=dtype, img_shape=shape, last_layer_all_rows=1)
    ctx.attn_enable(None, rollout=True)
    p, _ = ctx.forward(imgs, want_logits=True)
    cls, roll = ctx.attn_read(n)
    pack = binding.PackContext(model, device=0, max_tokens=n * ctx.tokens, max_images=n, dtype=dtype)
    pack.attn_enable(None, rollout=True)
    pp, _ = pack.forward(list(imgs))
    maps = pack.attn_read()
    assert np.array_equal(_bits(pp), _bits(p)) and len(maps) == n
    for i, (c, r) in enumerate(maps):
        assert c.shape == cls[i].shape and np.isfinite(c).all() and np.isfinite(r).all()
        assert np.array_equal(_bits(c), _bits(cls[i])), (i, "class maps")
        assert np.array_equal(_bits(r), _bits(roll[i])), (i, "rollout")
        assert np.allclose(r.sum(), 1.0, atol=1e-4) and pack.attn_grid(i, r).shape == ctx.grid_hw
    ctx.close(); pack.close(); model.close()


def _head(model):
    rng = np.random.default_rng(13)
    return (rng.standard_normal((5, model.hparams.hidden_size)) * 0.5).astype(np.float32), rng.standard_normal(5).astype(np.float32)


def _forward_all(pack, imgs, dense):
    p, lg = pack.forward(imgs)
    cls, tok = pack.feat_read()
    out = [p, lg, cls] + list(tok)
    if dense:
        out += list(pack.dense_read()[0])
    return out


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", E2E)
def test_mixed_pack_maps_and_what_maps_leave_alone(pkg, binding, torch_gpu, kind, dtype):
    """pack_data.mixed_shapes in one forward.  Each image's maps are those of a pack of that image alone; probabilities, logits, features and dense
    labels have the bits they have with maps off; launches and scratch_bytes return to their values after disabling; with maps on the forward adds
    pack_attn_data.map_launches launches."""
    model = binding.Model(KD.variant_file(pkg, kind))
    shapes = KD.mixed_shapes(model.hparams.patch_size)
    imgs = KD.pack_of(shapes)
    pack = binding.PackContext(model, device=0, max_tokens=256, max_images=8, dtype=dtype)
    pack.feat_enable(cls=True, tokens=True)
    pack.dense_set(*_head(model), None)
    off = _forward_all(pack, imgs, True)                 # (the first call builds the grids' tables: its launch count is not the steady one)
    off = _forward_all(pack, imgs, True)
    base, scratch = pack.launches, pack.scratch_bytes
    assert pack.attn_device == 0
    for layers, rollout in (([L - 1], False), ([0, 1], False), ([], True), ([1], True), ([0], True), (None, True)):
        pack.attn_enable(layers, rollout=rollout)
        assert pack.attn_device != 0 and pack.scratch_bytes > scratch
        on = _forward_all(pack, imgs, True)
        sel = [0, 1] if layers is None else layers
        assert pack.launches == (base[0] + AD.map_launches(L, sel, rollout), base[1]), (layers, rollout, pack.launches, base)
        assert all(_same_bytes(a, b) for a, b in zip(on, off)), (layers, rollout)
        maps = pack.attn_read()
        for i, (c, r) in enumerate(maps):
            assert c.shape[0] == len(sel) and np.isfinite(c).all() and (r is None) == (not rollout)
            assert np.allclose(c.sum(axis=-1), 1.0, atol=1e-4)
        pack.forward(imgs[::-1])                          # reversed: positions and neighbours change
        for i, (c, r) in enumerate(pack.attn_read()[::-1]):
            assert np.array_equal(_bits(c), _bits(maps[i][0])) and (r is None or np.array_equal(_bits(r), _bits(maps[i][1]))), (i, "reversed")
        for i in range(len(imgs)):
            pack.forward(imgs[i:i + 1])
            (c, r), = pack.attn_read()
            assert np.array_equal(_bits(c), _bits(maps[i][0])), (layers, rollout, i, "class maps alone")
            assert r is None or np.array_equal(_bits(r), _bits(maps[i][1])), (layers, rollout, i, "rollout alone")
    pack.attn_disable()
    again = _forward_all(pack, imgs, True)
    assert pack.launches == base and pack.scratch_bytes == scratch and pack.attn_device == 0
    assert all(_same_bytes(a, b) for a, b in zip(again, off))
    pack.close(); model.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_maps_that_were_there(pkg, binding, torch_gpu):
    model = binding.Model(KD.variant_file(pkg, "p16h4"))
    P = model.hparams.patch_size
    shapes = KD.mixed_shapes(P)
    imgs = KD.pack_of(shapes)
    sq = int(AD.tables(KD.row0_of(shapes, P, 0))[1][-1])
    pack = binding.PackContext(model, device=0, max_tokens=1100, max_images=8, dtype=binding.BF16)
    with pytest.raises(binding.VitxError) as e:           # off: nothing to read
        pack.attn_read()
    assert e.value.code == binding.ERR_ARG
    pack.attn_enable([1], rollout=True, max_sq_tokens=sq)
    with pytest.raises(binding.VitxError) as e:           # on, but no forward yet
        pack.attn_read()
    assert e.value.code == binding.ERR_ARG and "no forward" in str(e.value)
    pack.forward(imgs)                                    # (the first call builds the grids' tables: its launch count is not the steady one)
    p, _ = pack.forward(imgs)
    maps = pack.attn_read()
    launches = pack.launches
    # refused calls: one float too many for the arenas; an image above 1024 tokens (named)
    more = imgs + [XD.images(1, P, P, seed=99)[0]]
    with pytest.raises(binding.VitxError) as e:
        pack.forward(more)
    assert e.value.code == binding.ERR_ARG and "max_sq_tokens" in str(e.value)
    big = [imgs[0], XD.images(1, 32 * P, 32 * P, seed=5)[0]]
    with pytest.raises(binding.VitxError) as e:
        pack.forward(big)
    assert e.value.code == binding.ERR_UNSUPPORTED and "image 1" in str(e.value)
    # refused enables: the maps stay on as they were
    for mask, flags, msq in ((1 << L, 0, 0), (1, 2, 0), (1, binding.ATTN_ROLLOUT, 0), (1, binding.ATTN_ROLLOUT, 2 ** 31)):
        rc = binding.lib().vitx_pack_attn_enable(pack._h, mask, flags, msq)
        assert rc == binding.ERR_ARG, (mask, flags, msq, rc)
    assert binding.lib().vitx_pack_attn_floats(pack._h) == model.hparams.num_attention_heads + 1 and pack.launches == launches
    again = pack.attn_read()
    for (c, r), (c0, r0) in zip(again, maps):
        assert np.array_equal(_bits(c), _bits(c0)) and np.array_equal(_bits(r), _bits(r0))
    p2, _ = pack.forward(imgs)
    assert np.array_equal(_bits(p2), _bits(p)) and pack.launches == launches
    for (c, r), (c0, r0) in zip(pack.attn_read(), maps):
        assert np.array_equal(_bits(c), _bits(c0)) and np.array_equal(_bits(r), _bits(r0))
    # class maps alone take the large image
    pack.attn_enable([1], rollout=False)
    pack.forward(big)
    (c0, _), (c1, _) = pack.attn_read()
    assert c1.shape == (1, model.hparams.num_attention_heads, 1025) and np.array_equal(_bits(c0), _bits(maps[0][0]))
    # the kernel entry points' own checks
    B, UNS, ARG = binding, binding.ERR_UNSUPPORTED, binding.ERR_ARG
    torch = torch_gpu
    buf = torch.zeros(1025 * 1025 + 64, dtype=torch.float32, device="cuda")
    q = torch.zeros((1025, 3 * 128), dtype=torch.bfloat16, device="cuda")
    for call, code in ((lambda: B.op_attention_map_packed(B.BF16, 0, buf.data_ptr(), 0, [0, 5], 128, 4), ARG),
                       (lambda: B.op_attention_map_packed(B.BF16, q.data_ptr(), 0, 0, [0, 5], 128, 4), ARG),
                       (lambda: B.op_attention_map_packed(B.BF16, q.data_ptr(), buf.data_ptr(), 0, [0, 5, 5], 128, 4), ARG),
                       (lambda: B.op_attention_map_packed(B.BF16, q.data_ptr(), 0, buf.data_ptr(), [0, 1025], 128, 4), UNS),
                       (lambda: B.op_rollout_step_packed(0, buf.data_ptr(), [0, 5]), ARG),
                       (lambda: B.op_rollout_step_packed(buf.data_ptr(), buf.data_ptr() + 4 * 24, [0, 5]), ARG),
                       (lambda: B.op_rollout_step_packed(buf.data_ptr(), buf.data_ptr() + 4 * 1025 * 1025, [0, 1025]), UNS),
                       (lambda: B.op_rollout_row_packed(0, 0, buf.data_ptr(), [0, 5], 4), ARG),
                       (lambda: B.op_rollout_row_packed(buf.data_ptr(), 0, 0, [0, 5], 4), ARG),
                       (lambda: B.op_rollout_row_packed(buf.data_ptr(), 0, buf.data_ptr() + 4 * 4 * 1025, [0, 1025], 4), UNS)):
        with pytest.raises(B.VitxError) as e:
            call()
        assert e.value.code == code, str(e.value)
    B.op_attention_map_packed(B.BF16, q.data_ptr(), buf.data_ptr(), 0, [0, 1025], 128, 4)      # the class maps have no token bound
    pack.close(); model.close()


# ------------------------------------------------------------------------------------------------ 6. stream order
class AttnPackStep(SO.S.Step):
    """vitx_pack_forward_device with the last layer's class maps and rollout on, packs = (stalled, fenced): the maps through vitx_pack_attn_device."""

    def __init__(self, torch, packs, model, shapes, seed):
        self.packs, self.shapes = packs, shapes
        real = np.concatenate([i.ravel() for i in KD.pack_of(shapes, seed=seed)])
        self.x = SO.S.Input(SO._dev(torch, real), SO._dev(torch, SO.S.decoy_f32(real, seed, 1.0)))
        self.inputs = [self.x]
        n, Cn = len(shapes), model.num_classes
        P, Tp = model.hparams.patch_size, model.num_prefix
        floats = sum(Tp + (h // P) * (w // P) for h, w in shapes) * (model.hparams.num_attention_heads + 1)
        self.probs = torch.empty(n * Cn, dtype=torch.float32, device="cuda")
        pack = packs[0]
        self.snaps = [SO.S.Snap(torch, "probabilities", self.probs.data_ptr(), n * Cn, torch.float32),
                      SO.S.Snap(torch, "attention maps", lambda: pack.attn_device, floats, torch.float32)]
        assert pack.attn_device

    def call(self, fenced, stream):
        self.packs[1 if fenced else 0].forward_device(self.x.p, self.shapes, self.probs.data_ptr(), 0, stream)

    def expected(self):
        maps = self.packs[1].attn_read()
        return {"probabilities": SO.S.device_bytes(self.probs.data_ptr(), self.probs.numel() * 4),
                "attention maps": np.concatenate([np.concatenate([c.ravel(), r]) for c, r in maps])}


def test_forward_device_with_rollout_only_enqueues(pkg, binding, torch_gpu):
    """One call with rollout on, the caller's stream stalled in front of it: the call returns under the stall, and probabilities and maps (snapshot on
    the caller's stream from vitx_pack_attn_device) are those of the fenced call.  The contexts have run the shapes before, so the table cache is warm."""
    torch = torch_gpu
    model = binding.Model(KD.variant_file(pkg, "p14ropeh4"))
    shapes = [(2 * 14, 5 * 14), (14, 14), (4 * 14, 4 * 14)]
    packs = tuple(binding.PackContext(model, device=0, max_tokens=64, max_images=3, dtype=binding.BF16) for _ in range(2))
    for p in packs:
        p.attn_enable([L - 1], rollout=True)
        p.forward(KD.pack_of(shapes, seed=1))
    SO.S.harness(torch).check("packed forward bf16, last layer's class maps + rollout", lambda: [AttnPackStep(torch, packs, model, shapes, 77)])
    SO._close(packs)
    model.close()


# ------------------------------------------------------------------------------------------------ 7. the CLI
@pytest.mark.parametrize("kind", ["rollout", "last"])
def test_cli_pack_attn_map_writes_the_pictures_of_the_per_image_path(pkg, binding, torch_gpu, tmp_path, kind):
    """vit_cli --pack --img-fit 32 --attn-map PREFIX on two golden assets, the 4-head patch-16 variant: PREFIX.<i>.pgm has the bytes of the per-image
    --img-fit --attn-map run, a w_i x h_i picture of the image's own grid."""
    from vitcpp_amd import cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = KD.variant_file(pkg, "p16h4")
    files = [os.path.join(root, "tests", "golden", "assets", f) for f in ("tench.jpg", "kiwi.jpg")]
    common = ["-m", src, "--dtype", "bf16", "--img-fit", "32", "--attn-kind", kind]
    single = []
    for k, f in enumerate(files):
        out = str(tmp_path / f"single{k}.pgm")
        assert cli.main(common + ["-i", f, "--attn-map", out]) == 0
        single.append(open(out, "rb").read())
    prefix = str(tmp_path / "packed")
    assert cli.main(common + ["--pack", "-i", ",".join(files), "--attn-map", prefix]) == 0
    for k in range(len(files)):
        got = open(f"{prefix}.{k}.pgm", "rb").read()
        assert got[:2] == b"P5" and got == single[k], (kind, k, got[:20], single[k][:20])
    assert single[0] != single[1]
