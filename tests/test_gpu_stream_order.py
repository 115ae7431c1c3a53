"""Stream order: every entry point of include/vitx.h that "only enqueues on `stream`", and every *_device accessor whose buffer is "written by the
forward's streams", on a caller stream that is STALLED while the host enqueues (harness, conditions and what a fault shows as: tests/stream_data.py;
the tables of who is stalled and who is not: there and in tests/test_cpu_stream_contract.py).

Every scenario: the stall, the producer of the real input over a decoy, the call, snapshots of every output in stream order, the decoy back, one
synchronise -- against the same call made the fenced way on a second context of the same options, bit for bit; on each of four caller streams,
each with its broken-caller control.  `pytest -s` prints one STALL line per scenario (profiles/stream_order.txt).

  main context     micro fixture: 3 images on one stream; 16 images on two sub-batch streams (F16, BF16, F16 with f16_fast_attention); graph = 1
                   (direct, captured, replayed under one stall); the smallest LayerNorm-fusing batch; two calls back to back on one stream and on
                   two caller streams joined by an event
  opt-in outputs   16 images, two streams: features, attention maps + rollout, zero-shot, nearest neighbours, dense head, depth head, one at a
                   time and all together, each through its *_device pointer (the maps, which have none: vitx_attn_read after the synchronise)
  pipeline         u8 source -> vitx_preprocess_ex_device -> vitx_forward_device under one stall
  packed context   pack_data.B2B_CALLS (eviction, table build, arena restart) with the stall in front of A, of B, of C; dense and depth heads
                   through vitx_pack_dense_device / vitx_pack_depth_device, features through feat_read; a caller stream and the context's own
  text context     two vitx_text_embed_device calls back to back, the host ids overwritten the moment each call returns
  vitx_op_*        every entry of OPS at a small shape its own checks accept, operands produced behind the stall

NOT stalled (stream_data.HOST_WAITS: the header calls them test-only or synchronising): vitx_op_gemm_ln, vitx_op_attention_f32,
vitx_op_patch_embed, vitx_op_attention_packed, vitx_op_rope_packed, vitx_op_dense_labels_packed, vitx_op_depth_fine_packed,
vitx_op_depth_resize_packed.  A packed context's OWN stream cannot be stalled by a caller (it has no handle to it): that case runs the three
calls back to back and reads through the functions that "wait for the forward", with no device synchronise.
"""
import ctypes as C

import numpy as np
import pytest

import arch_data as AD
import pack_data as KD
import rect_data as XD
import stream_data as S
import text_data as TD
import wide_data as WD
import zs_data as Z

pytestmark = pytest.mark.gpu

MODES = {"f16": (0, {}), "bf16": (1, {}), "f16_fast": (0, {"f16_fast_attention": 1})}


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _images(ctx, model, n, seed):
    """(real, decoy) f32 images [n, ...] of the context's shape (one grey plane for a one-channel file)."""
    h, w = ctx.img_shape
    shape = (n, h, w, 3) if model.in_channels == 3 else (n, h, w)
    real = S.real_f32(shape, seed)
    return real, S.decoy_f32(real, seed, 1.0)


# ================================================================================================ the main context
HEADS = ("features", "maps", "zeroshot", "gallery", "dense", "depth")


def _set_heads(binding, ctx, model, heads):
    """The opt-in outputs `heads` on one context, random head weights from fixed seeds (both contexts of a pair get the same)."""
    rng = np.random.default_rng(11)
    D = model.hparams.hidden_size
    if "features" in heads:
        ctx.feat_enable(cls=True, mean=True, tokens=True)
    if "maps" in heads:
        ctx.attn_enable(None, rollout=True)
    if "zeroshot" in heads:
        ctx.zeroshot_set(Z.unit_rows(rng.standard_normal((7, Z.CLIP_E))), Z.SOFTMAX, 100.0, 0.0)
    if "gallery" in heads:
        ctx.nn_set(Z.unit_rows(rng.standard_normal((40, ctx.nn_width(binding.NN_EMBED)))).astype(np.float32), 3, binding.NN_EMBED)
    if "dense" in heads:
        ctx.dense_set((rng.standard_normal((5, D)) * 0.5).astype(np.float32), rng.standard_normal(5).astype(np.float32), None, score=True, logits=True)
    if "depth" in heads:
        K = 8
        ctx.depth_set((rng.standard_normal((K, D)) * 0.5).astype(np.float32), (rng.standard_normal((K, D)) * 0.5).astype(np.float32), rng.standard_normal(K).astype(np.float32),
                      binding.depth_bins(K, 0.5, 10.0), None, 4, 0.5, 10.0, logits=True, fine=True)


class ForwardStep(S.Step):
    """vitx_forward_device of n images on ctxs = (stalled, fenced); share: a ForwardStep whose input buffer and output buffers this one uses too (the
    graph cache keys on the pointers)."""

    def __init__(self, torch, binding, ctxs, model, real, decoy, heads=(), share=None):
        self.torch, self.binding, self.ctxs, self.model, self.heads, self.n = torch, binding, ctxs, model, tuple(heads), real.shape[0]
        n, ctx = self.n, ctxs[0]
        self.x = S.Input(_dev(torch, real), _dev(torch, decoy))
        if share is not None:
            self.x.buf = share.x.buf
        self.inputs = [self.x]
        floats = n * model.num_classes * max(model.seq_len, 1)
        self.probs = share.probs if share is not None else torch.empty(floats, dtype=torch.float32, device="cuda")
        self.logits = share.logits if share is not None else torch.empty(floats, dtype=torch.float32, device="cuda")
        f32, L = torch.float32, binding.lib()
        self.snaps = [S.Snap(torch, "probabilities", self.probs.data_ptr(), floats, f32), S.Snap(torch, "logits", self.logits.data_ptr(), floats, f32)]
        if "features" in heads:
            self.snaps.append(S.Snap(torch, "features", lambda: ctx.feat_device()[0], n * int(L.vitx_feat_floats(ctx._h)), f32))
        if "zeroshot" in heads:
            self.snaps.append(S.Snap(torch, "zero-shot probabilities and logits", lambda: ctx.zeroshot_device()[0], n * 2 * int(L.vitx_zeroshot_classes(ctx._h)), f32))
        if "gallery" in heads:
            self.snaps.append(S.Snap(torch, "neighbour pairs", lambda: ctx.nn_device()[0], n * 2 * int(L.vitx_nn_k(ctx._h)), torch.int32))
        if "dense" in heads:
            oh, ow = ctx.dense_shape()
            self.snaps.append(S.Snap(torch, "label maps", lambda: ctx.dense_device()[0], n * oh * ow, torch.uint8))
        if "depth" in heads:
            oh, ow = ctx.depth_shape()[:2]
            self.snaps.append(S.Snap(torch, "depth maps", lambda: ctx.depth_device()[0], n * oh * ow, f32))
        for sn in self.snaps:
            assert sn.src(), f"the {sn.name} have no device buffer"

    def call(self, fenced, stream):
        self.ctxs[1 if fenced else 0].forward_device(self.x.p, self.n, self.probs.data_ptr(), self.logits.data_ptr(), stream)

    def _maps(self, ctx):
        L, n = self.binding.lib(), self.n
        out = np.empty((n, int(L.vitx_attn_floats(ctx._h))), np.float32)
        self.binding.check(L.vitx_attn_read(ctx._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "vitx_attn_read")
        return out

    def expected(self):
        """The fenced context's *_read, laid out as the *_device buffers are (include/vitx.h); probabilities and logits from the caller's buffers."""
        ctx, n, L = self.ctxs[1], self.n, self.binding.lib()
        out = {"probabilities": S.device_bytes(self.probs.data_ptr(), self.probs.numel() * 4), "logits": S.device_bytes(self.logits.data_ptr(), self.logits.numel() * 4)}
        if "features" in self.heads:
            f = np.empty((n, int(L.vitx_feat_floats(ctx._h))), np.float32)
            self.binding.check(L.vitx_feat_read(ctx._h, f.ctypes.data_as(C.POINTER(C.c_float)), f.size), "vitx_feat_read")
            out["features"] = f
        if "zeroshot" in self.heads:
            p, lg = ctx.zeroshot_read(n, want_logits=True)
            out["zero-shot probabilities and logits"] = np.stack([p, lg], axis=1)                     # [n][2][K]: per image the probabilities, then the logits
        if "gallery" in self.heads:
            idx, score, _ = ctx.nn_read(n)
            out["neighbour pairs"] = np.stack([score.view(np.uint32), idx.view(np.uint32)], axis=2)   # [n][k] {f32 score, i32 index}
        if "dense" in self.heads:
            out["label maps"] = ctx.dense_read(n)[0]
        if "depth" in self.heads:
            out["depth maps"] = ctx.depth_read(n)[0]
        if "maps" in self.heads:
            out["class-token maps and rollout"] = self._maps(ctx)
        return out

    def late(self):
        return {"class-token maps and rollout": self._maps(self.ctxs[0])} if "maps" in self.heads else {}

    def dirty(self):
        """The maps have no device pointer to refill: a fenced forward of the decoy leaves other maps in the buffer."""
        if "maps" in self.heads:
            self.ctxs[0].forward_device(self.x.p, self.n, self.probs.data_ptr(), self.logits.data_ptr(), 0)
            self.torch.cuda.synchronize()


def _pair(binding, model, n, dtype, heads=(), **opts):
    """(stalled, fenced): two contexts of the same options, each warmed by one fenced forward -- the documented probe of the first multi-stream
    forward has then happened."""
    ctxs = tuple(binding.Context(model, 0, n, dtype, **opts) for _ in range(2))
    for c in ctxs:
        _set_heads(binding, c, model, heads)
        c.forward(_images(c, model, n, 99)[0])
    return ctxs


def _close(*things):
    for t in things:
        for c in (t if isinstance(t, (tuple, list)) else (t,)):
            c.close()


def _micro(pkg, binding, zs=False):
    return binding.Model(Z.model_file(pkg, "clip") if zs else pkg.synth.cached_synthetic(AD.MICRO, head_scale=4.0))


def test_three_images_on_one_stream(pkg, binding, torch_gpu):
    """The single-stream forward: every launch of it sits behind the producer on the caller's stream."""
    model = _micro(pkg, binding)
    ctxs = _pair(binding, model, 3, 1)
    assert ctxs[0].split(3) == [3]
    real, decoy = _images(ctxs[0], model, 3, 1)
    S.harness(torch_gpu).check("forward micro bf16, 3 images, one stream", lambda: [ForwardStep(torch_gpu, binding, ctxs, model, real, decoy)])
    _close(ctxs, model)


@pytest.mark.parametrize("mode", list(MODES))
def test_sixteen_images_on_two_sub_batch_streams(pkg, binding, torch_gpu, mode):
    """Fork and join: slice 1 runs on the context's internal stream, which must wait for the caller's stream (the producer) and be waited for by it
    (the snapshots of the second sub-batch's rows)."""
    dtype, opts = MODES[mode]
    model = _micro(pkg, binding)
    ctxs = _pair(binding, model, 16, dtype, **opts)
    parts = ctxs[0].split(16)
    assert len(parts) == 2 and min(parts) >= 3, parts
    real, decoy = _images(ctxs[0], model, 16, 2)
    S.harness(torch_gpu).check(f"forward micro {mode}, 16 images = {parts[0]} + {parts[1]}, two streams", lambda: [ForwardStep(torch_gpu, binding, ctxs, model, real, decoy)])
    _close(ctxs, model)


def test_graph_option_direct_captured_replayed(pkg, binding, torch_gpu):
    """graph = 1, 3 images: the same stalled call three times back to back on the same pointers, each with its own input produced behind the one
    before -- launched directly, captured (and launched), replayed.  Every run uses fresh buffers, so every run sees all three."""
    torch = torch_gpu
    model = _micro(pkg, binding)
    ctxs = _pair(binding, model, 3, 0, graph=1)
    data = [_images(ctxs[0], model, 3, 20 + k) for k in range(3)]
    runs = []

    def make():
        first = ForwardStep(torch, binding, ctxs, model, *data[0])
        runs.append(first)
        return [first] + [ForwardStep(torch, binding, ctxs, model, *data[k], share=first) for k in (1, 2)]
    S.harness(torch).check("forward micro f16 graph = 1, 3 images, direct + captured + replayed", make, fresh=True)
    # per run one capture (launched) and one replay; the fenced context saw one run, the stalled one the unstalled run and 2 x 4 stalled ones
    assert ctxs[1].graph_launches() == 2 and ctxs[0].graph_launches() == 2 * (len(runs) - 1), (ctxs[1].graph_launches(), ctxs[0].graph_launches(), len(runs))
    _close(ctxs, model)


def test_smallest_layernorm_fusing_batch(pkg, binding, torch_gpu):
    """wide_data.batch_for: proj and fc2 of both sub-batches carry the LayerNorms (statistics exchange between workgroups, the fall-back counter
    copied to the host behind the last kernel), streams = 2 with the cut at split_first."""
    key = "vit_erf"
    N = WD.FIXTURES[key].tokens
    n, s1 = WD.batch_for(N)
    model = binding.Model(WD.fixture_file(pkg, key))
    ctxs = _pair(binding, model, n, 1, streams=2, split_first=s1)
    assert all(c.ln_fusion_active() == 1 and c.split(n) == [s1, n - s1] for c in ctxs)
    real, decoy = _images(ctxs[0], model, n, 3)
    S.harness(torch_gpu).check(f"forward wide {key} bf16, {n} images = {s1} + {n - s1}, LayerNorm fusion", lambda: [ForwardStep(torch_gpu, binding, ctxs, model, real, decoy)])
    assert all(c.ln_fusion_active() == 1 for c in ctxs)
    _close(ctxs, model)


@pytest.mark.parametrize("streams", ["one-stream", "two-streams-joined-by-an-event"])
def test_two_calls_back_to_back(pkg, binding, torch_gpu, streams):
    """Two calls of 16 images with different inputs and outputs: the second producer sits behind the first call, and the second call's fork behind
    the first call's join.  On two caller streams the caller joins them with an event, as one that alternates streams would (unordered concurrent
    use of one context is not promised and not tested)."""
    torch = torch_gpu
    h = S.harness(torch)
    model = _micro(pkg, binding)
    ctxs = _pair(binding, model, 16, 1)
    assert len(ctxs[0].split(16)) == 2
    steps = [ForwardStep(torch, binding, ctxs, model, *_images(ctxs[0], model, 16, 30 + k)) for k in range(2)]
    other = lambda s: h.streams[(h.streams.index(s) + 1) % len(h.streams)]
    plan = None if streams == "one-stream" else (lambda s, n: [s, other(s)])
    h.check(f"forward micro bf16, 2 x 16 images back to back, {streams}", lambda: steps, plan=plan)
    _close(ctxs, model)


# ================================================================================================ opt-in outputs
@pytest.mark.parametrize("heads", [(h,) for h in HEADS] + [HEADS], ids=list(HEADS) + ["all"])
def test_opt_in_outputs_through_their_device_pointers(pkg, binding, torch_gpu, heads):
    """16 images on two sub-batch streams; slice 1 writes its images' part of every output buffer on the internal stream.  Snapshots through
    vitx_feat_device, vitx_zeroshot_device, vitx_nn_device, vitx_dense_device and vitx_depth_device on the caller's stream, against the fenced
    context's *_read; the maps through vitx_attn_read after the synchronise."""
    model = _micro(pkg, binding, zs="zeroshot" in heads)
    ctxs = _pair(binding, model, 16, 1, heads=heads)
    parts = ctxs[0].split(16)
    assert len(parts) == 2, parts
    real, decoy = _images(ctxs[0], model, 16, 4)
    S.harness(torch_gpu).check(f"forward micro bf16, 16 images, two streams, {' + '.join(heads)}", lambda: [ForwardStep(torch_gpu, binding, ctxs, model, real, decoy, heads=heads)])
    _close(ctxs, model)


# ================================================================================================ u8 source -> preprocess -> forward
class PipelineStep(S.Step):
    def __init__(self, torch, binding, ctxs, model, n, nx, ny):
        self.binding, self.ctxs, self.n, self.nx, self.ny = binding, ctxs, n, nx, ny
        side = ctxs[0].img_size
        self.pp = binding.Preproc.make(binding.PP_STRETCH, side, side, binding.PP_PIL_BICUBIC, 0, 0, (123.675, 116.28, 103.53), (58.395, 57.12, 57.375))
        real = S.real_u8((n, ny, nx, 3), 5)
        self.src = S.Input(_dev(torch, real), _dev(torch, S.decoy_u8(real, 5)))
        self.inputs = [self.src]
        self.imgs = torch.empty(n * side * side * 3, dtype=torch.float32, device="cuda")
        self.probs, self.logits = (torch.empty(n * model.num_classes, dtype=torch.float32, device="cuda") for _ in range(2))
        self.snaps = [S.Snap(torch, name, t.data_ptr(), t.numel(), torch.float32) for name, t in (("preprocessed images", self.imgs), ("probabilities", self.probs), ("logits", self.logits))]

    def call(self, fenced, stream):
        self.binding.preprocess_ex_device(self.pp, self.src.p, self.n, self.nx, self.ny, self.imgs.data_ptr(), stream)
        self.ctxs[1 if fenced else 0].forward_device(self.imgs.data_ptr(), self.n, self.probs.data_ptr(), self.logits.data_ptr(), stream)


def test_pipeline_u8_preprocess_forward(pkg, binding, torch_gpu):
    """The producer writes the u8 source; vitx_preprocess_ex_device and vitx_forward_device follow on the one stalled stream."""
    model = _micro(pkg, binding)
    ctxs = _pair(binding, model, 3, 1)
    S.harness(torch_gpu).check("u8 80 x 60 -> preprocess_ex_device -> forward micro bf16, 3 images", lambda: [PipelineStep(torch_gpu, binding, ctxs, model, 3, 80, 60)])
    _close(ctxs, model)


# ================================================================================================ the packed context
class PackStep(S.Step):
    """vitx_pack_forward_device of one call of pack_data.B2B_CALLS on packs = (stalled, fenced), a dense and a depth head set.  last: the step whose
    features feat_read gives after the synchronise."""

    def __init__(self, torch, packs, model, call, seed, last):
        self.packs, self.last = packs, last
        self.shapes = [(gh * 14, gw * 14) for gh, gw in call]
        real = np.concatenate([i.ravel() for i in KD.pack_of(self.shapes, seed=seed)])
        self.x = S.Input(_dev(torch, real), _dev(torch, S.decoy_f32(real, seed, 1.0)))
        self.inputs = [self.x]
        n, Cn, px = len(call), model.num_classes, sum(h * w for h, w in self.shapes)
        self.probs, self.logits = (torch.empty(n * Cn, dtype=torch.float32, device="cuda") for _ in range(2))
        pack = packs[0]
        self.snaps = [S.Snap(torch, "probabilities", self.probs.data_ptr(), n * Cn, torch.float32), S.Snap(torch, "logits", self.logits.data_ptr(), n * Cn, torch.float32),
                      S.Snap(torch, "label maps", lambda: pack.dense_device(), px, torch.uint8), S.Snap(torch, "depth maps", lambda: pack.depth_device(), px, torch.float32)]
        for sn in self.snaps:
            assert sn.src()

    def call(self, fenced, stream):
        self.packs[1 if fenced else 0].forward_device(self.x.p, self.shapes, self.probs.data_ptr(), self.logits.data_ptr(), stream)

    @staticmethod
    def _features(pack):
        cls, tok = pack.feat_read()
        return np.concatenate([cls.ravel()] + [t.ravel() for t in tok])

    def expected(self):
        pack = self.packs[1]
        out = {"probabilities": S.device_bytes(self.probs.data_ptr(), self.probs.numel() * 4), "logits": S.device_bytes(self.logits.data_ptr(), self.logits.numel() * 4),
               "label maps": np.concatenate([m.ravel() for m in pack.dense_read()[0]]), "depth maps": np.concatenate([m.ravel() for m in pack.depth_read()[0]])}
        if self.last:
            out["features"] = self._features(pack)
        return out

    def late(self):
        return {"features": self._features(self.packs[0])} if self.last else {}

    def close(self):
        if self.last:
            _close(self.packs)


def _pack_pair(binding, model):
    rng = np.random.default_rng(13)
    D, K = model.hparams.hidden_size, 8
    W, b = (rng.standard_normal((5, D)) * 0.5).astype(np.float32), rng.standard_normal(5).astype(np.float32)
    wp, wc, bias = (rng.standard_normal((K, D)) * 0.5).astype(np.float32), (rng.standard_normal((K, D)) * 0.5).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    packs = tuple(binding.PackContext(model, device=0, max_tokens=KD.B2B_MAX_TOKENS, max_images=2, dtype=binding.BF16, max_grids=2) for _ in range(2))
    for p in packs:
        p.feat_enable(cls=True, tokens=True)
        p.dense_set(W, b, None)
        p.depth_set(wp, wc, bias, binding.depth_bins(K, 0.5, 10.0), None, 2, 0.5, 10.0)
    return packs


def _pack_steps(torch, binding, model):
    packs = _pack_pair(binding, model)
    return [PackStep(torch, packs, model, call, 50 + k, k == len(KD.B2B_CALLS) - 1) for k, call in enumerate(KD.B2B_CALLS)]


@pytest.mark.parametrize("stall_at", [0, 1, 2], ids=["stall-before-A", "stall-before-B", "stall-before-C"])
def test_packed_calls_back_to_back_on_a_caller_stream(pkg, binding, torch_gpu, stall_at):
    """pack_data.B2B_CALLS, max_grids 2, a fresh pair of contexts per run: A (builds grids a, b: allocates, resamples, uploads the rotary tables), B
    (evicts b, builds c in its place), C (restarts the rotary arena, drops every table and builds its own).  The stalled call -- A, B or C -- must
    return under the stall: a dropped table is retired, not freed (freeing waits for the whole device), and the rotary upload is asynchronous on
    the call's stream.  In front of B and of C the calls before the stall run freely, so the documented waits of the stalled call (the previous
    upload, the previous forward before a table is dropped) are over when it is made; behind the stall in front of A, B meets them on the host."""
    torch = torch_gpu
    model = binding.Model(XD.fixture_file(pkg, KD.CACHE_KIND))
    trace = KD.cache_trace(KD.B2B_CALLS, KD.B2B_MAX_TOKENS, KD.CACHE_HALF, 2)
    assert trace[1]["evicted"] and trace[2]["restarted"]
    S.harness(torch).check(f"packed B2B_CALLS bf16, dense + depth heads, features, stall before {'ABC'[stall_at]}", lambda: _pack_steps(torch, binding, model), stall_at=stall_at, fresh=True)
    model.close()


def test_packed_calls_back_to_back_on_the_contexts_own_stream(pkg, binding, torch_gpu):
    """stream = NULL: the three calls back to back on the context's own stream, inputs complete before; then only the functions that "wait for the
    forward" (dense_read, depth_read, feat_read) and no device synchronise: call C's outputs have the bits of the fenced calls."""
    torch = torch_gpu
    model = binding.Model(XD.fixture_file(pkg, KD.CACHE_KIND))
    steps = _pack_steps(torch, binding, model)
    want = S.harness(torch).reference(steps)
    for st in steps:
        st.x.buf.copy_(st.x.real)
        for sn in st.snaps[:2]:
            S.copy_async(sn.src(), sn.sent.data_ptr(), sn.nbytes, 0)
    torch.cuda.synchronize()
    pack = steps[0].packs[0]
    for st in steps:
        pack.forward_device(st.x.p, st.shapes, st.probs.data_ptr(), st.logits.data_ptr(), 0)
    labels, depth, feats = pack.dense_read()[0], pack.depth_read()[0], PackStep._features(pack)            # each waits for the forward
    last = steps[-1]
    got = {"label maps": np.concatenate([m.ravel() for m in labels]), "depth maps": np.concatenate([m.ravel() for m in depth]), "features": feats,
           "probabilities": S.device_bytes(last.probs.data_ptr(), last.probs.numel() * 4), "logits": S.device_bytes(last.logits.data_ptr(), last.logits.numel() * 4)}
    torch.cuda.synchronize()
    failed = S._differences([got], [want[-1]], "own stream")
    for k, st in enumerate(steps[:-1]):
        got_k = {"probabilities": S.device_bytes(st.probs.data_ptr(), st.probs.numel() * 4), "logits": S.device_bytes(st.logits.data_ptr(), st.logits.numel() * 4)}
        failed += S._differences([got_k], [{n: want[k][n] for n in got_k}], f"own stream, call {'ABC'[k]}")
    assert not failed, "\n  ".join(failed)
    steps[-1].close(); model.close()


# ================================================================================================ the text context
class TextStep(S.Step):
    """vitx_text_embed_device: ids are a HOST array, free when the call returns -- it is overwritten with other valid ids that moment."""

    def __init__(self, torch, texts, ids, decoy, l2):
        self.texts, self.real, self.decoy, self.l2 = texts, ids, decoy, l2
        self.host = ids.copy()
        self.out = torch.empty(ids.shape[0] * texts[0].width, dtype=torch.float32, device="cuda")
        self.snaps = [S.Snap(torch, "embeddings", self.out.data_ptr(), self.out.numel(), torch.float32)]

    def call(self, fenced, stream):
        self.host[:] = self.real
        self.texts[1 if fenced else 0].embed_device(self.host, self.out.data_ptr(), l2=self.l2, stream=stream)

    def after_call(self):
        self.host[:] = self.decoy


@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_text_embed_device_twice_with_the_host_ids_overwritten(pkg, binding, torch_gpu, family):
    """Two calls back to back (the second with VITX_TEXT_L2); the second waits, as documented, for the first call's upload -- so only the first is
    asked to return under the stall.  No device input: the control races a canary buffer of the harness."""
    torch = torch_gpu
    model = binding.Model(TD.text_file(pkg, family))
    V, eos = model.text_info["vocab"], model.text_info["eos"]
    texts = tuple(binding.TextContext(model, max_prompts=4, dtype=binding.BF16) for _ in range(2))
    steps = []
    for k in range(2):
        ids = TD.prompts(family, 4, seed=40 + k)
        decoy = S.decoy_prompts(ids, V, eos, 40 + k)
        binding.text_check_ids(model, decoy)
        steps.append(TextStep(torch, texts, ids, decoy, l2=bool(k)))
    for t in texts:
        t.embed(steps[0].real)                               # (first-call set-up of the kernels happens here)
    S.harness(torch).check(f"text {family} bf16, 2 x 4 prompts back to back, host ids overwritten", lambda: steps)
    _close(texts, model)


# ================================================================================================ the vitx_op_* entries
class Kit:
    """The operands of one vitx_op_* case: inp() an input with its decoy (produced behind the stall), const() a weight or table that is just there,
    out() an output (sentinel-filled, snapshotted), scratch() zeroed workspace."""

    def __init__(self, torch, binding):
        self.torch, self.B, self.L = torch, binding, binding.lib()
        self.inputs, self.snaps, self.keep = [], [], []
        self.t16 = {0: torch.float16, 1: torch.bfloat16}

    def f32(self, shape, seed, scale=1.0):
        return S.real_f32(shape, seed, scale)

    def inp(self, real, decoy=None, dtype=None, race=True, out=None, seed=1, positive=False):
        """real: an np array (f32 by default; dtype 0 / 1: rounded to fp16 / bf16 on the device) or a device tensor with its decoy.  out = a name: the
        call works in place, the buffer is snapshotted under that name."""
        torch = self.torch
        if isinstance(real, np.ndarray):
            if decoy is None:
                decoy = S.decoy_f32(real, seed, positive=positive) if real.dtype == np.float32 else S.decoy_u8(real, seed)
            real, decoy = _dev(torch, real), _dev(torch, decoy)
            if dtype is not None:
                real, decoy = real.to(self.t16[dtype]), decoy.to(self.t16[dtype])
                assert bool((real != decoy).all())
        i = S.Input(real.contiguous(), decoy.contiguous(), race=race)
        self.inputs.append(i)
        if out:
            self.snaps.append(S.Snap(torch, out, lambda: i.p, i.buf.numel(), i.buf.dtype, refill=False))
        return i

    def const(self, a, dtype=None):
        t = _dev(self.torch, a) if isinstance(a, np.ndarray) else a
        if dtype is not None:
            t = t.to(self.t16[dtype])
        self.keep.append(t)
        return t.data_ptr()

    def out(self, name, numel, tdtype):
        t = self.torch.empty(numel, dtype=tdtype, device="cuda")
        self.keep.append(t)
        self.snaps.append(S.Snap(self.torch, name, t.data_ptr(), numel, tdtype))
        return t.data_ptr()

    def scratch(self, nbytes):
        t = self.torch.zeros(nbytes, dtype=self.torch.uint8, device="cuda")
        self.keep.append(t)
        return t.data_ptr()


class OpStep(S.Step):
    def __init__(self, kit, name, launch):
        self.kit, self.name, self.launch, self.inputs, self.snaps = kit, name, launch, kit.inputs, kit.snaps

    def call(self, fenced, stream):
        rc = self.launch(stream)
        self.kit.B.check(rc, self.name)


BF, HF = 1, 0
QKV = dict(n=2, N=17, D=128, H=2)          # head dim 64, the tuned attention families


def _qkv(k, n, N, D, dtype, **kw):
    return k.inp(k.f32((n * N, 3 * D), 3, 0.8), dtype=dtype, **kw)


def _attention(kernel, N=17, dtype=BF):
    def build(k):
        n, D, H = 2, 128, 2
        x, o = _qkv(k, n, N, D, dtype), k.out("attention", n * N * D, k.t16[dtype])
        if kernel is None:
            return lambda st: k.L.vitx_op_attention(dtype, x.p, o, n, N, D, H, st)
        return lambda st: k.L.vitx_op_attention_ex(dtype, kernel, x.p, o, n, N, D, H, st)
    return build


def _op_layernorm(k):
    M, D = 5, 128
    x, w, b, y = k.inp(k.f32((M, D), 1)), k.const(k.f32((D,), 2)), k.const(k.f32((D,), 3)), k.out("y", M * D, k.t16[BF])
    return lambda st: k.L.vitx_op_layernorm(BF, x.p, w, b, y, M, D, 1e-6, st)


def _op_layernorm_f32(k):
    M, D = 5, 128
    x, w, b = k.inp(k.f32((M, D), 1), out="x, in place"), k.const(k.f32((D,), 2)), k.const(k.f32((D,), 3))
    return lambda st: k.L.vitx_op_layernorm_f32(x.p, w, b, x.p, M, D, 1e-6, st)


def _op_gemm(k):
    M, N, K = 128, 64, 64
    a, w, bias = k.inp(k.f32((M, K), 1), dtype=BF), k.const(np.concatenate([k.f32((N, K), 2), np.zeros((256 - N, K), np.float32)]), BF), k.const(np.zeros(256, np.float32) + 0.5)
    o = k.out("out", M * N, k.t16[BF])
    return lambda st: k.L.vitx_op_gemm(BF, 0, a.p, w, bias, o, M, N, K, st)


def _op_gemm_ex(k):
    M, Mr, N, K = 128, 100, 64, 64
    a, w, bias = k.inp(k.f32((M, K), 1), dtype=HF), k.const(np.concatenate([k.f32((N, K), 2), np.zeros((256 - N, K), np.float32)]), HF), k.const(np.zeros(256, np.float32) + 0.5)
    o = k.out("out", M * N, k.torch.float32)
    return lambda st: k.L.vitx_op_gemm_ex(HF, 3, 0, a.p, w, bias, o, None, M, Mr, N, K, 0, st)


def _q4(k, N, K):
    """q4_0 planes of N rows: nibbles [N][K / 32][16] u8 and f16 scales [N][K / 32]."""
    return S.real_u8((N, K // 32, 16), 4), (np.abs(k.f32((N, K // 32), 5)) * 0.05 + 0.01).astype(np.float16)


def _op_gemm_q4(k):
    M, N, K = 128, 128, 64
    qs, sc = _q4(k, N, K)
    a, q, s, bias = k.inp(k.f32((M, K), 1), dtype=BF), k.const(qs), k.const(sc), k.const(np.zeros(N, np.float32) + 0.5)
    o = k.out("out", M * N, k.t16[BF])
    return lambda st: k.L.vitx_op_gemm_q4(BF, 0, a.p, q, s, bias, o, M, M, N, K, st)


def _op_dequant(k):
    N, K = 8, 64
    qs, sc = _q4(k, N, K)
    q, s, o = k.inp(qs), k.const(sc), k.out("out", N * K, k.t16[BF])
    return lambda st: k.L.vitx_op_dequant(BF, 2, q.p, s, o, N, N, K, st)


def _op_dequant_jobs(k):
    N, K = 8, 64
    qs, sc = _q4(k, N, K)
    q, s, o = k.inp(qs), k.const(sc), k.out("out", N * K, k.t16[BF])
    vp, ip = C.c_void_p * 1, C.c_int * 1
    return lambda st: k.L.vitx_op_dequant_jobs(BF, 2, 1, vp(q.p), vp(s), vp(o), ip(N), ip(N), ip(K), st)


def _op_attention_cls(k):
    n, N, D, H = 2, 17, 128, 2
    x, o = _qkv(k, n, N, D, BF), k.out("class rows", n * D, k.t16[BF])
    return lambda st: k.L.vitx_op_attention_cls(BF, x.p, 0, o, n, N, D, H, st)


def _op_attention_planes(k):
    n, N, D, H = 2, 17, 128, 2
    x = k.inp(k.f32((2, n * N, 3 * D), 3, 0.8), dtype=HF)                  # the hi plane, the lo plane right behind it
    o = k.out("attention", n * N * D, k.torch.float16)
    return lambda st: k.L.vitx_op_attention_planes(x.p, n * N * 3 * D, o, n, N, D, H, st)


def _op_attention_generic(k):
    n, N, D, H = 2, 17, 64, 2
    x, o = _qkv(k, n, N, D, BF), k.out("attention", n * N * D, k.t16[BF])
    return lambda st: k.L.vitx_op_attention_generic(BF, x.p, o, n, N, D, H, st)


def _op_attention_text(k):
    n, T, D, H = 2, 16, 128, 2
    x, o = _qkv(k, n, T, D, BF), k.out("attention", n * T * D, k.t16[BF])
    return lambda st: k.L.vitx_op_attention_text(BF, x.p, o, n, T, D, H, 1, st)


def _op_attention_packed_tables(k):
    """Two images of 40 + 60 rows; the decoy table cuts at 50: a valid table of the same shape and the same block counts (qb0 = 0, 1, 2 for both)."""
    rows, D, H = 100, 64, 2
    x = k.inp(k.f32((rows, 3 * D), 3, 0.8), dtype=BF)
    row0 = k.inp(_dev(k.torch, np.array([0, 40, rows], np.int32)), _dev(k.torch, np.array([0, 50, rows], np.int32)), race=False)
    qb0, o = k.const(np.array([0, 1, 2], np.int32)), k.out("attention", rows * D, k.t16[BF])
    return lambda st: k.L.vitx_op_attention_packed_tables(BF, x.p, o, row0.p, qb0, 2, 2, D, H, st)


def _op_rope(k):
    n, N, T, D, H = 2, 17, 1, 128, 2
    x = _qkv(k, n, N, D, BF, out="qkv, in place")
    ang = k.f32((N - T, D // H // 2), 6, 1.5)
    cs, sn = k.const(np.cos(ang).astype(np.float32)), k.const(np.sin(ang).astype(np.float32))
    return lambda st: k.L.vitx_op_rope(BF, x.p, 0, cs, sn, n, N, T, D, H, st)


def _op_swiglu(k):
    rows, F = 5, 64
    x, o = k.inp(k.f32((rows, 2 * F), 1), dtype=BF), k.out("gated", rows * F, k.t16[BF])
    return lambda st: k.L.vitx_op_swiglu(BF, x.p, 2 * F, o, F, rows, F, st)


def _softmax(dt):
    def build(k):
        rows, cols, ld = 3, 10, 12
        x, o = k.inp(k.f32((rows, ld), 1, 2.0)), k.out("probabilities", rows * cols, k.torch.float32)
        if dt is None:
            return lambda st: k.L.vitx_op_softmax(x.p, o, rows, cols, ld, st)
        return lambda st: k.L.vitx_op_softmax_dt(dt, x.p, o, rows, cols, ld, st)
    return build


def _op_topk(k):
    rows, cols, kk = 3, 10, 5
    x, o = k.inp(np.abs(k.f32((rows, cols), 1, 0.2)), positive=True), k.out("pairs", rows * kk * 2, k.torch.int32)
    return lambda st: k.L.vitx_op_topk(x.p, rows, cols, kk, o, st)


def _op_attention_map(k):
    n, N, D, H = 2, 17, 128, 2
    x, c, m = _qkv(k, n, N, D, BF), k.out("class-token maps", n * H * N, k.torch.float32), k.out("head mean", n * N * N, k.torch.float32)
    return lambda st: k.L.vitx_op_attention_map(BF, x.p, 0, c, m, n, N, D, H, st)


def _op_rollout_factor(k):
    n, N, D, H = 2, 17, 128, 2
    x, o = _qkv(k, n, N, D, BF), k.out("factor", n * N * N, k.torch.float32)
    return lambda st: k.L.vitx_op_rollout_factor(BF, x.p, 0, o, n, N, D, H, st)


def _op_rollout_step(k):
    n, N = 2, 17
    a, r = k.inp(np.abs(k.f32((n, N, N), 1, 0.1)), out="a, in place", positive=True), k.inp(np.abs(k.f32((n, N, N), 2, 0.1)), seed=2, positive=True)
    return lambda st: k.L.vitx_op_rollout_step(a.p, r.p, n, N, st)


def _op_rollout_row(k):
    n, N, H = 2, 17, 2
    c, r, o = k.inp(np.abs(k.f32((n, H * N), 1, 0.1)), positive=True), k.inp(np.abs(k.f32((n, N, N), 2, 0.1)), seed=2, positive=True), k.out("rollout row", n * N, k.torch.float32)
    return lambda st: k.L.vitx_op_rollout_row(c.p, H * N, r.p, o, N, n, N, H, st)


def _features(ex):
    def build(k):
        n, N, D, first = 2, 9, 128, (3 if ex else 1)
        fpi = (2 + N - first) * D
        x, w, b = k.inp(k.f32((n, N, D), 1)), k.const(k.f32((D,), 2)), k.const(k.f32((D,), 3))
        o = k.out("cls | mean | tokens", n * fpi, k.torch.float32)
        if not ex:
            return lambda st: k.L.vitx_op_features(x.p, D, N * D, w, b, o, o + 4 * D, o + 8 * D, fpi, n, N, D, 1e-6, 0, st)
        z = k.out("head operand", n * 2 * D, k.t16[BF])
        return lambda st: k.L.vitx_op_features_ex(x.p, D, N * D, w, b, o, o + 4 * D, o + 8 * D, fpi, n, N, first, D, 1e-6, 0, z, BF, st)
    return build


def _op_attention_pool(k):
    n, N, D, H = 2, 16, 128, 2
    x, w, b, u = k.inp(k.f32((n, N, D), 1)), k.const(k.f32((D,), 2)), k.const(k.f32((D,), 3)), k.const(k.f32((H, D), 4, 0.1))
    m, p = k.out("M", n * H * D, k.torch.float32), k.out("p", n * H * N, k.torch.float32)
    return lambda st: k.L.vitx_op_attention_pool(x.p, D, N * D, w, b, 1e-6, u, m, p, n, N, D, H, st)


def _op_zeroshot(k):
    n, K, E = 3, 7, 64
    bank = np.concatenate([Z.unit_rows(k.f32((K, E), 2)).astype(np.float32), np.zeros((128 - K, E), np.float32)])
    z, bk = k.inp(k.f32((n, E), 1)), k.const(bank, BF)
    a, acc = k.scratch(256 * E * 2), k.scratch((256 + 1) * 128 * 4)
    p, lg = k.out("probabilities", n * K, k.torch.float32), k.out("logits", n * K, k.torch.float32)
    return lambda st: k.L.vitx_op_zeroshot(BF, z.p, E, bk, a, acc, p, lg, n, K, E, 0, 100.0, 0.0, st)


def _nn_state(k, scores, n, cols, kk):
    """The selection state of `scores` [n][cols], made the fenced way (vitx_op_nn_finish's input)."""
    torch = k.torch
    state = torch.zeros(int(k.L.vitx_op_nn_state_bytes(n, kk)), dtype=torch.uint8, device="cuda")
    s = _dev(torch, scores)
    k.B.check(k.L.vitx_op_nn_select(s.data_ptr(), cols, n, cols, 0, state.data_ptr(), kk, 1, None), "vitx_op_nn_select")
    torch.cuda.synchronize()
    return state


def _op_nn_select(k):
    n, cols, kk = 3, 40, 3
    x, state = k.inp(k.f32((n, cols), 1)), k.out("state", int(k.L.vitx_op_nn_state_bytes(n, kk)), k.torch.uint8)
    return lambda st: k.L.vitx_op_nn_select(x.p, cols, n, cols, 0, state, kk, 1, st)


def _op_nn_finish(k):
    n, cols, kk = 3, 40, 3
    real = k.f32((n, cols), 1)
    state = k.inp(_nn_state(k, real, n, cols, kk), _nn_state(k, S.decoy_f32(real, 1), n, cols, kk))
    pairs = k.out("pairs", n * kk * 2, k.torch.int32)
    return lambda st: k.L.vitx_op_nn_finish(state.p, n, kk, None, 0, 0.0, pairs, None, st)


def _op_nn(k):
    n, G, E, kk, chunk = 3, 40, 64, 3, 128
    gal = np.concatenate([Z.unit_rows(k.f32((G, E), 2)).astype(np.float32), np.zeros((128 - G, E), np.float32)])
    z, g = k.inp(k.f32((n, E), 1)), k.const(gal, BF)
    a, acc, state = k.scratch(256 * E * 2), k.scratch((256 + 1) * chunk * 4), k.scratch(int(k.L.vitx_op_nn_state_bytes(n, kk)))
    pairs = k.out("pairs", n * kk * 2, k.torch.int32)
    return lambda st: k.L.vitx_op_nn(BF, z.p, E, 0, n, g, G, E, kk, chunk, a, acc, state, pairs, st)


def _op_dense_labels(k):
    n, gh, gw, K, ld, oh, ow = 2, 2, 3, 5, 8, 5, 7
    x, lab, sc = k.inp(k.f32((n * gh * gw, ld), 1)), k.out("labels", n * oh * ow, k.torch.uint8), k.out("score", n * oh * ow, k.torch.float32)
    return lambda st: k.L.vitx_op_dense_labels(x.p, ld, n, gh, gw, K, oh, ow, lab, sc, st)


def _dense_operand(k, rows, Dc, dtype):
    """[256][Dc] operand rows: `rows` real ones, the pad rows zero in the real data and in the decoy (the call zeroes them anyway)."""
    real = k.f32((rows, Dc), 1)
    pad = np.zeros((256 - rows, Dc), np.float32)
    r, d = _dev(k.torch, np.concatenate([real, pad])).to(k.t16[dtype]), _dev(k.torch, np.concatenate([S.decoy_f32(real, 1), pad])).to(k.t16[dtype])
    return k.inp(r, d)


def _op_dense(k):
    n, gh, gw, K, Dc, oh, ow = 2, 2, 3, 5, 64, 5, 7
    a = _dense_operand(k, n * gh * gw, Dc, BF)
    w = k.const(np.concatenate([k.f32((K, Dc), 2, 0.5), np.zeros((128 - K, Dc), np.float32)]), BF)
    bias, lg = k.const(np.zeros(128, np.float32)), k.scratch(256 * 128 * 4)
    lab, sc = k.out("labels", n * oh * ow, k.torch.uint8), k.out("score", n * oh * ow, k.torch.float32)
    return lambda st: k.L.vitx_op_dense(BF, a.p, w, bias, lg, n, gh, gw, K, Dc, oh, ow, lab, sc, st)


def _op_depth_fine(k):
    n, gh, gw, K, ld, u = 2, 2, 3, 8, 8, 2
    x, off, bins = k.inp(k.f32((n * gh * gw, ld), 1)), k.inp(k.f32((n, ld), 2, 0.3), seed=2), k.const(k.B.depth_bins(K, 0.5, 10.0))
    fine = k.out("fine plane", n * u * gh * u * gw, k.torch.float32)
    return lambda st: k.L.vitx_op_depth_fine(x.p, ld, off.p, bins, n, gh, gw, K, u, fine, st)


def _op_depth_resize(k):
    n, fh, fw, oh, ow = 2, 4, 6, 9, 11
    x, o = k.inp(np.abs(k.f32((n, fh, fw), 1, 2.0)) + 0.5, positive=True), k.out("depth", n * oh * ow, k.torch.float32)
    return lambda st: k.L.vitx_op_depth_resize(x.p, n, fh, fw, oh, ow, 0.5, 10.0, o, st)


def _op_depth(k):
    n, gh, gw, K, Dc, u, oh, ow = 2, 2, 3, 8, 64, 2, 9, 13
    a = _dense_operand(k, n * gh * gw, Dc, BF)
    wp = k.const(np.concatenate([k.f32((K, Dc), 2, 0.5), np.zeros((128 - K, Dc), np.float32)]), BF)
    bias, bins, lg = k.const(np.zeros(128, np.float32)), k.const(k.B.depth_bins(K, 0.5, 10.0)), k.scratch((256 + 1) * 128 * 4)
    fine, depth = k.out("fine plane", n * u * gh * u * gw, k.torch.float32), k.out("depth", n * oh * ow, k.torch.float32)
    return lambda st: k.L.vitx_op_depth(BF, a.p, wp, None, None, bias, bins, lg, None, n, gh, gw, K, Dc, u, oh, ow, 0.5, 10.0, fine, depth, st)


def _op_depth_rows(k):
    rows, D = 5, 64
    x, y = k.inp(k.f32((rows, D), 1)), k.out("rows", rows * D, k.t16[BF])
    return lambda st: k.L.vitx_op_depth_rows(BF, x.p, D, y, D, rows, D, st)


PACK_GRIDS, PACK_OUTS = [(2, 3), (1, 5)], [(5, 7), (3, 9)]


def _op_dense_labels_packed_tables(k):
    """Two images; the decoy table is the valid table of the same two images in the other order (same shape, same tile count and window)."""
    K, ld, n = 5, 8, 2
    rows = sum(a * b for a, b in PACK_GRIDS)
    tab, tiles, cells = k.B.dense_pack_tables(PACK_GRIDS, PACK_OUTS, [0, 6])
    tab2, tiles2, cells2 = k.B.dense_pack_tables(PACK_GRIDS[::-1], PACK_OUTS[::-1], [0, 5])
    assert (tiles, cells, tab.shape) == (tiles2, cells2, tab2.shape) and not np.array_equal(tab, tab2)
    px = sum(a * b for a, b in PACK_OUTS)
    x, t = k.inp(k.f32((rows, ld), 1)), k.inp(_dev(k.torch, tab), _dev(k.torch, tab2), race=False)
    lab, sc = k.out("labels", px, k.torch.uint8), k.out("score", px, k.torch.float32)
    return lambda st: k.L.vitx_op_dense_labels_packed_tables(x.p, ld, t.p, n, tiles, cells, K, lab, sc, st)


def _op_depth_fine_packed_tables(k):
    K, ld, n, u = 8, 8, 2, 2
    rows = sum(a * b for a, b in PACK_GRIDS)
    fines = [(u * a, u * b) for a, b in PACK_GRIDS]
    tab, ft, _, cells = k.B.depth_pack_tables(PACK_GRIDS, fines, [0, 6], [0, 1], u)
    tab2, ft2, _, cells2 = k.B.depth_pack_tables(PACK_GRIDS[::-1], fines[::-1], [0, 5], [0, 1], u)
    assert (ft, cells, tab.shape) == (ft2, cells2, tab2.shape) and not np.array_equal(tab, tab2)
    x, off, bins = k.inp(k.f32((rows, ld), 1)), k.inp(k.f32((n, ld), 2, 0.3), seed=2), k.const(k.B.depth_bins(K, 0.5, 10.0))
    t = k.inp(_dev(k.torch, tab), _dev(k.torch, tab2), race=False)
    fine = k.out("fine planes", sum(a * b for a, b in fines), k.torch.float32)
    return lambda st: k.L.vitx_op_depth_fine_packed_tables(x.p, ld, off.p, ld, bins, t.p, n, ft, cells, K, fine, st)


def _op_depth_resize_packed_tables(k):
    """The table vitx_op_depth_resize_packed builds: the fine planes stand in for the grids (u = 1), rows and offsets zero."""
    n = 2
    fines, outs = [(4, 6), (2, 10)], [(9, 11), (5, 17)]
    tab, _, ot, _ = k.B.depth_pack_tables(fines, outs, [0, 0], [0, 0], 1)
    tab2, _, ot2, _ = k.B.depth_pack_tables(fines[::-1], outs[::-1], [0, 0], [0, 0], 1)
    assert (ot, tab.shape) == (ot2, tab2.shape) and not np.array_equal(tab, tab2)
    x = k.inp(np.abs(k.f32((sum(a * b for a, b in fines),), 1, 2.0)) + 0.5, positive=True)
    t = k.inp(_dev(k.torch, tab), _dev(k.torch, tab2), race=False)
    o = k.out("depth", sum(a * b for a, b in outs), k.torch.float32)
    return lambda st: k.L.vitx_op_depth_resize_packed_tables(x.p, t.p, n, ot, 0.5, 10.0, o, st)


def _op_text_embed(k):
    """The ids are not checked by the entry point: the decoy ids are other ids inside the vocabulary."""
    n, T, D, V = 2, 16, 64, 96
    ids = np.random.default_rng(7).integers(0, V, (n, T)).astype(np.int32)
    tok, pos = k.const(k.f32((V, D), 1)), k.const(k.f32((T, D), 2))
    i, x = k.inp(_dev(k.torch, ids), _dev(k.torch, S.decoy_index(ids, V, 7))), k.out("x", n * T * D, k.torch.float32)
    return lambda st: k.L.vitx_op_text_embed(0, tok, pos, i.p, x, n, T, D, st)


def _op_text_pool(k):
    n, T, D = 2, 16, 128
    pooled = np.array([5, 15], np.int32)
    x, w, b = k.inp(k.f32((n * T, D), 1)), k.const(k.f32((D,), 2)), k.const(k.f32((D,), 3))
    p, z = k.inp(_dev(k.torch, pooled), _dev(k.torch, S.decoy_index(pooled, T, 7)), race=False), k.out("z", n * D, k.t16[BF])
    return lambda st: k.L.vitx_op_text_pool(BF, x.p, p.p, w, b, z, n, T, D, 1e-6, st)


def _pos_resample(gout):
    def build(k):
        D, gin = 64, (2, 2)
        x, o = k.inp(k.f32((1 + gin[0] * gin[1], D), 1)), k.out("table", (1 + gout[0] * gout[1]) * D, k.torch.float32)
        return lambda st: k.L.vitx_op_pos_embed_resample(x.p, gin[0], gin[1], D, gout[0], gout[1], 0, o, st)
    return build


def _op_quantize_mxfp8(k):
    rows, K, kp = 5, 64, 128
    x, q, s = k.inp(k.f32((rows, K), 1)), k.out("elements", rows * kp, k.torch.uint8), k.out("scales", rows * kp // 32, k.torch.uint8)
    return lambda st: k.L.vitx_op_quantize_mxfp8(x.p, rows, K, kp, q, s, st)


def _op_layernorm_mxfp8(k):
    M, D = 5, 128
    x, w, b = k.inp(k.f32((M, D), 1)), k.const(k.f32((D,), 2)), k.const(k.f32((D,), 3))
    q, s = k.out("elements", M * D, k.torch.uint8), k.out("scales", M * D // 32, k.torch.uint8)
    return lambda st: k.L.vitx_op_layernorm_mxfp8(x.p, w, b, q, s, M, D, 1e-6, st)


def _op_gemm_mxfp8(k):
    M, N, K = 5, 64, 64
    real = k.f32((M, K), 1)
    (qa, sa), (qd, sd) = k.B.mxfp8_quantize(real), k.B.mxfp8_quantize(S.decoy_f32(real, 1))
    qw, sw = k.B.mxfp8_quantize(np.concatenate([k.f32((N, K), 2), np.zeros((128 - N, K), np.float32)]))
    a, as_ = k.inp(_dev(k.torch, qa), _dev(k.torch, qd)), k.inp(_dev(k.torch, sa), _dev(k.torch, sd), race=False)
    w, ws, bias, o = k.const(qw), k.const(sw), k.const(np.zeros(N, np.float32) + 0.5), k.out("out", M * N, k.torch.bfloat16)
    return lambda st: k.L.vitx_op_gemm_mxfp8(0, a.p, as_.p, w, ws, bias, o, None, M, N, K, st)


def _op_preprocess_u8_device(k):
    n, nx, ny, side = 2, 23, 17, 16
    x, o = k.inp(S.real_u8((n, ny, nx, 3), 1)), k.out("images", n * side * side * 3, k.torch.float32)
    return lambda st: k.L.vitx_preprocess_u8_device(x.p, n, nx, ny, side, 0, o, st)


def _op_preprocess_rect_device(k):
    n, nx, ny, ow, oh = 2, 23, 17, 16, 12
    pp = k.B.Preproc.make(k.B.PP_STRETCH, ow, ow, k.B.PP_PIL_BICUBIC, 0, 0, (123.675, 116.28, 103.53), (58.395, 57.12, 57.375))
    k.keep.append(pp)
    x, o = k.inp(S.real_u8((n, ny, nx, 3), 1)), k.out("images", n * oh * ow * 3, k.torch.float32)
    return lambda st: k.L.vitx_preprocess_rect_device(C.byref(pp), x.p, n, nx, ny, ow, oh, o, st)


# case id -> (the entry point, its builder)
OPS = {
    "layernorm": ("vitx_op_layernorm", _op_layernorm),
    "layernorm_f32": ("vitx_op_layernorm_f32", _op_layernorm_f32),
    "gemm": ("vitx_op_gemm", _op_gemm),
    "gemm_ex": ("vitx_op_gemm_ex", _op_gemm_ex),
    "gemm_q4": ("vitx_op_gemm_q4", _op_gemm_q4),
    "dequant": ("vitx_op_dequant", _op_dequant),
    "dequant_jobs": ("vitx_op_dequant_jobs", _op_dequant_jobs),
    "attention": ("vitx_op_attention", _attention(None)),
    "attention_ex-single": ("vitx_op_attention_ex", _attention(1)),
    "attention_ex-flow": ("vitx_op_attention_ex", _attention(3)),
    "attention_ex-persist": ("vitx_op_attention_ex", _attention(4, N=197)),
    "attention_ex-stream": ("vitx_op_attention_ex", _attention(5)),
    "attention_ex-single-f16": ("vitx_op_attention_ex", _attention(1, dtype=HF)),
    "attention_cls": ("vitx_op_attention_cls", _op_attention_cls),
    "attention_planes": ("vitx_op_attention_planes", _op_attention_planes),
    "attention_generic": ("vitx_op_attention_generic", _op_attention_generic),
    "attention_text": ("vitx_op_attention_text", _op_attention_text),
    "attention_packed_tables": ("vitx_op_attention_packed_tables", _op_attention_packed_tables),
    "rope": ("vitx_op_rope", _op_rope),
    "swiglu": ("vitx_op_swiglu", _op_swiglu),
    "softmax": ("vitx_op_softmax", _softmax(None)),
    "softmax_dt": ("vitx_op_softmax_dt", _softmax(BF)),
    "topk": ("vitx_op_topk", _op_topk),
    "attention_map": ("vitx_op_attention_map", _op_attention_map),
    "rollout_factor": ("vitx_op_rollout_factor", _op_rollout_factor),
    "rollout_step": ("vitx_op_rollout_step", _op_rollout_step),
    "rollout_row": ("vitx_op_rollout_row", _op_rollout_row),
    "features": ("vitx_op_features", _features(False)),
    "features_ex": ("vitx_op_features_ex", _features(True)),
    "attention_pool": ("vitx_op_attention_pool", _op_attention_pool),
    "zeroshot": ("vitx_op_zeroshot", _op_zeroshot),
    "nn_select": ("vitx_op_nn_select", _op_nn_select),
    "nn_finish": ("vitx_op_nn_finish", _op_nn_finish),
    "nn": ("vitx_op_nn", _op_nn),
    "dense_labels": ("vitx_op_dense_labels", _op_dense_labels),
    "dense": ("vitx_op_dense", _op_dense),
    "depth_fine": ("vitx_op_depth_fine", _op_depth_fine),
    "depth_resize": ("vitx_op_depth_resize", _op_depth_resize),
    "depth": ("vitx_op_depth", _op_depth),
    "depth_rows": ("vitx_op_depth_rows", _op_depth_rows),
    "dense_labels_packed_tables": ("vitx_op_dense_labels_packed_tables", _op_dense_labels_packed_tables),
    "depth_fine_packed_tables": ("vitx_op_depth_fine_packed_tables", _op_depth_fine_packed_tables),
    "depth_resize_packed_tables": ("vitx_op_depth_resize_packed_tables", _op_depth_resize_packed_tables),
    "text_embed": ("vitx_op_text_embed", _op_text_embed),
    "text_pool": ("vitx_op_text_pool", _op_text_pool),
    "pos_embed_resample": ("vitx_op_pos_embed_resample", _pos_resample((3, 4))),
    "pos_embed_resample-identity": ("vitx_op_pos_embed_resample", _pos_resample((2, 2))),       # equal grids: a copy, not a kernel
    "quantize_mxfp8": ("vitx_op_quantize_mxfp8", _op_quantize_mxfp8),
    "layernorm_mxfp8": ("vitx_op_layernorm_mxfp8", _op_layernorm_mxfp8),
    "gemm_mxfp8": ("vitx_op_gemm_mxfp8", _op_gemm_mxfp8),
    "preprocess_u8_device": ("vitx_preprocess_u8_device", _op_preprocess_u8_device),
    "preprocess_rect_device": ("vitx_preprocess_rect_device", _op_preprocess_rect_device),
}

# the enqueue-only entry points that take a context, and the tests above that stall them
COVERED = {
    "vitx_forward_device": "test_sixteen_images_on_two_sub_batch_streams",
    "vitx_pack_forward_device": "test_packed_calls_back_to_back_on_a_caller_stream",
    "vitx_text_embed_device": "test_text_embed_device_twice_with_the_host_ids_overwritten",
    "vitx_preprocess_ex_device": "test_pipeline_u8_preprocess_forward",
}
COVERED.update({entry: "test_op_entry_under_the_stall" for entry, _ in OPS.values()})


@pytest.mark.parametrize("case", list(OPS))
def test_op_entry_under_the_stall(binding, torch_gpu, case):
    """One vitx_op_* entry at a small shape its own checks accept: its operands produced behind the stall (tables in order, data also as the
    control's race), every output snapshotted in stream order, bit for bit the fenced launch."""
    entry, build = OPS[case]
    kit = Kit(torch_gpu, binding)
    launch = build(kit)
    S.harness(torch_gpu).check(f"{entry} [{case}]", lambda: [OpStep(kit, entry, launch)])
