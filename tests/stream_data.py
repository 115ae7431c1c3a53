"""Stream order: the stall harness of tests/test_gpu_stream_order.py and the two tables of tests/test_cpu_stream_contract.py.

include/vitx.h promises of every entry point with a `void *stream` that it "only enqueues on `stream`", and of the buffers behind the *_device
accessors that they are "written by the forward's streams: work that reads it is ordered after the caller's stream, like d_probs".  A test that
synchronises before and after a call cannot see a missing dependency edge: on the tiny fixtures the GPU is idle again before the host has enqueued
the next thing.  Here the caller's stream is STALLED while the host enqueues, so that nothing on it can have run when the call returns.

A scenario is a list of steps (Step); on the caller's stream s, with no host wait anywhere:
    the stall, the `open` event behind it
    per step:  producers     hipMemcpyAsync of the real input over the decoy that has been sitting in the input buffer
               the call      under test, on s
               snapshots     hipMemcpyAsync of every output into buffers prefilled with a sentinel
               decoy back    hipMemcpyAsync of the decoy over the input again
    one s.synchronize().
The snapshots must carry the bits of the same calls made the fenced way (a synchronise before and after each) on a second context of the same
options.  A consumer that starts early reads the decoy; a missing join leaves the sentinel in place (every output source is refilled with the
sentinel before a run) or reads the decoy that came back; an output written behind the join leaves the sentinel.

What keeps a pass from being vacuous, all asserted:
  1. `still_stalled(open)` right after the stalled call returns: the host did not wait for the stream, and the GPU cannot have begun.
  2. The stall is 5 x the measured host time of the same enqueue sequence (unstalled, time.perf_counter) + 5 ms, at most MAX_STALL_MS.
  3. Few hardware queues serve many streams; a caller stream that shares a queue with the stream a missing edge would let run ahead serialises
     behind the stall and hides the fault.  So every scenario runs on each of four caller streams that stay alive, and each gets a CONTROL: the
     same scenario with the stall and the producer on another stream (`rogue`) and NO event to the stream passed to the call -- a race of the
     test's own making on its own finite buffers.  Where the call's stream really runs beside `rogue` the call reads the decoy and the result
     differs from the fenced one: the stream discriminates.  Where it does not differ the stream is reported as non-discriminating; at least one
     of the four must discriminate.
One `STALL` line per scenario (pytest -s): host enqueue ms, stall ms, the discriminating streams and, for a scenario of several calls, the streams
on which the stall was still running when the LAST call had been enqueued (a report: calls behind a documented host wait cannot be).

What it cannot prove: an edge that is missing between two streams that happen to share a hardware queue on this run, and anything about timing.

Decoys are valid finite data of another seed (ids: other valid ids; tables: other valid tables of the same shape), never NaN and never out of
range: a wrong read gives a wrong answer and nothing else.  Sentinels are finite values no output takes (sentinel()).
"""
import ctypes as C
import re
import time

import numpy as np

MAX_STALL_MS = 250.0
STALL_FACTOR, STALL_FLOOR_MS = 5.0, 5.0
N_STREAMS = 4

# ================================================================================================ the two tables (tests/test_cpu_stream_contract.py)
# Every prototype of include/vitx.h with a `void *stream` parameter stands in exactly one of them.
# ENQUEUE_ONLY: name -> the header's words for a host wait the entry point documents all the same (None: none); tests/test_gpu_stream_order.py
# stalls each of them (its COVERED table says where).
ENQUEUE_ONLY = {
    "vitx_forward_device": "synchronises the host once for ~0.2 ms while it measures whether its internal sub-batch stream really runs beside the caller's",
    "vitx_pack_forward_device": "after waiting for the previous call's upload of the segment tables -- not for its forward",
    "vitx_text_embed_device": "after waiting for the previous call's upload of ids -- not for its forward -- to leave the context's staging buffer",
    "vitx_preprocess_ex_device": None,
    "vitx_preprocess_u8_device": None,
    "vitx_preprocess_rect_device": None,
    "vitx_op_pos_embed_resample": None,
    "vitx_op_rope": None,
    "vitx_op_swiglu": None,
    "vitx_op_layernorm": None,
    "vitx_op_layernorm_f32": None,
    "vitx_op_gemm": None,
    "vitx_op_gemm_ex": None,
    "vitx_op_gemm_q4": None,
    "vitx_op_dequant": None,
    "vitx_op_dequant_jobs": None,
    "vitx_op_attention": None,
    "vitx_op_attention_ex": None,
    "vitx_op_attention_cls": None,
    "vitx_op_attention_planes": None,
    "vitx_op_attention_generic": None,
    "vitx_op_attention_text": None,
    "vitx_op_attention_packed_tables": None,
    "vitx_op_softmax": None,
    "vitx_op_softmax_dt": None,
    "vitx_op_topk": None,
    "vitx_op_attention_map": None,
    "vitx_op_rollout_factor": None,
    "vitx_op_rollout_step": None,
    "vitx_op_rollout_row": None,
    "vitx_op_features": None,
    "vitx_op_features_ex": None,
    "vitx_op_attention_pool": None,
    "vitx_op_zeroshot": None,
    "vitx_op_nn_select": None,
    "vitx_op_nn_finish": None,
    "vitx_op_nn": None,
    "vitx_op_dense_labels": None,
    "vitx_op_dense": None,
    "vitx_op_depth_fine": None,
    "vitx_op_depth_resize": None,
    "vitx_op_depth": None,
    "vitx_op_depth_rows": None,
    "vitx_op_dense_labels_packed_tables": None,
    "vitx_op_depth_fine_packed_tables": None,
    "vitx_op_depth_resize_packed_tables": None,
    "vitx_op_text_embed": None,
    "vitx_op_text_pool": None,
    "vitx_op_quantize_mxfp8": None,
    "vitx_op_layernorm_mxfp8": None,
    "vitx_op_gemm_mxfp8": None,
}
# HOST_WAITS: name -> the header's own words for the wait.  Test-only or synchronising entry points: listed, not stalled.
HOST_WAITS = {
    "vitx_op_gemm_ln": "Synchronous.",
    "vitx_op_attention_f32": "it allocates and frees its own scratch and synchronises `stream` on every call",
    "vitx_op_patch_embed": "TEST ONLY: it allocates, uploads and synchronises",
    "vitx_op_attention_packed": "it reads d_row0 back to build that count (synchronises)",
    "vitx_op_rope_packed": "reads both tables back to check them (synchronises)",
    "vitx_op_dense_labels_packed": "it builds and uploads the tables and frees them after the launch (synchronises)",
    "vitx_op_depth_fine_packed": "they build and upload the tables and free them after the launch (synchronise)",
    "vitx_op_depth_resize_packed": "they build and upload the tables and free them after the launch (synchronise)",
}


def header_text(path):
    """include/vitx.h with its comment decoration (line breaks, the leading ` * `) folded to single blanks: the form HOST_WAITS quotes."""
    with open(path) as f:
        lines = [re.sub(r"^\s*/?\*+/?\s?", "", ln.rstrip("\n")) for ln in f]
    return re.sub(r"\s+", " ", " ".join(lines))


def stream_prototypes(path):
    """Names of the prototypes of include/vitx.h that take a `void *stream`, in file order."""
    with open(path) as f:
        src = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    names = []
    for m in re.finditer(r"\b(vitx_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            names.append(m.group(1))
    return names


# ================================================================================================ decoys and sentinels (numpy; CPU-checked)
def real_f32(shape, seed, scale=1.0):
    """Finite f32 data: scale * N(0, 1), clipped to 4 scale."""
    x = np.random.default_rng(seed).standard_normal(shape) * scale
    return np.clip(x, -4.0 * scale, 4.0 * scale).astype(np.float32)


def decoy_f32(real, seed, scale=None, positive=False):
    """Valid finite f32 data of another seed, the same shape and range as `real`, and at least scale / 8 away from it in EVERY element: the
    difference survives the rounding to fp16 and to bf16 (an ulp at 4 scale is scale / 64).  positive: no element is negative (weights of a
    map, probabilities, depths)."""
    real = np.asarray(real, np.float32)
    s = float(scale if scale is not None else max(float(np.abs(real).max()) / 4.0, 1e-3))
    d = real_f32(real.shape, seed + 7919, s)
    if positive:
        d = np.abs(d)
    near = np.abs(d - real) < s / 8.0
    away = real + s / 2.0 if positive else np.where(real > 0, real - s / 2.0, real + s / 2.0)
    return np.where(near, away, d).astype(np.float32)


def real_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def decoy_u8(real, seed):
    """Other bytes: every element differs (real + 1 .. 255 modulo 256)."""
    step = np.random.default_rng(seed + 7919).integers(1, 256, size=np.shape(real))
    return ((np.asarray(real).astype(np.int64) + step) % 256).astype(np.uint8)


def decoy_index(real, bound, seed):
    """Other valid indices in [0, bound): every element differs (real + 1 .. bound - 1 modulo bound); bound >= 2."""
    assert bound >= 2
    step = np.random.default_rng(seed + 7919).integers(1, bound, size=np.shape(real))
    return ((np.asarray(real).astype(np.int64) + step) % bound).astype(np.int32)


def decoy_prompts(real, V, eos, seed):
    """Other valid prompts for a text tower: ids in [0, V), every row still holds `eos` where it held it (eos < 0: none needed), every other
    position differs from `real`."""
    real = np.asarray(real, np.int32)
    if eos < 0:
        return decoy_index(real, V, seed)
    # a draw from the V - 2 ids that are neither the real one nor EOS (a new early EOS would move the pooled position): skip the two in order
    d = np.random.default_rng(seed + 7919).integers(0, V - 2, size=real.shape)
    lo, hi = np.minimum(real, eos), np.maximum(real, eos)
    d = d + (d >= lo)
    d = d + (d >= hi)
    return np.where(real == eos, eos, d).astype(np.int32)


SENTINELS = {"float32": -3.0e38, "float16": -65504.0, "bfloat16": -3.0e38, "uint8": 255, "int32": -0x7B7B7B7B}


def sentinel(dtype_name):
    """A finite value of the type that no output of this project takes: probabilities, logits, features, maps, depths and operands are orders of
    magnitude inside +-3e38 (fp16: the one value a GEMM output reaches only by overflowing); labels are below 255 classes in every case here and
    255 is NaN as an e4m3 byte and as an E8M0 scale, which the MX encoders never write; indices are non-negative."""
    return SENTINELS[dtype_name]


# ================================================================================================ HIP through ctypes
_hip = None


def hip():
    global _hip
    if _hip is None:
        h = C.cdll.LoadLibrary("libamdhip64.so")
        h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        h.hipMemcpyAsync.restype = C.c_int
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipMemcpy.restype = C.c_int
        _hip = h
    return _hip


def copy_async(dst_ptr, src_ptr, nbytes, stream):
    """hipMemcpyAsync device to device on the raw stream handle `stream`: a snapshot (or a producer) in stream order."""
    rc = hip().hipMemcpyAsync(C.c_void_p(dst_ptr), C.c_void_p(src_ptr), nbytes, 3, C.c_void_p(stream))
    assert rc == 0, f"hipMemcpyAsync: {rc}"


def device_bytes(ptr, nbytes):
    """Blocking copy of device memory to the host (the fenced way)."""
    out = np.empty(nbytes, np.uint8)
    rc = hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), nbytes, 2)
    assert rc == 0, f"hipMemcpy: {rc}"
    return out


def still_stalled(open_event):
    return not open_event.query()


_rate = {}


def cycles_per_ms(torch):
    """torch.cuda._sleep cycles per millisecond, once per session: two sleeps of different lengths timed with events; the DIFFERENCE, so that
    the launch latency cancels."""
    if "r" not in _rate:
        s = torch.cuda.Stream()

        def timed(cycles):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                a.record(s); torch.cuda._sleep(cycles); b.record(s)
            s.synchronize()
            return a.elapsed_time(b)
        timed(100_000)                                   # wake the queue up
        short, long = 1_000_000, 5_000_000
        t_short, t_long = min(timed(short) for _ in range(2)), min(timed(long) for _ in range(2))
        assert t_long > t_short > 0.0, (t_short, t_long)
        _rate["r"] = (long - short) / (t_long - t_short)
    return _rate["r"]


def stall(torch, stream, ms):
    """A do-nothing kernel of `ms` milliseconds on `stream`."""
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * cycles_per_ms(torch)))


# ================================================================================================ steps
class Input:
    """An input buffer of a call: `buf` (what the call reads; the decoy sits in it), the real data and the decoy, device tensors of one shape.
    race: the control may produce it on the rogue stream (tables are always produced in order: a torn table is not finite data)."""

    def __init__(self, real, decoy, race=True):
        assert real.shape == decoy.shape and real.dtype == decoy.dtype and real.is_contiguous() and decoy.is_contiguous()
        self.real, self.decoy, self.buf, self.race = real, decoy, decoy.clone(), race
        self.nbytes = real.numel() * real.element_size()

    @property
    def p(self):
        return self.buf.data_ptr()


class Snap:
    """A snapshot of `nbytes` at src() (a device pointer, resolved when enqueued) into a buffer prefilled with the sentinel of `dtype`.
    refill: the source is refilled with the sentinel before a run too (everything but an in-place input, which gets its decoy back)."""

    def __init__(self, torch, name, src, numel, dtype, refill=True):
        self.name, self.src, self.refill = name, (src if callable(src) else (lambda p=src: p)), refill
        self.sent = torch.full((numel,), sentinel(str(dtype).replace("torch.", "")), dtype=dtype, device="cuda")
        self.dst = self.sent.clone()
        self.nbytes = numel * self.sent.element_size()

    @property
    def p(self):
        return self.src()


class Step:
    """One call under test with its producers and snapshots.  call(fenced, stream): the call on the raw stream handle -- fenced: on the second
    context, between synchronises.  expected(): {name: bytes} after the fenced call (default: the snapshots' sources, read the blocking way).
    late(): {name: bytes} of outputs that have no device accessor, read after the final synchronise on the stalled side (default: none).
    after_call(): a host action the moment the call has returned (the text context: the id array is overwritten).  dirty(): before a run, leaves
    something other than the expected values in outputs that late() reads."""
    inputs = ()
    snaps = ()

    def call(self, fenced, stream):
        raise NotImplementedError

    def expected(self):
        return {s.name: device_bytes(s.src(), s.nbytes) for s in self.snaps}

    def late(self):
        return {}

    def after_call(self):
        pass

    def dirty(self):
        pass

    def close(self):
        pass


class Harness:
    """Four caller streams and the rogue stream of the controls, alive together for the whole session."""

    def __init__(self, torch):
        self.torch = torch
        self.streams = [torch.cuda.Stream() for _ in range(N_STREAMS)]
        self.rogue = torch.cuda.Stream()
        self.fence = torch.cuda.Stream()               # the stream of the fenced calls
        cycles_per_ms(torch)
        c_real = torch.arange(64, dtype=torch.int32, device="cuda")
        self.canary = Input(c_real, c_real + 1000)
        self.canary_snap = Snap(torch, "canary", self.canary.p, 64, torch.int32, refill=False)
        self.lines = []

    # ---- the fenced way
    def reference(self, steps):
        torch = self.torch
        want = []
        self.reset(steps)                                # what a call leaves unwritten (pad rows) holds the sentinel on both sides
        for st in steps:
            for i in st.inputs:
                i.buf.copy_(i.real)
            torch.cuda.synchronize()
            st.call(True, self.fence.cuda_stream)
            torch.cuda.synchronize()
            want.append(st.expected())
            for i in st.inputs:
                i.buf.copy_(i.decoy)
            torch.cuda.synchronize()
        return want

    def reset(self, steps):
        torch = self.torch
        torch.cuda.synchronize()
        for st in steps:
            for i in st.inputs:
                i.buf.copy_(i.decoy)
        torch.cuda.synchronize()
        for st in steps:
            st.dirty()
        torch.cuda.synchronize()
        for st in steps:
            for sn in st.snaps:
                sn.dst.copy_(sn.sent)
                if sn.refill:
                    copy_async(sn.src(), sn.sent.data_ptr(), sn.nbytes, 0)
        self.canary.buf.copy_(self.canary.decoy); self.canary_snap.dst.copy_(self.canary_snap.sent)
        torch.cuda.synchronize()

    # ---- the stalled way: no host wait from the first enqueue to the synchronise
    def enqueue(self, steps, plan, stall_at, stall_ms, control):
        torch = self.torch
        stalled, opened = None, None
        t0 = time.perf_counter()
        for k, st in enumerate(steps):
            s = plan[k]
            if k > 0 and plan[k - 1] is not s:           # a caller that alternates streams joins them with an event
                ev = torch.cuda.Event(); ev.record(plan[k - 1]); s.wait_event(ev)
            first = k == stall_at
            lead = self.rogue if (control and first) else s
            if first and stall_ms > 0.0:
                stall(torch, lead, stall_ms)
                opened = torch.cuda.Event(); opened.record(lead)
            racing = [i for i in st.inputs if i.race]
            for i in st.inputs:
                copy_async(i.p, i.real.data_ptr(), i.nbytes, (lead if i.race else s).cuda_stream)
            if first and not racing:
                copy_async(self.canary.p, self.canary.real.data_ptr(), self.canary.nbytes, lead.cuda_stream)
            st.call(False, s.cuda_stream)
            if first and opened is not None and not control:
                stalled = still_stalled(opened)
            st.after_call()
            for sn in st.snaps:
                copy_async(sn.dst.data_ptr(), sn.src(), sn.nbytes, s.cuda_stream)
            if first and not racing:
                copy_async(self.canary_snap.dst.data_ptr(), self.canary.p, self.canary.nbytes, s.cuda_stream)
            for i in st.inputs:
                copy_async(i.p, i.decoy.data_ptr(), i.nbytes, s.cuda_stream)
        host_ms = (time.perf_counter() - t0) * 1e3
        self.stalled_at_end = opened is not None and still_stalled(opened)
        plan[len(steps) - 1].synchronize()               # the one synchronise that ends it (later streams wait for the earlier ones)
        if control:
            self.rogue.synchronize()
        torch.cuda.synchronize()                         # (after the scenario: nothing of it may still run when the buffers are reset)
        return host_ms, stalled

    def collect(self, steps, stall_at):
        got = []
        for k, st in enumerate(steps):
            d = {sn.name: _bytes(self.torch, sn.dst) for sn in st.snaps}
            d.update(st.late())
            if k == stall_at and not any(i.race for i in st.inputs):
                d["canary"] = _bytes(self.torch, self.canary_snap.dst)
            got.append(d)
        return got

    def check(self, name, make, stall_at=0, plan=None, fresh=False):
        """Run the scenario of make() -> [Step] on each caller stream, stalled and as its control; print the STALL line; assert the snapshots,
        the three conditions.  plan(s) -> the caller stream of every step (default: all on s).  fresh: make() builds new contexts per run
        (closed after it); otherwise it is called once."""
        try:
            self._check(name, make, stall_at, plan, fresh)
        except Exception:
            # trouble ends it: once the device reports an error of its own (a fault is sticky), nothing more is started on it in this session
            rc = hip().hipDeviceSynchronize()
            if rc != 0:
                import pytest
                pytest.exit(f"{name}: the device reports HIP error {rc}: no further GPU work is started", returncode=3)
            raise

    def _check(self, name, make, stall_at, plan, fresh):
        torch = self.torch
        built = []

        def steps_of():
            if fresh or not built:
                built.append(make())
            return built[-1]

        def done(steps):
            if fresh:
                for st in steps:
                    st.close()
        plan = plan or (lambda s, n: [s] * n)
        steps = steps_of()
        want = self.reference(steps)
        canary_want = _bytes(torch, self.canary.real)
        for w in want:
            assert all(v.size for v in w.values())
        if not any(i.race for i in steps[stall_at].inputs):
            want[stall_at] = dict(want[stall_at], canary=canary_want)
        done(steps)
        # the host side of the same enqueue sequence, unstalled
        steps = steps_of()
        self.reset(steps)
        host_ms, _ = self.enqueue(steps, plan(self.streams[0], len(steps)), stall_at, 0.0, False)
        failed = _differences(self.collect(steps, stall_at), want, "unstalled")
        done(steps)
        stall_ms = STALL_FACTOR * host_ms + STALL_FLOOR_MS
        assert stall_ms <= MAX_STALL_MS, f"{name}: the host needs {host_ms:.1f} ms to enqueue: a stall of {stall_ms:.0f} ms is above the {MAX_STALL_MS:.0f} ms a scenario may wait"
        discriminating, to_the_end = [], []
        for j, s in enumerate(self.streams):
            steps = steps_of()
            self.reset(steps)
            _, stalled = self.enqueue(steps, plan(s, len(steps)), stall_at, stall_ms, False)
            if self.stalled_at_end:
                to_the_end.append(j)
            if not stalled:
                failed.append(f"stream {j}: the stall had ended when the call returned: the host waited for the stream (or for {stall_ms:.0f} ms)")
            failed += _differences(self.collect(steps, stall_at), want, f"stream {j}")
            done(steps)
            steps = steps_of()
            self.reset(steps)
            self.enqueue(steps, plan(s, len(steps)), stall_at, stall_ms, True)
            if _differences(self.collect(steps, stall_at)[stall_at:stall_at + 1], want[stall_at:stall_at + 1], ""):
                discriminating.append(j)
            done(steps)
        line = f"STALL {name}: host enqueue {host_ms:.3f} ms, stall {stall_ms:.1f} ms, discriminating streams {discriminating} ({len(discriminating)} of {N_STREAMS})"
        if len(steps) > 1:
            line += f"; still stalled after the last call's enqueue on streams {to_the_end}"
        print(line); self.lines.append(line)
        assert not failed, f"{name}: {len(failed)} differences from the fenced calls:\n  " + "\n  ".join(failed[:40])
        assert discriminating, f"{name}: the control differs on none of the {N_STREAMS} caller streams: no stream here can show a missing edge"


def _bytes(torch, t):
    return t.contiguous().view(torch.uint8).cpu().numpy().copy()


def _differences(got, want, where):
    out = []
    for k, (g, w) in enumerate(zip(got, want)):
        for name, wv in w.items():
            gv = g.get(name)
            wv = np.ascontiguousarray(wv).view(np.uint8).ravel()
            if gv is None:
                out.append(f"{where}: call {k}: no {name}"); continue
            gv = np.ascontiguousarray(gv).view(np.uint8).ravel()
            if gv.shape != wv.shape:
                out.append(f"{where}: call {k}: the {name} have {gv.size} bytes, the fenced call's {wv.size}")
            elif not np.array_equal(gv, wv):
                bad = np.flatnonzero(gv != wv)
                out.append(f"{where}: call {k}: {bad.size} of {wv.size} bytes of the {name} differ from the fenced call, first at byte {int(bad[0])}")
    return out


_harness = {}


def harness(torch):
    if "h" not in _harness:
        _harness["h"] = Harness(torch)
    return _harness["h"]
