"""Packed batches at the sizes where the dispatcher, the segment tables and the table cache stop doing the trivial thing (include/vitx.h "packed
batches"; data and restatements in tests/pack_data.py, their host checks in tests/test_cpu_pack.py).

1. The wide fixtures (D 512: every GEMM of a layer can leave the 64 x 128 tiles) on a ladder of row counts that walks every combination of GEMM
   families from "all 122" to "all pp", one context per (fixture, type), largest call first so that smaller calls see stale pad rows: every image of
   every call has the bits of the same image in a reference call of one row block (probabilities, logits, VITX_FEAT_CLS, VITX_FEAT_TOKENS); so has
   a call of 1025 (513) images of two (six) rows; NaN neighbours change nothing; `launches` is the count derived from pack_forward; the probes lie
   inside the gates of tests/test_gpu_pack.py around their float64 restatement, the mutants of pack_data.SCALE_MUTANTS outside.
2. The rotary arena restart on the p14rope micro fixture against a context whose arena never fills, bit for bit, with scratch_bytes following the
   cache trace.
3. Back-to-back vitx_pack_forward_device calls with no host synchronisation, one of them evicting and one restarting, against the same calls
   made one at a time.

Measured on an MI355X, worst probe, distance / gate (max|dprob| against 2e-2; patch rows rms(d) / rms against 2.5e-2):
    vit_erf      F16 1.85e-4 = 0.009, 1.41e-4 = 0.006      BF16 2.01e-3 = 0.101, 9.85e-4 = 0.039      (six probes)
    dinov3_rope  F16 4.94e-4 = 0.025, 4.54e-4 = 0.018      BF16 4.67e-3 = 0.234, 3.40e-3 = 0.136      (six probes)
    glu_hplus    F16 9.93e-4 = 0.050, 9.96e-4 = 0.040      BF16 1.46e-3 = 0.073, 8.31e-3 = 0.332      (the 2 x 2 probe)
"""
import numpy as np
import pytest

import pack_data as KD
import prefix_data as PD
import rect_data as XD
import wide_data as WD
from test_gpu_pack import GATE, SENT, TOKEN_GATE

pytestmark = pytest.mark.gpu

NAME = {0: "F16", 1: "BF16"}
CASES = [(k, d) for k in KD.SCALE_KEYS for d in (0, 1)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the ladder
class _State:
    """The context of a (fixture, type) -- created at the top rung's row count -- with the reference outputs of the 14 distinct images."""

    def __init__(self, pkg, binding, key, dtype):
        self.key, self.dtype, self.Tp = key, dtype, KD.prefix_rows(key)
        self.model = binding.Model(WD.fixture_file(pkg, key))
        assert self.model.hparams.num_hidden_layers == WD.L and (self.model.rope is not None) == (key != "vit_erf") and (self.model.glu is not None) == (key == "glu_hplus")
        self.pack = binding.PackContext(self.model, device=0, max_tokens=KD.ladder(key)[-1], max_images=KD.max_images(key), dtype=dtype)
        self.pack.feat_enable(cls=True, tokens=True)
        self.seen = {(WD.S // WD.P,) * 2}                # grids that need no position-table launch any more: the file's own never does
        self.imgs = KD.distinct_images()
        self.ref = [None] * KD.N_DISTINCT
        for call in KD.reference_calls(self.Tp):
            p, lg, cls, tok = self.run(call)
            for k, i in enumerate(call):
                self.ref[i] = (_bits(p[k]), _bits(lg[k]), _bits(cls[k]), _bits(tok[k]))
        self.rp, self.rl, self.rc = (np.stack([r[j] for r in self.ref]) for j in range(3))

    def run(self, ids, nan_at=()):
        """One forward of the images `ids` (those at the positions `nan_at` all NaN); `launches` is checked against the derivation on the way."""
        imgs = [np.full_like(self.imgs[i], np.nan) if k in nan_at else self.imgs[i] for k, i in enumerate(ids)]
        shapes = KD.shapes_of(ids)
        new = {KD.GRIDS[i] for i in ids} - self.seen
        p, lg = self.pack.forward(imgs)
        cls, tok = self.pack.feat_read()
        want = KD.pack_launches(shapes, WD.L, len(new), rope=self.key != "vit_erf", glu=self.key == "glu_hplus", feat=True)
        assert self.pack.launches == want, (self.key, len(ids), self.pack.launches, want)
        self.seen |= new
        return p, lg, cls, tok

    def check(self, ids, out, skip=(), what=""):
        """Every image of the call (but the positions `skip`) has the reference bits and is finite."""
        p, lg, cls, tok = out
        idx = np.asarray(ids)
        keep = np.ones(len(ids), bool); keep[list(skip)] = False
        bad = ((_bits(p) != self.rp[idx]).any(1) | (_bits(lg) != self.rl[idx]).any(1) | (_bits(cls) != self.rc[idx]).any(1)) & keep
        for k in np.flatnonzero(keep):
            if bad[k] or not np.array_equal(_bits(tok[k]), self.ref[ids[k]][3]):
                r0, rows = KD.row0_of_ids(ids, self.Tp), KD.rows_of(ids, self.Tp)
                which = [nm for nm, a, b in (("probs", _bits(p[k]), self.rp[idx[k]]), ("logits", _bits(lg[k]), self.rl[idx[k]]), ("cls", _bits(cls[k]), self.rc[idx[k]]),
                                             ("tokens", _bits(tok[k]), self.ref[ids[k]][3])) if not np.array_equal(a, b)]
                pytest.fail(f"{self.key} {NAME[self.dtype]} {what}: {rows} rows, families {KD.families(self.key, rows)}: image {k} (id {ids[k]}, grid {KD.GRIDS[ids[k]]}, rows "
                            f"{r0[k]} .. {r0[k + 1] - 1}) differs from the reference call in {which}")
        finite = np.isfinite(p[keep]).all() and np.isfinite(lg[keep]).all() and np.isfinite(cls[keep]).all() and all(np.isfinite(tok[k]).all() for k in np.flatnonzero(keep))
        assert finite, (self.key, what)

    def close(self):
        self.pack.close(); self.model.close()


_STATES = {}


@pytest.fixture(scope="module")
def states(pkg, binding, torch_gpu):
    def get(key, dtype):
        if (key, dtype) not in _STATES:
            _STATES[key, dtype] = _State(pkg, binding, key, dtype)
        return _STATES[key, dtype]
    yield get
    for s in _STATES.values():
        s.close()
    _STATES.clear()


@pytest.mark.parametrize("key,dtype", CASES)
def test_every_image_of_every_rung_has_the_reference_bits(states, key, dtype):
    """pack_data.ladder, largest call first, then the call of 1 x 1 images, then the reference calls again (behind all that stale data): every image
    equals its copy in the first reference calls in all four outputs.  Each call repeats 14 images over all of its rows, so every row block of
    every family a rung selects (pack_data.families; tests/test_cpu_pack.py) is compared with the 64 x 128 tiling of one row block, no tolerance."""
    s = states(key, dtype)
    for rows in KD.ladder(key)[::-1]:
        ids = KD.pack_ids(rows, s.Tp)
        s.check(ids, s.run(ids), what="ladder")
    ids = KD.small_pack_ids(s.Tp)
    s.check(ids, s.run(ids), what="1 x 1 images")
    for call in KD.reference_calls(s.Tp):
        s.check(call, s.run(call), what="reference again")


@pytest.mark.parametrize("key,dtype", CASES)
def test_poisoned_neighbours_at_scale(states, key, dtype):
    """The top rung and a middle rung with every other filler copy all NaN: the other images keep the reference bits and are finite."""
    s = states(key, dtype)
    lad = KD.ladder(key)
    for rows in (lad[-1], lad[len(lad) // 2]):
        ids = KD.pack_ids(rows, s.Tp)
        nan = KD.poisoned(ids)
        out = s.run(ids, nan_at=nan)
        assert all(np.isnan(out[0][k]).all() for k in list(nan)[:8])           # the poison did go through
        s.check(ids, out, skip=nan, what="poisoned")


_REF64 = {}


def _ref64(pkg, binding, key, dtype, i, mutant=None):
    k = (key, dtype, i, mutant)
    if k not in _REF64:
        if ("t", key) not in _REF64:
            _REF64["t", key] = PD.file_tensors(pkg, WD.fixture_file(pkg, key))
        _REF64[k] = KD.probe_ref(key, _REF64["t", key], i, dtype, mutant, binding)
    return _REF64[k]


@pytest.mark.parametrize("key,dtype", CASES)
def test_probes_against_float64(pkg, binding, states, key, dtype):
    """The probes' bits are those of every rung (the test above), so the reference call's outputs stand for all of them: each probe against
    ref64.forward64 at its own shape (glu_hplus: its 2 x 2 probe against wide_data.forward64) inside GATE and TOKEN_GATE; every mutant of
    pack_data.SCALE_MUTANTS outside one of them on at least one probe.  The preconditions are tests/test_cpu_pack.py::test_scale_probe_preconditions."""
    assert (GATE, TOKEN_GATE) == (KD.GATE, KD.TOKEN_GATE)
    s = states(key, dtype)
    got = {i: (s.ref[i][0].view(np.float32), s.ref[i][3].view(np.float32)) for i in KD.parity_probes(key)}
    d = {i: KD.probe_distance(*got[i], _ref64(pkg, binding, key, dtype, i)) for i in got}
    print(f"{key} {NAME[dtype]}: worst probe max|dprob| {max(a for a, _ in d.values()):.3e} = {max(a for a, _ in d.values()) / GATE:.3f} gates, "
          f"patch rows rms(d) / rms {max(b for _, b in d.values()):.3e} = {max(b for _, b in d.values()) / TOKEN_GATE:.3f} gates")
    assert all(a <= GATE and b <= TOKEN_GATE for a, b in d.values()), d
    for mut in KD.SCALE_MUTANTS.get(key, ()):
        dm = [KD.probe_distance(*got[i], _ref64(pkg, binding, key, dtype, i, mut)) for i in got if KD.mutant_applies(mut, KD.GRIDS[i])]
        assert any(a > GATE or b > TOKEN_GATE for a, b in dm), (key, dtype, mut, dm)


# ------------------------------------------------------------------------------------------------ 2. the rotary arena restart
def _cache_imgs(call, k):
    return KD.pack_of([(gh * 14, gw * 14) for gh, gw in call], seed=31 + k)


@pytest.mark.parametrize("max_grids", [32, 2])
@pytest.mark.parametrize("dtype", [0, 1])
def test_arena_restart_against_an_arena_that_never_fills(pkg, binding, torch_gpu, dtype, max_grids):
    """pack_data.CACHE_CALLS on a context of 40 tokens (an arena of 80 patch rows: restarts in calls 4 and 7, both naming a cached and a missing
    grid; with max_grids 2 evictions in between) and on one of 1024 tokens, where the trace shows neither: after every call the same bits in
    probabilities, logits and features, and scratch_bytes is what the trace says is held -- base + feature buffer + the pixel buffer of the host
    entry point + (gh gw + 1) D 4 per held grid other than the file's."""
    model = binding.Model(XD.fixture_file(pkg, KD.CACHE_KIND))
    D, P = model.hparams.hidden_size, model.hparams.patch_size
    small = binding.PackContext(model, device=0, max_tokens=KD.CACHE_MAX_TOKENS, max_images=2, dtype=dtype, max_grids=max_grids)
    roomy = binding.PackContext(model, device=0, max_tokens=KD.CACHE_ROOMY_TOKENS, max_images=2, dtype=dtype, max_grids=32)
    base = small.scratch_bytes
    fixed = base + KD.CACHE_MAX_TOKENS * D * 4 + KD.CACHE_MAX_TOKENS * P * P * 3 * 4
    trace = KD.cache_trace(KD.CACHE_CALLS, KD.CACHE_MAX_TOKENS, KD.CACHE_HALF, max_grids)
    assert sum(t["restarted"] for t in trace) >= 2
    for c in (small, roomy):
        c.feat_enable(cls=True, tokens=True)
    for k, (call, t) in enumerate(zip(KD.CACHE_CALLS, trace)):
        imgs = _cache_imgs(call, k)
        (p1, l1), (c1, t1) = small.forward(imgs), small.feat_read()
        (p2, l2), (c2, t2) = roomy.forward(imgs), roomy.feat_read()
        assert np.isfinite(p1).all() and np.isfinite(l1).all()
        same = np.array_equal(_bits(p1), _bits(p2)) and np.array_equal(_bits(l1), _bits(l2)) and np.array_equal(_bits(c1), _bits(c2)) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(t1, t2))
        assert same, (k, call, t)
        held = fixed + sum((gh * gw + 1) * D * 4 for gh, gw in t["held"] if (gh, gw) != KD.CACHE_FILE_GRID)
        assert small.scratch_bytes == held, (k, call, t, small.scratch_bytes - fixed)
    small.close(); roomy.close(); model.close()


# ------------------------------------------------------------------------------------------------ 3. back-to-back device calls
@pytest.mark.parametrize("own_stream", [True, False], ids=["context-stream", "caller-stream"])
def test_back_to_back_device_calls(pkg, binding, torch_gpu, own_stream):
    """pack_data.B2B_CALLS, max_grids 2: A (grids a, b), B (c, a: evicts b, builds c while A may still run) and C (restarts the arena) enqueued with no
    host synchronisation in between, pixels and outputs in the caller's device buffers: after one synchronise, probabilities and logits of all
    three have the bits of the same calls made one at a time with a synchronise after each.  Every call is valid; only host waits the API lets the
    caller omit are left out."""
    torch = torch_gpu
    model = binding.Model(XD.fixture_file(pkg, KD.CACHE_KIND))
    C = model.num_classes
    trace = KD.cache_trace(KD.B2B_CALLS, KD.B2B_MAX_TOKENS, KD.CACHE_HALF, 2)
    assert trace[1]["evicted"] and trace[2]["restarted"]
    shapes = [[(gh * 14, gw * 14) for gh, gw in call] for call in KD.B2B_CALLS]
    pix = [torch.from_numpy(np.concatenate([i.ravel() for i in _cache_imgs(call, 50 + k)])).cuda() for k, call in enumerate(KD.B2B_CALLS)]

    def outputs():
        return [(torch.full((2, C), SENT, dtype=torch.float32, device="cuda"), torch.full((2, C), SENT, dtype=torch.float32, device="cuda")) for _ in shapes]

    def context():
        return binding.PackContext(model, device=0, max_tokens=KD.B2B_MAX_TOKENS, max_images=2, dtype=binding.BF16, max_grids=2)
    one, want = context(), outputs()
    torch.cuda.synchronize()
    for x, s, (p, lg) in zip(pix, shapes, want):
        one.forward_device(x.data_ptr(), s, p.data_ptr(), lg.data_ptr())
        torch.cuda.synchronize()
    ctx, got = context(), outputs()
    stream = None if own_stream else torch.cuda.Stream()
    torch.cuda.synchronize()
    for x, s, (p, lg) in zip(pix, shapes, got):
        ctx.forward_device(x.data_ptr(), s, p.data_ptr(), lg.data_ptr(), stream=0 if own_stream else stream.cuda_stream)
    torch.cuda.synchronize()
    for k, ((p, lg), (wp, wl)) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(wp).all()) and bool((wp != SENT).all()) and bool((wl != SENT).all()), k
        assert np.array_equal(_bits(p.cpu().numpy()), _bits(wp.cpu().numpy())) and np.array_equal(_bits(lg.cpu().numpy()), _bits(wl.cpu().numpy())), ("call", "ABC"[k])
    one.close(); ctx.close(); model.close()
