"""Fixtures of the packed-batch tests (include/vitx.h "packed batches"), shared by tests/test_cpu_pack.py and tests/test_gpu_pack.py.

The restatement is tests/ref64.py::forward64 on every image of a pack alone, at its own shape: a packed context promises that an image's result
is a function of its own pixels and shape.  The micro fixtures are rect_data's (p16, p14r4, p14rope: D 128, L 2, 2 heads of 64).

VARIANTS are the same tensors read with 4 heads of 32 -- the head count is a header field, the qkv rows are laid out head by head either way -- so
that an image context runs the generic attention arithmetic too and a pack of one shape can be compared with a rectangular context bit for bit:
    p16h4, p14r4h4, p14ropeh4      rect_data's three fixtures
    gluh4                          swiglu_data's "hplus" (4 registers, `rope`, a gated MLP, class-token head)
    preerfh4                       arch_data's "tanh_pre" (a pre-norm, eps 1e-5) with the erf activation
ref64.forward64(..., heads=4) restates all five.

The second half serves tests/test_gpu_pack_scale.py: the GEMM dispatcher's rule (gemm_family), the ladder of row counts over the wide fixtures of
tests/wide_data.py and the packs of its rungs, the launch count of a packed forward, the probes' float64 references, and the table cache
(cache_trace) with the call sequences that restart the rotary arena."""
import dataclasses
import functools

import numpy as np

import arch_data as AD
import rect_data as XD
import ref64 as R64
import swiglu_data as SD
import wide_data as WD

HEADS4 = 4
VARIANTS = ("p16h4", "p14r4h4", "p14ropeh4", "gluh4", "preerfh4")
UNIFORM_SHAPE = {16: (48, 80), 14: (28, 70)}        # the one-shape pack of each patch size (rect_data.CASES' shapes)


def mixed_shapes(P):
    """The mixed pack: grids 1 x 1, 1 x 7, 5 x 2, 4 x 4 (the micro files' own grid), 2 x 5, 4 x 4 again and 1 x 1 again -- five distinct grids, token
    counts 2 .. 17 (6 .. 21 with registers), a repeated shape that is not adjacent to its twin."""
    return [(P, P), (P, 7 * P), (5 * P, 2 * P), (4 * P, 4 * P), (2 * P, 5 * P), (4 * P, 4 * P), (P, P)]


def pack_of(shapes, seed=3):
    """One exact image (rect_data.images) per shape, each from its own seed: the twins of a repeated shape differ."""
    return [XD.images(1, h, w, seed=seed + 7 * i)[0] for i, (h, w) in enumerate(shapes)]


def variant_tensors(pkg, kind):
    assert kind in VARIANTS
    if kind == "gluh4":
        hp, t = SD.fixture_tensors(pkg, "hplus")
    elif kind == "preerfh4":
        hp, t = AD.fixture_tensors(pkg, "tanh_pre")
        t = dict(t); t["arch"] = np.array([AD.ACT_ERF, 1e-5, 0, 0], np.float32)
    else:
        hp, t = XD.fixture_tensors(pkg, kind[:-2])
    return dataclasses.replace(hp, num_attention_heads=HEADS4), t


def variant_file(pkg, kind, ftype=1):
    """Path of the (cached) model file of a 4-head variant."""
    return R64.cached_file(f"pack-{kind}-p{XD.POS_SCALE:g}-q{XD.QK_SCALE:g}-ft{ftype}", lambda tmp: pkg.ggml_file.write_model(tmp, *variant_tensors(pkg, kind), ftype=ftype))


def row0_of(shapes, P, registers):
    """row0 [n + 1] of a pack: image i holds 1 + registers + (h / P)(w / P) token rows."""
    n = [1 + registers + (h // P) * (w // P) for h, w in shapes]
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int32)


# ================================================================================================ large packs (tests/test_gpu_pack_scale.py)
# The wide fixtures of tests/wide_data.py that a packed context accepts (a class-token head): D 512, 3 layers, 8 heads of 64, patch 16, file grid
# 2 x 2.  Every GEMM of a layer has a column count that is a multiple of 256 there, so the row count of a call moves each of them through all three
# kernel families.  Everything below is host arithmetic, checked by tests/test_cpu_pack.py.

SCALE_KEYS = ("vit_erf", "dinov3_rope", "glu_hplus")
TILE_M = 256                                         # gemm.hip gemm_tile_m(): the row padding of every activation buffer
SKINNY_TILES = 128                                   # kernels.h Tuning::skinny_tiles, the default


def round_up(a, b):
    return -(-a // b) * b


def _ring_supports(M, N_pad, K, cfg):
    """gemm_ring.hip gemm_ring_supports (l. 414-419) on parse_cfg's tiles (l. 350-358): 445 / 945 256 x 256, 245 128 x 256, 122 64 x 128; ks = 2."""
    bm, bn = {445: (256, 256), 945: (256, 256), 245: (128, 256), 122: (64, 128)}[cfg]
    if cfg == 945 and K < 128:
        return False
    return M % bm == 0 and N_pad % bn == 0 and K % 64 == 0 and K >= 64


def _pp_supports(M, N, N_pad, K, ldo):
    """gemm_pp.hip gemm_pp_supports (l. 580-585), BM = BN = 256, BK = 64 (l. 67); lda = ldw = K."""
    lim = 0xf0000000
    if M * K * 2 > lim or N_pad * K * 2 > lim or (M + M // 64 + 2) * ldo * 4 > lim:
        return False
    return M % 256 == 0 and N_pad % 256 == 0 and K % 128 == 0 and K >= 128 and N % 4 == 0 and ldo % 4 == 0


def gemm_family(M, N, K):
    """The kernel family launch_gemm (gemm.hip l. 224-256) gives a dense GEMM of M padded rows under the default tuning (gemm_cfg < 0, no split,
    skinny_tiles 128): "pp" the persistent ping-pong kernel, 245 the 128 x 256 ring tiles, 122 the 64 x 128 ring tiles (445 / 945: the 256 x 256 ring
    kernels of a wide shape whose K the ping-pong kernel cannot walk; None: no kernel).  N_pad = round_up(N, 128), ldo = N, as dense_gemm builds
    the GEMMs of a layer.  is_wide: gemm.hip l. 187-190; launch_wide: l. 202-212; gemm_ring_cfg: l. 217-222."""
    assert M > 0 and M % TILE_M == 0
    N_pad = round_up(N, 128)
    pp = _pp_supports(M, N, N_pad, K, N)
    if M % 256 == 0 and N_pad % 256 == 0 and (M // 256) * (N_pad // 256) >= 128 and (pp or _ring_supports(M, N_pad, K, 445)):      # is_wide
        return "pp" if pp else (945 if _ring_supports(M, N_pad, K, 945) else 445)
    cfg = 245
    if (M // 128) * (N_pad // 256) < SKINNY_TILES and _ring_supports(M, N_pad, K, 122):
        cfg = 122
    if _ring_supports(M, N_pad, K, cfg):
        return cfg
    return 122 if _ring_supports(M, N_pad, K, 122) else None


def layer_gemms(key):
    """{name: (N, K)} of the four GEMMs of a layer (packed_forward.cpp pack_forward): fc1's N is 2 F and fc2's K is F with a gated MLP."""
    D, F = WD.D, WD.FIXTURES[key].glu
    return {"qkv": (3 * D, D), "proj": (D, D), "fc1": (2 * F if F else 4 * D, D), "fc2": (D, F if F else 4 * D)}


def families(key, rows):
    """{name: family} of a call of `rows` token rows: M = round_up(rows, 256)."""
    return {nm: gemm_family(round_up(rows, TILE_M), N, K) for nm, (N, K) in layer_gemms(key).items()}


def thresholds(key, top=1 << 15):
    """The padded row counts at which one of the four GEMMs changes its family, ascending."""
    return [M for M in range(2 * TILE_M, top + 1, TILE_M) if families(key, M) != families(key, M - TILE_M)]


def prefix_rows(key):
    return WD.FIXTURES[key].prefix


def ladder(key):
    """Row counts of the calls of a fixture, ascending.  vit_erf: the last row block below and the first at every threshold (so every combination of
    families, from all 122 to all pp, and both sides of every switch); the other two: all 122, a middle combination, all pp.  The remainders
    rows % 256 cycle through 0, 1, 255 and 77: a full last block, one real row, one pad row, something in between."""
    th = thresholds(key)
    Ms = sorted({M for t in th for M in (t - TILE_M, t)}) if key == "vit_erf" else [th[0] - TILE_M, th[len(th) // 2], th[-1]]
    rem = (0, 1, 255, 77)
    return [M - (TILE_M - rem[i % 4]) % TILE_M for i, M in enumerate(Ms)]


# ---- the images: six probes of distinct grids, eight fillers over four grids
PROBE_GRIDS = ((2, 2), (14, 14), (1, 7), (5, 3), (1, 1), (9, 20))          # in pack order: the file's own grid first, the largest rectangle last
FILLER_GRIDS = ((1, 1), (1, 1), (1, 2), (6, 4), (11, 11), (11, 11), (1, 2), (6, 4))      # round-robin order: two runs of one shape, four single images
N_PROBES, N_DISTINCT = len(PROBE_GRIDS), len(PROBE_GRIDS) + len(FILLER_GRIDS)
GRIDS = PROBE_GRIDS + FILLER_GRIDS                   # image id -> grid; ids 0 .. 5 are the probes
SMALL = (N_PROBES + 0, N_PROBES + 1)                 # the two 1 x 1 fillers
SMALL2 = (N_PROBES + 2, N_PROBES + 6)                # the two 1 x 2 fillers


def tokens_of(i, Tp):
    return Tp + GRIDS[i][0] * GRIDS[i][1]


@functools.lru_cache(maxsize=None)
def distinct_images():
    """The 14 distinct images at patch 16, exact in both operand types (rect_data.images), each from its own seed."""
    return tuple(XD.images(1, gh * WD.P, gw * WD.P, seed=100 + 7 * i)[0] for i, (gh, gw) in enumerate(GRIDS))


def _fill(target, Tp, start, prev):
    """Image ids of fillers holding exactly `target` rows: round-robin from position `start` of FILLER_GRIDS while whatever is left can still be
    made of 1 x 1 and 1 x 2 images (every count from (s1 - 1)(s2 - 1) on is a s1 + b s2), then those: two distinct images of each, alternating.
    No image follows itself (`prev`: the id in front)."""
    s1, s2 = Tp + 1, Tp + 2
    assert target >= s1 * s2, (target, s1 * s2)
    out, k = [], start
    while True:
        i = N_PROBES + k % len(FILLER_GRIDS)
        if target - tokens_of(i, Tp) < s1 * s2:
            break
        out.append(i); target -= tokens_of(i, Tp); k += 1
    b = next(b for b in range(s1) if (target - b * s2) >= 0 and (target - b * s2) % s1 == 0)
    a = (target - b * s2) // s1
    last = out[-1] if out else prev
    for pair, cnt in ((SMALL, a), (SMALL2, b)):
        for _ in range(cnt):
            last = pair[1] if last == pair[0] else pair[0]
            out.append(last)
    return out, k


def pack_ids(rows, Tp):
    """Image ids of the pack of a rung, exactly `rows` token rows: probe, fillers, probe, ..., probe.  The stretch in front of the 14 x 14 probe puts
    its first row 128 rows into a row block, so its 197 and more rows straddle the next multiple of 256."""
    probe_rows = sum(tokens_of(i, Tp) for i in range(N_PROBES))
    left = rows - probe_rows
    s0 = tokens_of(0, Tp)
    first = next(t for t in range((Tp + 1) * (Tp + 2), 4096) if (s0 + t) % TILE_M == 128)
    rest = left - first
    assert rest >= 4 * (Tp + 1) * (Tp + 2), rows
    stretches = [first] + [rest // 4] * 3 + [rest - 3 * (rest // 4)]
    ids, k = [], 0
    for p in range(N_PROBES):
        ids.append(p)
        if p < N_PROBES - 1:
            f, k = _fill(stretches[p], Tp, k, p)
            ids += f
    return ids


def small_pack_ids(Tp):
    """The rung of the smallest images only: n images of 1 x 1 grids -- the 1 x 1 probe and the two 1 x 1 fillers in turn.  n = 1025 images of 2 rows
    (513 of 6 rows with four registers): the call still has a GEMM on the 128 x 256 tiles, Mh = round_up(n, 256) is 1280 (768) -- class-row gather,
    head GEMM and softmax over several row blocks -- and the binary searches of row0 go 11 (10) levels deep."""
    three = (4, SMALL[0], SMALL[1])
    return [three[i % 3] for i in range(1025 if Tp == 1 else 513)]


def rows_of(ids, Tp):
    return sum(tokens_of(i, Tp) for i in ids)


def row0_of_ids(ids, Tp):
    return np.concatenate([[0], np.cumsum([tokens_of(i, Tp) for i in ids])]).astype(np.int64)


def shapes_of(ids):
    return [(GRIDS[i][0] * WD.P, GRIDS[i][1] * WD.P) for i in ids]


def reference_calls(Tp):
    """The distinct images in calls of at most 256 rows each (first fit in id order): every GEMM of a reference call is one row block on family 122."""
    calls = []
    for i in range(N_DISTINCT):
        for c in calls:
            if rows_of(c, Tp) + tokens_of(i, Tp) <= TILE_M:
                c.append(i); break
        else:
            calls.append([i])
    return calls


def poisoned(ids):
    """Positions in `ids` of every other filler copy (the 1st, 3rd, ... filler of the pack): their pixels become NaN."""
    fill = [k for k, i in enumerate(ids) if i >= N_PROBES]
    return set(fill[::2])


def max_images(key):
    Tp = prefix_rows(key)
    return max([len(small_pack_ids(Tp))] + [len(pack_ids(r, Tp)) for r in ladder(key)])


def pe_runs(shapes):
    """Patch-embedding launches of a call: one per run of consecutive images of one shape (pack_forward)."""
    return 1 + sum(1 for a, b in zip(shapes, shapes[1:]) if tuple(a) != tuple(b))


def pack_launches(shapes, L, new_grids, rope=False, glu=False, pre=False, feat=False):
    """(kernel launches, patch embeddings among them) of one packed forward, counted from packed_context.cpp (resolve_grids) and packed_forward.cpp (pack_forward):
    resolve_grids  one launch_pos_resample per grid the cache does not hold and that is not the file's own (`new_grids`; rotary tables are host copies)
    pack_forward   the patch-embedding runs; the pre-norm of a file that has one;
                   per layer 7: norm1, qkv, attention, proj, norm2, fc1, fc2 -- + 1 rope.hip with `rope`, + 1 swiglu.hip with `glu`;
                   the tail 3: class-row gather with the final norm, head GEMM, softmax; + 1 f32 final norm of every row with features on."""
    pe = pe_runs(shapes)
    return new_grids + pe + int(pre) + L * (7 + int(rope) + int(glu)) + 3 + int(feat), pe


# ---- parity of the probes against float64
# Mutants of rect_data on the six probes, as max over the probes of max(max|dprob| / GATE, rms(d) / rms / TOKEN_GATE) against the operand-rounded
# restatement (F16, BF16), computed by tests/test_cpu_pack.py::test_scale_probe_preconditions.  The GPU test asserts "outside a gate on at least one
# probe" for those two gates or more away (SCALE_MUTANTS); the others are listed here with their distance and not asserted.
SCALE_MUTANTS = {"vit_erf": ("grid_transposed", "square_pitch"), "dinov3_rope": ("grid_transposed", "square_pitch", "rope_transposed")}
# Farthest probe, gates, the same in both types to two digits.  Asserted: grid_transposed 55.95 (vit_erf) / 56.02 (dinov3_rope) on the 9 x 20 probe
# (0 on the 1 x 1 and 1 x 7 probes, which have no other order), square_pitch 56.35 / 56.37 (0 on square probes), rope_transposed 12.03 (F16) /
# 11.80 (BF16) on the probabilities of the 9 x 20 probe, 9.76 on the patch rows of the 1 x 7 probe.  Not asserted: the wide vit_erf file draws
# pos_embed at 0.02 like every matrix (no POS_SCALE as on rect_data's micro fixtures), so a wrong position table stays inside the gates.
SCALE_MUTANTS_NEAR = {"vit_erf": {"pos_transposed": 0.59, "pos_square": 0.53}, "dinov3_rope": {}}


GATE = R64.PROB_TOL[1]                               # tests/test_gpu_pack.py GATE: the bf16 probability gate, for both operand types
TOKEN_GATE = 2.5e-2                                  # tests/test_gpu_pack.py TOKEN_GATE: rms(d) / rms on the final norm's patch rows


def mutant_applies(mutant, grid, g_in=WD.S // WD.P):
    """pos_square reads the file's table without resampling: it exists only on grids with no more patches than the file's."""
    return mutant != "pos_square" or grid[0] * grid[1] <= g_in * g_in


def parity_probes(key):
    """The probes whose parity is asserted: all six, but of the gated MLP the file's own 2 x 2 grid alone (ref64.forward64 restates the other five
    as well; gates for them are not set yet)."""
    return (0,) if key == "glu_hplus" else tuple(range(N_PROBES))


def probe_ref(key, t, i, dtype=None, mutant=None, binding=None):
    """(probs [C], final-norm patch rows [gh gw][D]) of probe i alone at its own shape; dtype None: no operand rounding."""
    im = distinct_images()[i][None]
    T = prefix_rows(key)
    r = WD.forward64(key, t, im, dtype, mutant=mutant, binding=binding)
    return r["probs"][0], r["final"][0, T:]


def probe_distance(p, tok, ref):
    """(max|dprob|, rms(d) / rms on the patch rows) of one image against probe_ref's pair."""
    rp, rt = ref
    tok = np.asarray(tok, np.float64).reshape(rt.shape)
    return float(np.abs(p - rp).max()), float(np.sqrt(((tok - rt) ** 2).mean()) / np.sqrt((rt ** 2).mean()))


def gates(d):
    """A distance pair in gates: the larger of the two ratios."""
    return max(d[0] / GATE, d[1] / TOKEN_GATE)


# ================================================================================================ the table cache (packed_context.cpp resolve_grids)
def cache_trace(calls, max_tokens, half, max_grids=32):
    """resolve_grids restated.  calls: per call the grids (gh, gw) it names, in order; half: head_dim / 2 of a `rope` file, 0 without rope (no arena).
    Per call: dict(held = the grids in the cache afterwards, in cache order; rope_off = {grid: floats into the arenas}; restarted; evicted).
    A call bumps tick and stamps the grids it names and holds; counts the missing ones and the floats they need; if the arena (2 max_tokens half
    floats) cannot take them it drops EVERY grid and starts at 0; then evicts least-recently-used grids the call does not name (ties: the first
    in cache order) while held + missing (as counted before any drop) exceeds max_grids; then builds every named grid it does not hold, in
    order of first appearance, each at the arena's top."""
    cap, top, tick, cache, out = 2 * max_tokens * half, 0, 0, [], []
    for call in calls:
        tick += 1
        want = list(dict.fromkeys(tuple(g) for g in call))
        assert len(want) <= max_grids
        missing, need = 0, 0
        for g in want:
            e = next((e for e in cache if e["grid"] == g), None)
            if e:
                e["used"] = tick
            else:
                missing += 1; need += g[0] * g[1] * half
        restarted, evicted = False, []
        if missing:
            if half and top + need > cap:
                cache, top, restarted = [], 0, True
            while len(cache) + missing > max_grids:
                cand = [e for e in cache if e["used"] != tick]
                if not cand:
                    break
                lru = min(cand, key=lambda e: e["used"])
                evicted.append(lru["grid"]); cache.remove(lru)
            for g in want:
                if not any(e["grid"] == g for e in cache):
                    cache.append(dict(grid=g, used=tick, off=top))
                    top += g[0] * g[1] * half
            assert top <= cap or not half
        out.append(dict(held=[e["grid"] for e in cache], rope_off={e["grid"]: e["off"] for e in cache}, restarted=restarted, evicted=evicted, top=top))
    return out


# The p14rope micro fixture: patch 14, file grid 4 x 4, 4 registers (5 prefix rows), 2 heads of 64 (half = 32).
CACHE_KIND, CACHE_HALF, CACHE_PREFIX, CACHE_FILE_GRID = "p14rope", 32, 5, (4, 4)
_a, _b, _c, _d, _e, _g, _k = (2, 5), (5, 2), (3, 3), (4, 4), (1, 7), (3, 5), (2, 7)
# max_tokens 40: an arena of 80 patch rows.  By cache_trace with max_grids 32: call 4 names the cached (2, 5) and the missing (2, 7) at top 67 and
# restarts; call 7 names the cached (2, 5) and the missing (3, 5) at top 66 and restarts; call 8 names what call 7 built, in the other order.
CACHE_MAX_TOKENS = 40
CACHE_CALLS = ([_a, _b], [_c, _d], [_e, _g], [_a, _k], [_b, _c], [_d, _e], [_g, _a], [_a, _g], [_k, _b])
CACHE_ROOMY_TOKENS = 1024                            # the arena that never fills

# Back-to-back device calls, max_grids 2, max_tokens 70 (an arena of 140 patch rows): A names a and b; B names c and a (evicts b, builds c at 60);
# C names two new grids that need 60 patch rows at top 108 and restarts.
B2B_MAX_TOKENS = 70
B2B_CALLS = ([(2, 2), (7, 8)], [(6, 8), (2, 2)], [(5, 10), (2, 5)])


def call_rows(call, prefix=CACHE_PREFIX):
    return sum(gh * gw + prefix for gh, gw in call)
