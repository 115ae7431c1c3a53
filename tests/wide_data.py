"""Wide fixtures of every model family: files on synth's `vit_wide_patch16_32` (D 512, 3 layers, 8 heads of 64, patch 16, image 32) at batches whose
sub-batches take the persistent 256 x 256 GEMMs with the LayerNorms fused into proj / fc2 (forward.cpp SliceForward::run, gemm.hip gemm_ln_fusable).
Shared by tests/test_cpu_wide_data.py, which checks without a GPU what tests/test_gpu_wide_families.py leans on.

D = 512 is the smallest width at which a row block has a column-tile peer (two tiles exchange their statistics; D = 256 has one tile), three layers
the smallest depth with a layer whose proj and fc2 are both fused and whose qkv and fc1 both consume a fused output: the last layer of a class-token
model carries the class rows only (cls_tail) and is never fused.  Every fixture is built by its family's own fixture_tensors on that geometry
(fixture_tensors below), with the q / k and head factors that D = 512 asks for (QK_WIDE, HEAD_WIDE, HEAD_WIDE_MAP); the mutants are
that family's, the float64 restatement is tests/ref64.py.

    key          family (fixture builder)     what it puts on the fused path
    vit_erf      arch_data                    fc1 epilogue 6 (erf-GELU), eps 1e-12
    clip         arch_data                    fc1 epilogue 7 (QuickGELU), eps 1e-5, the pre-norm in place on X in front of layer 0
    dinov2_reg   prefix_data, 4 registers     5 prefix rows, the cls + mean head fed by the last layer's feature launch, never cls_tail
    siglip_map   map_data                     no class row, the attention-pooling tail after the last layer
    dinov3_rope  rope_data, 4 registers       rope.hip between the qkv GEMM (whose prologue repairs the fused norm1) and attention; erf-GELU, eps 1e-5
    glu_g        swiglu_data g, F 1408        fc1 with the plain bias epilogue at N = 2816, swiglu.hip, a fused fc2 at K = 1408 (K % 128 == 0, K % 256 != 0)
    glu_hplus    swiglu_data hplus, F 1408    the same with 4 registers and rope
    glu_odd      swiglu_data g, F 1344        K % 128 != 0: fc2 cannot take the ping-pong kernel, so the WHOLE forward runs stand-alone LayerNorms

Mutants that no end-to-end gate can see are not listed: erf- against tanh-GELU (max |difference| 4.7e-4 per element, tests/test_gpu_arch.py) and eps
1e-12 against 1e-6.  The wrong activation of the clip and siglip_map fixtures is listed for F16 only: under the BF16 gates it lies 0.4 and 1.9 gates
away (tests/test_gpu_arch.py asserts it in F16 alone as well; the families' builders take no other MLP scale).  The eps mutant of the two arch_data
fixtures is 1e-2, as that file's `eps_1e-2` fixture has it the other way round.  rope_data's `rope_on_prefix` needs a patch row per prefix row."""
import functools

import numpy as np

import arch_data as AD
import map_data as MD
import prefix_data as PD
import ref64 as R64
import rope_data as RD
import swiglu_data as SD

NAME = "vit_wide_patch16_32"
D, L, H, P, S = 512, 3, 8, 16, 32
G2 = (S // P) ** 2                                  # patch rows of an image
ROUND = {0: PD.f16_round, 1: PD.bf16_round}
F_WIDE, F_ODD = 1408, 1344
# The q / k factor of the two rope fixtures.  rope_data.QK_SCALE = 12 makes the scores of unit size at D 128; q and k grow with sqrt(D), so at D 512
# the same factor makes the softmaxes four times as peaked and F16 operand rounding alone moves the probabilities by 7 gates (measured by
# tests/test_cpu_wide_data.py: the rounded restatement against the unrounded one).  Half the factor gives the scores of the micro fixture back.
QK_WIDE = 6.0
# The factor on head.weight of every fixture.  The families draw the head at scale 4 (0.08 per weight): the logits grow with sqrt(D) as well, and at
# D 512 F16 operand rounding alone moves the probabilities of four fixtures by 0.84 .. 0.98 of the 1e-3 gate (the same measurement).  Half the
# factor gives the logit spread of the micro fixtures back (0.7 .. 0.9 against their 0.6 .. 0.8) and that figure falls to 0.53 of a gate at most.
HEAD_WIDE = 0.5
# ... and of the attention-pooling fixture: its head reads the pooled embedding e, which no LayerNorm brings back to unit size and which grows with D
# through the pooling head's MLP (arch_data.CLIP_MLP_SCALE); with HEAD_WIDE its logits spread over 7.3 where the micro fixture's spread over 1.95
# (standard deviation over the classes, 17 images), and five of six boundary images have a top-1 probability of 0.99 or more.
HEAD_WIDE_MAP = 0.125


class Fixture:
    def __init__(self, family, tokens, prefix, mutants, pool=False, pooled_map=False, pre=False, glu=0, kind=None, fusable=True, f16_only=()):
        self.family, self.tokens, self.prefix, self._mutants, self._f16_only = family, tokens, prefix, mutants, f16_only
        self.pool, self.map, self.pre, self.glu, self.kind, self.fusable = pool, pooled_map, pre, glu, kind, fusable
        self.cls_tail = not pool and not pooled_map      # context.cpp: the class-rows-only last layer of a class-token head

    def mutants(self, dtype):
        """{name: ref64.forward64 arguments} of the mutants listed for operand type `dtype`."""
        return {k: v for k, v in self._mutants.items() if dtype == 0 or k not in self._f16_only}


_GLU_MUTANTS = {m: dict(mutant=m) for m in SD.MUTANTS}
FIXTURES = {
    "vit_erf": Fixture("arch", 1 + G2, 1, {"eps_1e-2": dict(eps=1e-2)}, kind="vit_erf"),
    "clip": Fixture("arch", 1 + G2, 1, {"eps_1e-2": dict(eps=1e-2), "no_pre_norm": dict(pre_norm=False), "tanh_for_quick": dict(activation=AD.ACT_TANH)}, pre=True, kind="clip",
                    f16_only=("tanh_for_quick",)),
    "dinov2_reg": Fixture("prefix", 5 + G2, 5, {m: dict(mutant=m) for m in PD.MUTANTS}, pool=True),
    "siglip_map": Fixture("map", G2, 0, {"flat_softmax": dict(flat=True), "quick_for_tanh": dict(activation=AD.ACT_QUICK)}, pooled_map=True,
                          f16_only=("quick_for_tanh",)),
    "dinov3_rope": Fixture("rope", 5 + G2, 5, {m: dict(mutant=m) for m in RD.MUTANTS if m != "rope_on_prefix"}),      # that mutant needs a patch row per prefix row: 4 < 5
    "glu_g": Fixture("glu", 1 + G2, 1, _GLU_MUTANTS, pool=True, glu=F_WIDE, kind="g"),
    "glu_hplus": Fixture("glu", 5 + G2, 5, _GLU_MUTANTS, glu=F_WIDE, kind="hplus"),
    "glu_odd": Fixture("glu", 1 + G2, 1, _GLU_MUTANTS, pool=True, glu=F_ODD, kind="g", fusable=False),
}


# ------------------------------------------------------------------------------------------------ the files
def fixture_tensors(pkg, key):
    """(hparams, tensors) of a wide fixture: the family's own builder on NAME, then the two factors this width asks for (QK_WIDE, HEAD_WIDE)."""
    fx = FIXTURES[key]
    if fx.family == "arch":
        hp, t = AD.fixture_tensors(pkg, fx.kind, NAME)
    elif fx.family == "prefix":                                           # tests/test_gpu_registers.py _file: plain synthetic weights, 4 registers, cls + mean head
        hp = pkg.synth.hparams_for(NAME)
        t = pkg.synth.make_weights(hp, head_scale=4.0, registers=fx.prefix - 1, head_pool=1)
    elif fx.family == "map":
        hp, t = MD.fixture_tensors(pkg, NAME)
    elif fx.family == "rope":
        hp, t = RD.fixture_tensors(pkg, NAME, qk_scale=QK_WIDE)
    else:
        hp, t = SD.fixture_tensors(pkg, fx.kind, NAME, Fw=fx.glu)
        if fx.kind == "hplus":                                            # its q and k rows come at rope_data.QK_SCALE
            for i in range(hp.num_hidden_layers):
                for nm in (f"blocks.{i}.attn.qkv.weight", f"blocks.{i}.attn.qkv.bias"):
                    a = t[nm].copy(); a[:2 * D] *= np.float32(QK_WIDE / RD.QK_SCALE); t[nm] = a
    t = dict(t)
    t["head.weight"] = t["head.weight"] * np.float32(HEAD_WIDE_MAP if fx.map else HEAD_WIDE)
    return hp, t


def fixture_file(pkg, key):
    """Path of the (cached) ftype-1 file of a wide fixture."""
    return R64.cached_file(f"wide-{NAME}-{key}-qk{QK_WIDE:g}-h{HEAD_WIDE_MAP if FIXTURES[key].map else HEAD_WIDE:g}-ft1",
                           lambda tmp: pkg.ggml_file.write_model(tmp, *fixture_tensors(pkg, key), ftype=1))


def forward64(key, t, imgs, dtype=None, **mutant):
    """ref64.forward64 of `imgs`; dtype 0 / 1: with that operand type's rounding on matrices and GEMM operands, None: without any."""
    rnd = {} if dtype is None else dict(wround=ROUND[dtype], uround=ROUND[dtype])
    return R64.forward64(t, imgs, H, **rnd, **mutant)


# ------------------------------------------------------------------------------------------------ the batch
def rows_needed(d):
    """Padded rows of a sub-batch from which its proj / fc2 GEMMs are wide (gemm.hip is_wide: at least 128 tiles of 256 x 256) -- 64 row blocks at D 512."""
    assert d % 256 == 0
    return -(-128 // (d // 256)) * 256


def padded_rows(images, tokens):
    return -(-images * tokens // 256) * 256


def batch_for(tokens, d=D):
    """(batch, split_first): the first sub-batch is the smallest that pads to exactly rows_needed(d) with a ragged last row block, the second the
    smallest that needs one row block more (its last block holds a handful of real rows): both wide, neither a whole number of blocks, sizes differ."""
    need = rows_needed(d)
    s1 = (need - 256) // tokens + 1
    while s1 * tokens % 256 == 0:
        s1 += 1
    s2 = need // tokens + 1
    while s2 * tokens % 256 == 0:
        s2 += 1
    assert padded_rows(s1, tokens) == need and padded_rows(s2, tokens) == need + 256
    return s1 + s2, s1


def boundary_ids(n, split_first):
    """binding.Context.boundary_rows of a batch cut at split_first."""
    return sorted({0, 1, n - 2, n - 1, split_first - 1, split_first})


@functools.lru_cache(maxsize=None)
def images(tokens):
    """The whole batch of batch_for(tokens): multiples of 1 / 16, exact in both operand types (the generator of every family's GPU test)."""
    n, _ = batch_for(tokens)
    return PD.exact_images(n, S, seed=tokens)


# ------------------------------------------------------------------------------------------------ what forward.cpp launches
def fusable(key, d=D):
    """gemm_ln_fusable of both residual GEMMs: K = D and K = F must be whole pairs of the ping-pong kernel's 64-deep K tiles (gemm_pp_supports)."""
    f = FIXTURES[key].glu or 4 * d
    return d % 256 == 0 and d // 256 <= 4 and d % 128 == 0 and f % 128 == 0


def launches(key, sub_batches=2, traced=False):
    """Per forward: dict(standalone = `layernorm` launches of a context with no_ln_fusion, fused = LayerNorms that ride in a proj / fc2 GEMM of a
    fusing context, layernorm = the `layernorm` launches that context still makes, cls_tail).  SliceForward::run, per sub-batch: the pre-norm, norm1
    of layer 0, norm2 and the next norm1 of every layer (the last layer has no next), the final norm (a class-token head: its own launch; the
    attention-pooling tail: the LayerNorm of the pooled row; the cls + mean head: none, the feature launch normalises).  Fused: both of every layer
    that carries all rows -- with cls_tail (never while tracing) the last layer carries the class rows and fuses nothing."""
    fx = FIXTURES[key]
    tail = fx.cls_tail and not traced
    final = 0 if fx.pool else 1
    standalone = int(fx.pre) + 2 * L + final
    fused = (2 * (L - 1) if tail else 2 * L - 1) if fusable(key) else 0
    return dict(standalone=sub_batches * standalone, fused=sub_batches * fused, layernorm=sub_batches * (standalone - fused), cls_tail=tail)


def forced_tiles(key, tokens, traced=False):
    """Lower bound of vitx_ctx_ln_fallbacks per forward with ln_test 1: every fifth tile of every fusing launch, counted as
    tests/test_gpu_parity_r03.py::test_gemm_ln_fallback_path_gives_the_same_bits counts them (row blocks x column tiles // 5)."""
    n, s1 = batch_for(tokens)
    per_launch = sum(padded_rows(s, tokens) // 256 * (D // 256) // 5 for s in (s1, n - s1))
    return launches(key, traced=traced)["fused"] // 2 * per_launch


# ------------------------------------------------------------------------------------------------ the gates (tests/ref64.py, tests/test_gpu_map_head.py)
def stage_ratio(e_max, e_rms, dtype):
    """Worst figure / gate of ref64.stage_ok."""
    return max(e_max / R64.F16_STAGE[0], e_rms / R64.F16_STAGE[1]) if dtype == 0 else e_rms / R64.BF16_STAGE_RMS


def distance(key, got, ref, dtype, exact=None):
    """How far `got` (dict: trace [L + 1][n][N][D], probs [n][C]; the attention-pooling family: e [n][D] too) lies from the restatement `ref` of the
    same images, as the LARGEST figure / gate over the gates of that family's GPU test: <= 1 inside every gate, > 1 outside at least one.
    trace stages and probabilities: tests/test_gpu_arch.py _check_trace (ref64.stage_ok, PROB_TOL); the attention-pooling family adds tests/test_gpu_map_head.py's two
    gates on e, which that test takes against the UNROUNDED restatement (`exact`; ref when None).  Returns (worst, {gate name: ratio})."""
    r = {"probs": float(np.abs(got["probs"] - ref["probs"]).max()) / R64.PROB_TOL[dtype]}
    if not FIXTURES[key].pre:       # stage 0, the patch embedding (tests/test_gpu_arch.py _check_trace; behind a pre-norm that test leaves it out)
        r["stage0"] = float(np.abs(got["trace"][0] - ref["trace"][0]).max()) / (2e-5 * max(1.0, float(np.abs(ref["trace"][0]).max())))
    for il, (e_max, e_rms) in enumerate(R64.stage_errors(got["trace"], ref["trace"]), 1):
        r[f"stage{il}"] = stage_ratio(e_max, e_rms, dtype)
    if FIXTURES[key].map:
        ex = ref if exact is None else exact
        r["cos"] = float(MD.one_minus_cos(got["e"], ex["e"]).min()) / MD.cos_gate(dtype)       # best image: a mutant must be out on every one
        r["len"] = abs(MD.mean_length(got["e"], ex["e"])) / MD.len_gate(dtype)
    return max(r.values()), r


def inside(key, got, ref, dtype, exact=None):
    """Every gate of distance() holds, the cos gate on the WORST image (tests/test_gpu_map_head.py).  Returns (ok, {gate name: ratio})."""
    _, r = distance(key, got, ref, dtype, exact)
    if FIXTURES[key].map:
        ex = ref if exact is None else exact
        r["cos"] = float(MD.one_minus_cos(got["e"], ex["e"]).max()) / MD.cos_gate(dtype)
    return max(r.values()) <= 1.0, r
