"""Files with a gated (SwiGLU) MLP (include/vitx.h "gated MLP"), shared by tests/test_cpu_swiglu.py -- which pins the restatement of such a file to
transformers' Dinov2Model (use_swiglu_ffn) and DINOv3ViTModel (use_gated_mlp) -- and tests/test_gpu_swiglu.py.

What the family owns of the float64 restatement tests/ref64.py: the gate (swiglu64, silu64), the exact grid of the kernel test and the micro
fixtures.  ref64.blocks64 puts the gated MLP in place of every block's plain one.  With F = glu[1], y = uround(norm2(x)), fc1.weight [2 F][D],
fc1.bias [2 F]:
    a = uround(y fc1.weight^T + fc1.bias)          the STORED fc1 output, [.., 2 F]
    g = a[.., :F], u = a[.., F:]                   gate rows first, then up rows: HuggingFace's weights_in.chunk(2), cat(gate_proj, up_proj)
    h = uround(silu(g) u), silu(g) = g / (1 + exp(-g))     the STORED product; nothing between the two is rounded
    x = x + h fc2.weight^T + fc2.bias
The `arch` activation of such a file is not applied.

MUTANTS are the mistakes the tests must be able to see; ref64.forward64(..., mutant=name) and swiglu64(..., mutant=name) make one of them:
    gate_up_swapped      h = silu(u) g
    gate_is_sigmoid      h = sigmoid(g) u: the g factor is lost
    gelu_gate            h = erf-GELU(g) u
    no_up                h = silu(g)
    halves_interleaved   gate = the even columns of a, up = the odd ones
    up_bias_dropped      the up half of fc1.bias is not added (a forward mutant: the gate kernel never sees a bias)

The micro fixtures (fixture_tensors; both on arch_data.MICRO: D 128, 2 layers, 2 heads of 64, patch 14, image 56; both F = 320: 2 F = 640 > 4 D = 512,
so a buffer or a bias pad still sized by 4 D breaks, and 320 is a multiple of 64 but of neither 128 nor 256, so fc1's N and fc2's K are ragged for
the wide tiles):
    g       DINOv2-giant-like: no registers, the cls + mean head, a position table, `arch` {erf, 1e-6} (carried, not applied)       N = 17
    hplus   DINOv3-H+-like: 4 registers, `rope` {1, 100}, a zero pos_embed, rope_data.QK_SCALE on q and k, `arch` {tanh, 1e-5}       N = 21
pkg.synth.make_weights draws every matrix at 0.02: the gate arguments then stay near 0, where silu(g) ~ g / 2 and silu(g) u ~ silu(u) g -- the
swapped halves are invisible.  So mlp.fc1.weight, mlp.fc1.bias and mlp.fc2.weight are multiplied by the factors GLU_SCALE, chosen so that BOTH of
these hold on the 17 images of the GPU tests and against tests/ref64.py's gates (stage_ok, PROB_TOL), computed by
tests/test_cpu_swiglu.py::test_fixtures_separate_the_mutants_from_operand_rounding and not assumed:
    the operand-rounded restatement lies inside HALF a gate of the unrounded one, and every mutant more than TWICE a gate away."""
import numpy as np

import arch_data as AD
import rope_data as RD

MUTANTS = ("gate_up_swapped", "gate_is_sigmoid", "gelu_gate", "no_up", "halves_interleaved", "up_bias_dropped")
OP_MUTANTS = MUTANTS[:5]                      # those a single launch of the gate kernel could make
MICRO = AD.MICRO
F = 320
FIXTURES = ("g", "hplus")
HEADS = 2
# (mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight), starting from arch_data.CLIP_MLP_SCALE = (8, 4) for the two matrices, the bias with fc1.  Chosen and measured by
# test_fixtures_separate_the_mutants_from_operand_rounding on the 17 images of the GPU tests, per stage (layer 1, layer 2) as
# (max|d| / rms, rms(d) / rms); the gates are fp16 (2.5e-2, 2e-3), bf16 rms 2.5e-2, probabilities 1e-3 / 2e-2.  Fixture g / fixture hplus:
#   rounded against unrounded  fp16 (1.9e-3, 4.4e-4) (2.7e-3, 6.2e-4), max|dprob| 1.7e-4 / (5.7e-3, 5.7e-4) (6.8e-3, 7.8e-4), 2.5e-4
#                              bf16 rms 4.8e-3, 6.7e-3, max|dprob| 2.1e-3 / rms 6.2e-3, 8.4e-3, max|dprob| 4.7e-3
#   gate_up_swapped     (4.3, 0.83) (4.7, 1.02), max|dprob| 0.18 / 0.37        gate_is_sigmoid  (2.9, 0.65) (3.3, 0.74), 0.22 / 0.20
#   gelu_gate           (0.49, 0.10) (0.61, 0.14), 0.045 / 0.039               no_up            (5.3, 1.08) (5.3, 1.11), 0.26 / 0.36
#   halves_interleaved  (5.7, 1.30) (5.8, 1.36), 0.24 / 0.45                   up_bias_dropped  (0.38, 0.083) (0.52, 0.12), 0.030 / 0.032
# (stage figures of fixture g; hplus's agree to two digits, and both operand types give the mutants the same figures).  The nearest mutant,
# up_bias_dropped, is at rms 0.083: 1.7 x the doubled bf16 gate and 20 x the doubled fp16 one.  The starting point needed no change: with the
# bias at its drawn size (factor 1) up_bias_dropped moves the stream by an eighth of that (rms 0.011 / 0.016), inside twice the bf16 gate.
GLU_SCALE = (8.0, 8.0, 4.0)
U_VALUES = (1.0, -1.0, 0.5, -0.5, 3.0, -7.25)      # the up values of the exact grid, cycled per column


def sigmoid64(g):
    g = np.asarray(g, np.float64)
    e = np.exp(-np.abs(g))
    return np.where(g >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def silu64(g):
    """g / (1 + exp(-g)) in float64, stable in both tails."""
    g = np.asarray(g, np.float64)
    return g * sigmoid64(g)


def swiglu64(a, Fw, mutant=None):
    """a [.., >= 2 Fw] float64 (gate columns, then up columns) -> h [.., Fw]."""
    a = np.asarray(a, np.float64)
    g, u = a[..., :Fw], a[..., Fw:2 * Fw]
    if mutant == "halves_interleaved":
        g, u = a[..., 0:2 * Fw:2], a[..., 1:2 * Fw:2]
    if mutant == "gate_up_swapped":
        g, u = u, g
    if mutant == "gate_is_sigmoid":
        return sigmoid64(g) * u
    if mutant == "gelu_gate":
        return AD.act64(g, AD.ACT_ERF) * u
    if mutant == "no_up":
        return silu64(g)
    return silu64(g) * u


def glu_of(t):
    """F of a file's `glu` tensor (kind 1), or None."""
    if "glu" not in t:
        return None
    r = np.asarray(t["glu"], np.float32).reshape(-1)
    assert r.shape == (4,) and r[0] == 1 and r[2] == 0 and r[3] == 0 and r[1] == int(r[1])
    return int(r[1])


# ------------------------------------------------------------------------------------------------ the exact grid of the kernel test
def grid_operands(rows, Fw, dtype):
    """(g, u) [rows][Fw] float64 as the operand type holds them: g walks arch_data.grid() (k / 64, |g| <= 8) over the elements in row-major order,
    rounded to `dtype` (fp16 holds every k / 64, bf16 the multiples of 1 / 16 beyond |g| = 4 ...), u is U_VALUES cycled per column (exact in both)."""
    gr = AD.grid()
    g = gr[np.arange(rows * Fw) % len(gr)].reshape(rows, Fw)
    g = RD.from_bits16(RD.to_bits16(g, dtype), dtype).astype(np.float64)
    u = np.broadcast_to(np.array(U_VALUES)[np.arange(Fw) % len(U_VALUES)], (rows, Fw)).copy()
    assert np.array_equal(RD.from_bits16(RD.to_bits16(u, dtype), dtype), u.astype(np.float32))
    return g, u


def separated_share(mutant, dtype):
    """Share of the points of the exact grid (one pass over arch_data.grid(), F = 1026 columns so that every (g, u) pairing and both column parities
    occur) where `mutant` lies more than two act_tol from the truth."""
    g, u = grid_operands(6, 1026, dtype)
    a = np.concatenate([g, u], 1)
    want = swiglu64(a, 1026)
    return float((np.abs(swiglu64(a, 1026, mutant) - want) > 2 * AD.act_tol(want, dtype)).mean())


# ------------------------------------------------------------------------------------------------ the micro fixtures
def fixture_tensors(pkg, kind, name=MICRO, scale=GLU_SCALE, Fw=F, glu=True):
    """make_weights(glu=F) + the extensions of `kind`, in the converter's order (`arch`, `rope`, `glu`, then the model), the three MLP tensors times
    `scale`.  glu=False: the same model with the plain 4 x hidden MLP (tools/swiglu_cost.py's counterpart)."""
    assert kind in FIXTURES
    hp = pkg.synth.hparams_for(name)
    hplus = kind == "hplus"
    w = pkg.synth.make_weights(hp, head_scale=4.0, registers=RD.REGISTERS if hplus else 0, head_pool=0 if hplus else 1, glu=Fw if glu else 0)
    D = hp.hidden_size
    out = {"arch": np.array([AD.ACT_TANH, 1e-5, 0, 0] if hplus else [AD.ACT_ERF, 1e-6, 0, 0], np.float32)}
    if hplus:
        out["rope"] = np.array([1, RD.THETA, 0, 0], np.float32)
    if glu:
        out["glu"] = w.pop("glu")
    out.update(w)
    for i in range(hp.num_hidden_layers):
        for nm, f in zip(("mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight"), scale):
            out[f"blocks.{i}.{nm}"] = out[f"blocks.{i}.{nm}"] * np.float32(f)
    if hplus:
        out["pos_embed"] = np.zeros_like(out["pos_embed"])
        for i in range(hp.num_hidden_layers):
            for nm in (f"blocks.{i}.attn.qkv.weight", f"blocks.{i}.attn.qkv.bias"):
                a = out[nm].copy(); a[:2 * D] *= np.float32(RD.QK_SCALE); out[nm] = a
    return hp, out


def fixture_file(pkg, kind, ftype=1, name=MICRO):
    from ref64 import cached_file
    return cached_file(f"glu-{name}-{kind}-F{F}-s{'x'.join(f'{s:g}' for s in GLU_SCALE)}-ft{ftype}",
                       lambda tmp: pkg.ggml_file.write_model(tmp, *fixture_tensors(pkg, kind, name), ftype=ftype))
