"""tests/ref64.py itself, on micro fixtures: a mutant name must apply to the file, a square image needs no table of its own, and the combinations
no single family's fixtures cover run (a gated MLP with rope on a rectangle).  What pins the arithmetic to transformers are the family tests
(tests/test_cpu_arch.py, _registers, _rope, _swiglu, _rect, _map_head, _text)."""
import numpy as np
import pytest

import arch_data as AD
import map_data as MD
import prefix_data as PD
import rect_data as XD
import ref64 as R64
import swiglu_data as SD

KEYS = ("embed", "trace", "final", "mean", "q", "k", "logits", "probs")


@pytest.mark.parametrize("family,mutant", [("arch", "no_such_mutant"), ("arch", "no_rope"), ("arch", "rope_transposed"), ("arch", "gate_up_swapped"),
                                           ("map", "pos_on_registers"), ("map", "pos_square")])
def test_a_mutant_that_cannot_apply_is_an_error(pkg, family, mutant):
    """An unknown name, a rope mutant without `rope`, a gate mutant without `glu`, a prefix and a position mutant without a class token."""
    _, t = AD.fixture_tensors(pkg, "vit_erf") if family == "arch" else MD.fixture_tensors(pkg)
    imgs = PD.exact_images(1, 56, seed=2)
    assert np.isfinite(R64.forward64(t, imgs, 2)["probs"]).all()
    with pytest.raises(ValueError):
        R64.forward64(t, imgs, 2, mutant=mutant)


def test_a_misplaced_head_or_table_argument_is_an_error(pkg):
    _, t = AD.fixture_tensors(pkg, "vit_erf")
    imgs = PD.exact_images(1, 56, seed=2)
    with pytest.raises(ValueError):
        R64.forward64(t, imgs, 2, flat=True)
    with pytest.raises(ValueError):
        R64.forward64(t, imgs, 2, pos=t["pos_embed"][0], mutant="pos_square")


@pytest.mark.parametrize("kind", ["dinov2_erf", "clip"])
def test_square_image_needs_no_table_of_its_own(pkg, kind):
    """The same bits on every key whether the file's table is found by forward64 or handed to it."""
    _, t = AD.fixture_tensors(pkg, kind)
    imgs = PD.exact_images(2, 56, seed=3)
    a, b = R64.forward64(t, imgs, 2), R64.forward64(t, imgs, 2, pos=t["pos_embed"][0])
    assert set(a) == set(KEYS)
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key


def test_gated_mlp_with_rope_on_a_rectangle(pkg, binding):
    """A smoke test of a combination no family restated: finite values of the right shapes, and the rotation is there."""
    hp, t = SD.fixture_tensors(pkg, "hplus")
    imgs = XD.images(2, 28, 70)
    N, D, L, H = 2 * 5 + 1 + 4, hp.hidden_size, hp.num_hidden_layers, SD.HEADS
    r = R64.forward64(t, imgs, H, binding=binding)
    assert r["trace"].shape == (L + 1, 2, N, D) and r["embed"].shape == r["final"].shape == (2, N, D) and r["mean"].shape == (2, D)
    assert r["q"].shape == r["k"].shape == (L, 2, H, N, D // H) and r["logits"].shape == r["probs"].shape == (2, hp.num_classes)
    assert all(np.isfinite(r[key]).all() for key in KEYS) and np.allclose(r["probs"].sum(1), 1.0)
    for mutant in ("rope_transposed", "gate_up_swapped"):
        assert np.abs(R64.forward64(t, imgs, H, mutant=mutant, binding=binding)["final"] - r["final"]).max() > 1e-3, mutant


def test_attention_pooling_head_on_a_rectangle(pkg, binding):
    """The table of a file without a class row is resampled like any other; at the file's own grid it is the file's, bit for bit."""
    _, t = MD.fixture_tensors(pkg)
    r = R64.forward64(t, XD.images(2, 28, 70), 2, binding=binding)
    assert r["trace"].shape[2] == 10 and r["e"].shape == (2, t["pos_embed"].shape[-1]) and all(np.isfinite(r[k]).all() for k in KEYS + ("e", "M", "p"))
    sq = PD.exact_images(2, 56, seed=3)
    assert np.array_equal(R64.forward64(t, sq, 2)["probs"], R64.forward64(t, sq, 2, pos=t["pos_embed"][0])["probs"])
