"""The conditions tests/test_gpu_poison.py relies on (tests/poison_data.py), checked without a GPU: the poison sits where a kernel that
reads past an image's last key finds it, the clean images keep their values, and their one correct result does not move."""
import numpy as np
import pytest

import exact_data as X
import poison_data as P

CASE = (P.N_IMG, 17, P.HEADS, 64)


def _base(case=CASE):
    n_img, N, H, hd = case
    return X.spread_qkv(n_img, N, H, hd, X.attn_seed(n_img, N, H, hd))


def test_every_image_with_a_successor_is_clean_in_front_of_a_poisoned_one():
    """Keys past N of image b are the first rows of image b + 1: over the two image sets every image that HAS a successor is clean with a
    poisoned successor once, the last image is clean once (the end of the tensor behind it), and one clean image has a poisoned predecessor
    (a kernel that reads in front of an image's first row)."""
    seen_succ, seen_pred, seen_clean = set(), set(), set()
    for images in P.IMAGE_SETS:
        assert set(images) < set(range(P.N_IMG))
        for b in P.clean_images(P.N_IMG, images):
            seen_clean.add(b)
            if b + 1 < P.N_IMG:
                assert b + 1 in images, (images, b)           # within one launch: EVERY clean image that has a successor has a poisoned one
                seen_succ.add(b)
            if b - 1 in images:
                seen_pred.add(b)
    assert seen_succ == set(range(P.N_IMG - 1)) and seen_clean == set(range(P.N_IMG)) and seen_pred
    clean, bad = P.sandwich(3)
    assert clean == (0, 2, 4) and bad == (1, 3)


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
def test_values_are_what_they_are_called_in_the_operand_type(dtype_name):
    import torch
    tdt = torch.float16 if dtype_name == "f16" else torch.bfloat16
    assert np.isnan(P.value_of("nan", dtype_name)) and P.value_of("+inf", dtype_name) == np.inf and P.value_of("-inf", dtype_name) == -np.inf
    mx = torch.tensor(P.value_of("max", dtype_name), dtype=torch.float32)
    assert float(mx.to(tdt).float()) == float(mx) == torch.finfo(tdt).max        # exact in the type, and its largest finite number
    assert set(P.HARMFUL) | {"max"} == set(P.VALUES)


@pytest.mark.parametrize("images", P.IMAGE_SETS)
@pytest.mark.parametrize("value", P.VALUES)
def test_poison_touches_the_named_parts_of_the_named_images_only(images, value):
    n_img, N, H, hd = CASE
    base = _base()
    v = P.value_of(value, "f16")
    same = (lambda a: np.isnan(a).all()) if value == "nan" else (lambda a: (a == v).all())
    for parts in ("qkv", "q", "k", "v"):
        got = P.poison(base, n_img, N, H, hd, images, v, parts).reshape(n_img, N, 3, H, hd)
        want = base.reshape(n_img, N, 3, H, hd)
        assert np.isfinite(base).all()                                            # poison() copies
        for b in range(n_img):
            for i, p in enumerate("qkv"):
                if b in images and p in parts:
                    assert same(got[b, :, i]), (b, p)
                else:
                    assert np.array_equal(got[b, :, i], want[b, :, i]), (b, p)
    got = P.poison_heads(base, n_img, N, H, hd, images, v).reshape(n_img, N, 3, H, hd)
    want = base.reshape(n_img, N, 3, H, hd)
    assert P.clean_heads(H) == (1,)
    for b in range(n_img):
        for h in range(H):
            if b in images or h not in P.clean_heads(H):
                assert same(got[b, :, :, h]), (b, h)
            else:
                assert np.array_equal(got[b, :, :, h], want[b, :, :, h]), (b, h)


@pytest.mark.parametrize("case", [CASE, (P.N_IMG, 33, P.HEADS, 120)], ids=lambda c: "n%d_N%d_H%d_hd%d" % c)
def test_the_float64_attention_of_the_clean_images_does_not_move(case):
    """Attention is computed per (image, head): the float64 result of a clean image's rows is the same array whatever its neighbours hold,
    and on flat data it is c."""
    n_img, N, H, hd = case
    base = _base(case)
    ref = X.attention64(base, n_img, N, H, hd).reshape(n_img, N, H, hd)
    flat, c = X.flat_qkv(n_img, N, H, hd, -1, 5)
    with np.errstate(invalid="ignore", over="ignore"):
        for images in P.IMAGE_SETS:
            for value in P.VALUES:
                v = P.value_of(value, "bf16")
                got = X.attention64(P.poison(base, n_img, N, H, hd, images, v), n_img, N, H, hd).reshape(n_img, N, H, hd)
                goth = X.attention64(P.poison_heads(base, n_img, N, H, hd, images, v), n_img, N, H, hd).reshape(n_img, N, H, hd)
                gotf = X.attention64(P.poison(flat, n_img, N, H, hd, images, v), n_img, N, H, hd).reshape(n_img, N, H, hd)
                for b in P.clean_images(n_img, images):
                    assert np.array_equal(got[b], ref[b]), (images, value, b)
                    for h in P.clean_heads(H):
                        assert np.array_equal(goth[b, :, h], ref[b, :, h]), (images, value, b, h)
                    assert np.abs(gotf[b] - c[b][None]).max() <= 1e-12, (images, value, b)
                if value in ("nan", "+inf"):
                    for b in images:
                        assert not np.isfinite(got[b]).any(), (images, value, b)          # ... and the poison is real: its own image is lost


def test_poisoned_image_batches():
    imgs = np.random.default_rng(0).standard_normal((5, 3, 8, 8)).astype(np.float32)
    clean, bad = P.sandwich(3)
    for kind in P.IMAGE_POISONS:
        got = P.poison_images(imgs, bad, kind)
        for p in clean:
            assert np.array_equal(got[p], imgs[p])
        for p in bad:
            assert not np.array_equal(got[p], imgs[p], equal_nan=True)
            if kind == "inf-pixel":
                assert np.isinf(got[p]).sum() == 1 and (np.isfinite(got[p]).sum() == got[p].size - 1)
            elif kind == "nan":
                assert np.isnan(got[p]).all()
            else:
                assert (got[p] == np.float32(1e30)).all()
