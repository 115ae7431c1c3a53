"""Non-finite neighbours for the attention kernels and the forward (tests/test_gpu_poison.py; conditions: test_cpu_poison_data.py).

include/vitx.h promises that the images of a batch are independent.  A kernel that stages a whole tile of keys reads, behind the last key
of an image, the first rows of the NEXT image; it masks their scores to -inf, so their probabilities are exactly 0 -- and 0 . NaN and
0 . Inf are NaN in the P.V product.  Finite neighbours cannot show that read (0 . v = 0), and a NaN planted BEHIND the tensor is never
fetched (a buffer load returns zeros out of range): the poison has to sit in a neighbouring image.  poison() overwrites q, k and / or v of
whole images, poison_heads() every other head of the images that stay clean (the convention of test_attention_poisoned_neighbours in
test_gpu_head_dims.py: a head's neighbours in the row are the dims before and behind its slice)."""
import numpy as np

N_IMG, HEADS = 3, 2
# the images that are poisoned, one set after the other: between them every image that has a successor is clean in front of a poisoned
# one (0 in the second set, 1 in the first), image 1 also behind a poisoned one, and image 2 is clean with the end of the tensor behind it
IMAGE_SETS = ((0, 2), (1,))
VALUES = ("nan", "+inf", "-inf", "max")          # "max": the type's largest finite number, the control that must be harmless (0 . max = 0)
HARMFUL = ("nan", "+inf", "-inf")
FINITE_MAX = {"f16": 65504.0, "bf16": float(np.float32(2.0 ** 127 * (2.0 - 2.0 ** -7)))}
PART_INDEX = {"q": 0, "k": 1, "v": 2}


def value_of(name: str, dtype_name: str) -> float:
    """The f32 value a poison name stands for in an operand type (exact in that type)."""
    if name == "nan":
        return float("nan")
    if name in ("+inf", "-inf"):
        return float(name)
    if name == "max":
        return FINITE_MAX[dtype_name]
    raise ValueError(name)


def clean_images(n_img: int, images) -> tuple:
    return tuple(b for b in range(n_img) if b not in images)


def poison(qkv: np.ndarray, n_img: int, N: int, H: int, hd: int, images, value: float, parts: str = "qkv") -> np.ndarray:
    """A copy of qkv [n_img * N][3 * H * hd] with q and / or k and / or v (`parts`) of the named images set to `value`, all heads, all tokens."""
    out = np.array(qkv, dtype=np.float32, copy=True)
    x = out.reshape(n_img, N, 3, H, hd)
    for b in images:
        for p in parts:
            x[b, :, PART_INDEX[p]] = value
    return out


def poison_heads(qkv: np.ndarray, n_img: int, N: int, H: int, hd: int, images, value: float) -> np.ndarray:
    """poison(..., images, value) and, in the images that stay clean, every EVEN head too: the odd heads of the clean images are what is left."""
    out = poison(qkv, n_img, N, H, hd, images, value)
    x = out.reshape(n_img, N, 3, H, hd)
    for b in clean_images(n_img, images):
        x[b, :, :, 0::2] = value
    return out


def clean_heads(H: int) -> tuple:
    return tuple(range(1, H, 2))


def poison_images(imgs: np.ndarray, positions, kind: str) -> np.ndarray:
    """A copy of the image batch [n][...] (any image layout) with the images at `positions` replaced: "nan" = all NaN, "inf-pixel" = the
    image as it is with ONE +Inf value (the patch embedding spreads it over the patch's token, LayerNorm over the row, attention over the
    image), "1e30" = all 1e30 (finite on input, overflowing in the first products)."""
    out = np.array(imgs, dtype=np.float32, copy=True)
    for p in positions:
        if kind == "nan":
            out[p] = np.nan
        elif kind == "inf-pixel":
            out[p].flat[out[p].size // 3] = np.inf
        elif kind == "1e30":
            out[p] = 1e30
        else:
            raise ValueError(kind)
    return out


IMAGE_POISONS = ("nan", "inf-pixel", "1e30")


def sandwich(n_clean: int = 3):
    """Positions of the batch [A, P, B, P, C]: (clean positions, poisoned positions) -- every clean image but the last has a poisoned
    successor, every clean image but the first a poisoned predecessor."""
    n = 2 * n_clean - 1
    return tuple(range(0, n, 2)), tuple(range(1, n, 2))
