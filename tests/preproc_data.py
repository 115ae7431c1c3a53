"""Case tables of the preprocessing tests (include/vitx.h "each model's own preprocessing"), shared by tests/test_cpu_preproc.py -- which pins
the host path to Pillow -- and tests/test_gpu_preproc.py -- which pins the device kernel to the host path, bit for bit.

The oracle is Pillow itself, called live: Image.fromarray(a).resize((W, H), BILINEAR | BICUBIC), a numpy slice for the crop, float64 for the
normalisation.  tests/golden/preproc_pil.json holds the sha1 of Pillow 12.2.0's u8 result for every (geometry, pattern, filter), recorded by
tests/golden/make_preproc_golden.py, so that the library is also held to a fixed record and a Pillow that changed its arithmetic is noticed.

The library's outputs are square, so a case is the geometry's resize followed by the centre crop of side min(W, H) (floor offsets): one axis
is covered from border to border, the other through its centre; the four square geometries cover both borders of both axes."""
import hashlib
import json
import os

import numpy as np

PP_REF_BICUBIC, PP_REF_BILINEAR, PP_PIL_BILINEAR, PP_PIL_BICUBIC = 0, 1, 2, 3
PP_STRETCH, PP_SHORTEST_EDGE = 0, 1
FILTERS = {"bilinear": PP_PIL_BILINEAR, "bicubic": PP_PIL_BICUBIC}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preproc_pil.json")

# (nx, ny, W, H): down-scale, up-scale, mixed, equal size, extreme aspect, non-integer and integer factors, a 3 x 2 source
GEOMETRIES = [(37, 23, 16, 16), (500, 375, 298, 224), (640, 480, 341, 256), (100, 60, 224, 134), (17, 400, 14, 329), (224, 224, 224, 224),
              (1000, 31, 224, 7), (33, 33, 32, 32), (64, 64, 16, 16), (3, 2, 8, 8)]
PATTERNS = ["random", "checker", "zeros", "ones"]

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
CLIP = ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))


def geo_id(g):
    return f"{g[0]}x{g[1]}-to-{g[2]}x{g[3]}"


def image(pattern, nx, ny, seed=0):
    """u8 [ny][nx][3].  checker: 0 / 255 by pixel parity, the three channels in three phases -- bicubic's negative lobes overshoot on it."""
    if pattern == "random":
        return np.random.default_rng(1000 * nx + ny + seed).integers(0, 256, (ny, nx, 3), dtype=np.uint8)
    if pattern == "checker":
        yy, xx = np.mgrid[0:ny, 0:nx]
        return np.stack([((yy + xx + c) & 1) * 255 for c in range(3)], -1).astype(np.uint8)
    return np.full((ny, nx, 3), 0 if pattern == "zeros" else 255, np.uint8)


def mean_std255(ms):
    """f32(255.0 * m): the values the `preproc` tensor stores and the arithmetic uses."""
    return tuple((255.0 * np.asarray(v, np.float64)).astype(np.float32) for v in ms)


def crop_offset(d, crop_round):
    """d = resized - crop.  0: transformers' floor; 1: torchvision CenterCrop's int(round(d / 2.0)) (Python rounds half to even)."""
    return d // 2 if crop_round == 0 else int(round(d / 2.0))


def resized_size(nx, ny, mode, a, b):
    if mode == PP_STRETCH:
        return a, b
    short, long_ = (nx, ny) if nx <= ny else (ny, nx)
    le = int(a * long_ / short)                # truncates, as transformers' get_resize_output_image_size and torchvision do
    return (a, le) if nx <= ny else (le, a)


def pillow_window(a, spec):
    """The u8 window Pillow + numpy give for `spec` (dict of vitx_preproc's integer fields) on image a: (window [S][S][3], (W, H, left, top))."""
    from PIL import Image
    ny, nx = a.shape[:2]
    W, H = resized_size(nx, ny, spec["resize_mode"], spec["resize_a"], spec["resize_b"])
    r = np.asarray(Image.fromarray(a).resize((W, H), Image.BICUBIC if spec["filter"] == PP_PIL_BICUBIC else Image.BILINEAR))
    S = spec["crop"] or W
    left, top = (crop_offset(W - S, spec["crop_round"]), crop_offset(H - S, spec["crop_round"])) if spec["crop"] else (0, 0)
    return r[top:top + S, left:left + S], (W, H, left, top)


def geometry_spec(g, filt, crop_round=0):
    """The case of a geometry: stretch to W x H, centre crop min(W, H)."""
    return dict(resize_mode=PP_STRETCH, resize_a=g[2], resize_b=g[3], filter=filt, crop=min(g[2], g[3]), crop_round=crop_round)


def make_pp(binding, spec, mean255=(0.0, 0.0, 0.0), std255=(1.0, 1.0, 1.0)):
    return binding.Preproc.make(mean255=tuple(float(v) for v in mean255), std255=tuple(float(v) for v in std255), **spec)


def golden_key(g, pattern, fname):
    return f"{geo_id(g)}/{pattern}/{fname}"


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a, np.uint8).tobytes()).hexdigest()


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- the device table: (id, nx, ny, n images, spec) beyond the geometries above --------------------------------------------------
def _se(short, crop, filt, crop_round=0):
    return dict(resize_mode=PP_SHORTEST_EDGE, resize_a=short, resize_b=0, filter=filt, crop=crop, crop_round=crop_round)


DEVICE_EXTRA = []
for _fname, _f in FILTERS.items():
    DEVICE_EXTRA += [
        (f"three-images-{_fname}", 90, 70, 3, _se(48, 40, _f)),                    # the image stride; 40 = 32 + 8 columns, 5 tile rows
        (f"crop33-offset-{_fname}", 90, 70, 1, _se(48, 33, _f)),                   # 33: one column and one row past a tile in both directions;
                                                                                   #   61 x 48 resized: left 14, top 7 -- the window's first taps are not at 0
        (f"crop40-torchvision-{_fname}", 90, 71, 2, _se(47, 40, _f, 1)),           # 59 x 47: odd differences 19 and 7 under round-half-even
        (f"portrait-offset-{_fname}", 70, 130, 1, _se(40, 35, _f)),                # vertical offset 19: the tile's first source row is relative to the source
        (f"upscale-{_fname}", 13, 9, 1, _se(20, 16, _f)),                          # 28 x 20 from 13 x 9: fewer taps at the borders than inside
        (f"stretch-nocrop-{_fname}", 50, 37, 1, dict(resize_mode=PP_STRETCH, resize_a=40, resize_b=40, filter=_f, crop=0, crop_round=0)),
        (f"identity-x-{_fname}", 48, 200, 1, dict(resize_mode=PP_STRETCH, resize_a=48, resize_b=56, filter=_f, crop=48, crop_round=0)),   # the horizontal pass skipped
    ]
