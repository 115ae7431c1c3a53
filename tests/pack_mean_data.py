"""Cases of tests/test_gpu_pack_mean.py and tests/test_cpu_pack_mean.py (include/vitx.h "packed batches", pool_head = 2 and VITX_FEAT_MEAN)."""
import numpy as np

import feature_data as FD

T, GAP = 5, 3                                 # prefix rows per image (the class row and four registers); NaN rows in front of and behind a pack
WIDTHS = (128, 768, 1152)                     # a flat width, a tiled one, one above 1024 (8 waves, one row in flight)

def counts(R: int, W: int):
    """Patch rows per image, around the wave stride W and the chunk of R rows."""
    return [1, 2, W - 1, W, W + 1, R - 1, R, R + 1, 2 * R, 2 * R + 1, 3 * R + 7]

def image_rows(D: int, cnts):
    """One [T + c][D] f32 block per image: hostile rows (feature_data.mixed_images) for even images, ordinary ones for odd images."""
    return [(FD.mixed_images if i % 2 == 0 else FD.random_images)(D, 1, T + c, seed=i + 1)[0] for i, c in enumerate(cnts)]

def pack(blocks):
    """The blocks end to end between GAP rows of NaN: (x [rows][D], row0 [n + 1])."""
    nan = np.full((GAP, blocks[0].shape[1]), np.nan, np.float32)
    return np.concatenate([nan] + list(blocks) + [nan]), GAP + np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int32)
