"""Fixtures of the packed attention-map tests (include/vitx.h "packed batches", attention maps), shared by tests/test_cpu_pack_attn.py and
tests/test_gpu_pack_attn.py.  Everything here is host arithmetic.

The reference of every kernel test is the fixed-shape entry point on the image alone (op_attention_map, op_rollout_factor, op_rollout_step,
op_rollout_row), bit for bit: the packed kernels run the same bodies (csrc/attention_map_tile.h) and differ in how a workgroup finds its image."""
import numpy as np

MAX_TOKENS = 1024                                     # kernels.h kAttnMeanMaxTokens: the rollout kernels' bound per image

# One packed launch against the fixed-shape ops.  Around the 16-row block (15, 16, 17), the 64-key tile and NT = 1 | 2 (64, 65), NT = 4 | 8 (257), the
# largest image the kernels take (1024: NT = 16, the launch's NT) beside the two smallest (1 token, one on either side).
TOKENS = (17, 1, 64, 1024, 65, 16, 257, 15)

# (D, H): head dims 64, 32 and 48 (48: one and a half 32-dim chunks of the head-mean MFMA, six 16-byte pieces per key row in lane groups of 8)
SHAPES = ((128, 2), (128, 4), (192, 4))


def row0_of_tokens(tokens):
    return np.concatenate([[0], np.cumsum(tokens)]).astype(np.int32)


def tables(row0):
    """(rblk0 [n + 1], sq0 [n + 1]) of a pack: the running count of ceil(N_i / 16) and the running sum of N_i^2 (kernels.h attn_pack_tables)."""
    N = np.diff(np.asarray(row0, np.int64))
    rblk0 = np.concatenate([[0], np.cumsum((N + 15) // 16)])
    sq0 = np.concatenate([[0], np.cumsum(N * N)])
    return rblk0, sq0


def map_launches(L, layers, rollout):
    """Kernel launches a packed forward adds with maps on (packed_forward.cpp pack_attention_maps): one class-map launch per selected layer; with
    rollout the factor of every layer but the last (L - 1), the in-place step of every layer between the first and the last (max(L - 2, 0)), the row
    (1), and the last layer's class maps once more when that layer is not selected."""
    layers = sorted(set(layers))
    n = len(layers)
    if rollout:
        n += (L - 1) + max(L - 2, 0) + 1 + (0 if (L - 1) in layers else 1)
    return n
