"""The restatement of tests/nn_data.py, pinned without a GPU: its selection is the host's vitx_topk (hostile rows included), it does not depend on
how the columns are cut into chunks and segments -- the property the device kernel is held to --, the exact-data generator's conditions hold, a
hand-computed vote, and every error of the nearest-neighbour entry points that is raised before any device call."""
import ctypes as C

import numpy as np
import pytest

import nn_data as NN


def _host_topk(binding, row, k):
    idx, val = binding.topk(row, k)
    return np.array(idx, np.int32), np.array(val, np.float32)


@pytest.mark.parametrize("kind", NN.KINDS)
def test_select_is_the_hosts_topk(binding, kind):
    for cols, k in ((1, 1), (64, 64), (127, 5), (1000, 64), (1000, 1), (129, 63)):
        s = NN.score_rows(kind, 3, cols, seed=cols + k)
        idx, bits = NN.select(s, k)
        for i in range(3):
            hi, hv = _host_topk(binding, s[i], k)
            assert np.array_equal(idx[i], hi), (kind, cols, k, i)
            # the host returns a value as stored; the selection returns it as its rank names it (either zero as +0, any NaN as the quiet NaN)
            assert np.array_equal(bits[i], NN.rank_value(NN.rank(hv))), (kind, cols, k, i)
            assert np.array_equal(NN.rank(s[i][idx[i]]), NN.rank(bits[i].view(np.float32)))
        assert all(len(set(r)) == k and r.min() >= 0 and r.max() < cols for r in idx)


def test_rank_is_the_documented_order():
    v = np.array([np.nan, -np.inf, -3.4028235e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.4028235e38, np.inf], np.float32)
    r = NN.rank(v).astype(np.int64)
    assert r[0] == 0 and r[5] == r[6] and (np.diff(np.delete(r, 5)) > 0).all()
    ok = ~np.isnan(v) & (v != 0)
    assert np.array_equal(NN.rank_value(NN.rank(v))[ok], v.view(np.uint32)[ok])
    assert np.array_equal(NN.rank_value(NN.rank(v))[[0, 5, 6]], np.array([0x7fc00000, 0, 0], np.uint32))
    # all-equal rows return indices 0 .. k-1, also from an index base just below 2^31
    idx, _ = NN.select(np.full((2, 50), 1.5, np.float32), 7, base_index=2 ** 31 - 2000)
    assert np.array_equal(idx, np.tile(np.arange(7) + 2 ** 31 - 2000, (2, 1)))


@pytest.mark.parametrize("kind", NN.KINDS)
def test_select_is_invariant_under_any_cut(kind):
    rng = np.random.default_rng(len(kind))
    for trial in range(12):
        cols = int(rng.integers(1, 700))
        k = int(rng.integers(1, min(64, cols) + 1))
        s = NN.score_rows(kind, 2, cols, seed=trial)
        want = NN.select(s, k)
        cuts = []
        left = cols
        while left:
            c = int(rng.integers(1, left + 1)) if rng.random() < 0.7 else left
            cuts.append(c); left -= c
        for segs in (1, 3, 8):
            got = NN.select_cut(s, k, cuts, segs)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (kind, cols, k, cuts, segs)


def test_exact_data_conditions():
    """Every partial sum of every score of the exact case is exact in f32, in any order (the asserts of _exact_case in test_gpu_zeroshot.py)."""
    for n, G in ((1, 1), (3, 127), (129, 385)):
        z, t, a = NN.exact_case(n, G, seed=n * 1000 + G)
        exact, most = NN.exact_conditions(a, t)
        assert exact and most < 2 ** 24
        assert np.array_equal(np.abs(a), np.full_like(a, 0.125)) and np.abs(t).max() <= 1
        s = a.astype(np.float64) @ t.astype(np.float64).T
        assert np.array_equal(s, s.astype(np.float32).astype(np.float64))
        if G > 64:
            assert len(np.unique(s[0])) < G           # ties are frequent: the index half of the key decides


def test_vote_of_three_neighbours_by_hand():
    """Scores 0.9, 0.83, 0.76 at T = 0.07: w = 1, e^-1, e^-2 (to f32 rounding of the scores).  Labels 2, 0, 2 of 4 classes."""
    score = np.array([[0.9, 0.83, 0.76]], np.float32)
    idx = np.array([[5, 1, 3]], np.int32)
    labels = np.array([9, 0, 9, 2, 9, 2], np.int32) % 4          # rows 5, 1, 3 -> 2, 0, 2
    v = NN.vote64(score, idx, labels, 4, 0.07)
    e1, e2 = np.exp(-1.0), np.exp(-2.0)
    W = 1 + e1 + e2
    assert np.allclose(v[0], [e1 / W, 0, (1 + e2) / W, 0], rtol=1e-5, atol=0) and v[0, 1] == 0 and v[0, 3] == 0
    assert abs(v.sum() - 1) < 1e-12
    one = NN.vote64(score[:, :1], idx[:, :1], labels, 4, 0.07)
    assert np.array_equal(one[0], [0, 0, 1, 0])


def test_errors_that_need_no_device(binding):
    """NULL contexts, and every argument check of the vitx_op_nn* entry points: all raised before any device call."""
    L = binding.lib()
    A, U = binding.ERR_ARG, binding.ERR_UNSUPPORTED
    g = np.zeros(64, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert L.vitx_nn_set(None, g, 1, 64, 1, 0, None, 0, 0.07) == A
    i32 = np.zeros(4, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert L.vitx_nn_read(None, i32, g, None) == A
    assert L.vitx_nn_width(None, 0) == 0 and L.vitx_nn_rows(None) == 0 and L.vitx_nn_k(None) == 0 and L.vitx_nn_labels(None) == 0
    assert L.vitx_nn_images(None) == 0 and L.vitx_nn_device(None) is None and L.vitx_nn_scratch_bytes(None) == 0
    assert binding.op_nn_state_bytes(3, 5) == binding.op_nn_state_bytes(1, 5) * 3 and binding.op_nn_state_bytes(3, 5) % 8 == 0
    p = 0x10000
    ok = dict(d_scores=p, ld=100, n=2, cols=100, base_index=0, d_state=p, k=5, first=True)
    for change, code in [(dict(d_scores=0), A), (dict(d_state=0), A), (dict(n=0), A), (dict(cols=0), A), (dict(ld=99), A), (dict(k=0), A), (dict(base_index=-1), A),
                         (dict(d_scores=p + 2), A), (dict(d_state=p + 4), A), (dict(k=65), U), (dict(base_index=2 ** 31 - 100), U)]:
        with pytest.raises(binding.VitxError) as ei:
            binding.op_nn_select(**{**ok, **change})
        assert ei.value.code == code, change
    ok = dict(d_state=p, n=2, k=5, d_pairs=p, d_labels=p, n_labels=3, temperature=0.07, d_vote=p)
    for change, code in [(dict(d_state=0), A), (dict(d_pairs=0), A), (dict(n=0), A), (dict(k=0), A), (dict(n_labels=0), A), (dict(d_vote=0), A),
                         (dict(temperature=0.0), A), (dict(temperature=-1.0), A), (dict(temperature=float("inf")), A), (dict(temperature=float("nan")), A), (dict(k=65), U)]:
        with pytest.raises(binding.VitxError) as ei:
            binding.op_nn_finish(**{**ok, **change})
        assert ei.value.code == code, change
    ok = dict(dtype=1, d_z=p, z_stride=64, z_is_operand=False, n=2, d_gallery=p, G=300, E=64, k=5, chunk=128, d_a=p, d_acc=p, d_state=p, d_pairs=p)
    for change, code in [(dict(d_z=0), A), (dict(d_gallery=0), A), (dict(d_a=0), A), (dict(d_acc=0), A), (dict(d_state=0), A), (dict(d_pairs=0), A), (dict(n=0), A),
                         (dict(G=0), A), (dict(dtype=2), A), (dict(k=0), A), (dict(k=301), A), (dict(G=4, k=5), A), (dict(chunk=0), A), (dict(chunk=100), A), (dict(chunk=-128), A),
                         (dict(z_stride=60), A), (dict(z_stride=66), A), (dict(d_z=p + 4), A), (dict(d_gallery=p + 8), A), (dict(d_state=p + 8), A),
                         (dict(k=65), U), (dict(E=96, z_stride=96), U), (dict(G=2 ** 31 - 128), U)]:
        with pytest.raises(binding.VitxError) as ei:
            binding.op_nn(**{**ok, **change})
        assert ei.value.code == code, change
