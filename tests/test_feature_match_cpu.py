"""CPU checks of the feature matcher (include/sfmba.h, sfmba_match_features): the two restatements of the contract in
tests/match_oracle.py agree, hand-written cases give the answers spelled out here, the entry point refuses to run without
a GPU, and the C++ shim carries the reference's matchFeatures symbol."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import match_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows(*bit_lists, nbytes=4):
    """uint8 rows with the given set bits."""
    out = np.zeros((len(bit_lists), nbytes), np.uint8)
    for r, bits in enumerate(bit_lists):
        for b in bits:
            out[r, b // 8] |= np.uint8(1 << (b % 8))
    return out


def both(dq, dt, ratio=mo.RATIO_F32):
    a = mo.match_pair(dq, dt, ratio, knn=mo.knn_insertion)
    b = mo.match_pair(dq, dt, ratio, knn=mo.knn_lexsort)
    c = mo.match_pair(dq, dt, ratio, knn=mo.knn_keys)
    assert a == b == c
    return a


@pytest.mark.parametrize("seed", range(4))
def test_oracle_formulations_agree_on_random_and_adversarial_inputs(seed):
    rng = np.random.default_rng(seed)
    for nbytes in (1, 5, 32, 64):
        dq = rng.integers(0, 256, (int(rng.integers(1, 90)), nbytes), dtype=np.uint8)
        dt = rng.integers(0, 256, (int(rng.integers(2, 130)), nbytes), dtype=np.uint8)
        dt[5 % len(dt)] = dt[0]                                  # a duplicated train row
        dq[:3] = dt[0]                                           # queries with an exact tie at distance 0
        dt2 = np.repeat(dt[:1], 7, axis=0)                       # all-equal train rows
        ties = (rng.integers(0, 2, (40, nbytes), dtype=np.uint8) * 255).astype(np.uint8)   # few distinct distances: many ties
        for q, t in ((dq, dt), (dq, dt2), (ties, ties), (dq, dt[:2])):
            for knn in (mo.knn_insertion, mo.knn_keys):
                got = knn(q, t)
                want = mo.knn_lexsort(q, t)
                for g, w in zip(got, want):
                    assert np.array_equal(g, w)
            both(q, t)
    descs = __import__("sfm_toy_library_amd").make_descriptors(3, 300, 32, seed=seed)
    for l, r in ((0, 1), (1, 2), (0, 0), (2, 3), (3, 4), (4, 0)):
        both(descs[l], descs[r])


def test_planted_descriptors_give_matches():
    import sfm_toy_library_amd as sfm
    descs = sfm.make_descriptors(3, 400, 32, seed=3)
    assert [len(d) for d in descs] == [400, 400, 400, 0, 1]
    m = mo.match_pair(descs[0], descs[1], knn=mo.knn_keys)
    assert len(m) > 100


def test_duplicated_best_row_is_dropped():
    dq = rows([0, 1])
    dt = rows([0, 1, 2], [20], [0, 1, 2])                   # rows 0 and 2 both at distance 1
    i1, d1, i2, d2 = mo.knn_insertion(dq, dt)
    assert (i1[0], d1[0], i2[0], d2[0]) == (0, 1, 2, 1)     # the lower index is best, the duplicate second
    assert both(dq, dt) == []                                 # 1 < 0.8 * 1 is false


def test_tie_between_second_and_third():
    dq = rows([])
    dt = rows([1, 2, 3], [5], [6], [7, 8])                    # distances 3, 1, 1, 2
    i1, d1, i2, d2 = mo.knn_lexsort(dq, dt)
    assert (i1[0], d1[0], i2[0], d2[0]) == (1, 1, 2, 1)
    dt = rows([1, 2, 3, 4, 9], [5], [6, 7, 8, 9, 10], [11, 12, 13, 14, 15])   # 5, 1, 5, 5: second is the lowest index at 5
    i1, d1, i2, d2 = mo.knn_insertion(dq, dt)
    assert (i1[0], d1[0], i2[0], d2[0]) == (1, 1, 0, 5)
    assert both(dq, dt) == [(0, 1, 1.0)]


def test_ratio_of_four_to_five_needs_the_float_ratio():
    dq = rows([])
    dt = rows([0, 1, 2, 3], [4, 5, 6, 7, 8])                  # d = 4 and 5
    assert mo.RATIO_F32 == 0.800000011920929 or abs(mo.RATIO_F32 - 0.800000011920929) < 1e-15
    assert both(dq, dt) == [(0, 0, 4.0)]                      # 4 < 4.0000000596: kept
    assert both(dq, dt, ratio=0.8) == []                      # 4 < 4.0 is false: dropped


def test_one_train_row_gives_nothing():
    dq = rows([], [1])
    assert both(dq, rows([3])) == []


def test_empty_images():
    assert both(rows([1]), np.zeros((0, 4), np.uint8)) == []
    assert both(np.zeros((0, 4), np.uint8), rows([1], [2])) == []


def test_pair_on_the_diagonal():
    d = rows([0], [0, 1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16])
    # every row is its own best at 0, second > 0: 0 < 0.8 * d2 -> kept, matched to itself
    assert both(d, d) == [(0, 0, 0.0), (1, 1, 0.0), (2, 2, 0.0)]
    dup = np.concatenate([d, d[:1]])                         # row 3 == row 0: both best at 0 with second 0 -> dropped
    assert both(dup, dup) == [(1, 1, 0.0), (2, 2, 0.0)]


def test_plan_restates_the_header():
    # one 5000 x 5000 pair: 10 tiles, slices limited by the train rows (ceil(5000 / 256) = 20)
    assert mo.plan([5000], [5000]) == [(10, 20)]
    # 120 such pairs: 1200 tiles in 3 batches of at most 512, 8 slices for a full batch
    assert mo.plan([5000] * 120, [5000] * 120) == [(512, 8), (512, 8), (176, 20)]
    assert mo.plan([10, 5000], [1, 0]) == []


def test_match_features_refuses_without_device():
    from sfm_toy_library_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    descs = [np.zeros((3, 32), np.uint8), np.ones((4, 32), np.uint8)]
    with pytest.raises(capi.SfmbaError, match="no HIP device"):
        capi.match_features(descs)


def test_match_features_argument_refusals_come_before_the_device():
    from sfm_toy_library_amd import capi
    descs = [np.zeros((3, 32), np.uint8), np.ones((4, 32), np.uint8)]
    with pytest.raises(capi.SfmbaError, match="rc=1: desc_bytes"):
        capi.match_features([np.zeros((3, 65), np.uint8)] * 2)
    with pytest.raises(capi.SfmbaError, match="rc=1: pair index out of range"):
        capi.match_features(descs, pairs=[(0, 2)])
    with pytest.raises(capi.SfmbaError, match="rc=1: ratio"):
        capi.match_features(descs, ratio=float("nan"))
    with pytest.raises(capi.SfmbaError, match="rc=1: ratio"):
        capi.match_features(descs, ratio=0.0)


def test_shim_exports_match_features():
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    so = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    syms = subprocess.check_output(["nm", "-C", so]).decode()
    assert "sfmtoylib::SfM2DFeatureUtilities::matchFeatures(" in syms
    assert "sfmtoylib::SfMFeatureMatching::createFeatureMatchMatrix(" in syms
    L = C.CDLL(so)
    assert hasattr(L, "sfmba_shim_match_features") and hasattr(L, "sfmba_shim_feature_match_matrix")
