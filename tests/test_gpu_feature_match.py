"""The feature matcher on the MI355X (-m gpu) against the CPU restatement of the contract (tests/match_oracle.py,
include/sfmba.h sfmba_match_features).  Integer work: every comparison is EXACT -- the same entries, the same order, the
same float distances.  Calls go through the C ABI and through the reference-signature functions of
host/SfM2DFeatureUtilities.cpp (matchFeatures, createFeatureMatchMatrix)."""
import ctypes as C
import os

import numpy as np
import pytest

import match_oracle as mo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


@pytest.fixture(scope="module")
def sfm():
    import sfm_toy_library_amd
    return sfm_toy_library_amd


def gpu_lists(res):
    pl, pr, ptr, q, t, d = res
    out = []
    for p in range(len(pl)):
        s = slice(ptr[p], ptr[p + 1])
        out.append(((int(pl[p]), int(pr[p])), list(zip(q[s].tolist(), t[s].tolist(), d[s].tolist()))))
    return out


def check(capi, descs, pairs=None, ratio=mo.RATIO_F32, knn=mo.knn_keys):
    got = gpu_lists(capi.match_features(descs, pairs=pairs, ratio=ratio))
    want = mo.match_features(descs, pairs=pairs, ratio=ratio, knn=knn)
    assert got == want
    return got


def planted(rng, n_q, n_t, nbytes, flips=3):
    """query rows = noisy copies of some train rows, plus random rows and all-zero rows."""
    t = rng.integers(0, 256, (n_t, nbytes), dtype=np.uint8)
    q = rng.integers(0, 256, (n_q, nbytes), dtype=np.uint8)
    if n_t:
        src = rng.integers(0, n_t, n_q)
        take = rng.random(n_q) < 0.6
        q[take] = t[src[take]]
        bits = np.unpackbits(q, axis=1)
        for _ in range(flips):
            bits[np.arange(n_q), rng.integers(0, 8 * nbytes, n_q)] ^= 1
        q = np.packbits(bits, axis=1)[:, :nbytes]
    q[: max(1, n_q // 17)] = 0
    if n_t > 3:
        t[n_t // 3] = 0
        t[n_t // 2] = t[1]                        # a duplicated train row
    return [np.ascontiguousarray(q), np.ascontiguousarray(t)]


@pytest.mark.parametrize("nbytes", [32, 61, 64, 16, 1])
def test_sweep_train_counts_exact(capi, nbytes):
    rng = np.random.default_rng(nbytes)
    for n_t in (1, 2, 3, 63, 64, 65, 255, 256, 257):
        for n_q in (1, 37, 511, 513):
            descs = planted(rng, n_q, n_t, nbytes)
            check(capi, descs, pairs=[(0, 1), (1, 0), (0, 0)])


@pytest.mark.parametrize("nbytes", [32, 64])
def test_several_slices_exact(capi, nbytes):
    rng = np.random.default_rng(7 + nbytes)
    descs = planted(rng, 700, 9000, nbytes)                   # 2 tiles x ceil(9000 / 256) -> 32 slices of 282 rows
    assert mo.plan([700], [9000]) == [(2, 32)]
    got = check(capi, descs, pairs=[(0, 1)])
    assert len(got[0][1]) > 100


def test_hand_written_cases(capi):
    def rows(*bit_lists, nbytes=4):
        out = np.zeros((len(bit_lists), nbytes), np.uint8)
        for r, bits in enumerate(bit_lists):
            for b in bits:
                out[r, b // 8] |= np.uint8(1 << (b % 8))
        return out
    dup = [rows([0, 1]), rows([0, 1, 2], [20], [0, 1, 2])]                              # duplicated best row: dropped
    assert check(capi, dup, pairs=[(0, 1)])[0][1] == []
    tie = [rows([]), rows([1, 2, 3, 4, 9], [5], [6, 7, 8, 9, 10], [11, 12, 13, 14, 15])]   # 5, 1, 5, 5
    assert check(capi, tie, pairs=[(0, 1)])[0][1] == [(0, 1, 1.0)]
    four_five = [rows([]), rows([0, 1, 2, 3], [4, 5, 6, 7, 8])]                        # 4 vs 5
    assert check(capi, four_five, pairs=[(0, 1)])[0][1] == [(0, 0, 4.0)]
    assert check(capi, four_five, pairs=[(0, 1)], ratio=0.8)[0][1] == []
    one = [rows([], [1]), rows([3])]
    assert check(capi, one, pairs=[(0, 1), (1, 0)]) == [((0, 1), []), ((1, 0), [(0, 0, 1.0)])]   # 1 train row: nothing; 2: kept
    empty = [rows([1]), np.zeros((0, 4), np.uint8)]
    assert check(capi, empty, pairs=[(0, 1), (1, 0), (1, 1), (0, 0)])[:3] == [((0, 1), []), ((1, 0), []), ((1, 1), [])]
    diag = [rows([0], [0, 1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16], [0])]
    assert check(capi, diag, pairs=[(0, 0)])[0][1] == [(1, 1, 0.0), (2, 2, 0.0)]
    zeros = [np.zeros((5, 32), np.uint8), np.zeros((6, 32), np.uint8)]                 # all-equal rows: every query dropped
    assert check(capi, zeros)[0][1] == []


def test_generated_descriptors_all_pairs(capi, sfm):
    descs = sfm.make_descriptors(4, 1500, 32, seed=11)        # + an empty image and a one-row image
    got = check(capi, descs)
    assert len(got) == 15 and sum(len(m) for _, m in got) > 1000


def test_crazy_horse_shape_exact(capi, sfm):
    descs = sfm.make_descriptors(7, 5000, 32, seed=5, extras=False)
    got = check(capi, descs)
    assert len(got) == 21 and all(len(m) > 500 for _, m in got)


def test_batching_and_slicing_do_not_change_the_result(capi, sfm):
    descs = sfm.make_descriptors(3, 5000, 32, seed=21, extras=False)
    alone = capi.match_features(descs, pairs=[(1, 2)])
    assert gpu_lists(alone)[0][1] == mo.match_pair(descs[1], descs[2], knn=mo.knn_keys)
    pairs = [(0, 1)] * 70 + [(1, 2)] + [(2, 0)] * 50 + [(1, 2)]
    plan = mo.plan([5000] * len(pairs), [5000] * len(pairs))
    assert len(plan) >= 3 and mo.plan([5000], [5000])[0][1] not in {s for _, s in plan[:2]}
    batch = capi.match_features(descs, pairs=pairs)
    lists = gpu_lists(batch)
    assert lists[70][1] == lists[-1][1] == gpu_lists(alone)[0][1]
    again = capi.match_features(descs, pairs=pairs)
    for a, b in zip(batch, again):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_capacity_protocol(capi, sfm):
    descs = sfm.make_descriptors(3, 800, 32, seed=31, extras=False)
    full = capi.match_features(descs)
    n = int(full[2][-1])
    assert n > 10
    img_ptr = np.array([0, 800, 1600, 2400], np.int64)
    flat = np.ascontiguousarray(np.concatenate(descs))
    pl = np.array([0, 0, 1], np.int32); pr = np.array([1, 2, 2], np.int32)
    ptr = np.full(4, -7, np.int64)
    q = np.full(n, -5, np.int32); t = np.full(n, -5, np.int32); d = np.full(n, -5, np.float32)
    total = C.c_int64(0)
    L = capi.lib()
    lp, ip, fp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def call(cap):
        return L.sfmba_match_features(0, 3, img_ptr.ctypes.data_as(lp), flat.ctypes.data_as(C.POINTER(C.c_ubyte)), 32, 3,
                                      pl.ctypes.data_as(ip), pr.ctypes.data_as(ip), C.c_double(mo.RATIO_F32), ptr.ctypes.data_as(lp),
                                      q.ctypes.data_as(ip), t.ctypes.data_as(ip), d.ctypes.data_as(fp), C.c_int64(cap), C.byref(total))
    assert call(n - 1) == capi.SFMBA_ERR_CAPACITY
    assert total.value == n and np.array_equal(ptr, full[2])
    assert (q == -5).all() and (t == -5).all() and (d == -5).all()
    assert call(total.value) == 0
    assert np.array_equal(ptr, full[2]) and np.array_equal(q, full[3]) and np.array_equal(t, full[4]) and np.array_equal(d, full[5])


def test_argument_refusals(capi):
    descs = [np.zeros((3, 32), np.uint8), np.ones((4, 32), np.uint8)]
    for bad, msg in (([np.zeros((3, 65), np.uint8)] * 2, "desc_bytes"), ([np.zeros((3, 0), np.uint8)] * 2, "desc_bytes")):
        with pytest.raises(capi.SfmbaError, match=msg):
            capi.match_features(bad)
    for pairs in ([(0, 2)], [(-1, 0)], [(1, 5)]):
        with pytest.raises(capi.SfmbaError, match="pair index out of range"):
            capi.match_features(descs, pairs=pairs)
    for ratio in (float("nan"), float("inf"), 0.0, -0.5):
        with pytest.raises(capi.SfmbaError, match="ratio"):
            capi.match_features(descs, ratio=ratio)


def _shim():
    L = C.CDLL(SHIM)
    L.sfmba_shim_match_features.restype = C.c_int64
    L.sfmba_shim_feature_match_matrix.restype = C.c_int64
    return L


def test_shim_match_features(capi, sfm):
    L = _shim()
    descs = sfm.make_descriptors(2, 2000, 32, seed=41, extras=False)
    img_ptr = np.array([0, 2000, 4000], np.int64)
    flat = np.ascontiguousarray(np.concatenate(descs))
    cap = 4000
    q, t, im = (np.zeros(cap, np.int32) for _ in range(3))
    d = np.zeros(cap, np.float32)
    ip = C.POINTER(C.c_int32)
    n = L.sfmba_shim_match_features(img_ptr.ctypes.data_as(C.POINTER(C.c_int64)), flat.ctypes.data_as(C.POINTER(C.c_ubyte)), 32,
                                    C.c_int64(cap), q.ctypes.data_as(ip), t.ctypes.data_as(ip), im.ctypes.data_as(ip),
                                    d.ctypes.data_as(C.POINTER(C.c_float)))
    want = mo.match_pair(descs[0], descs[1], knn=mo.knn_keys)
    assert 0 < n <= cap
    assert list(zip(q[:n].tolist(), t[:n].tolist(), d[:n].tolist())) == want
    assert (im[:n] == 0).all()


def test_shim_create_feature_match_matrix(capi, sfm):
    L = _shim()
    descs = sfm.make_descriptors(5, 1200, 32, seed=51)        # 7 images: 5 + an empty one + a one-row one
    n_img = len(descs)
    img_ptr = np.zeros(n_img + 1, np.int64)
    img_ptr[1:] = np.cumsum([len(x) for x in descs])
    flat = np.ascontiguousarray(np.concatenate(descs))
    sizes = np.full(n_img * n_img, -1, np.int64)
    cap = 20000
    q, t, im = (np.zeros(cap, np.int32) for _ in range(3))
    d = np.zeros(cap, np.float32)
    ip = C.POINTER(C.c_int32)
    n = L.sfmba_shim_feature_match_matrix(n_img, img_ptr.ctypes.data_as(C.POINTER(C.c_int64)), flat.ctypes.data_as(C.POINTER(C.c_ubyte)), 32,
                                          sizes.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int64(cap), q.ctypes.data_as(ip),
                                          t.ctypes.data_as(ip), im.ctypes.data_as(ip), d.ctypes.data_as(C.POINTER(C.c_float)))
    assert 0 < n <= cap                                          # -1: device failure, -2: not n x n
    want = dict(mo.match_features(descs, knn=mo.knn_keys))
    sizes = sizes.reshape(n_img, n_img)
    o = 0
    for l in range(n_img):
        for r in range(n_img):
            k = int(sizes[l, r])
            got = list(zip(q[o:o + k].tolist(), t[o:o + k].tolist(), d[o:o + k].tolist()))
            if l < r:
                assert got == want[(l, r)], (l, r)
            else:
                assert k == 0                                    # the diagonal and below stay empty (SfM.cpp:163-210)
            o += k
    assert o == n and (im[:n] == 0).all()


def test_chain_into_find_2d3d_matches(capi, sfm):
    """GPU match matrix -> sfmba_find_2d3d_matches equals the association oracle on the oracle's match matrix."""
    from oracle import association_oracle as ao
    descs = sfm.make_descriptors(5, 600, 32, seed=61, extras=False)
    n_views = len(descs)
    res = capi.match_features(descs)
    gpu_mm = {k: v for k, v in gpu_lists(res)}
    orc_mm = dict(mo.match_features(descs, knn=mo.knn_keys))
    assert gpu_mm == orc_mm
    rng = np.random.default_rng(62)
    done = [0, 2]
    cloud = []
    for (l, r), lst in sorted(orc_mm.items()):                # a cloud triangulated from the done pair's matches
        if (l, r) != (0, 2):
            continue
        for qq, tt, _ in lst:
            cloud.append((rng.uniform(-1, 1, 3).astype(np.float32), {0: int(qq), 2: int(tt)}))
    assert len(cloud) > 20
    want = ao.find_2d3d_matches(n_views, done, cloud, orc_mm)
    vp, vi, fi = capi._flat_views([v for _, v in cloud])
    pl, pr, pp, q, t, _ = res
    ptr, op, of = capi.find_2d3d_matches(n_views, done, vp, vi, fi, pl, pr, pp, q, t)
    got = {v: list(zip(op[ptr[v]:ptr[v + 1]].tolist(), of[ptr[v]:ptr[v + 1]].tolist())) for v in range(n_views) if v not in done}
    assert got == want
    assert sum(len(v) for v in want.values()) > 0
