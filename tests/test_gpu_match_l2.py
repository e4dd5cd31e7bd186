"""The float matcher on the MI355X (-m gpu) against the CPU restatement of the contract (tests/match_l2_oracle.py, include/sfmba.h
sfmba_match_features_l2).  The squared distance is defined operation by operation, so every comparison is BIT FOR BIT: the same
pair_ptr, the same query and train indices, the same distances compared as uint32.  Calls go through the C ABI and through the
reference-signature functions of host/SfM2DFeatureUtilities.cpp (matchFeatures, createFeatureMatchMatrix) on CV_32F descriptors."""
import ctypes as C
import os

import numpy as np
import pytest

import match_l2_cases as cases
import match_l2_oracle as lo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
SFMBA_ERR_INVALID_ARG = 1                                     # include/sfmba.h


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


def gpu_lists(res):
    """[((l, r), [(q, j, bits of d), ...]), ...] -- the form of lo.match_features."""
    pl, pr, ptr, q, t, d = res
    assert d.dtype == np.float32 and ptr[0] == 0 and np.all(np.diff(ptr) >= 0) and ptr[-1] == len(q) == len(t) == len(d)
    db = d.view(np.uint32)
    return [((int(pl[p]), int(pr[p])), list(zip(q[ptr[p]:ptr[p + 1]].tolist(), t[ptr[p]:ptr[p + 1]].tolist(), db[ptr[p]:ptr[p + 1]].tolist())))
            for p in range(len(pl))]


def check(capi, descs, pairs=None, ratio=lo.RATIO_F32):
    got = gpu_lists(capi.match_features_l2(descs, pairs=pairs, ratio=ratio))
    want = lo.match_features(descs, pairs=pairs, ratio=ratio)
    assert got == want
    return got


def f32(*rows):
    return np.array(rows, np.float32)


def bits_of(x):
    return int(np.float32(x).view(np.uint32))


# ---- the case table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cases.CASES)), ids=["%dx%dx%d" % c for c in cases.CASES])
def test_case_table_exact(capi, index):
    nq, nt, dims = cases.CASES[index]
    descs = cases.case_rows(index)
    small = nq * nt * dims <= 200000
    got = check(capi, descs, pairs=[(0, 1), (1, 0), (0, 0), (1, 1)] if small else [(0, 1)])
    if cases.CASES[index] == cases.SLICED:
        assert lo.plan([nq], [nt]) == [(2, 3)]               # the unit's own plan cuts this train image into 3 slices
    if nq >= 37 and nt >= 15 and dims > 1:                   # (one column of unit-norm rows is +-1: all duplicates, all dropped)
        assert len(got[0][1]) > 0                            # the planted near matches are kept


# ---- special rows -----------------------------------------------------------------------------------------------------------------
def test_special_rows(capi):
    # duplicate train rows: the tie goes to the lower index (as second neighbour here: the best is unique)
    tie = [f32([0, 0, 0]), f32([5, 0, 0], [0, 1, 0], [0, 5, 0], [0, 0, 5])]
    assert check(capi, tie, pairs=[(0, 1)])[0][1] == [(0, 1, bits_of(1.0))]
    first = [f32([0, 0]), f32([9, 9], [3, 4], [3, 4], [0, 1])]                        # best 1 (row 3); duplicates 5, 5 behind it
    assert check(capi, first, pairs=[(0, 1)])[0][1] == [(0, 3, bits_of(1.0))]
    # a query equal to one train row: kept (0 < 0.8 d); equal to two train rows: dropped (0 < 0 is false)
    one = [f32([1, 2, 3]), f32([7, 7, 7], [1, 2, 3], [1, 2, 4])]
    assert check(capi, one, pairs=[(0, 1)])[0][1] == [(0, 1, 0)]
    two = [f32([1, 2, 3]), f32([1, 2, 3], [7, 7, 7], [1, 2, 3])]
    assert check(capi, two, pairs=[(0, 1)])[0][1] == []
    # 1e19-scale rows: a best of +inf is dropped; a finite best with an infinite second is kept
    q = f32([0.0, 0.0])
    assert check(capi, [q, f32([3e19, 0.0], [-3e19, 1.0], [0.0, 2.5e19])], pairs=[(0, 1)])[0][1] == []
    assert check(capi, [q, f32([3e19, 0.0], [3.0, 4.0], [-3e19, 1.0])], pairs=[(0, 1)])[0][1] == [(0, 1, bits_of(5.0))]
    assert check(capi, [q, f32([3e19, 0.0], [1e19, 0.0], [-3e19, 1.0])], pairs=[(0, 1)])[0][1] == [(0, 1, bits_of(1e19))]   # s = 1e38 finite
    # 1e-21-scale rows: the squares are subnormal (1e-42); a flushed subnormal would give s = 0 and drop or reorder these
    tiny = [f32([0.0, 0.0, 0.0]), f32([2e-21, 0.0, 0.0], [1e-21, 0.0, 0.0], [0.0, 3e-21, 1e-21])]
    got = check(capi, tiny, pairs=[(0, 1)])[0][1]
    s = lo.sq_distances_chain(tiny[0], tiny[1])[0]
    assert np.all(s > 0) and np.all(s < np.finfo(np.float32).tiny) and got == [(0, 1, bits_of(np.sqrt(s[1])))]
    # integer rows 0..255
    rng = np.random.default_rng(3)
    ints = [rng.integers(0, 256, (70, 128)).astype(np.float32), rng.integers(0, 256, (90, 128)).astype(np.float32)]
    ints[0][:30] = ints[1][10:40]; ints[0][:30, 5] = (ints[0][:30, 5] + 1) % 256
    assert len(check(capi, ints)[0][1]) >= 30
    # -0.0 entries: s is +0, a duplicate of the query whatever the sign of its zeros
    neg = [f32([-0.0, 0.0, 1.0], [0.0, -0.0, -0.0]), f32([0.0, -0.0, 1.0], [-0.0, -0.0, 0.0], [2.0, 2.0, 2.0])]
    assert check(capi, neg, pairs=[(0, 1)])[0][1] == [(0, 0, 0), (1, 1, 0)]
    # all rows equal: every query dropped; the reference's own ratio keeps 4 against 5 only as (double)0.8f
    assert check(capi, [np.ones((5, 9), np.float32), np.ones((6, 9), np.float32)])[0][1] == []
    four_five = [f32([0.0]), f32([4.0], [5.0])]
    assert check(capi, four_five)[0][1] == [(0, 0, bits_of(4.0))]
    assert check(capi, four_five, ratio=0.8)[0][1] == []


# ---- cut independence -------------------------------------------------------------------------------------------------------------
def test_cut_independence(capi):
    rng = np.random.default_rng(17)
    base = rng.normal(size=(60, 8)).astype(np.float32)
    descs = []
    for _ in range(40):                                      # 40 images x 30 rows x 8 dims: noisy copies of a common pool
        rows = base[rng.choice(60, 30, replace=False)] + rng.normal(scale=0.02, size=(30, 8)).astype(np.float32)
        descs.append(np.ascontiguousarray(rows, np.float32))
    pairs = [(i, j) for i in range(40) for j in range(i + 1, 40)]
    assert len(pairs) == 780
    whole = check(capi, descs, pairs=pairs)                  # all 780 pairs in one call, against the oracle
    by_pair = dict(whole)
    assert sum(len(m) for m in by_pair.values()) > 780
    for p in pairs[::78][:10]:                               # each of 10 chosen pairs alone
        assert gpu_lists(capi.match_features_l2(descs, pairs=[p])) == [(p, by_pair[p])]
    back = gpu_lists(capi.match_features_l2(descs, pairs=pairs[::-1]))
    assert back == whole[::-1]
    odd = [(7, 3), (5, 5), (0, 1), (3, 7), (0, 1), (39, 0)]  # l > r, l == r and a repeated pair
    got = check(capi, descs, pairs=odd)
    assert got[2] == got[4] == ((0, 1), by_pair[(0, 1)]) and got[3] == ((3, 7), by_pair[(3, 7)])
    assert all(q == t and d == 0 for q, t, d in got[1][1]) and len(got[1][1]) == 30       # an image against itself: every row finds itself


# ---- against the merged Hamming unit ----------------------------------------------------------------------------------------------
def test_cross_check_against_the_hamming_unit(capi):
    """32-byte rows expanded to 256 floats of 0.0 / 1.0: s IS the Hamming distance, and sqrt(d1) < 0.8 sqrt(d2) gives d1 < 0.64 d2, so
    every L2 match is a Hamming match with the same train index, its distance the fp32 root of the Hamming distance."""
    rng = np.random.default_rng(23)
    t = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    tb = np.unpackbits(t[:200], axis=1)                      # planted near-duplicates: 200 query rows = train rows with 6 flipped bits
    for _ in range(6):
        tb[np.arange(200), rng.integers(0, 256, 200)] ^= 1
    q[:200] = np.packbits(tb, axis=1)
    byte_descs = [q, t]
    float_descs = [np.unpackbits(x, axis=1).astype(np.float32) for x in byte_descs]
    assert float_descs[0].shape == (300, 256)
    pairs = [(0, 1), (1, 0)]
    l2 = gpu_lists(capi.match_features_l2(float_descs, pairs=pairs))
    pl, pr, ptr, hq, ht, hd = capi.match_features(byte_descs, pairs=pairs)
    for p, (pair, lst) in enumerate(l2):
        ham = {int(a): (int(b), float(c)) for a, b, c in zip(hq[ptr[p]:ptr[p + 1]], ht[ptr[p]:ptr[p + 1]], hd[ptr[p]:ptr[p + 1]])}
        assert len(ham) > 0
        if p == 0:
            assert len(lst) >= 150
        for qq, tt, dbits in lst:
            assert qq in ham and ham[qq][0] == tt, (pair, qq)
            assert dbits == bits_of(np.sqrt(np.float32(ham[qq][1]))), (pair, qq)
    assert len(l2[0][1]) > 0
    assert l2 == lo.match_features(float_descs, pairs=pairs)


# ---- refusals and capacity --------------------------------------------------------------------------------------------------------
def raw_call(capi, img_ptr, flat, dims, pl, pr, ratio, ptr, q, t, d, cap, total):
    lp, ip, fp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    return capi.lib().sfmba_match_features_l2(0, len(img_ptr) - 1, img_ptr.ctypes.data_as(lp), flat.ctypes.data_as(fp), C.c_int(dims), len(pl),
                                              pl.ctypes.data_as(ip), pr.ctypes.data_as(ip), C.c_double(ratio), ptr.ctypes.data_as(lp),
                                              q.ctypes.data_as(ip), t.ctypes.data_as(ip), d.ctypes.data_as(fp), C.c_int64(cap), C.byref(total))


def test_argument_refusals(capi):
    descs = [np.zeros((3, 8), np.float32), np.ones((4, 8), np.float32)]
    for bad in ([np.zeros((3, 513), np.float32)] * 2, [np.zeros((3, 0), np.float32)] * 2):
        with pytest.raises(capi.SfmbaError, match="dims"):
            capi.match_features_l2(bad)
    for value in (np.nan, np.inf, -np.inf):
        bad = [descs[0].copy(), descs[1].copy()]
        bad[1][2, 5] = value
        with pytest.raises(capi.SfmbaError, match="non-finite descriptor value in image 1, row 2"):
            capi.match_features_l2(bad)
    for pairs in ([(0, 2)], [(-1, 0)], [(1, 5)]):
        with pytest.raises(capi.SfmbaError, match="pair index out of range"):
            capi.match_features_l2(descs, pairs=pairs)
    for ratio in (float("nan"), float("inf"), 0.0, -0.5):
        with pytest.raises(capi.SfmbaError, match="ratio"):
            capi.match_features_l2(descs, ratio=ratio)
    # too many rows: decided from img_ptr alone, before desc is read (a 1-float buffer stands in for it)
    one = np.zeros(1, np.float32)
    ptr = np.full(3, -7, np.int64)
    q = np.full(1, -5, np.int32); t = np.full(1, -5, np.int32); d = np.full(1, -5, np.float32)
    total = C.c_int64(-3)
    pl = np.array([0, 0], np.int32); pr = np.array([1, 1], np.int32)
    big = np.array([0, 1 << 22, (1 << 22) + 2], np.int64)                                  # an image with 2^22 rows
    assert raw_call(capi, big, one, 1, pl, pr, lo.RATIO_F32, ptr, q, t, d, 1, total) == SFMBA_ERR_INVALID_ARG
    assert b"2^22" in capi.lib().sfmba_last_error()
    many = np.array([0, (1 << 22) - 1, (1 << 22) + 1], np.int64)                           # 513 pairs x (2^22 - 1) query rows > 2^31 - 1
    pl = np.zeros(513, np.int32); pr = np.ones(513, np.int32)
    ptr = np.full(514, -7, np.int64)
    assert raw_call(capi, many, one, 1, pl, pr, lo.RATIO_F32, ptr, q, t, d, 1, total) == SFMBA_ERR_INVALID_ARG
    assert b"too many query rows" in capi.lib().sfmba_last_error()
    assert (ptr == -7).all() and q[0] == -5 and t[0] == -5 and d[0] == -5 and total.value == -3   # nothing was written


def test_capacity_protocol(capi):
    rng = np.random.default_rng(31)
    pool = rng.normal(size=(500, 16)).astype(np.float32)
    descs = [np.ascontiguousarray(pool[rng.choice(500, 300, replace=False)] + rng.normal(scale=0.01, size=(300, 16)).astype(np.float32))
             for _ in range(3)]
    full = capi.match_features_l2(descs)
    n = int(full[2][-1])
    assert n > 10
    img_ptr = np.array([0, 300, 600, 900], np.int64)
    flat = np.ascontiguousarray(np.concatenate(descs))
    pl = np.array([0, 0, 1], np.int32); pr = np.array([1, 2, 2], np.int32)
    ptr = np.full(4, -7, np.int64)
    q = np.full(n, -5, np.int32); t = np.full(n, -5, np.int32); d = np.full(n, -5, np.float32)
    total = C.c_int64(0)
    assert raw_call(capi, img_ptr, flat, 16, pl, pr, lo.RATIO_F32, ptr, q, t, d, n - 1, total) == capi.SFMBA_ERR_CAPACITY
    assert total.value == n and np.array_equal(ptr, full[2])
    assert (q == -5).all() and (t == -5).all() and (d == -5).all()
    assert raw_call(capi, img_ptr, flat, 16, pl, pr, lo.RATIO_F32, ptr, q, t, d, total.value, total) == 0
    assert np.array_equal(ptr, full[2]) and np.array_equal(q, full[3]) and np.array_equal(t, full[4])
    assert np.array_equal(d.view(np.uint32), full[5].view(np.uint32))


# ---- the shim on CV_32F descriptors -----------------------------------------------------------------------------------------------
def test_shim_on_float_descriptors_equals_the_c_abi(capi):
    L = C.CDLL(SHIM)
    L.sfmba_shim_match_features_f32.restype = C.c_int64
    L.sfmba_shim_feature_match_matrix_f32.restype = C.c_int64
    rng = np.random.default_rng(41)
    pool = rng.integers(0, 256, (400, 24)).astype(np.float32)
    sizes_in = [200, 150, 0, 1, 180]                          # + an empty image and a one-row image
    descs = [np.ascontiguousarray(pool[rng.choice(400, n, replace=False)] + rng.integers(-2, 3, (n, 24)).astype(np.float32)) for n in sizes_in]
    lp, ip, fp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    cap = 4000
    q, t, im = (np.zeros(cap, np.int32) for _ in range(3))
    d = np.zeros(cap, np.float32)
    # matchFeatures
    two = [descs[0], descs[1]]
    img_ptr = np.array([0, 200, 350], np.int64)
    flat = np.ascontiguousarray(np.concatenate(two))
    n = L.sfmba_shim_match_features_f32(img_ptr.ctypes.data_as(lp), flat.ctypes.data_as(fp), 24, C.c_int64(cap), q.ctypes.data_as(ip),
                                        t.ctypes.data_as(ip), im.ctypes.data_as(ip), d.ctypes.data_as(fp))
    want = gpu_lists(capi.match_features_l2(two, pairs=[(0, 1)]))[0][1]
    assert 0 < n <= cap and list(zip(q[:n].tolist(), t[:n].tolist(), d[:n].view(np.uint32).tolist())) == want
    assert (im[:n] == 0).all()
    # createFeatureMatchMatrix
    n_img = len(descs)
    img_ptr = np.zeros(n_img + 1, np.int64)
    img_ptr[1:] = np.cumsum(sizes_in)
    flat = np.ascontiguousarray(np.concatenate(descs))
    sizes = np.full(n_img * n_img, -1, np.int64)
    n = L.sfmba_shim_feature_match_matrix_f32(n_img, img_ptr.ctypes.data_as(lp), flat.ctypes.data_as(fp), 24, sizes.ctypes.data_as(lp), C.c_int64(cap),
                                              q.ctypes.data_as(ip), t.ctypes.data_as(ip), im.ctypes.data_as(ip), d.ctypes.data_as(fp))
    assert 0 < n <= cap                                       # -1: failure, -2: not n x n
    want = dict(gpu_lists(capi.match_features_l2(descs)))
    assert want == dict(lo.match_features(descs))
    sizes = sizes.reshape(n_img, n_img)
    o = 0
    for l in range(n_img):
        for r in range(n_img):
            k = int(sizes[l, r])
            got = list(zip(q[o:o + k].tolist(), t[o:o + k].tolist(), d[o:o + k].view(np.uint32).tolist()))
            if l < r:
                assert got == want[(l, r)], (l, r)
            else:
                assert k == 0                                 # the diagonal and below stay empty (SfM.cpp:163-210)
            o += k
    assert o == n and (im[:n] == 0).all()
