"""The feature extractor on the MI355X (-m gpu) against the CPU restatement of its contract (tests/orb_oracle.py, include/sfmba.h
sfmba_orb_extract).  Integer work end to end: every comparison is EXACT -- the same key points in the same order, the same level
coordinates, responses, bins, descriptor bytes and float fields, the same candidate count per level.  Calls go through the C ABI
and through the reference-signature functions of host/SfM2DFeatureUtilities.cpp (extractFeatures, single and batch).  The images
are those of tests/orb_cases.py; the oracle's answer for each is computed once and shared."""
import ctypes as C
import os

import numpy as np
import pytest

import match_oracle as mo
import orb_cases as oc
import orb_oracle as oo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
SFMBA_ERR_INVALID_ARG, SFMBA_ERR_CAPACITY = 1, 5


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


def assert_same(got, want, what=""):
    """got: a debug tuple of capi.orb_extract; want: a dict of orb_oracle.extract."""
    kp, desc, lxy, bn, hr, cand = got
    assert kp.dtype == oo.KP_DTYPE
    assert cand.tolist() == want["candidates"].tolist(), what
    assert len(kp) == len(want["kp"]), what
    assert np.array_equal(lxy, want["level_xy"]), what
    assert np.array_equal(kp["octave"], want["kp"]["octave"]), what
    assert np.array_equal(hr, want["harris"]), what
    assert np.array_equal(bn, want["bin"]), what
    assert np.array_equal(desc, want["desc"]), what
    assert kp.tobytes() == want["kp"].tobytes(), what             # the six fields, bit for bit


def run_case(capi, name):
    got = capi.orb_extract([oc.image(name)], debug=True, **oc.params(name))[0]
    assert_same(got, oc.oracle(name), name)
    return got


def test_header_constants_match_capi(capi):
    assert oc.tile_dims() == (64, 16)
    assert capi.ORB_KEYPOINT == oo.KP_DTYPE and capi.ORB_KEYPOINT.itemsize == 24


@pytest.mark.parametrize("name", [n for n in oc.CASES if n.startswith(("one_pixel", "none_", "width_", "height_", "noise_"))])
def test_sizes_exact(capi, name):
    got = run_case(capi, name)
    if name.startswith("one_pixel"):
        assert got[2].tolist() == [[31, 31]] and got[5][0] == 1
    if name.startswith("none_"):
        assert len(got[0]) == 0 and not got[5].any()


def test_tile_edge_sizes_are_the_published_tile():
    tw, th = oc.tile_dims()
    for d in (-1, 0, 1):
        assert oc.image("width_%d" % (62 + tw + d)).shape == (70, 62 + tw + d)
        assert oc.image("height_%d" % (62 + th + d)).shape == (62 + th + d, 70)


def test_a_level_that_drops_out(capi):
    got = run_case(capi, "level_drops_100x80")
    assert oo.level_sizes(100, 80, 1.2, 8)[:3] == [(100, 80), (83, 67), (69, 56)]
    assert got[5][0] > 0 and got[5][1] > 0 and not got[5][2:].any()
    assert set(got[0]["octave"].tolist()) == {0, 1}


def test_one_level(capi):
    got = run_case(capi, "one_level_131x97")
    assert len(got[0]) == min(500, got[5][0]) and not got[0]["octave"].any()


def test_ties_keep_the_lowest_y_x(capi):
    img, p = oc.image("ties_221x190"), oc.params("ties_221x190")
    full = oo.extract(img, **dict(p, n_features=5000))
    assert len(full["kp"]) > 1500 and len(np.unique(full["harris"])) < 40
    n = p["n_features"]
    R = full["harris"]
    assert R[n - 1] == R[n] and R[0] != R[n]                      # the cut falls inside a group of equal R, not the first one
    got = run_case(capi, "ties_221x190")
    assert len(got[0]) == n
    tied = np.nonzero(R == R[n - 1])[0]
    yx = full["level_xy"][tied][:, ::-1]
    assert np.array_equal(yx, yx[np.lexsort((yx[:, 1], yx[:, 0]))])          # the oracle's group is in (y, x) order ...
    kept = got[2][got[4] == R[n - 1]]
    assert np.array_equal(kept, full["level_xy"][tied][:len(kept)])          # ... and the device kept its head


@pytest.mark.parametrize("name", ["render_320x240", "render_640x480", "render_1024x768", "uniform_100x100"])
def test_renderings_exact(capi, name):
    got = run_case(capi, name)
    if name == "uniform_100x100":
        assert len(got[0]) == 0
    if name == "render_1024x768":
        assert len(got[0]) > 3000


def test_batch_equals_single_calls_and_the_oracle(capi):
    imgs = [oc.image(n) for n in oc.BATCH]
    assert len({im.shape for im in imgs}) == 5
    batch = capi.orb_extract(imgs, debug=True, **oc.P8)
    assert len(batch[2][0]) == 0                                  # the image without key points sits inside the batch
    for name, got in zip(oc.BATCH, batch):
        assert_same(got, oc.oracle(name), name)
        single = capi.orb_extract([oc.image(name)], debug=True, **oc.P8)[0]
        for a, b in zip(got, single):
            assert a.tobytes() == b.tobytes(), name


def test_repeatable(capi):
    imgs = [oc.image(n) for n in oc.BATCH]
    a = capi.orb_extract(imgs, debug=True, **oc.P8)
    b = capi.orb_extract(imgs, debug=True, **oc.P8)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes()


def test_bgr_equals_gray_conversion(capi):
    img = oc.image("bgr_131x97")
    got = run_case(capi, "bgr_131x97")
    g = oo.gray(img)
    assert np.array_equal(g, oo.gray_plain(img))
    gray = capi.orb_extract([g], debug=True, **oc.P8)[0]
    assert len(got[0]) > 0
    for a, b in zip(got, gray):
        assert a.tobytes() == b.tobytes()


def raw_call(capi, imgs, channels=1, n_features=500, scale_factor=1.2, n_levels=8, fast_threshold=20, cap=None, width=None, height=None, img_ptr=None):
    n = len(imgs)
    flat = np.ascontiguousarray(np.concatenate([im.reshape(-1) for im in imgs]))
    wd = np.asarray([im.shape[1] for im in imgs] if width is None else width, np.int32)
    ht = np.asarray([im.shape[0] for im in imgs] if height is None else height, np.int32)
    if img_ptr is None:
        img_ptr = np.concatenate([[0], np.cumsum([im.size for im in imgs])])
    img_ptr = np.asarray(img_ptr, np.int64)
    cap = n * n_features if cap is None else cap
    kp = np.full(max(cap, 1), 0x55, np.uint8).repeat(24).view(oo.KP_DTYPE)
    desc = np.full((max(cap, 1), 32), 0x55, np.uint8)
    kp_ptr = np.full(n + 1, -7, np.int64)
    total = C.c_int64(-7)
    lp, bp, ip = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte), C.POINTER(C.c_int32)
    rc = capi.lib().sfmba_orb_extract(C.c_int(0), C.c_int(n), img_ptr.ctypes.data_as(lp), flat.ctypes.data_as(bp), wd.ctypes.data_as(ip),
                                      ht.ctypes.data_as(ip), C.c_int(channels), C.c_int(n_features), C.c_float(scale_factor), C.c_int(n_levels),
                                      C.c_int(fast_threshold), kp_ptr.ctypes.data_as(lp), kp.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(bp),
                                      C.c_int64(cap), C.byref(total), None, None, None, None)
    return rc, kp_ptr, total.value, kp, desc


def test_capacity_protocol(capi):
    imgs = [oc.image("noise_131x97"), oc.image("level_drops_100x80")]
    want = [oc.oracle("noise_131x97"), oc.oracle("level_drops_100x80")]
    n = sum(len(w["kp"]) for w in want)
    rc, kp_ptr, total, kp, desc = raw_call(capi, imgs, cap=n - 1)
    assert rc == SFMBA_ERR_CAPACITY and total == n
    assert kp_ptr.tolist() == [0, len(want[0]["kp"]), n]
    assert (desc == 0x55).all() and (kp.view(np.uint8) == 0x55).all()           # nothing else is written
    rc, kp_ptr, total, kp, desc = raw_call(capi, imgs, cap=n)
    assert rc == 0 and total == n and kp_ptr.tolist() == [0, len(want[0]["kp"]), n]
    assert np.array_equal(desc[:n], np.concatenate([w["desc"] for w in want]))
    assert kp[:n].tobytes() == np.concatenate([w["kp"] for w in want]).tobytes()
    small = capi.orb_extract(imgs, cap=3, **oc.P8)                              # the binding retries with the reported size
    assert [len(s[0]) for s in small] == [len(w["kp"]) for w in want]


def test_invalid_arguments(capi):
    img = oc.image("noise_131x97")
    ok = raw_call(capi, [img])
    assert ok[0] == 0
    bad = [dict(channels=2), dict(channels=0), dict(channels=4), dict(width=[0], img_ptr=[0, 0]), dict(height=[0], img_ptr=[0, 0]),
           dict(width=[16385], img_ptr=[0, 16385 * 97]), dict(height=[16385], img_ptr=[0, 16385 * 131]), dict(width=[-1]),
           dict(img_ptr=[0, img.size - 1]), dict(img_ptr=[0, img.size + 1]), dict(img_ptr=[1, img.size + 1]), dict(width=[130]),
           dict(n_features=0), dict(n_features=-5), dict(n_levels=0), dict(n_levels=13), dict(scale_factor=1.0), dict(scale_factor=0.5),
           dict(scale_factor=2.0000002), dict(scale_factor=float("nan")), dict(scale_factor=float("inf")), dict(fast_threshold=0),
           dict(fast_threshold=255), dict(fast_threshold=-1)]
    for kw in bad:
        assert raw_call(capi, [img], **kw)[0] == SFMBA_ERR_INVALID_ARG, kw
    assert raw_call(capi, [oc.image("bgr_131x97")], channels=1)[0] == SFMBA_ERR_INVALID_ARG          # three times the bytes of a gray image
    for kw in (dict(scale_factor=2.0), dict(n_levels=12), dict(n_levels=1), dict(fast_threshold=1), dict(fast_threshold=254), dict(n_features=1)):
        assert raw_call(capi, [img], **kw)[0] == 0, kw


def shim_lib():
    assert os.path.exists(SHIM)
    L = C.CDLL(SHIM)
    L.sfmba_shim_extract_features.restype = C.c_int64
    L.sfmba_shim_extract_features_batch.restype = C.c_int64
    return L


def test_shim_single_and_batch_equal_the_c_abi(capi):
    L = shim_lib()
    names = ["noise_131x97", "level_drops_100x80", "none_62x200"]
    imgs = [oc.image(n) for n in names]
    want = capi.orb_extract(imgs)                                 # the reference's parameters are the binding's defaults
    fp, bp, lp, ip = C.POINTER(C.c_float), C.POINTER(C.c_ubyte), C.POINTER(C.c_int64), C.POINTER(C.c_int32)

    def same(kp7, pts, desc, w):
        k = w[0]
        assert np.array_equal(kp7[:, :5], np.stack([k["x"], k["y"], k["size"], k["angle"], k["response"]], axis=1).reshape(-1, 5))
        assert np.array_equal(kp7[:, 5], k["octave"].astype(np.float32)) and (kp7[:, 6] == -1).all()
        assert np.array_equal(pts, kp7[:, :2]) and np.array_equal(desc, w[1])
    cap = 5000
    for im, w in zip(imgs + [oc.image("bgr_131x97")], want + capi.orb_extract([oc.image("bgr_131x97")])):
        kp7, pts, desc = np.zeros((cap, 7), np.float32), np.zeros((cap, 2), np.float32), np.zeros((cap, 32), np.uint8)
        n = L.sfmba_shim_extract_features(C.c_int(im.shape[1]), C.c_int(im.shape[0]), C.c_int(1 if im.ndim == 2 else 3), im.ctypes.data_as(bp),
                                          C.c_int64(cap), kp7.ctypes.data_as(fp), pts.ctypes.data_as(fp), desc.ctypes.data_as(bp))
        assert n == len(w[0])
        same(kp7[:n], pts[:n], desc[:n], w)
    flat = np.ascontiguousarray(np.concatenate([im.reshape(-1) for im in imgs]))
    img_ptr = np.concatenate([[0], np.cumsum([im.size for im in imgs])]).astype(np.int64)
    wd, ht = np.asarray([im.shape[1] for im in imgs], np.int32), np.asarray([im.shape[0] for im in imgs], np.int32)
    kp_ptr = np.zeros(len(imgs) + 1, np.int64)
    cap = 3 * 5000
    kp7, pts, desc = np.zeros((cap, 7), np.float32), np.zeros((cap, 2), np.float32), np.zeros((cap, 32), np.uint8)
    n = L.sfmba_shim_extract_features_batch(C.c_int(len(imgs)), img_ptr.ctypes.data_as(lp), flat.ctypes.data_as(bp), wd.ctypes.data_as(ip),
                                            ht.ctypes.data_as(ip), C.c_int(1), kp_ptr.ctypes.data_as(lp), C.c_int64(cap), kp7.ctypes.data_as(fp),
                                            pts.ctypes.data_as(fp), desc.ctypes.data_as(bp))
    assert n == sum(len(w[0]) for w in want)
    assert kp_ptr.tolist() == np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).tolist()
    for i, w in enumerate(want):
        a, b = kp_ptr[i], kp_ptr[i + 1]
        same(kp7[a:b], pts[a:b], desc[a:b], w)


def test_chain_extract_match_homography(capi):
    """orb_extract -> match_features -> homography_ransac on the identity / 17 degree pair at 640 x 480."""
    from sfm_toy_library_amd import synthetic as sy
    names = ["render_640x480", "render_640x480_rot17"]
    feats = capi.orb_extract([oc.image(n) for n in names], **oc.params(names[0]))
    wants = [oc.oracle(n) for n in names]
    for f, w in zip(feats, wants):
        assert np.array_equal(f[1], w["desc"]) and f[0].tobytes() == w["kp"].tobytes()
    res = capi.match_features([f[1] for f in feats])
    want = mo.match_pair(wants[0]["desc"], wants[1]["desc"], knn=mo.knn_keys)
    got = list(zip(res[3].tolist(), res[4].tolist(), res[5].tolist()))
    assert got == want and len(got) >= 100
    pts = [np.stack([f[0]["x"], f[0]["y"]], axis=1) for f in feats]
    hom = capi.homography_ransac(pts, None, res)[0]
    assert hom["status"] == 0 and hom["n_inliers"] >= 50
    W, H = 640, 480
    c = np.array([0.5 * W, 0.5 * H])
    true = sy.orb_scene_to_view(sy.orb_view_to_scene(c, W, H, *oc.VIEWS["identity"]), W, H, *oc.VIEWS["rot17"])
    q = hom["H"] @ np.array([c[0], c[1], 1.0])
    assert np.hypot(*(q[:2] / q[2] - true)) <= 3.0
