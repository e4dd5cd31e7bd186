"""Plane-sweep stereo and the consistency filter on the MI355X (-m gpu) against the CPU restatement of their contract
(tests/depth_oracle.py; include/sfmba.h, sfmba_depth_sweep / sfmba_depth_fuse).  Every comparison is EXACT: the bit patterns of depth
and score, plane, the fused points, colours, origins and pt_ptr.  The shapes are those of tests/depth_cases.py -- the smallest at
which the kernel can still go wrong -- and the restatement's answer for each is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import depth_cases as dc
import depth_oracle as do

pytestmark = pytest.mark.gpu
SFMBA_ERR_INVALID_ARG, SFMBA_ERR_CAPACITY = 1, 5


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_job(got, want, what=""):
    depth, score, plane = got
    bad = np.argwhere(depth.view(np.uint32) != want[0].view(np.uint32))
    assert len(bad) == 0, (what, "depth", len(bad), bad[:5].tolist())
    assert same_bits(score, want[1]), (what, "score")
    assert same_bits(plane, want[2]), (what, "plane")


@pytest.mark.parametrize("name", list(dc.CASES))
def test_cases_exact(capi, name):
    c, o = dc.case(name), dc.oracle(name)
    got = capi.depth_sweep(c["images"], c["K"], c["P"], c["jobs"], **c["params"])
    assert len(got) == 1
    assert_job(got[0], (o["depth"], o["score"], o["plane"]), name)
    if name.startswith(("size_1x1", "size_4x4", "size_8x8", "blind", "const_ref")):
        assert not got[0][0].any() and not got[0][1].any() and (got[0][2] == -1).all()
    if name == "tie":                    # min_score lies exactly on the produced cost 1.0: accepted, lowest plane
        part = o["part"]
        assert (got[0][0][part] > 0).all() and (got[0][2][part] == 0).all() and (got[0][1][part] == 1.0).all()


def test_plane_pointer_may_be_null(capi):
    c, o = dc.case("size_17x33_r2_d3"), dc.oracle("size_17x33_r2_d3")
    depth, score, plane = capi.depth_sweep(c["images"], c["K"], c["P"], c["jobs"], want_plane=False, **c["params"])[0]
    assert plane is None and same_bits(depth, o["depth"]) and same_bits(score, o["score"])


def test_batch_equals_single_calls(capi):
    b = dc.batch()
    want = do.sweep(b["images"], b["K"], b["P"], b["jobs"], **b["params"])
    got = capi.depth_sweep(b["images"], b["K"], b["P"], b["jobs"], **b["params"])
    assert len(got) == 5
    for j, job in enumerate(b["jobs"]):
        assert_job(got[j], want[j], "batch job %d" % j)
        single = capi.depth_sweep(b["images"], b["K"], b["P"], [job], **b["params"])[0]
        assert_job(single, got[j], "single job %d" % j)
    assert sum((g[0] > 0).sum() for g in got) > 500


def test_bgr_equals_its_gray_reduction(capi):
    b = dc.batch()
    bgr = dc.bgr_of(b["images"])
    gray = [do.gray(im).astype(np.uint8) for im in bgr]
    assert any((g != im).any() for g, im in zip(gray, b["images"]))
    got = capi.depth_sweep(bgr, b["K"], b["P"], b["jobs"][:3], **b["params"])
    want = do.sweep(gray, b["K"], b["P"], b["jobs"][:3], **b["params"])
    for j in range(3):
        assert_job(got[j], want[j], "bgr job %d" % j)


# ---- fuse -------------------------------------------------------------------------------------------------------------------
CHECKS = [[1, 2], [0], [0]]


@pytest.fixture(scope="module")
def fused():
    return dc.fuse_scene()


def assert_cloud(got, want, what=""):
    assert got["pt_ptr"].tolist() == want["pt_ptr"].tolist(), what
    for f in ("xyz", "bgr", "src_image", "src_pixel"):
        assert same_bits(got[f], want[f]), (what, f)


@pytest.mark.parametrize("min_consistent", [0, 1, 2])
def test_fuse_exact(capi, fused, min_consistent):
    images, K, P, maps = fused
    got = capi.depth_fuse(images, K, P, maps, CHECKS, rel_tol=0.01, min_consistent=min_consistent)
    want = do.fuse(images, K, P, maps, CHECKS, rel_tol=0.01, min_consistent=min_consistent)
    assert_cloud(got, want, min_consistent)
    assert want["pt_ptr"][-1] > 50


def test_fuse_sweep_output_goes_in_as_it_comes(capi, fused):
    images, K, P, _ = fused
    jobs = [(0, [1, 2], dc.Z_NEAR, dc.Z_FAR), (1, [0], dc.Z_NEAR, dc.Z_FAR), (2, [0], dc.Z_NEAR, dc.Z_FAR)]
    maps = [d for d, _, _ in capi.depth_sweep(images, K, P, jobs, n_planes=24, radius=2, min_std=2, min_score=0.6, min_sources=1)]
    assert all(same_bits(a, b) for a, b in zip(maps, fused[3]))
    assert_cloud(capi.depth_fuse(images, K, P, maps, CHECKS), do.fuse(images, K, P, maps, CHECKS))


def test_fuse_check_image_without_a_map_and_zero_tolerance(capi, fused):
    images, K, P, maps = fused
    holes = [maps[0], None, maps[2]]                              # image 1 has no map: it yields no points and agrees with nobody
    for tol, mc in ((0.01, 1), (0.0, 1), (0.0, 0)):
        got = capi.depth_fuse(images, K, P, holes, CHECKS, rel_tol=tol, min_consistent=mc)
        want = do.fuse(images, K, P, holes, CHECKS, rel_tol=tol, min_consistent=mc)
        assert_cloud(got, want, (tol, mc))
        assert got["pt_ptr"][1] == got["pt_ptr"][2]
    zero = [maps[0], np.zeros_like(maps[1]), maps[2]]             # an all-zero map means the same
    assert_cloud(capi.depth_fuse(images, K, P, zero, CHECKS), do.fuse(images, K, P, holes, CHECKS))


def test_fuse_bgr_colours(capi, fused):
    images, K, P, maps = fused
    bgr = dc.bgr_of(images)
    assert_cloud(capi.depth_fuse(bgr, K, P, maps, CHECKS), do.fuse(bgr, K, P, maps, CHECKS))


def raw_fuse(capi, images, K, P, maps, checks, cap, rel_tol=0.01, min_consistent=1, n_images=None, fill=0x5a):
    imgs, channels, img_ptr, flat, wd, ht = capi._flat_images(images)
    K = np.ascontiguousarray(K, np.float32).reshape(9)
    P = np.ascontiguousarray(P, np.float32).reshape(-1)
    fp, lp, bp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_ubyte), C.POINTER(C.c_int32)
    maps = [None if m is None else np.ascontiguousarray(m, np.float32) for m in maps]
    ptrs = (fp * len(imgs))(*[None if m is None else m.ctypes.data_as(fp) for m in maps])
    chk_ptr, chk = capi._csr(checks)
    n = max(cap, 1)
    out = dict(xyz=np.full((n, 3), np.float32(7.5)), bgr=np.full((n, 3), fill, np.uint8), src_image=np.full(n, fill, np.int32),
               src_pixel=np.full(n, fill, np.int32), pt_ptr=np.full(len(imgs) + 1, -1, np.int64))
    total = C.c_int64(-1)
    rc = capi.lib().sfmba_depth_fuse(0, len(imgs) if n_images is None else n_images, img_ptr.ctypes.data_as(lp), flat.ctypes.data_as(bp),
                                     wd.ctypes.data_as(ip), ht.ctypes.data_as(ip), channels, K.ctypes.data_as(fp), P.ctypes.data_as(fp), ptrs,
                                     chk_ptr.ctypes.data_as(lp), chk.ctypes.data_as(ip), C.c_float(rel_tol), min_consistent,
                                     out["pt_ptr"].ctypes.data_as(lp), out["xyz"].ctypes.data_as(fp), out["bgr"].ctypes.data_as(bp),
                                     out["src_image"].ctypes.data_as(ip), out["src_pixel"].ctypes.data_as(ip), C.c_int64(cap), C.byref(total))
    return rc, int(total.value), out


def test_fuse_capacity_protocol(capi, fused):
    images, K, P, maps = fused
    want = do.fuse(images, K, P, maps, CHECKS)
    n = int(want["pt_ptr"][-1])
    rc, total, out = raw_fuse(capi, images, K, P, maps, CHECKS, cap=n - 1)
    assert rc == SFMBA_ERR_CAPACITY and total == n and out["pt_ptr"].tolist() == want["pt_ptr"].tolist()
    assert (out["xyz"] == np.float32(7.5)).all() and (out["bgr"] == 0x5a).all() and (out["src_image"] == 0x5a).all()      # nothing written
    rc, total, out = raw_fuse(capi, images, K, P, maps, CHECKS, cap=total)
    assert rc == 0 and total == n
    assert_cloud({k: v[:n] if k != "pt_ptr" else v for k, v in out.items()}, want)


# ---- argument checks --------------------------------------------------------------------------------------------------------
def test_sweep_refuses_what_the_contract_says(capi):
    c = dc.case("size_17x33_r2_d3")
    im, K, P, prm = c["images"], c["K"], c["P"], c["params"]

    def refused(images=im, K=K, P=P, jobs=c["jobs"], **over):
        with pytest.raises(capi.SfmbaError) as e:
            capi.depth_sweep(images, K, P, jobs, **dict(prm, **over))
        return str(e.value).startswith("sfmba rc=%d:" % SFMBA_ERR_INVALID_ARG)

    for over in (dict(n_planes=1), dict(n_planes=257), dict(radius=0), dict(radius=5), dict(min_std=-1), dict(min_std=128),
                 dict(min_score=1.5), dict(min_score=-1.5), dict(min_score=float("nan")), dict(min_sources=0), dict(min_sources=5)):
        assert refused(**over), over
    for jobs in ([(2, [1], 8.0, 12.0)], [(0, [2], 8.0, 12.0)], [(0, [0], 8.0, 12.0)], [(0, [1, 1], 8.0, 12.0)], [(0, [], 8.0, 12.0)],
                 [(0, [1], 12.0, 8.0)], [(0, [1], 8.0, 8.0)], [(0, [1], 0.0, 8.0)], [(0, [1], -1.0, 8.0)], [(0, [1], 8.0, float("inf"))],
                 [(0, [1], float("nan"), 8.0)]):
        assert refused(jobs=jobs), jobs
    five = [im[0]] * 6
    assert refused(images=five, P=np.repeat(P[:1], 6, axis=0), jobs=[(0, [1, 2, 3, 4, 5], 8.0, 12.0)])
    bad_K = K.copy(); bad_K[0, 0] = 0.0
    assert refused(K=bad_K)
    bad_K = K.copy(); bad_K[1, 2] = np.nan
    assert refused(K=bad_K)
    bad_P = P.copy(); bad_P[1, 2, 3] = np.inf
    assert refused(P=bad_P)
    with pytest.raises(capi.SfmbaError, match="z_near"):                        # the message comes through sfmba_last_error
        capi.depth_sweep(im, K, P, [(0, [1], 12.0, 8.0)], **prm)


def test_fuse_refuses_what_the_contract_says(capi, fused):
    images, K, P, maps = fused
    for kw in (dict(rel_tol=-0.1), dict(rel_tol=float("nan")), dict(rel_tol=float("inf")), dict(min_consistent=-1), dict(min_consistent=5)):
        rc, _, _ = raw_fuse(capi, images, K, P, maps, CHECKS, cap=10, **kw)
        assert rc == SFMBA_ERR_INVALID_ARG, kw
    for checks in ([[0], [0], [0]], [[3], [0], [0]], [[1, 1], [0], [0]], [[-1], [0], [0]]):
        rc, _, _ = raw_fuse(capi, images, K, P, maps, checks, cap=10)
        assert rc == SFMBA_ERR_INVALID_ARG, checks
    bad_K = np.asarray(K).copy(); bad_K[1, 1] = -1.0
    assert raw_fuse(capi, images, bad_K, P, maps, CHECKS, cap=10)[0] == SFMBA_ERR_INVALID_ARG
