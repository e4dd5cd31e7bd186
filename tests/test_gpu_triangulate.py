"""HIP triangulation (sfmba_triangulate, csrc/triangulate.hip) vs the oracle restatement of
SfMStereoUtilities::triangulateViews and vs the reference's own known-answer test (-m gpu)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_kat.json")


@pytest.fixture(scope="module")
def capi():
    import sfm_toy_library_amd  # noqa: F401
    from sfm_toy_library_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def tri():
    from oracle import triangulate_oracle
    return triangulate_oracle


def test_reference_kat_on_gpu(capi):
    """triangulate_from_2_views (SfMUnitTests.cpp:221-251): every point within 0.01 of its canned 3D point."""
    g = json.load(open(GOLD))
    X, keep, err = capi.triangulate(g["K"], g["P_left"], g["P_right"], g["left"], g["right"])
    assert keep.all()
    assert np.linalg.norm(X.astype(np.float64) - np.array(g["points3d"], dtype=np.float64), axis=1).max() < g["tolerance"]
    assert err.max() < 1e-2


def _random_scene(n, seed, outlier_frac=0.1):
    rng = np.random.default_rng(seed)
    import sfm_toy_library_amd as sfm
    K = np.array([[2500.0, 0, 512.0], [0, 2500.0, 384.0], [0, 0, 1]], dtype=np.float32)
    Rl = np.eye(3)
    Rr = sfm.synthetic.rotvec_to_matrix(np.array([[0.02, -0.15, 0.01]]))[0]
    Pl = np.concatenate([Rl, np.zeros((3, 1))], axis=1).astype(np.float32)
    Pr = np.concatenate([Rr, np.array([[-1.0], [0.02], [0.1]])], axis=1).astype(np.float32)
    X = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.8, 0.8, n), rng.uniform(4, 8, n)], axis=1)

    def proj(P):
        p = X @ P[:, :3].astype(np.float64).T + P[:, 3].astype(np.float64)
        return (np.stack([K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]], axis=1)
                + rng.normal(0, 0.5, (n, 2))).astype(np.float32)
    l, r = proj(Pl), proj(Pr)
    bad = rng.random(n) < outlier_frac
    r[bad] += rng.normal(0, 40.0, (int(bad.sum()), 2)).astype(np.float32)      # mismatches
    return K, Pl, Pr, l, r, X


@pytest.mark.parametrize("n,seed", [(1, 1), (63, 2), (5000, 3), (200000, 4)])
def test_matches_oracle(capi, tri, n, seed):
    K, Pl, Pr, l, r, _ = _random_scene(n, seed)
    X_o, keep_o, el_o, er_o = tri.triangulate_views(K, Pl, Pr, l, r)
    X, keep, err = capi.triangulate(K, Pl, Pr, l, r)
    # same points (float containers: a few ulp of the coordinates, which are O(1..10))
    assert np.allclose(X, X_o, rtol=2e-5, atol=2e-5)
    assert np.allclose(err[:, 0], el_o, rtol=1e-3, atol=2e-3) and np.allclose(err[:, 1], er_o, rtol=1e-3, atol=2e-3)
    # same keep decisions except where an error sits within float round-off of the 10 px threshold
    border = (np.abs(el_o - 10.0) < 5e-3) | (np.abs(er_o - 10.0) < 5e-3)
    assert np.array_equal(keep[~border], keep_o[~border])
    if n >= 5000:
        assert 0.02 * n < (~keep).sum() < 0.2 * n      # the planted mismatches are rejected, the inliers kept


def test_empty_and_bad_arguments(capi):
    K = np.eye(3, dtype=np.float32); P = np.zeros((3, 4), dtype=np.float32)
    X, keep, err = capi.triangulate(K, P, P, np.zeros((0, 2)), np.zeros((0, 2)))
    assert X.shape == (0, 3) and keep.shape == (0,)


def test_shim_with_the_reference_signature(tri):
    """sfmtoylib::SfMStereoUtilities::triangulateViews(Intrinsics, ImagePair, Matching, Features, Features, Matx34f, Matx34f,
    PointCloud&) through the flat-array harness: unaligned matches (queryIdx / trainIdx), back references, filter."""
    import ctypes as C
    shim = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    lib = C.CDLL(shim)
    K, Pl, Pr, l, r, _ = _random_scene(3000, 9)
    rng = np.random.default_rng(5)
    perm_l, perm_r = rng.permutation(len(l)), rng.permutation(len(r))
    feats_l, feats_r = l[perm_l], r[perm_r]                      # features in arbitrary order ...
    q = np.argsort(perm_l).astype(np.int32); t = np.argsort(perm_r).astype(np.int32)   # ... match i = (q[i], t[i])
    sel = rng.permutation(len(l))[:2500]                          # not every feature is matched
    q, t = np.ascontiguousarray(q[sel]), np.ascontiguousarray(t[sel])
    X_o, keep_o, el_o, er_o = tri.triangulate_views(K, Pl, Pr, feats_l[q], feats_r[t])
    cap = len(q)
    X = np.zeros((cap, 3), np.float32); lr = np.zeros(cap, np.int32); rr = np.zeros(cap, np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    Kf, Plf, Prf = [np.ascontiguousarray(a, np.float32) for a in (K, Pl, Pr)]
    fl, fr = np.ascontiguousarray(feats_l, np.float32), np.ascontiguousarray(feats_r, np.float32)
    n = lib.sfmba_shim_triangulate_views(Kf.ctypes.data_as(fp), C.c_int(0), C.c_int(1), C.c_int(len(fl)), fl.ctypes.data_as(fp),
                                         C.c_int(len(fr)), fr.ctypes.data_as(fp), C.c_int(len(q)), q.ctypes.data_as(ip), t.ctypes.data_as(ip),
                                         Plf.ctypes.data_as(fp), Prf.ctypes.data_as(fp), C.c_int(cap), X.ctypes.data_as(fp),
                                         lr.ctypes.data_as(ip), rr.ctypes.data_as(ip))
    border = (np.abs(el_o - 10.0) < 5e-3) | (np.abs(er_o - 10.0) < 5e-3)
    assert not border.any()                                       # seed chosen so that no error sits on the threshold
    assert n == int(keep_o.sum())
    assert np.array_equal(lr[:n], q[keep_o]) and np.array_equal(rr[:n], t[keep_o])     # back references, match order
    assert np.allclose(X[:n], X_o[keep_o], rtol=2e-5, atol=2e-5)


# ---- the geometries of tests/triangulate_cases.py -----------------------------------------------------------------------
# Bounds (set by the issue that added these tests, none taken from the device's output; tests/test_triangulate_cases_cpu.py
# re-measures what they rest on without a GPU):
#   4 ulps    per coordinate between points3d and the long-double reference on CONDITIONED matches (the float-rounded h_i and w
#             may each flip one rounding, and an ulp spans a factor of 2 in relative size); the two CPU references are 0 ulps
#             apart, 2 on `far`
#   4 ulps    of the largest pixel coordinate involved, observed or projected, between reproj_err and the errors recomputed in
#             fp64 from the device's OWN points3d; the same band around the threshold is where keep may go either way
#   1 %       of a case's matches may be unconditioned, and 1 % may sit inside the band
import triangulate_cases as tc  # noqa: E402

ULP_BOUND = 4.0


@pytest.fixture(scope="module")
def cases():
    """name -> (case, the long-double reference at 10 px): computed once, never modified."""
    out = {}
    for name in tc.CASES:
        c = tc.make_case(name)
        out[name] = (c, tc.reference(c["K"], c["P_left"], c["P_right"], c["left"], c["right"], 10.0))
    return out


def run_case(capi, c, thr=10.0, **kw):
    return capi.triangulate(c["K"], c["P_left"], c["P_right"], c["left"], c["right"], max_reproj_px=thr, **kw)


def same_or_both_non_finite(got, want, tol):
    """|got - want| <= tol, or both NaN, or both the same infinity."""
    with np.errstate(invalid="ignore"):
        return (np.abs(got - want) <= tol) | (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & (got == want))


@pytest.mark.parametrize("thr", [10.0, 1.0])
@pytest.mark.parametrize("name", tc.CASES)
def test_case_against_long_double_reference(capi, cases, name, thr):
    c, ref = cases[name]
    X, keep, err = run_case(capi, c, thr)
    # points
    cond = tc.conditioned(ref)
    left_out = 1.0 - cond.mean()
    ulps = tc.ulp_distance(X, ref["points3d"])
    worst_ulp = ulps[cond].max()
    # errors, from the device's own points
    e, tol, band, keep_want = tc.error_check(c["K"], c["P_left"], c["P_right"], c["left"], c["right"], X, thr)
    err64 = err.astype(np.float64)
    fin = np.isfinite(e) & np.isfinite(err64)
    worst_gap = (np.abs(err64 - e)[fin] / tol[fin]).max() if fin.any() else 0.0
    ref_keep = ~((ref["err_left"] > thr) | (ref["err_right"] > thr))
    print("front_end_edges triangulate %-18s thr %4.1f  left out %.4f  worst %.2f ulps  worst error gap %.3f of its band  band matches %d  kept %d (reference %d)"
          % (name, thr, left_out, worst_ulp, worst_gap, int(band.sum()), int(keep.sum()), int(ref_keep.sum())))
    assert left_out <= tc.MAX_LEFT_OUT
    assert worst_ulp <= ULP_BOUND, (name, worst_ulp, int(np.argmax(np.where(cond[:, None], ulps, 0).max(axis=1))))
    assert np.all(same_or_both_non_finite(err64, e, tol)), (name, worst_gap)
    # keep
    assert band.mean() <= 0.01
    assert np.array_equal(keep[~band], keep_want[~band])
    assert abs(int(keep.sum()) - int(ref_keep.sum())) <= int(band.sum())
    if name == "pure_rotation":                                   # the common centre itself: 0 / 1, NaN errors, every match kept
        assert not X.any() and np.all(np.isnan(err)) and keep.all()
    else:
        assert keep.any() and not keep.all()
    if name == "behind":                                          # no depth test: the matches behind the right camera are kept
        depth_right = X.astype(np.float64) @ c["P_right"][2, :3].astype(np.float64) + float(c["P_right"][2, 3])
        assert np.all(depth_right[keep & cond] < 0) and keep.sum() > 0.8 * tc.N


@pytest.mark.parametrize("name", ["general"])
def test_without_the_error_output(capi, cases, name):
    c, _ = cases[name]
    X, keep, err = run_case(capi, c)
    X0, keep0, err0 = run_case(capi, c, reproj_err=False)
    assert err0 is None and err is not None
    assert X0.tobytes() == X.tobytes() and keep0.tobytes() == keep.tobytes()


NAN_AT, INF_AT = 7, tc.N - 1          # a lane of the first block, the last lane of the partial block


@pytest.fixture(scope="module")
def non_finite(capi, cases):
    """base1 as it is, and with the left pixel of one match NaN and the right pixel of another +inf."""
    c, _ = cases["base1"]
    d = dict(c, left=c["left"].copy(), right=c["right"].copy())
    d["left"][NAN_AT] = np.nan
    d["right"][INF_AT] = np.inf
    return run_case(capi, c), run_case(capi, d)


def test_non_finite_pixels_leave_every_other_match_alone(non_finite):
    (X, keep, err), (Xn, keepn, errn) = non_finite
    rest = np.ones(tc.N, bool)
    rest[[NAN_AT, INF_AT]] = False
    assert Xn[rest].tobytes() == X[rest].tobytes() and keepn[rest].tobytes() == keep[rest].tobytes() and errn[rest].tobytes() == err[rest].tobytes()


def test_nan_pixel_gives_a_non_finite_point_that_is_kept(non_finite):
    """The reference drops a match on norm(...) > 10 (SfMStereoUtilities.cpp:186); a NaN error compares False: kept."""
    _, (Xn, keepn, errn) = non_finite
    assert not np.isfinite(Xn[NAN_AT]).any() and keepn[NAN_AT]
    assert np.all(np.isnan(errn[NAN_AT]))


def test_inf_pixel_gives_a_non_finite_point_that_is_kept(non_finite):
    """undistortPoints takes the normalised point through a homogeneous product with R = I, where an infinite coordinate meets
    0 * inf: both normalised coordinates are NaN, then the point and both errors, and the filter keeps a NaN error.  (Before
    normalise_px of triangulate.hip did the same, the device gave the finite point (1, 0, 0), errors (NaN, +inf), keep 0: the
    rotation skip of the Jacobi read inf <= inf and left V the identity.)"""
    _, (Xn, keepn, errn) = non_finite
    print("front_end_edges triangulate +inf right pixel: point", Xn[INF_AT], "errors", errn[INF_AT], "keep", bool(keepn[INF_AT]))
    assert not np.isfinite(Xn[INF_AT]).any() and keepn[INF_AT]
    assert np.all(np.isnan(errn[INF_AT]))


def test_non_finite_pixels_are_judged_by_the_comparison_on_their_own_errors(non_finite):
    """keep = neither error > max_reproj_px, on the two planted matches too: NaN errors are kept."""
    _, (Xn, keepn, errn) = non_finite
    for i in (NAN_AT, INF_AT):
        assert not np.all(np.isfinite(errn[i]))
        with np.errstate(invalid="ignore"):
            assert bool(keepn[i]) == (not (errn[i] > 10.0).any()), (i, errn[i], keepn[i])


def test_shim_on_the_general_case(cases):
    """The shim once more, on a pair of which neither camera is [I|0]; back references and kept count from the long-double reference."""
    import ctypes as C
    shim = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    lib = C.CDLL(shim)
    c, _ = cases["general"]
    K, Pl, Pr, l, r = c["K"], c["P_left"], c["P_right"], c["left"], c["right"]
    rng = np.random.default_rng(5)
    perm_l, perm_r = rng.permutation(len(l)), rng.permutation(len(r))
    feats_l, feats_r = l[perm_l], r[perm_r]
    q = np.argsort(perm_l).astype(np.int32); t = np.argsort(perm_r).astype(np.int32)
    sel = rng.permutation(len(l))[:3500]                          # not every feature is matched, and not in feature order
    q, t = np.ascontiguousarray(q[sel]), np.ascontiguousarray(t[sel])
    ref = tc.reference(K, Pl, Pr, feats_l[q], feats_r[t])
    cond, keep_r = tc.conditioned(ref), ref["keep"]
    _, _, band, _ = tc.error_check(K, Pl, Pr, feats_l[q], feats_r[t], ref["points3d"], 10.0)
    assert not band.any() and cond.all()                          # no error on the threshold: the kept set is the reference's
    cap = len(q)
    X = np.zeros((cap, 3), np.float32); lr = np.zeros(cap, np.int32); rr = np.zeros(cap, np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    Kf, Plf, Prf = [np.ascontiguousarray(a, np.float32) for a in (K, Pl, Pr)]
    fl, fr = np.ascontiguousarray(feats_l, np.float32), np.ascontiguousarray(feats_r, np.float32)
    n = lib.sfmba_shim_triangulate_views(Kf.ctypes.data_as(fp), C.c_int(0), C.c_int(1), C.c_int(len(fl)), fl.ctypes.data_as(fp),
                                         C.c_int(len(fr)), fr.ctypes.data_as(fp), C.c_int(len(q)), q.ctypes.data_as(ip), t.ctypes.data_as(ip),
                                         Plf.ctypes.data_as(fp), Prf.ctypes.data_as(fp), C.c_int(cap), X.ctypes.data_as(fp),
                                         lr.ctypes.data_as(ip), rr.ctypes.data_as(ip))
    assert n == int(keep_r.sum()) and 0.8 * cap < n < cap
    assert np.array_equal(lr[:n], q[keep_r]) and np.array_equal(rr[:n], t[keep_r])     # back references, match order
    assert tc.ulp_distance(X[:n], ref["points3d"][keep_r]).max() <= ULP_BOUND
