"""sfmba_triangulate_pairs on the MI355X (-m gpu): the match lists of many pairs in one call, held byte for byte to sfmba_triangulate on
every pair's aligned points, and SfMStereoUtilities::triangulateViewsBatch held to per-pair triangulateViews.

Geometry and pixels come from tests/triangulate_cases.py: pair p of a batch is the first n_p matches of one of its named cases (its
own P_left / P_right), the key points of its two images shuffled and a few left unmatched.  The launch does not cap its grid (one lane
per entry, at most 2^31 - 257 entries per call, more is refused), so there is no list-past-the-cap case."""
import ctypes as C
import os

import numpy as np
import pytest

import sfm_scene
import triangulate_cases as tc

pytestmark = pytest.mark.gpu
SHIM = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sfm-toy-library_amd", "host", "libsfmba_shim.so")
ULP_BOUND = 4.0                       # tests/test_gpu_triangulate.py
EXTRA = 5                             # unmatched key points per image
SIZES = (("base1", 0), ("base1e-2", 1), ("forward", 255), ("rot90", 256), ("general", 257), ("rot180", 64 + 1), ("behind", 0))


@pytest.fixture(scope="module")
def capi():
    import sfm_toy_library_amd  # noqa: F401
    from sfm_toy_library_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def cases():
    return {name: tc.make_case(name) for name in tc.CASES if name != "big_image"}      # one K per call: the cases of K_DEFAULT


def make_batch(cases, specs, seed=0, own_images=True):
    """specs: (case name, n) per pair.  dict(pts, pairs, matches=(ptr, q, t), K, Pl [p,3,4], Pr, aligned = (left, right) per pair)."""
    rng = np.random.default_rng(seed)
    pts, pairs, q, t, ptr, Pl, Pr, aligned = [], [], [], [], [0], [], [], []
    for name, n in specs:
        c = cases[name]
        l, r = c["left"][:n], c["right"][:n]
        extra_l = rng.uniform(0, 700, (EXTRA, 2)).astype(np.float32)
        extra_r = rng.uniform(0, 700, (EXTRA, 2)).astype(np.float32)
        perm_l, perm_r = rng.permutation(n + EXTRA), rng.permutation(n + EXTRA)
        img_l, img_r = np.concatenate([l, extra_l])[perm_l], np.concatenate([r, extra_r])[perm_r]
        order = rng.permutation(n)                                 # the matches in an order of their own
        qi, ti = np.argsort(perm_l)[:n][order], np.argsort(perm_r)[:n][order]
        pairs.append((len(pts), len(pts) + 1))
        pts += [img_l, img_r]
        q.append(qi); t.append(ti); ptr.append(ptr[-1] + n)
        Pl.append(c["P_left"]); Pr.append(c["P_right"])
        aligned.append((img_l[qi], img_r[ti]))
    K = cases[specs[0][0]]["K"]
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)
    return dict(pts=pts, pairs=pairs, matches=(np.asarray(ptr, np.int64), cat(q), cat(t)), K=K, Pl=np.array(Pl, np.float32),
                Pr=np.array(Pr, np.float32), aligned=aligned)


def run(capi, b, **kw):
    return capi.triangulate_pairs(b["pts"], b["pairs"], b["matches"], b["K"], b["Pl"], b["Pr"], **kw)


def singles(capi, b, **kw):
    """capi.triangulate on every pair's aligned points with that pair's cameras."""
    return [capi.triangulate(b["K"], b["Pl"][p], b["Pr"][p], l, r, **kw) for p, (l, r) in enumerate(b["aligned"])]


def check_kept_lists(res):
    ptr = res["pair_ptr"]
    kept = np.flatnonzero(res["keep"])
    assert np.array_equal(res["kept_idx"], kept)
    assert np.array_equal(res["kept_ptr"], np.searchsorted(kept, ptr))          # the list cut at pair_ptr
    for p in range(len(ptr) - 1):
        want = ptr[p] + np.flatnonzero(res["keep"][ptr[p]:ptr[p + 1]])
        assert np.array_equal(res["kept_idx"][res["kept_ptr"][p]:res["kept_ptr"][p + 1]], want)


def same_as_singles(res, want, with_err=True):
    ptr = res["pair_ptr"]
    for p, (X, keep, err) in enumerate(want):
        a, b = int(ptr[p]), int(ptr[p + 1])
        assert res["points3d"][a:b].tobytes() == X.tobytes(), p
        assert np.array_equal(res["keep"][a:b], keep), p
        if with_err:
            assert res["err"][a:b].tobytes() == err.tobytes(), p


@pytest.fixture(scope="module")
def sized(capi, cases):
    """The batch of every boundary size, its result and the single calls: computed once, never modified."""
    b = make_batch(cases, SIZES, seed=11)
    return b, run(capi, b), singles(capi, b)


def test_every_list_size_in_one_call_equals_the_single_calls(sized):
    b, res, want = sized
    assert [int(n) for n in np.diff(b["matches"][0])] == [0, 1, 255, 256, 257, 65, 0]
    same_as_singles(res, want)
    assert res["keep"].any() and not res["keep"].all()


def test_kept_lists_are_the_kept_entries_cut_at_pair_ptr(sized):
    _, res, _ = sized
    check_kept_lists(res)
    assert res["kept_ptr"][0] == 0 and res["kept_ptr"][1] == 0 and res["kept_ptr"][-1] == res["kept_ptr"][-2] == res["keep"].sum()


def test_entries_in_front_of_the_first_pair_are_not_kept(capi, sized):
    b, res, _ = sized
    ptr, q, t = b["matches"]
    front = 3
    m = (ptr + front, np.concatenate([np.full(front, -7, np.int32), q]), np.concatenate([np.full(front, 10 ** 6, np.int32), t]))
    got = capi.triangulate_pairs(b["pts"], b["pairs"], m, b["K"], b["Pl"], b["Pr"])
    assert not got["keep"][:front].any() and not got["points3d"][:front].any() and not got["err"][:front].any()
    assert got["points3d"][front:].tobytes() == res["points3d"].tobytes() and got["err"][front:].tobytes() == res["err"].tobytes()
    assert np.array_equal(got["keep"][front:], res["keep"])
    assert np.array_equal(got["kept_idx"], res["kept_idx"] + front) and np.array_equal(got["kept_ptr"], res["kept_ptr"])


@pytest.mark.parametrize("thr", [10.0, 1.0])
def test_general_case_as_a_pair_of_a_batch_against_long_double_reference(capi, cases, thr):
    """The conditions of test_gpu_triangulate.py::test_case_against_long_double_reference, on pair 1 of 3."""
    b = make_batch(cases, (("base1", 300), ("general", tc.N), ("forward", 257)), seed=12)
    res = run(capi, b, max_reproj_px=thr)
    a, e_ = int(res["pair_ptr"][1]), int(res["pair_ptr"][2])
    X, keep, err = res["points3d"][a:e_], res["keep"][a:e_], res["err"][a:e_]
    l, r = b["aligned"][1]
    c = cases["general"]
    ref = tc.reference(c["K"], c["P_left"], c["P_right"], l, r, thr)
    cond = tc.conditioned(ref)
    ulps = tc.ulp_distance(X, ref["points3d"])
    e, tol, band, keep_want = tc.error_check(c["K"], c["P_left"], c["P_right"], l, r, X, thr)
    err64 = err.astype(np.float64)
    ref_keep = ~((ref["err_left"] > thr) | (ref["err_right"] > thr))
    print("triangulate_pairs general thr %4.1f  left out %.4f  worst %.2f ulps  band matches %d  kept %d (reference %d)"
          % (thr, 1.0 - cond.mean(), ulps[cond].max(), int(band.sum()), int(keep.sum()), int(ref_keep.sum())))
    assert 1.0 - cond.mean() <= tc.MAX_LEFT_OUT
    assert ulps[cond].max() <= ULP_BOUND
    with np.errstate(invalid="ignore"):
        assert np.all((np.abs(err64 - e) <= tol) | (np.isnan(err64) & np.isnan(e)) | (np.isinf(err64) & (err64 == e)))
    assert band.mean() <= 0.01
    assert np.array_equal(keep[~band], keep_want[~band])
    assert abs(int(keep.sum()) - int(ref_keep.sum())) <= int(band.sum())
    assert keep.any() and not keep.all()
    check_kept_lists(res)


@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
def test_mask(capi, sized, kind):
    b, res, _ = sized
    total = int(b["matches"][0][-1])
    mask = {"random": np.random.default_rng(5).integers(0, 2, total), "zeros": np.zeros(total, int), "ones": np.ones(total, int)}[kind].astype(np.uint8)
    if kind == "random":
        mask[mask > 0] = np.random.default_rng(6).integers(1, 256, int((mask > 0).sum()))       # any non-zero byte is "in"
    got = run(capi, b, mask=mask)
    off, on = mask == 0, mask != 0
    assert not got["keep"][off].any() and not got["points3d"][off].any() and not got["err"][off].any()
    assert got["points3d"][on].tobytes() == res["points3d"][on].tobytes() and got["err"][on].tobytes() == res["err"][on].tobytes()
    assert np.array_equal(got["keep"][on], res["keep"][on])
    check_kept_lists(got)
    assert not np.isin(got["kept_idx"], np.flatnonzero(off)).any()
    if kind == "zeros":
        assert len(got["kept_idx"]) == 0 and not got["kept_ptr"].any()
    if kind == "ones":
        assert np.array_equal(got["kept_idx"], res["kept_idx"])


def test_non_finite_pixels_touch_their_own_entry_only(capi, cases, sized):
    b, res, _ = sized
    ptr, q, t = b["matches"]
    p = 4                                                          # the pair of 257: a NaN left pixel and an infinite right pixel
    e_nan, e_inf = int(ptr[p]) + 7, int(ptr[p + 1]) - 1
    pts = [x.copy() for x in b["pts"]]
    pts[b["pairs"][p][0]][q[e_nan]] = np.nan
    pts[b["pairs"][p][1]][t[e_inf], 0] = np.inf
    got = capi.triangulate_pairs(pts, b["pairs"], b["matches"], b["K"], b["Pl"], b["Pr"])
    for e in (e_nan, e_inf):
        assert not np.isfinite(got["points3d"][e]).any() and got["keep"][e] and np.all(np.isnan(got["err"][e]))
    rest = np.ones(int(ptr[-1]), bool)
    rest[[e_nan, e_inf]] = False
    assert got["points3d"][rest].tobytes() == res["points3d"][rest].tobytes() and got["err"][rest].tobytes() == res["err"][rest].tobytes()
    assert np.array_equal(got["keep"][rest], res["keep"][rest])
    check_kept_lists(got)
    assert e_nan in got["kept_idx"] and e_inf in got["kept_idx"]


def test_an_image_against_itself_and_repeated_indices(capi, cases):
    c = cases["base1"]
    img = c["left"][:300]
    rng = np.random.default_rng(3)
    q, t = rng.integers(0, 300, 500).astype(np.int32), rng.integers(0, 300, 500).astype(np.int32)      # repeated, left == right
    q[:50] = t[:50]                                                # a point against itself: on the baseline's null space or not, no fault
    got = capi.triangulate_pairs([img], [(0, 0)], ([0, 500], q, t), c["K"], c["P_left"][None], c["P_right"][None])
    X, keep, err = capi.triangulate(c["K"], c["P_left"], c["P_right"], img[q], img[t])
    assert got["points3d"].tobytes() == X.tobytes() and got["err"].tobytes() == err.tobytes() and np.array_equal(got["keep"], keep)
    check_kept_lists(got)


def test_two_calls_give_the_same_bytes_and_the_error_output_is_optional(capi, sized):
    b, res, _ = sized
    again = run(capi, b)
    for k in ("points3d", "keep", "err", "kept_ptr", "kept_idx"):
        assert again[k].tobytes() == res[k].tobytes(), k
    bare = run(capi, b, reproj_err=False)
    assert bare["err"] is None
    for k in ("points3d", "keep", "kept_ptr", "kept_idx"):
        assert bare[k].tobytes() == res[k].tobytes(), k


def test_one_pair_equals_the_single_call_and_nothing_is_nothing(capi, cases):
    b = make_batch(cases, (("general", 1000),), seed=13)
    res = run(capi, b)
    same_as_singles(res, singles(capi, b))
    check_kept_lists(res)
    for specs in ((), (("base1", 0),), (("base1", 0), ("forward", 0))):                            # n_pairs = 0; total = 0
        if specs:
            e = make_batch(cases, specs, seed=14)
            got = run(capi, e)
        else:
            got = capi.triangulate_pairs([], [], ([0], [], []), cases["base1"]["K"], np.zeros((0, 3, 4)), np.zeros((0, 3, 4)))
        assert got["points3d"].shape == (0, 3) and got["keep"].shape == (0,) and len(got["kept_idx"]) == 0 and not got["kept_ptr"].any()


# ---- refusals: SFMBA_ERR_INVALID_ARG and nothing written -------------------------------------------------------------------
def raw_call(capi, b, ptr=None, q=None, t=None, pairs=None, thr=10.0, mask=None):
    """The C entry point itself, every output filled with a sentinel first: (rc, the outputs as bytes)."""
    ps = [np.ascontiguousarray(x, np.float32) for x in b["pts"]]
    img_ptr = np.zeros(len(ps) + 1, np.int64)
    img_ptr[1:] = np.cumsum([len(x) for x in ps])
    pts = np.ascontiguousarray(np.concatenate(ps))
    ptr0, q0, t0 = b["matches"]
    ptr = np.ascontiguousarray(ptr0 if ptr is None else ptr, np.int64)
    q = np.ascontiguousarray(q0 if q is None else q, np.int32)
    t = np.ascontiguousarray(t0 if t is None else t, np.int32)
    pairs = np.asarray(b["pairs"] if pairs is None else pairs, np.int32)
    pl, pr = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    n_pairs, total = len(pl), len(q)
    K, Pl, Pr = (np.ascontiguousarray(a, np.float32) for a in (b["K"], b["Pl"], b["Pr"]))
    outs = [np.full((total, 3), 7.0, np.float32), np.full(total, 9, np.uint8), np.full((total, 2), 5.0, np.float32),
            np.full(n_pairs + 1, -3, np.int64), np.full(total, -4, np.int64)]
    before = [o.tobytes() for o in outs]
    lp, ip, fp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    rc = capi.lib().sfmba_triangulate_pairs(
        C.c_int(0), C.c_int(len(ps)), img_ptr.ctypes.data_as(lp), pts.ctypes.data_as(fp), K.ctypes.data_as(fp), C.c_int(n_pairs),
        pl.ctypes.data_as(ip), pr.ctypes.data_as(ip), ptr.ctypes.data_as(lp), q.ctypes.data_as(ip), t.ctypes.data_as(ip),
        None if mask is None else mask.ctypes.data_as(bp), Pl.ctypes.data_as(fp), Pr.ctypes.data_as(fp), C.c_float(thr), outs[0].ctypes.data_as(fp),
        outs[1].ctypes.data_as(bp), outs[2].ctypes.data_as(fp), outs[3].ctypes.data_as(lp), outs[4].ctypes.data_as(lp))
    return rc, before == [o.tobytes() for o in outs]


def test_refused_arguments_leave_the_outputs_alone(capi, sized):
    b, _, _ = sized
    ptr, q, t = b["matches"]
    INVALID = 1                                                    # SFMBA_ERR_INVALID_ARG
    assert raw_call(capi, b)[0] == 0                               # the harness itself: the untouched call goes through
    last = len(q) - 1
    bad = {}
    for name, (arr, where, val) in {"query past its image": (q, last, 65 + EXTRA), "query negative": (q, 1, -1),
                                    "train past its image": (t, 300, 256 + EXTRA), "train negative": (t, last, -1)}.items():
        a = arr.copy()
        a[where] = val
        bad[name] = dict(q=a) if arr is q else dict(t=a)
    dec = ptr.copy(); dec[3] = dec[2] - 1
    bad["pair_ptr decreasing"] = dict(ptr=dec)
    neg = ptr.copy(); neg[0] = -1
    bad["pair_ptr negative"] = dict(ptr=neg)
    for name, val in (("pair index past the images", len(b["pts"])), ("pair index negative", -1)):
        pairs = np.array(b["pairs"], np.int32)
        pairs[2, 1] = val
        bad[name] = dict(pairs=pairs)
    for name, thr in (("NaN threshold", np.nan), ("negative threshold", -1.0), ("infinite threshold", np.inf)):
        bad[name] = dict(thr=thr)
    for name, kw in bad.items():
        rc, untouched = raw_call(capi, b, **kw)
        assert rc == INVALID, (name, rc)
        assert untouched, name
        assert capi.lib().sfmba_last_error()
    assert raw_call(capi, b, thr=0.0)[0] == 0                       # zero is a threshold: everything with an error is dropped


# ---- the chain from the matcher ------------------------------------------------------------------------------------------
def test_match_features_essential_ransac_triangulate_pairs(capi):
    sc = sfm_scene.make_box(seed=0, n_views=2)
    pts = [v["xy"] for v in sc["views"]]
    m = capi.match_features([v["desc"] for v in sc["views"]])
    ess = capi.essential_ransac(pts, None, m, sc["K"])
    assert len(ess) == 1 and ess[0]["status"] == 0 and ess[0]["inlier"].sum() >= 100
    Pl = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]
    Pr = ess[0]["pose"][None]
    res = capi.triangulate_pairs(pts, None, m, sc["K"], Pl, Pr, mask=ess[0]["inlier"])
    check_kept_lists(res)
    kept = res["kept_idx"]
    assert ess[0]["inlier"][kept].all() and len(kept) >= 0.9 * ess[0]["inlier"].sum()
    X = res["points3d"][kept].astype(np.float64)
    assert np.isfinite(X).all()
    assert (X[:, 2] > 0).all() and ((X @ Pr[0][:, :3].T + Pr[0][:, 3])[:, 2] > 0).all()         # in front of both cameras
    right = sfm_scene.right_matches(sc, 0, 1, m[3], m[4])
    assert right[kept].mean() > 0.99


# ---- the shim ------------------------------------------------------------------------------------------------------------
def shim_single(lib, K, view_l, view_r, img_l, img_r, q, t, Pl, Pr):
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    cap = max(len(q), 1)
    X = np.zeros((cap, 3), np.float32); lr = np.zeros(cap, np.int32); rr = np.zeros(cap, np.int32)
    K, Pl, Pr, img_l, img_r = (np.ascontiguousarray(a, np.float32) for a in (K, Pl, Pr, img_l, img_r))
    q, t = np.ascontiguousarray(q, np.int32), np.ascontiguousarray(t, np.int32)
    n = lib.sfmba_shim_triangulate_views(K.ctypes.data_as(fp), C.c_int(view_l), C.c_int(view_r), C.c_int(len(img_l)), img_l.ctypes.data_as(fp),
                                         C.c_int(len(img_r)), img_r.ctypes.data_as(fp), C.c_int(len(q)), q.ctypes.data_as(ip), t.ctypes.data_as(ip),
                                         Pl.ctypes.data_as(fp), Pr.ctypes.data_as(fp), C.c_int(cap), X.ctypes.data_as(fp), lr.ctypes.data_as(ip),
                                         rr.ctypes.data_as(ip))
    assert n >= 0
    return X[:n], lr[:n], rr[:n]


def test_shim_batch_equals_per_pair_triangulate_views(sized):
    lib = C.CDLL(SHIM)
    b, _, _ = sized
    ptr, q, t = b["matches"]
    ps = [np.ascontiguousarray(x, np.float32) for x in b["pts"]]
    img_ptr = np.zeros(len(ps) + 1, np.int64)
    img_ptr[1:] = np.cumsum([len(x) for x in ps])
    xy = np.ascontiguousarray(np.concatenate(ps))
    pairs = np.asarray(b["pairs"], np.int32)
    pl, pr = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    n_pairs, cap = len(pl), int(ptr[-1])
    K, Pl, Pr = (np.ascontiguousarray(a, np.float32) for a in (b["K"], b["Pl"], b["Pr"]))
    ok = np.zeros(n_pairs, np.uint8); cloud_ptr = np.zeros(n_pairs + 1, np.int64)
    X = np.zeros((cap, 3), np.float32); lr = np.zeros(cap, np.int32); rr = np.zeros(cap, np.int32)
    lp, ip, fp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    rc = lib.sfmba_shim_triangulate_views_batch(K.ctypes.data_as(fp), C.c_int(len(ps)), img_ptr.ctypes.data_as(lp), xy.ctypes.data_as(fp), C.c_int(n_pairs),
                                                pl.ctypes.data_as(ip), pr.ctypes.data_as(ip), ptr.ctypes.data_as(lp), q.ctypes.data_as(ip),
                                                t.ctypes.data_as(ip), Pl.ctypes.data_as(fp), Pr.ctypes.data_as(fp), ok.ctypes.data_as(bp),
                                                cloud_ptr.ctypes.data_as(lp), C.c_int64(cap), X.ctypes.data_as(fp), lr.ctypes.data_as(ip),
                                                rr.ctypes.data_as(ip))
    assert rc == 1 and ok.all()
    assert 0 < cloud_ptr[-1] < cap
    for p in range(n_pairs):
        a, e = int(ptr[p]), int(ptr[p + 1])
        Xs, ls, rs = shim_single(lib, K, int(pl[p]), int(pr[p]), ps[pl[p]], ps[pr[p]], q[a:e], t[a:e], Pl[p], Pr[p])
        c0, c1 = int(cloud_ptr[p]), int(cloud_ptr[p + 1])
        assert c1 - c0 == len(Xs), p
        assert X[c0:c1].tobytes() == Xs.tobytes() and np.array_equal(lr[c0:c1], ls) and np.array_equal(rr[c0:c1], rs), p
    # an empty K is refused, as findCameraMatricesFromMatchBatch refuses it
    rc = lib.sfmba_shim_triangulate_views_batch(None, C.c_int(len(ps)), img_ptr.ctypes.data_as(lp), xy.ctypes.data_as(fp), C.c_int(n_pairs),
                                                pl.ctypes.data_as(ip), pr.ctypes.data_as(ip), ptr.ctypes.data_as(lp), q.ctypes.data_as(ip),
                                                t.ctypes.data_as(ip), Pl.ctypes.data_as(fp), Pr.ctypes.data_as(fp), ok.ctypes.data_as(bp),
                                                cloud_ptr.ctypes.data_as(lp), C.c_int64(cap), X.ctypes.data_as(fp), lr.ctypes.data_as(ip),
                                                rr.ctypes.data_as(ip))
    assert rc == 0 and not ok.any() and cloud_ptr[-1] == 0
