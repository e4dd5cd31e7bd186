"""sfmba_homography_ransac on the MI355X (-m gpu) against the CPU restatement of its contract (tests/homography_oracle.py,
include/sfmba.h).  The contract is this project's own; nothing here claims parity with cv::findHomography.

Bounds (all set by the contract's issue, none taken from the device's output; tests/test_homography_oracle_cpu.py re-measures the
figures they rest on without a GPU):
  1e-6 px   a valid hypothesis' H at its own four sample points (closed form against SVD on the host: below 1e-9 px; a lost factor
            or a wrong determinant order is off by pixels)
  1e-6      of max|H| between the device's H and the oracle's (measured: below 1e-10)
  5e-3 px   the band around the threshold inside which the fp32 inlier decision may differ from fp64 (the margin
            tests/test_gpu_triangulate.py and tests/test_gpu_pnp_ransac.py give float decisions); |w| <= 1e-6 counts as border too
  2 %       of the hypotheses of a scene may be left out as ill-conditioned (a determinant within 1e-9 of the validity threshold or
            of 0); the oracle alone finds none
Scene sizes: the minimum (4, 5), one wave +- 1 (64, 65), several waves (300), two chunks (2000) and the score kernel's LDS chunk
- 1, + 0, + 1; the 2000-point scene once more on a 4096 x 3072 image, where fp32 has the fewest bits left for the decision.  Every
scene reaches the device through shuffled key point lists and index arrays, as a match list does.  Section 8: one list past the
score kernel's grid cap (HOM_MAX_CHUNK_BLOCKS * HOM_CHUNK + HOM_CHUNK + 1 correspondences), alone and inside a batch of short ones."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import homography_oracle as ho

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
CHUNK = int(re.search(r"HOM_CHUNK\s*=\s*(\d+)", open(os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "homography_ransac.h")).read()).group(1))
SCENES = [(4, 0.0, 1), (5, 0.0, 2), (64, 0.3, 3), (65, 0.3, 4), (300, 0.45, 5), (2000, 0.3, 6),
          (CHUNK - 1, 0.3, 7), (CHUNK, 0.3, 8), (CHUNK + 1, 0.3, 9), (2000, 0.3, 6, (4096, 3072))]
THR = 10.0
MAX_HYP = 128


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


@pytest.fixture(scope="module")
def scenes():
    """key -> (scene, its arrays as the C ABI takes them, the oracle's 128 hypotheses for seed 0, pair 0): computed once, never modified."""
    import sfm_toy_library_amd as sfm
    out = {}
    for key in SCENES:
        sc = sfm.make_homography_scene(*key[:3], **({"size": key[3]} if len(key) > 3 else {}))
        out[key] = (sc, ho.scene_arrays(sc, key[2]), ho.hypotheses(sc["left"], sc["right"], MAX_HYP))
    return out


def call(capi, arrays, **kw):
    """One pair in a call of its own: images 0 and 1."""
    pl, pr, q, t = arrays
    return capi.homography_ransac([pl, pr], [(0, 1)], ([0, len(q)], q, t), **kw)[0]


@pytest.fixture(scope="module")
def runs(capi, scenes):
    """The device's answer for every scene at 100 hypotheses with debug outputs: one call per scene."""
    return {k: call(capi, arr, n_hyp=100, debug=True) for k, (_, arr, _) in scenes.items()}


# ---- 1. samples and hypotheses ---------------------------------------------------------------------------------------
def test_scene_arrays_gather_back_the_scene(scenes):
    for key, (sc, (pl, pr, q, t), _) in scenes.items():
        assert np.array_equal(pl[q], sc["left"]) and np.array_equal(pr[t], sc["right"]) and len(pl) > len(q)
        if len(q) > 4:
            assert not np.array_equal(q, np.arange(len(q)))


@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 100, 128])
def test_hypotheses_against_oracle(capi, scenes, n_hyp):
    for key, (sc, arr, hyp) in scenes.items():
        L, R = sc["left"].astype(np.float64), sc["right"].astype(np.float64)
        r = call(capi, arr, n_hyp=n_hyp, debug=True)
        assert r["n_matches"] == len(L)
        left_out = 0
        for h in range(n_hyp):
            s, H_o, info = hyp[h]
            valid = r["hyp_count"][h] >= 0
            H = r["hyp_H"][h]
            if not valid:
                assert r["hyp_count"][h] == -1 and not H.any(), (key, h)                          # an invalid hypothesis has a zero H
            if ho.ill_conditioned(info):
                left_out += 1
                continue
            assert valid == (H_o is not None), (key, h, info)
            if not valid:
                continue
            err, w = ho.transfer_errors(H, L[s], R[s])
            assert np.all(w > 0) and err.max() < 1e-6, (key, h, err, w)
            assert np.abs(H - H_o).max() <= 1e-6 * np.abs(H_o).max(), (key, h, np.abs(H - H_o).max())
        assert left_out <= 0.02 * n_hyp, (key, left_out)


# ---- 2. counts ---------------------------------------------------------------------------------------------------------
def test_counts_against_fp64_recount(scenes, runs):
    for key, (sc, _, _) in scenes.items():
        r = runs[key]
        L, R = sc["left"], sc["right"]
        counts = r["hyp_count"]
        for h in np.flatnonzero(counts >= 0):
            want = int(ho.inlier_mask(r["hyp_H"][h], L, R, THR).sum())
            border = ho.border_points(r["hyp_H"][h], L, R, THR)
            if counts[h] != want:
                print("count differs from fp64:", key, h, int(counts[h]), want, "border", border)
            assert abs(int(counts[h]) - want) <= border, (key, h, counts[h], want)
        assert r["status"] == 0 and counts.max() >= 0
        assert r["best_hypothesis"] == int(np.argmax(counts))                                    # the first maximum
        assert int(r["inlier"].sum()) == r["n_inliers"] == int(counts[r["best_hypothesis"]])
        assert r["H"].tobytes() == r["hyp_H"][r["best_hypothesis"]].tobytes()                    # the winner as it stands, no refit
        assert abs(int(r["inlier"].sum()) - int(ho.inlier_mask(r["H"], L, R, THR).sum())) <= ho.border_points(r["H"], L, R, THR)


# ---- 3. consensus ------------------------------------------------------------------------------------------------------
def test_consensus(scenes, runs):
    for key, (sc, _, hyp) in scenes.items():
        r = runs[key]
        L, R = sc["left"], sc["right"]
        oc = np.array([-1 if H is None else int(ho.inlier_mask(H, L, R, THR).sum()) for _, H, _ in hyp[:100]])
        best = int(np.argmax(oc))
        assert r["n_inliers"] >= oc[best] - ho.border_points(hyp[best][1], L, R, THR), (key, r["n_inliers"], oc[best])
        good = ~sc["bad"]
        assert (r["inlier"] & good).sum() >= 0.98 * good.sum(), (key, (r["inlier"] & good).sum(), good.sum())


# ---- 4. batch ----------------------------------------------------------------------------------------------------------
def same_bytes(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def as_batch(arrays):
    """Pairs (2 k, 2 k + 1) over the images of all the scenes, one pair per scene: (pts_per_image, pairs, (pair_ptr, query, train))."""
    imgs, pairs, ptr, q, t = [], [], [0], [], []
    for k, (pl, pr, qi, ti) in enumerate(arrays):
        imgs += [pl, pr]
        pairs.append((2 * k, 2 * k + 1))
        q.append(qi); t.append(ti)
        ptr.append(ptr[-1] + len(qi))
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)
    return imgs, pairs, (np.array(ptr, np.int64), cat(q), cat(t))


def test_batch_equals_single_calls(capi, scenes):
    arrays = [scenes[tuple(k)][1] for k in SCENES[:6]]
    seed = 41
    batch = capi.homography_ransac(*as_batch(arrays), n_hyp=100, seed=seed, debug=True)
    for p, arr in enumerate(arrays):
        same_bytes(batch[p], call(capi, arr, n_hyp=100, seed=seed + p, debug=True))
        assert batch[p]["status"] == 0


def test_batch_with_degenerate_pairs(capi, scenes):
    a, b = scenes[(64, 0.3, 3)][1], scenes[(300, 0.45, 5)][1]
    none = np.zeros(0, np.int32)
    empty = (a[0], a[1], none, none)
    three = (a[0], a[1], a[2][:3], a[3][:3])
    line = np.array([[10, 10], [20, 15], [30, 20], [50, 30], [400, 300]], np.float32)          # the first four on one line
    collinear = (line, a[1], np.arange(4, dtype=np.int32), a[3][:4])
    batch = capi.homography_ransac(*as_batch([a, empty, three, collinear, b]), n_hyp=64, seed=5, debug=True)
    for p, status, n in ((1, 1, 0), (2, 1, 3), (3, 2, 4)):
        r = batch[p]
        assert r["status"] == status and r["best_hypothesis"] == -1 and r["n_inliers"] == 0 and r["n_matches"] == n
        assert np.array_equal(r["H"], np.eye(3)) and not r["inlier"].any() and len(r["inlier"]) == n
        assert np.all(r["hyp_count"] == -1) and not r["hyp_H"].any()
    same_bytes(batch[0], call(capi, a, n_hyp=64, seed=5, debug=True))
    same_bytes(batch[4], call(capi, b, n_hyp=64, seed=9, debug=True))
    assert batch[0]["status"] == 0 and batch[4]["status"] == 0


def test_same_image_and_repeated_indices_are_legal(capi, scenes):
    pl, pr, q, t = scenes[(300, 0.45, 5)][1]
    r = capi.homography_ransac([pl], [(0, 0)], ([0, len(q)], q, q), n_hyp=100, debug=True)[0]      # an image against itself: the identity fits
    assert r["status"] == 0 and r["n_inliers"] == len(q) and r["inlier"].all()
    assert np.abs(r["H"] - np.eye(3)).max() < 1e-9 and np.all(np.isfinite(r["hyp_H"]))
    r = capi.homography_ransac([pl], [(0, 0)], ([0, len(q)], q, t), n_hyp=100, debug=True)[0]      # ... and against a shuffle of itself
    assert r["status"] in (0, 2) and np.all(np.isfinite(r["H"])) and np.all(np.isfinite(r["hyp_H"]))
    rep = np.repeat(np.arange(len(q) // 2), 2)
    r = capi.homography_ransac([pl, pr], [(0, 1)], ([0, len(rep)], q[rep], t[rep]), n_hyp=100, debug=True)[0]
    assert r["status"] == 0 and np.all(np.isfinite(r["H"])) and np.all(np.isfinite(r["hyp_H"]))
    assert int(r["inlier"].sum()) == r["n_inliers"] == int(r["hyp_count"].max())
    same = np.zeros(8, np.int32)                                                                    # one correspondence eight times: no quad has a scale
    r = capi.homography_ransac([pl, pr], [(0, 1)], ([0, 8], q[same], t[same]), n_hyp=64, debug=True)[0]
    assert r["status"] == 2 and np.array_equal(r["H"], np.eye(3)) and not r["inlier"].any()


# ---- 5. determinism and arguments --------------------------------------------------------------------------------------
def test_two_calls_are_byte_equal(capi, scenes):
    args = as_batch([scenes[(2000, 0.3, 6)][1], scenes[(CHUNK + 1, 0.3, 9)][1]])
    a = capi.homography_ransac(*args, n_hyp=128, seed=3, debug=True)
    b = capi.homography_ransac(*args, n_hyp=128, seed=3, debug=True)
    for x, y in zip(a, b):
        same_bytes(x, y)


def raw(capi, img_ptr, pts, left, right, pair_ptr, q, t, n_hyp=100, thr=10.0):
    """The entry point itself, on arrays as they are given (the binding builds img_ptr; this does not)."""
    img_ptr, pair_ptr = np.asarray(img_ptr, np.int64), np.asarray(pair_ptr, np.int64)
    pts = np.ascontiguousarray(pts, np.float32)
    left, right, q, t = (np.ascontiguousarray(x, np.int32) for x in (left, right, q, t))
    n_pairs = len(left)
    H, inl = np.zeros(9 * max(n_pairs, 1)), np.zeros(max(len(q), 1), np.uint8)
    res = (C.c_int * (4 * max(n_pairs, 1)))()
    lp, ip, fp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    return capi.lib().sfmba_homography_ransac(
        C.c_int(0), C.c_int(len(img_ptr) - 1), img_ptr.ctypes.data_as(lp), pts.ctypes.data_as(fp), C.c_int(n_pairs), left.ctypes.data_as(ip),
        right.ctypes.data_as(ip), pair_ptr.ctypes.data_as(lp), q.ctypes.data_as(ip), t.ctypes.data_as(ip), C.c_int(n_hyp), C.c_float(thr),
        C.c_uint64(0), H.ctypes.data_as(C.POINTER(C.c_double)), inl.ctypes.data_as(C.POINTER(C.c_ubyte)), res, None, None)


def test_invalid_arguments_are_refused(capi, scenes):
    pl, pr, q, t = scenes[(64, 0.3, 3)][1]
    n, nl, nr = len(q), len(pl), len(pr)
    ok = dict(img_ptr=[0, nl, nl + nr], pts=np.concatenate([pl, pr]), left=[0], right=[1], pair_ptr=[0, n], q=q, t=t)
    assert raw(capi, **ok) == 0

    def refused(**kw):
        assert raw(capi, **dict(ok, **kw)) == 1, kw

    for n_hyp in (0, -1, 65537):
        refused(n_hyp=n_hyp)
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        refused(thr=thr)
    refused(img_ptr=[-1, nl, nl + nr])                                   # negative
    refused(img_ptr=[0, nl + nr, nl])                                    # decreasing
    refused(pair_ptr=[-1, n])
    refused(pair_ptr=[0, n, n - 1], left=[0, 0], right=[1, 1])           # decreasing
    for bad in (-1, 2):                                                  # a pair index out of range, either side
        refused(left=[bad])
        refused(right=[bad])
    for side, size in (("q", nl), ("t", nr)):                            # an index outside its image, either side, either end
        for bad in (-1, size):
            idx = ok[side].copy()
            idx[n // 2] = bad
            refused(**{side: idx})
    refused(pair_ptr=[0, 2 ** 31])                                       # refused before any entry is read
    # through the binding: the error carries rc = 1 and its reason
    with pytest.raises(capi.SfmbaError, match="rc=1:.*n_hyp"):
        call(capi, (pl, pr, q, t), n_hyp=0)
    assert call(capi, (pl, pr, q, t), n_hyp=65536)["status"] == 0      # the largest n_hyp is accepted


# ---- 6. the chain from the matcher -------------------------------------------------------------------------------------
def test_match_features_output_goes_straight_in(capi):
    import sfm_toy_library_amd as sfm
    descs = sfm.make_descriptors(3, 300, 32, seed=71)                    # + an empty image and a one-row image
    rng = np.random.default_rng(72)
    pts = [rng.uniform(0, 1000, (len(d), 2)).astype(np.float32) for d in descs]
    m = capi.match_features(descs)
    pair_left, pair_right, ptr, q, t, _ = m
    res = capi.homography_ransac(pts, None, m, n_hyp=64, seed=7, debug=True)
    assert len(res) == len(pair_left) == 10 and ptr[-1] > 100
    for p, (l, r) in enumerate(zip(pair_left, pair_right)):
        qi, ti = q[ptr[p]:ptr[p + 1]], t[ptr[p]:ptr[p + 1]]
        n = len(qi)
        # the correspondences gathered by hand are their own two images, matched in order
        want = capi.homography_ransac([pts[l][qi], pts[r][ti]], [(0, 1)], ([0, n], np.arange(n), np.arange(n)), n_hyp=64, seed=7 + p, debug=True)[0]
        same_bytes(res[p], want)
        assert res[p]["n_matches"] == n and (n >= 4 or res[p]["status"] == 1)
    assert sum(r["n_matches"] >= 4 for r in res) == 3 and sum(r["n_matches"] == 0 for r in res) == 7


# ---- 7. the shim -------------------------------------------------------------------------------------------------------
def test_shim_find_homography_inliers(capi, scenes):
    lib = C.CDLL(SHIM)
    lp, ip, fp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    for key in ((300, 0.45, 5), (CHUNK + 1, 0.3, 9)):
        pl, pr, q, t = scenes[key][1]
        img_ptr = np.array([0, len(pl), len(pl) + len(pr)], np.int64)
        xy = np.ascontiguousarray(np.concatenate([pl, pr]))
        want = call(capi, (pl, pr, q, t), n_hyp=2000, threshold_px=10.0, seed=0)
        got = lib.sfmba_shim_find_homography_inliers(img_ptr.ctypes.data_as(lp), xy.ctypes.data_as(fp), C.c_int(len(q)), q.ctypes.data_as(ip), t.ctypes.data_as(ip))
        assert want["status"] == 0 and got == want["n_inliers"] > 0.5 * len(q)
        assert lib.sfmba_shim_find_homography_inliers(img_ptr.ctypes.data_as(lp), xy.ctypes.data_as(fp), C.c_int(3), q.ctypes.data_as(ip), t.ctypes.data_as(ip)) == 0


def planted_pair(seed, n=150, n_bad=45):
    """A pair whose best count is known: n - n_bad correspondences under one homography (0.5 px noise) and n_bad that are each
    100 px and more away from where that homography sends them, no two by the same offset."""
    import sfm_toy_library_amd as sfm
    sc = sfm.make_homography_scene(n, 0.0, seed)
    right = sc["right"].copy()
    right[:n_bad] += np.stack([100.0 + 10.0 * np.arange(n_bad), -100.0 - 7.0 * np.arange(n_bad)], axis=1).astype(np.float32)
    return sc["left"], right


def test_shim_sort_views_for_baseline(capi):
    import sfm_toy_library_amd as sfm
    n_img = 5
    imgs = [[] for _ in range(n_img)]
    pairs, ptr, q, t = [], [0], [], []
    for i in range(n_img):
        for j in range(i + 1, n_img):
            if (i, j) == (1, 3):                                           # too few matches for a homography: key 1.0
                sc = sfm.make_homography_scene(60, 0.3, 100)
                left, right = sc["left"], sc["right"]
            elif (i, j) in ((0, 2), (2, 4)):                               # built identically: the same count, the same key
                left, right = planted_pair(101)
            else:
                sc = sfm.make_homography_scene(120 + 10 * (i + j), 0.1 * (i + j), 102 + 5 * i + j)
                left, right = sc["left"], sc["right"]
            q.append(sum(len(x) for x in imgs[i]) + np.arange(len(left)))
            t.append(sum(len(x) for x in imgs[j]) + np.arange(len(right)))
            imgs[i].append(left); imgs[j].append(right)
            pairs.append((i, j)); ptr.append(ptr[-1] + len(left))
    pts = [np.concatenate(x) for x in imgs]
    ptr, q, t = np.array(ptr, np.int64), np.concatenate(q).astype(np.int32), np.concatenate(t).astype(np.int32)
    pl, pr = np.array(pairs, np.int32)[:, 0].copy(), np.array(pairs, np.int32)[:, 1].copy()
    # what the shim must do, in Python: ONE call over the qualifying pairs, then the reference's map (SfM.cpp:339-361)
    sizes = np.diff(ptr)
    qual = [p for p in range(len(pairs)) if sizes[p] >= 100]
    sub_ptr = np.concatenate([[0], np.cumsum(sizes[qual])]).astype(np.int64)
    sub_q, sub_t = np.concatenate([q[ptr[p]:ptr[p + 1]] for p in qual]), np.concatenate([t[ptr[p]:ptr[p + 1]] for p in qual])
    res = capi.homography_ransac(pts, [pairs[p] for p in qual], (sub_ptr, sub_q, sub_t), n_hyp=2000, threshold_px=10.0, seed=0)
    ratio = {pairs[p]: np.float32(r["n_inliers"]) / np.float32(sizes[p]) for p, r in zip(qual, res)}
    assert ratio[(0, 2)] == ratio[(2, 4)] == np.float32(105) / np.float32(150)
    want = {}
    for p, pair in enumerate(pairs):
        want[np.float32(1.0) if sizes[p] < 100 else ratio[pair]] = pair
    assert (0, 2) not in want.values() and (2, 4) in want.values() and want[np.float32(1.0)] == (1, 3)
    lib = C.CDLL(SHIM)
    lp, ip, fp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    img_ptr = np.concatenate([[0], np.cumsum([len(x) for x in pts])]).astype(np.int64)
    xy = np.ascontiguousarray(np.concatenate(pts), np.float32)
    keys, out = np.zeros(16, np.float32), np.zeros((16, 2), np.int32)
    n = lib.sfmba_shim_sort_views_for_baseline(C.c_int(n_img), img_ptr.ctypes.data_as(lp), xy.ctypes.data_as(fp), C.c_int(len(pairs)), pl.ctypes.data_as(ip),
                                               pr.ctypes.data_as(ip), ptr.ctypes.data_as(lp), q.ctypes.data_as(ip), t.ctypes.data_as(ip), C.c_int(16),
                                               keys.ctypes.data_as(fp), out.ctypes.data_as(ip))
    assert n == len(want)
    assert [(k, tuple(v)) for k, v in zip(keys[:n], out[:n])] == [(k, want[k]) for k in sorted(want)]


# ---- 8. a list past the score kernel's grid cap -------------------------------------------------------------------------
# k_hom_score caps grid.y at HOM_MAX_CHUNK_BLOCKS; past HOM_MAX_CHUNK_BLOCKS * HOM_CHUNK correspondences a block walks several
# chunks and reuses its LDS tile.  LONG_N: two blocks make a second trip, and the last chunk, reached on that trip, holds ONE
# correspondence.  65 hypotheses: the second tile has one live lane.
MAX_CHUNK_BLOCKS = int(re.search(r"HOM_MAX_CHUNK_BLOCKS\s*=\s*(\d+)", open(os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "homography_ransac.h")).read()).group(1))
FIRST_TRIP = MAX_CHUNK_BLOCKS * CHUNK
LONG_N = FIRST_TRIP + CHUNK + 1
LONG_SEED = 21
LONG_HYP = 65


@pytest.fixture(scope="module")
def long_scene():
    """(scene, its arrays as the C ABI takes them, the oracle's answer for seed 0): computed once, never modified.  The tail must
    matter: the oracle's winner has more inliers past the first trip than border points, so a count without them cannot pass."""
    import sfm_toy_library_amd as sfm
    sc = sfm.make_homography_scene(LONG_N, 0.3, LONG_SEED)
    want = ho.homography_ransac(sc["left"], sc["right"], n_hyp=LONG_HYP, threshold_px=THR, seed=0)
    assert want["status"] == 0
    tail, border = int(want["inlier"][FIRST_TRIP:].sum()), ho.border_points(want["H"], sc["left"], sc["right"], THR)
    print("front_end_edges homography long list: n %d, oracle winner %d with %d inliers, %d of them past the first trip, %d border points"
          % (LONG_N, want["best_hypothesis"], want["n_inliers"], tail, border))
    assert len(sc["left"]) == LONG_N == FIRST_TRIP + CHUNK + 1 and tail > border and tail > 0.5 * (LONG_N - FIRST_TRIP)
    assert want["inlier"][-1] or want["inlier"][FIRST_TRIP:FIRST_TRIP + CHUNK].sum() > border      # either later chunk alone would show
    return sc, ho.scene_arrays(sc, LONG_SEED), want


@pytest.fixture(scope="module")
def long_run(capi, long_scene):
    return call(capi, long_scene[1], n_hyp=LONG_HYP, debug=True)


def test_long_list_counts_against_fp64_recount(long_scene, long_run):
    sc, _, want = long_scene
    r = long_run
    L, R = sc["left"], sc["right"]
    counts = r["hyp_count"]
    assert r["status"] == 0 and r["n_matches"] == LONG_N and len(counts) == LONG_HYP
    worst = 0.0
    for h in np.flatnonzero(counts >= 0):
        recount = int(ho.inlier_mask(r["hyp_H"][h], L, R, THR).sum())
        border = ho.border_points(r["hyp_H"][h], L, R, THR)
        worst = max(worst, abs(int(counts[h]) - recount) / max(border, 1))
        assert abs(int(counts[h]) - recount) <= border, (h, counts[h], recount, border)
    print("front_end_edges homography long list: worst |count - fp64 recount| / border count over %d valid hypotheses: %.3f" % ((counts >= 0).sum(), worst))
    sure = np.array([not ho.ill_conditioned(info) for _, _, info in want["hyp"]])
    assert np.array_equal((counts >= 0)[sure], (want["hyp_count"] >= 0)[sure]) and sure.sum() >= LONG_HYP - 1
    assert counts[LONG_HYP - 1] >= 0 and want["hyp_count"][LONG_HYP - 1] >= 0           # the one live lane of the second tile is a valid one
    assert r["best_hypothesis"] == int(np.argmax(counts))                                # the first maximum
    assert int(r["inlier"].sum()) == r["n_inliers"] == int(counts[r["best_hypothesis"]])
    assert r["H"].tobytes() == r["hyp_H"][r["best_hypothesis"]].tobytes()
    assert r["n_inliers"] >= want["n_inliers"] - ho.border_points(want["H"], L, R, THR)
    assert int(r["inlier"][FIRST_TRIP:].sum()) > 0.5 * (LONG_N - FIRST_TRIP)


def test_long_list_in_a_mixed_batch(capi, scenes, long_scene):
    """grid.y is at its cap while three of the four pairs have one chunk: 5, LONG_N, 300 and HOM_CHUNK correspondences."""
    arrays = [scenes[(5, 0.0, 2)][1], long_scene[1], scenes[(300, 0.45, 5)][1], scenes[(CHUNK, 0.3, 8)][1]]
    assert [len(a[2]) for a in arrays] == [5, LONG_N, 300, CHUNK]
    seed = 41
    batch = capi.homography_ransac(*as_batch(arrays), n_hyp=LONG_HYP, seed=seed, debug=True)
    for p, arr in enumerate(arrays):
        same_bytes(batch[p], call(capi, arr, n_hyp=LONG_HYP, seed=seed + p, debug=True))
        assert batch[p]["status"] == 0


def test_long_list_two_calls_are_byte_equal(capi, long_scene, long_run):
    same_bytes(long_run, call(capi, long_scene[1], n_hyp=LONG_HYP, debug=True))
