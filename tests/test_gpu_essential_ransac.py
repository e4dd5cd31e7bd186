"""sfmba_essential_ransac on the MI355X (-m gpu) against the CPU restatement of its contract (tests/essential_oracle.py,
include/sfmba.h).  The contract is this project's own; nothing here claims parity with cv::findEssentialMat.

Bounds (all set by the contract's issue, none taken from the device's output; tests/test_essential_oracle_cpu.py re-measures the
figures they rest on without a GPU):
  1e-6 px      a valid hypothesis' Sampson distance at its own five sample points (both routes on the host: below 1e-10 px)
  1e-6 sqrt 2  between the device's E and the oracle's, |E|_F = sqrt 2 and the sign fixed (measured on the host: below 1e-12)
  5e-3 px      the band around the threshold inside which the device's inlier decision may differ from fp64 (the margin
               tests/test_gpu_homography_ransac.py and tests/test_gpu_pnp_ransac.py give float decisions; the device takes the
               residual in fp64 and needs about 1e-6 px of it)
  2 %          of the hypotheses of a scene may be left out as ill-conditioned (essential_oracle.ill_conditioned); the oracle alone
               finds none on these scenes
  1e-12        R orthonormal with det 1, |t| = 1, [t]x R = +-E
  1e-9 / 1e-12 a depth within 1e-9 relative of 0 or 50, or a 2 x 2 determinant below 1e-12, counts as border for the in-front test
  2 / 3 deg    rotation / translation direction against the planted pose at 128 hypotheses on the 0.2 px scenes with >= 64 matches
               (measured with the numpy route: <= 0.5 / <= 0.8 deg); the planar scene is exempt
Scene sizes: the minimum (6, 7), one wave +- 1 (64, 65), several waves (300), two chunks (2000) and the score kernel's LDS chunk
- 1, + 0, + 1; a planar scene; the 2000-point scene once more on a 4096 x 3072 image, where fp32 has the fewest bits left for the
decision.  Every scene reaches the device through shuffled key point lists and index arrays, as a match list does.  Section 8: one
list past the score kernel's grid cap (ESS_MAX_CHUNK_BLOCKS * ESS_CHUNK + ESS_CHUNK + 1 correspondences), alone and inside a batch
of short ones."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import essential_oracle as eo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
HDR = open(os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "essential_ransac.h")).read()
CHUNK = int(re.search(r"ESS_CHUNK\s*=\s*(\d+)", HDR).group(1))
SCENES = [(6, 0.0, 1), (7, 0.0, 2), (64, 0.3, 3), (65, 0.3, 4), (300, 0.45, 5), (2000, 0.3, 6),
          (CHUNK - 1, 0.3, 7), (CHUNK, 0.3, 8), (CHUNK + 1, 0.3, 9), (300, 0.3, 10, "planar"), (2000, 0.3, 6, (4096, 3072))]
THR = 1.0
MAX_HYP = 128
TOL_E = 1e-6 * np.sqrt(2.0)


def make_scene(sfm, key):
    kw = {}
    if len(key) > 3:
        kw = {"planar": True} if key[3] == "planar" else {"size": key[3]}
    return sfm.make_essential_scene(*key[:3], **kw)


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
        sc = make_scene(sfm, key)
        out[key] = (sc, eo.scene_arrays(sc, key[2]), eo.hypotheses(sc["left"], sc["right"], sc["K"], MAX_HYP))
    return out


def call(capi, arrays, K, **kw):
    """One pair in a call of its own: images 0 and 1."""
    pl, pr, q, t = arrays
    return capi.essential_ransac([pl, pr], [(0, 1)], ([0, len(q)], q, t), K, **kw)[0]


@pytest.fixture(scope="module")
def runs(capi, scenes):
    """The device's answer for every scene at 128 hypotheses with debug outputs: one call per scene."""
    return {k: call(capi, arr, sc["K"], n_hyp=MAX_HYP, debug=True) for k, (sc, arr, _) in scenes.items()}


# ---- 1. samples and hypotheses ---------------------------------------------------------------------------------------
def test_scene_arrays_gather_back_the_scene(scenes):
    for key, (sc, (pl, pr, q, t), _) in scenes.items():
        assert np.array_equal(pl[q], sc["left"]) and np.array_equal(pr[t], sc["right"]) and len(pl) > len(q)
        if len(q) > 6:
            assert not np.array_equal(q, np.arange(len(q)))


@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 100, 128])
def test_hypotheses_against_oracle(capi, scenes, n_hyp):
    for key, (sc, arr, hyp) in scenes.items():
        L, R, K = sc["left"], sc["right"], sc["K"]
        r = call(capi, arr, K, n_hyp=n_hyp, debug=True)
        assert r["n_matches"] == len(L) and len(r["hyp_count"]) == n_hyp
        left_out, worst_e, worst_px = 0, 0.0, 0.0
        for h in range(n_hyp):
            s, E_o, nsol_o, info = hyp[h]
            valid = r["hyp_count"][h] >= 0
            E = r["hyp_E"][h]
            if not valid:
                assert r["hyp_count"][h] == -1 and not E.any(), (key, h)                          # an invalid hypothesis has a zero E
            if eo.ill_conditioned(info):
                left_out += 1
                continue
            assert valid == (E_o is not None), (key, h, info)
            if not valid:
                continue
            # the same E can only come from the same sample: the sample stream is checked with it
            assert r["hyp_nsol"][h] == nsol_o, (key, h, r["hyp_nsol"][h], nsol_o)
            assert np.abs(E - E_o).max() <= TOL_E, (key, h, np.abs(E - E_o).max(), info)
            assert abs(np.linalg.norm(E) - np.sqrt(2.0)) < 1e-12 and E.ravel()[np.argmax(np.abs(E.ravel()))] > 0
            px = eo.sampson_px(E, L[s[:5]], R[s[:5]], K).max()
            assert px < 1e-6, (key, h, px)
            worst_e, worst_px = max(worst_e, np.abs(E - E_o).max()), max(worst_px, px)
        print("scene %s n_hyp %d: worst |E - oracle| %.2e, worst own Sampson %.2e px, left out %d" % (key, n_hyp, worst_e, worst_px, left_out))
        assert left_out <= 0.02 * n_hyp, (key, left_out)


# ---- 2. counts ---------------------------------------------------------------------------------------------------------
def test_counts_against_fp64_recount(scenes, runs):
    for key, (sc, _, _) in scenes.items():
        r = runs[key]
        L, R, K = sc["left"], sc["right"], sc["K"]
        counts = r["hyp_count"]
        for h in np.flatnonzero(counts >= 0):
            want = int(eo.inlier_mask(r["hyp_E"][h], L, R, K, THR).sum())
            border = int(eo.border_points(r["hyp_E"][h], L, R, K, THR).sum())
            if counts[h] != want:
                print("count differs from fp64:", key, h, int(counts[h]), want, "border", border)
            assert abs(int(counts[h]) - want) <= border, (key, h, counts[h], want)
        assert r["status"] == 0 and counts.max() >= 0
        assert r["best_hypothesis"] == int(np.argmax(counts))                                    # the first maximum
        assert r["n_inliers"] == int(counts[r["best_hypothesis"]])
        assert r["E"].tobytes() == r["hyp_E"][r["best_hypothesis"]].tobytes()                    # the winner as it stands, no refit
        # the mask before the pose has n_inliers members; the final one is a subset of it
        assert int(r["inlier"].sum()) == r["n_pose_inliers"] <= r["n_inliers"]
        before = eo.inlier_mask(r["E"], L, R, K, THR)
        border = eo.border_points(r["E"], L, R, K, THR)
        assert abs(int(before.sum()) - r["n_inliers"]) <= int(border.sum())
        assert not (r["inlier"] & ~before & ~border).any()


# ---- 3. pose -----------------------------------------------------------------------------------------------------------
def angle_deg(c):
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def test_pose(scenes, runs):
    for key, (sc, _, _) in scenes.items():
        r = runs[key]
        L, R, K = sc["left"], sc["right"], sc["K"]
        Rd, td = r["pose"][:, :3], r["pose"][:, 3]
        assert np.abs(Rd @ Rd.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rd) - 1.0) < 1e-12, key
        assert abs(np.linalg.norm(td) - 1.0) < 1e-12
        tR = eo.cross_matrix(td) @ Rd
        assert min(np.abs(tR - r["E"]).max(), np.abs(tR + r["E"]).max()) < 1e-12, key
        # the oracle's recoverPose on the device's E and the fp64 mask
        before = eo.inlier_mask(r["E"], L, R, K, THR)
        sampson_border = eo.border_points(r["E"], L, R, K, THR)
        rp = eo.recover_pose(r["E"], L, R, K, before)
        border = sampson_border | rp["border"]
        order = np.sort(rp["counts"])[::-1]
        if order[0] - order[1] > int(border.sum()):
            assert r["pose_candidate"] == rp["pose_candidate"], (key, r["pose_candidate"], rp["counts"])
        else:
            print("pose candidates within the border count of each other:", key, rp["counts"], int(border.sum()))
        cands = eo.svd_candidates(r["E"])
        Ro, to = cands[r["pose_candidate"]]
        assert np.abs(Rd - Ro).max() < 1e-9 and np.abs(td - to).max() < 1e-9, key
        want = before & rp["fronts"][r["pose_candidate"]]
        differ = (r["inlier"] != want) & ~border
        assert not differ.any(), (key, np.flatnonzero(differ))
        # no planted clutter row beyond what the fp64 oracle's mask holds
        assert not (r["inlier"] & sc["bad"] & ~want & ~border).any()
        ang_R = angle_deg((np.trace(Rd.T @ sc["R"]) - 1.0) / 2.0)
        ang_t = angle_deg(td @ sc["t"])
        good = ~sc["bad"]
        print("scene %s: candidate %d, %d of %d inliers in front, %d of %d planted good points kept, rotation %.3f deg, translation %.3f deg"
              % (key, r["pose_candidate"], r["n_pose_inliers"], r["n_inliers"], int((r["inlier"] & good).sum()), int(good.sum()), ang_R, ang_t))
        if len(L) >= 64 and "planar" not in key:
            assert ang_R < 2.0 and ang_t < 3.0, (key, ang_R, ang_t)
            assert (r["inlier"] & good).sum() >= 0.9 * good.sum()


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
    keys = SCENES[:6] + SCENES[9:10]
    arrays = [scenes[k][1] for k in keys]
    K = scenes[SCENES[0]][0]["K"]
    seed = 41
    batch = capi.essential_ransac(*as_batch(arrays), K, n_hyp=100, seed=seed, debug=True)
    for p, arr in enumerate(arrays):
        same_bytes(batch[p], call(capi, arr, K, n_hyp=100, seed=seed + p, debug=True))
        assert batch[p]["status"] == 0


def degenerate_ok(r, status, n):
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    assert r["status"] == status and r["best_hypothesis"] == -1 and r["n_inliers"] == 0 and r["n_matches"] == n
    assert r["n_pose_inliers"] == 0 and r["pose_candidate"] == -1
    assert not r["E"].any() and np.array_equal(r["pose"], eye) and not r["inlier"].any() and len(r["inlier"]) == n
    assert np.all(r["hyp_count"] == -1) and not r["hyp_E"].any()


def test_batch_with_degenerate_pairs(capi, scenes):
    sc = scenes[(64, 0.3, 3)][0]
    K = sc["K"]
    a, b = scenes[(64, 0.3, 3)][1], scenes[(300, 0.45, 5)][1]
    none = np.zeros(0, np.int32)
    empty = (a[0], a[1], none, none)
    five = (a[0], a[1], a[2][:5], a[3][:5])
    s = np.arange(8, dtype=np.float32)[:, None]
    line_l = (np.array([[100.0, 200.0]], np.float32) + s * np.array([[40.0, 20.0]], np.float32)).astype(np.float32)
    line_r = (np.array([[150.0, 90.0]], np.float32) + s * s * np.array([[8.0, 16.0]], np.float32)).astype(np.float32)
    ids = np.arange(8, dtype=np.int32)
    collinear = (line_l, line_r, ids, ids)                                   # every sample lies on one line in either image
    same = np.zeros(8, np.int32)
    identical = (a[0], a[1], a[2][same], a[3][same])                         # one correspondence eight times: no six distinct POINTS
    itself = (a[0], a[0], a[2], a[2])                                        # an image against itself: t = 0
    batch = capi.essential_ransac(*as_batch([a, empty, five, collinear, identical, itself, b]), K, n_hyp=64, seed=5, debug=True)
    degenerate_ok(batch[1], 1, 0)
    degenerate_ok(batch[2], 1, 5)
    degenerate_ok(batch[3], 2, 8)
    degenerate_ok(batch[4], 2, 8)
    r = batch[5]
    print("an image against itself: status %d, %d valid hypotheses, n_inliers %d" % (r["status"], int((r["hyp_count"] >= 0).sum()), r["n_inliers"]))
    assert r["status"] in (2, 3) and not r["inlier"].any() and r["n_pose_inliers"] == 0
    for k in ("E", "pose", "hyp_E"):
        assert np.all(np.isfinite(r[k])), k
    for p, arr in ((3, collinear), (4, identical), (5, itself)):
        same_bytes(batch[p], call(capi, arr, K, n_hyp=64, seed=5 + p, debug=True))
    same_bytes(batch[0], call(capi, a, K, n_hyp=64, seed=5, debug=True))
    same_bytes(batch[6], call(capi, b, K, n_hyp=64, seed=11, debug=True))
    assert batch[0]["status"] == 0 and batch[6]["status"] == 0


def test_repeated_indices_are_legal(capi, scenes):
    sc, (pl, pr, q, t), _ = scenes[(300, 0.45, 5)]
    rep = np.repeat(np.arange(len(q) // 2), 2)
    r = capi.essential_ransac([pl, pr], [(0, 1)], ([0, len(rep)], q[rep], t[rep]), sc["K"], n_hyp=100, debug=True)[0]
    assert r["status"] == 0 and np.all(np.isfinite(r["E"])) and np.all(np.isfinite(r["hyp_E"])) and np.all(np.isfinite(r["pose"]))
    assert r["n_inliers"] == int(r["hyp_count"].max()) and int(r["inlier"].sum()) == r["n_pose_inliers"]


# ---- 5. determinism and arguments --------------------------------------------------------------------------------------
def test_two_calls_are_byte_equal(capi, scenes):
    args = as_batch([scenes[(2000, 0.3, 6)][1], scenes[(CHUNK + 1, 0.3, 9)][1]])
    K = scenes[(2000, 0.3, 6)][0]["K"]
    a = capi.essential_ransac(*args, K, n_hyp=128, seed=3, debug=True)
    b = capi.essential_ransac(*args, K, n_hyp=128, seed=3, debug=True)
    for x, y in zip(a, b):
        same_bytes(x, y)


def raw(capi, img_ptr, pts, left, right, pair_ptr, q, t, K, n_hyp=100, thr=1.0):
    """The entry point itself, on arrays as they are given (the binding builds img_ptr; this does not)."""
    img_ptr, pair_ptr = np.asarray(img_ptr, np.int64), np.asarray(pair_ptr, np.int64)
    pts = np.ascontiguousarray(pts, np.float32)
    K = np.ascontiguousarray(K, np.float32).reshape(9)
    left, right, q, t = (np.ascontiguousarray(x, np.int32) for x in (left, right, q, t))
    n_pairs = len(left)
    E, pose, inl = np.zeros(9 * max(n_pairs, 1)), np.zeros(12 * max(n_pairs, 1)), np.zeros(max(len(q), 1), np.uint8)
    res = (C.c_int * (6 * max(n_pairs, 1)))()
    lp, ip, fp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    return capi.lib().sfmba_essential_ransac(
        C.c_int(0), C.c_int(len(img_ptr) - 1), img_ptr.ctypes.data_as(lp), pts.ctypes.data_as(fp), C.c_int(n_pairs), left.ctypes.data_as(ip),
        right.ctypes.data_as(ip), pair_ptr.ctypes.data_as(lp), q.ctypes.data_as(ip), t.ctypes.data_as(ip), K.ctypes.data_as(fp), C.c_int(n_hyp),
        C.c_float(thr), C.c_uint64(0), E.ctypes.data_as(dp), pose.ctypes.data_as(dp), inl.ctypes.data_as(C.POINTER(C.c_ubyte)), res, None, None, None)


def test_invalid_arguments_are_refused(capi, scenes):
    sc, (pl, pr, q, t), _ = scenes[(64, 0.3, 3)]
    n, nl, nr = len(q), len(pl), len(pr)
    ok = dict(img_ptr=[0, nl, nl + nr], pts=np.concatenate([pl, pr]), left=[0], right=[1], pair_ptr=[0, n], q=q, t=t, K=sc["K"])
    assert raw(capi, **ok) == 0

    def refused(**kw):
        assert raw(capi, **dict(ok, **kw)) == 1, kw

    for n_hyp in (0, -1, 65537):
        refused(n_hyp=n_hyp)
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        refused(thr=thr)
    for at in (0, 4):                                                    # fx, fy
        for bad in (0.0, -2500.0, float("nan"), float("inf")):
            K = sc["K"].copy().reshape(9)
            K[at] = bad
            refused(K=K)
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
        call(capi, (pl, pr, q, t), sc["K"], n_hyp=0)
    assert call(capi, (pl, pr, q, t), sc["K"], n_hyp=65536)["status"] == 0      # the largest n_hyp is accepted


# ---- 6. the chain from the matcher -------------------------------------------------------------------------------------
def test_match_features_output_goes_straight_in(capi, scenes):
    import sfm_toy_library_amd as sfm
    K = scenes[SCENES[0]][0]["K"]
    descs = sfm.make_descriptors(3, 300, 32, seed=71)                    # + an empty image and a one-row image
    rng = np.random.default_rng(72)
    pts = [rng.uniform(0, 1000, (len(d), 2)).astype(np.float32) for d in descs]
    m = capi.match_features(descs)
    pair_left, pair_right, ptr, q, t, _ = m
    res = capi.essential_ransac(pts, None, m, K, n_hyp=64, seed=7, debug=True)
    assert len(res) == len(pair_left) == 10 and ptr[-1] > 100
    for p, (l, r) in enumerate(zip(pair_left, pair_right)):
        qi, ti = q[ptr[p]:ptr[p + 1]], t[ptr[p]:ptr[p + 1]]
        n = len(qi)
        # the correspondences gathered by hand are their own two images, matched in order
        want = capi.essential_ransac([pts[l][qi], pts[r][ti]], [(0, 1)], ([0, n], np.arange(n), np.arange(n)), K, n_hyp=64, seed=7 + p, debug=True)[0]
        same_bytes(res[p], want)
        assert res[p]["n_matches"] == n and (n >= 6 or res[p]["status"] == 1)
    assert sum(r["n_matches"] >= 6 for r in res) == 3 and sum(r["n_matches"] == 0 for r in res) == 7


# ---- 7. the shim -------------------------------------------------------------------------------------------------------
def shim_single(lib, K, pl, pr, q, t, n=None):
    lp, ip, fp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    n = len(q) if n is None else n
    img_ptr = np.array([0, len(pl), len(pl) + len(pr)], np.int64)
    xy = np.ascontiguousarray(np.concatenate([pl, pr]))
    Kf = None if K is None else np.ascontiguousarray(K, np.float32).reshape(9)
    Pl, Pr = np.full(12, 7.0, np.float32), np.full(12, 9.0, np.float32)                     # sentinels: untouched on failure
    pruned = np.zeros((max(len(q), 2), 2), np.int32)
    pruned[0] = (123, 456)
    n_pruned = C.c_int(1)
    ok = lib.sfmba_shim_find_camera_matrices(None if Kf is None else Kf.ctypes.data_as(fp), img_ptr.ctypes.data_as(lp), xy.ctypes.data_as(fp),
                                             C.c_int(n), q.ctypes.data_as(ip), t.ctypes.data_as(ip), Pl.ctypes.data_as(fp), Pr.ctypes.data_as(fp),
                                             pruned.ctypes.data_as(ip), C.byref(n_pruned))
    return ok, Pl.reshape(3, 4), Pr.reshape(3, 4), pruned[:n_pruned.value]


def test_shim_find_camera_matrices(capi, scenes):
    lib = C.CDLL(SHIM)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)
    for key in ((300, 0.45, 5), (CHUNK + 1, 0.3, 9)):
        sc, (pl, pr, q, t), _ = scenes[key]
        want = call(capi, (pl, pr, q, t), sc["K"], n_hyp=1000, threshold_px=1.0, seed=0)
        ok, Pl, Pr, pruned = shim_single(lib, sc["K"], pl, pr, q, t)
        assert want["status"] == 0 and ok == 1
        assert np.array_equal(Pl, eye) and np.array_equal(Pr, want["pose"].astype(np.float32))
        keep = np.flatnonzero(want["inlier"])
        assert len(keep) > 0.5 * (~sc["bad"]).sum() and np.array_equal(pruned, np.stack([q[keep], t[keep]], axis=1))     # in order
        # failures leave the outputs untouched: an empty K, fewer than six matches
        for K, n in ((None, len(q)), (sc["K"], 5)):
            ok, Pl, Pr, pruned = shim_single(lib, K, pl, pr, q, t, n=n)
            assert ok == 0 and np.all(Pl == 7.0) and np.all(Pr == 9.0) and np.array_equal(pruned, [[123, 456]])


def test_shim_batch_equals_single_calls_on_pair_zero(capi, scenes):
    lib = C.CDLL(SHIM)
    lp, ip, fp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    arrays = [scenes[(300, 0.45, 5)][1], scenes[(64, 0.3, 3)][1], (scenes[(64, 0.3, 3)][1][0], scenes[(64, 0.3, 3)][1][1], np.zeros(0, np.int32), np.zeros(0, np.int32))]
    K = scenes[(64, 0.3, 3)][0]["K"]
    imgs, pairs, (ptr, q, t) = as_batch(arrays)
    img_ptr = np.concatenate([[0], np.cumsum([len(x) for x in imgs])]).astype(np.int64)
    xy = np.ascontiguousarray(np.concatenate(imgs), np.float32)
    pl, pr = np.array(pairs, np.int32)[:, 0].copy(), np.array(pairs, np.int32)[:, 1].copy()
    Kf = np.ascontiguousarray(K, np.float32).reshape(9)
    n_pairs = len(pairs)
    ok, Pl, Pr = np.zeros(n_pairs, np.uint8), np.zeros((n_pairs, 12), np.float32), np.zeros((n_pairs, 12), np.float32)
    pruned_ptr, pruned = np.zeros(n_pairs + 1, np.int64), np.zeros((max(len(q), 1), 2), np.int32)
    assert lib.sfmba_shim_find_camera_matrices_batch(Kf.ctypes.data_as(fp), C.c_int(len(imgs)), img_ptr.ctypes.data_as(lp), xy.ctypes.data_as(fp), C.c_int(n_pairs),
                                                     pl.ctypes.data_as(ip), pr.ctypes.data_as(ip), ptr.ctypes.data_as(lp), q.ctypes.data_as(ip), t.ctypes.data_as(ip),
                                                     ok.ctypes.data_as(C.POINTER(C.c_ubyte)), Pl.ctypes.data_as(fp), Pr.ctypes.data_as(fp), pruned_ptr.ctypes.data_as(lp),
                                                     pruned.ctypes.data_as(ip)) == 1
    want = capi.essential_ransac(imgs, pairs, (ptr, q, t), K, n_hyp=1000, threshold_px=1.0, seed=0)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32).ravel()
    assert list(ok) == [1, 1, 0] and [w["status"] for w in want] == [0, 0, 1]
    for p in range(n_pairs):
        assert np.array_equal(Pl[p], eye) and np.array_equal(Pr[p], want[p]["pose"].astype(np.float32).ravel())
        keep = np.flatnonzero(want[p]["inlier"])
        qi, ti = q[ptr[p]:ptr[p + 1]], t[ptr[p]:ptr[p + 1]]
        assert np.array_equal(pruned[pruned_ptr[p]:pruned_ptr[p + 1]], np.stack([qi[keep], ti[keep]], axis=1).reshape(-1, 2))
    # pair 0 of the batch is what the single-pair member gives
    ok0, Pl0, Pr0, pruned0 = shim_single(lib, K, *arrays[0])
    assert ok0 == 1 and np.array_equal(Pl0.ravel(), Pl[0]) and np.array_equal(Pr0.ravel(), Pr[0]) and np.array_equal(pruned0, pruned[:pruned_ptr[1]])


# ---- 8. a list past the score kernel's grid cap -------------------------------------------------------------------------
# k_ess_score caps grid.y at ESS_MAX_CHUNK_BLOCKS; past ESS_MAX_CHUNK_BLOCKS * ESS_CHUNK correspondences a block walks several
# chunks and reuses its LDS tile.  LONG_N: two blocks make a second trip, and the last chunk, reached on that trip, holds ONE
# correspondence.  65 hypotheses: the second tile has one live lane.
MAX_CHUNK_BLOCKS = int(re.search(r"ESS_MAX_CHUNK_BLOCKS\s*=\s*(\d+)", HDR).group(1))
FIRST_TRIP = MAX_CHUNK_BLOCKS * CHUNK
LONG_N = FIRST_TRIP + CHUNK + 1
LONG_SEED = 21
LONG_HYP = 65


@pytest.fixture(scope="module")
def long_scene():
    """(scene, its arrays as the C ABI takes them, the oracle's answer for seed 0): computed once, never modified.  The tail must
    matter: the oracle's winner has more inliers past the first trip than border points, so a count without them cannot pass."""
    import sfm_toy_library_amd as sfm
    sc = sfm.make_essential_scene(LONG_N, 0.3, LONG_SEED)
    want = eo.essential_ransac(sc["left"], sc["right"], sc["K"], n_hyp=LONG_HYP, threshold_px=THR, seed=0)
    assert want["status"] == 0
    tail, border = int(want["winner_mask"][FIRST_TRIP:].sum()), int(eo.border_points(want["E"], sc["left"], sc["right"], sc["K"], THR).sum())
    print("essential long list: n %d, oracle winner %d with %d inliers, %d of them past the first trip, %d border points"
          % (LONG_N, want["best_hypothesis"], want["n_inliers"], tail, border))
    assert len(sc["left"]) == LONG_N == FIRST_TRIP + CHUNK + 1 and tail > border and tail > 0.3 * (LONG_N - FIRST_TRIP)
    return sc, eo.scene_arrays(sc, LONG_SEED), want


@pytest.fixture(scope="module")
def long_run(capi, long_scene):
    return call(capi, long_scene[1], long_scene[0]["K"], n_hyp=LONG_HYP, debug=True)


def test_long_list_counts_against_fp64_recount(long_scene, long_run):
    sc, _, want = long_scene
    r = long_run
    L, R, K = sc["left"], sc["right"], sc["K"]
    counts = r["hyp_count"]
    assert r["status"] == 0 and r["n_matches"] == LONG_N and len(counts) == LONG_HYP
    worst = 0.0
    for h in np.flatnonzero(counts >= 0):
        recount = int(eo.inlier_mask(r["hyp_E"][h], L, R, K, THR).sum())
        border = int(eo.border_points(r["hyp_E"][h], L, R, K, THR).sum())
        worst = max(worst, abs(int(counts[h]) - recount) / max(border, 1))
        assert abs(int(counts[h]) - recount) <= border, (h, counts[h], recount, border)
    print("essential long list: worst |count - fp64 recount| / border count over %d valid hypotheses: %.3f" % ((counts >= 0).sum(), worst))
    sure = np.array([not eo.ill_conditioned(info) for _, _, _, info in want["hyp"]])
    assert np.array_equal((counts >= 0)[sure], (want["hyp_count"] >= 0)[sure]) and sure.sum() >= LONG_HYP - 1
    assert counts[LONG_HYP - 1] >= 0 and want["hyp_count"][LONG_HYP - 1] >= 0           # the one live lane of the second tile is a valid one
    assert r["best_hypothesis"] == int(np.argmax(counts))                                # the first maximum
    assert r["n_inliers"] == int(counts[r["best_hypothesis"]]) and int(r["inlier"].sum()) == r["n_pose_inliers"]
    assert r["E"].tobytes() == r["hyp_E"][r["best_hypothesis"]].tobytes()
    assert r["n_inliers"] >= want["n_inliers"] - int(eo.border_points(want["E"], L, R, K, THR).sum())
    assert int(r["inlier"][FIRST_TRIP:].sum()) > 0.3 * (LONG_N - FIRST_TRIP)


def test_long_list_in_a_mixed_batch(capi, scenes, long_scene):
    """grid.y is at its cap while three of the four pairs have one chunk: 7, LONG_N, 300 and ESS_CHUNK correspondences."""
    arrays = [scenes[(7, 0.0, 2)][1], long_scene[1], scenes[(300, 0.45, 5)][1], scenes[(CHUNK, 0.3, 8)][1]]
    assert [len(a[2]) for a in arrays] == [7, LONG_N, 300, CHUNK]
    K = long_scene[0]["K"]
    seed = 41
    batch = capi.essential_ransac(*as_batch(arrays), K, n_hyp=LONG_HYP, seed=seed, debug=True)
    for p, arr in enumerate(arrays):
        same_bytes(batch[p], call(capi, arr, K, n_hyp=LONG_HYP, seed=seed + p, debug=True))
        assert batch[p]["status"] == 0


def test_long_list_two_calls_are_byte_equal(capi, long_scene, long_run):
    same_bytes(long_run, call(capi, long_scene[1], long_scene[0]["K"], n_hyp=LONG_HYP, debug=True))
