"""sfmba_pnp_ransac on the MI355X (-m gpu) against the CPU restatement of its contract (tests/pnp_oracle.py, include/sfmba.h)
and the reference's known-answer test (find_camera_pose_from_2d3d_match, SfMUnitTests.cpp:194-216; inputs in
tests/golden/stereo_kat.json).  The contract is this project's own; nothing here claims parity with cv::solvePnPRansac.

Bounds (all set by the contract's issue, none taken from the device's output):
  1e-9    orthonormality of a hypothesis' R (fp64 triads: ~1e-15)
  1e-3 px reprojection of a hypothesis' own three sample points, and the slack on its fourth-point error against the oracle's
          minimum (the oracle's quartic route leaves 6e-5 px at worst; a lost or wrong root is off by pixels)
  5e-3 px the band around the threshold inside which the fp32 inlier decision may differ from fp64 (the margin
          tests/test_gpu_triangulate.py gives float decisions)
  1e-8    per pose entry between the device's Gauss-Newton and the oracle's from the same start on the same inliers
          (the oracle against scipy: 2.7e-11), 1e-9 relative on the cost
Scene sizes: the minimum (4, 5), one wave +- 1 (64, 65), several waves (300), two chunks (2000) and the score kernel's LDS chunk
- 1, + 0, + 1.  Section 9: one list past the score kernel's grid cap (PNP_MAX_CHUNK_BLOCKS * PNP_CHUNK + PNP_CHUNK + 1 points),
alone and inside a batch of short ones."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import pnp_oracle as po

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
CHUNK = int(re.search(r"PNP_CHUNK\s*=\s*(\d+)", open(os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "pnp_ransac.h")).read()).group(1))
SCENES = [(4, 0.0, 1), (5, 0.0, 2), (64, 0.3, 3), (65, 0.3, 4), (300, 0.45, 5), (2000, 0.3, 6),
          (CHUNK - 1, 0.3, 7), (CHUNK, 0.3, 8), (CHUNK + 1, 0.3, 9)]
THR = 10.0
MAX_HYP = 128


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


@pytest.fixture(scope="module")
def scenes():
    """name -> (scene, the oracle's 128 hypotheses for seed 0, problem 0): computed once, never modified."""
    import sfm_toy_library_amd as sfm
    out = {}
    for n, frac, seed in SCENES:
        sc = sfm.make_pnp_scene(n, frac, seed)
        out[(n, frac, seed)] = (sc, po.hypotheses(sc["X"], sc["uv"], sc["K"], MAX_HYP))
    return out


@pytest.fixture(scope="module")
def runs(capi, scenes):
    """The device's answer for every scene at 100 hypotheses with debug outputs: one call per scene."""
    return {k: capi.pnp_ransac([(sc["X"], sc["uv"])], sc["K"], n_hyp=100, debug=True)[0] for k, (sc, _) in scenes.items()}


@pytest.fixture(scope="module")
def kat():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "stereo_kat.json")))
    return np.array(d["K"]), np.array(d["P_left"]), np.array(d["left"], np.float32), np.array(d["points3d"], np.float32)


def shim_pose(K, X, uv, pose0):
    lib = C.CDLL(SHIM)
    fp = C.POINTER(C.c_float)
    K = np.ascontiguousarray(K, np.float32).reshape(9)
    X = np.ascontiguousarray(X, np.float32)
    uv = np.ascontiguousarray(uv, np.float32)
    pose = np.ascontiguousarray(pose0, np.float32).reshape(12).copy()
    ok = lib.sfmba_shim_find_camera_pose(K.ctypes.data_as(fp), C.c_int(len(X)), X.ctypes.data_as(fp), uv.ctypes.data_as(fp), pose.ctypes.data_as(fp))
    return bool(ok), pose.reshape(3, 4)


# ---- 1. the reference's known answer -------------------------------------------------------------------------------
def test_reference_kat_c_abi(capi, kat):
    K, P, uv, X = kat
    r = capi.pnp_ransac([(X, uv)], K)[0]
    assert r["status"] == 0
    assert np.abs(r["pose"][:, :3] - P[:, :3]).max() < 0.01 and np.abs(r["pose"][:, 3] - P[:, 3]).max() < 0.1
    assert r["n_inliers"] == 12 and r["inlier"].all()


def test_reference_kat_shim(kat):
    K, P, uv, X = kat
    ok, pose = shim_pose(K, X, uv, np.zeros((3, 4)))
    assert ok
    assert np.abs(pose[:, :3] - P[:, :3]).max() < 0.01 and np.abs(pose[:, 3] - P[:, 3]).max() < 0.1


# ---- 2. samples and hypotheses ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 100, 128])
def test_hypotheses_against_oracle(capi, scenes, n_hyp):
    for key, (sc, hyp) in scenes.items():
        X, uv, K = sc["X"].astype(np.float64), sc["uv"].astype(np.float64), sc["K"]
        r = capi.pnp_ransac([(sc["X"], sc["uv"])], K, n_hyp=n_hyp, debug=True)[0]
        left_out = 0
        for h in range(n_hyp):
            s, pose_o, info = hyp[h]
            valid = r["hyp_count"][h] >= 0
            P = r["hyp_pose"][h]
            if not valid:
                assert not P.any(), (key, h)                                                     # an invalid hypothesis has a zero pose
            if po.ill_conditioned(info):
                left_out += 1
                continue
            assert valid == (pose_o is not None), (key, h, info)                                 # (d)
            if not valid:
                continue
            R = P[:, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1.0) < 1e-9, (key, h)   # (a)
            err, z = po.pixel_errors(P, X[s], uv[s], K)
            assert np.all(z > 0), (key, h)
            assert err[:3].max() < 1e-3, (key, h, err)                                           # (b)
            assert err[3] <= info["e4"][0] + 1e-3, (key, h, err[3], info["e4"])                  # (c)
        assert left_out <= 0.02 * n_hyp, (key, left_out)


# ---- 3. counts ---------------------------------------------------------------------------------------------------------
def test_counts_against_fp64_recount(scenes, runs):
    for key, (sc, _) in scenes.items():
        r = runs[key]
        X, uv, K = sc["X"], sc["uv"], sc["K"]
        counts = r["hyp_count"]
        for h in np.flatnonzero(counts >= 0):
            want = int(po.inlier_mask(r["hyp_pose"][h], X, uv, K, THR).sum())
            assert abs(int(counts[h]) - want) <= po.border_points(r["hyp_pose"][h], X, uv, K, THR), (key, h, counts[h], want)
        assert r["status"] == 0 and counts.max() >= 0
        assert r["best_hypothesis"] == int(np.argmax(counts))                                    # the first maximum
        assert int(r["inlier"].sum()) == r["n_inliers"] == int(counts[r["best_hypothesis"]])


# ---- 4. consensus ------------------------------------------------------------------------------------------------------
def test_consensus(scenes, runs):
    for key, (sc, hyp) in scenes.items():
        r = runs[key]
        X, uv, K = sc["X"], sc["uv"], sc["K"]
        oc = np.array([-1 if pose is None else int(po.inlier_mask(pose, X, uv, K, THR).sum()) for _, pose, _ in hyp[:100]])
        best = int(np.argmax(oc))
        assert r["n_inliers"] >= oc[best] - po.border_points(hyp[best][1], X, uv, K, THR), (key, r["n_inliers"], oc[best])
        good = ~sc["bad"]
        if sc["bad"].any():
            assert (r["inlier"] & good).sum() >= 0.98 * good.sum(), (key, (r["inlier"] & good).sum(), good.sum())


# ---- 5. refinement -----------------------------------------------------------------------------------------------------
def test_refinement_against_oracle(capi, scenes, runs):
    for key, (sc, _) in scenes.items():
        r = runs[key]
        X, uv, K = sc["X"].astype(np.float64), sc["uv"].astype(np.float64), sc["K"]
        start, mask = r["hyp_pose"][r["best_hypothesis"]], r["inlier"]
        pose, cost, iters, status = po.refine(start, X[mask], uv[mask], K, 20)
        assert status == 0 and r["status"] == 0
        assert 1 <= r["refine_iters"] <= 20
        assert np.abs(r["pose"] - pose).max() < 1e-8, (key, np.abs(r["pose"] - pose).max())
        assert abs(r["refine_cost"] - cost) <= 1e-9 * cost, (key, r["refine_cost"], cost)
        off = capi.pnp_ransac([(sc["X"], sc["uv"])], K, n_hyp=100, max_refine_iters=0, debug=True)[0]
        assert off["refine_iters"] == 0 and off["pose"].tobytes() == off["hyp_pose"][off["best_hypothesis"]].tobytes()
        assert off["pose"].tobytes() == start.tobytes()
        assert abs(off["refine_cost"] - po.cost(start, X[mask], uv[mask], K)) <= 1e-9 * po.cost(start, X[mask], uv[mask], K)


# ---- 6. batch ----------------------------------------------------------------------------------------------------------
def same_bytes(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (k, a[k], b[k])


def test_batch_equals_single_calls(capi, scenes):
    keys = [tuple(s) for s in SCENES[:6]]
    K = scenes[keys[0]][0]["K"]
    probs = [(scenes[k][0]["X"], scenes[k][0]["uv"]) for k in keys]
    seed = 41
    batch = capi.pnp_ransac(probs, K, n_hyp=100, seed=seed, debug=True)
    for p, prob in enumerate(probs):
        same_bytes(batch[p], capi.pnp_ransac([prob], K, n_hyp=100, seed=seed + p, debug=True)[0])
        assert batch[p]["status"] == 0


def test_batch_with_degenerate_problems(capi, scenes):
    a, b = scenes[(64, 0.3, 3)][0], scenes[(300, 0.45, 5)][0]
    K = a["K"]
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32))
    three = (a["X"][:3], a["uv"][:3])
    dup = (a["X"][[0, 0, 1, 1]], a["uv"][[0, 2, 1, 3]])               # any three of the four contain a coinciding pair
    batch = capi.pnp_ransac([(a["X"], a["uv"]), empty, three, dup, (b["X"], b["uv"])], K, n_hyp=64, seed=5, debug=True)
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    for p, status in ((1, 1), (2, 1), (3, 2)):
        r = batch[p]
        assert r["status"] == status and r["best_hypothesis"] == -1 and r["n_inliers"] == 0
        assert np.array_equal(r["pose"], ident) and not r["inlier"].any()
        assert np.all(r["hyp_count"] == -1) and not r["hyp_pose"].any()
    same_bytes(batch[0], capi.pnp_ransac([(a["X"], a["uv"])], K, n_hyp=64, seed=5, debug=True)[0])
    same_bytes(batch[4], capi.pnp_ransac([(b["X"], b["uv"])], K, n_hyp=64, seed=9, debug=True)[0])
    assert batch[0]["status"] == 0 and batch[4]["status"] == 0


def test_collinear_points_never_give_nan(capi, scenes):
    sc = scenes[(64, 0.3, 3)][0]
    t = np.linspace(-1, 1, 40)
    X = (np.array([0.1, 0.2, 0.3]) + t[:, None] * np.array([1.0, 0.5, -0.25])).astype(np.float32)
    uv, _ = po.project(np.concatenate([sc["R"], sc["t"][:, None]], axis=1), X, sc["K"])
    r = capi.pnp_ransac([(X, uv.astype(np.float32))], sc["K"], n_hyp=100, debug=True)[0]
    assert np.all(np.isfinite(r["pose"])) and np.all(np.isfinite(r["hyp_pose"])) and np.isfinite(r["refine_cost"])
    assert r["status"] in (0, 2, 3)


# ---- 7. determinism and arguments --------------------------------------------------------------------------------------
def test_two_calls_are_byte_equal(capi, scenes):
    sc = scenes[(2000, 0.3, 6)][0]
    sd = scenes[(CHUNK + 1, 0.3, 9)][0]
    probs = [(sc["X"], sc["uv"]), (sd["X"], sd["uv"])]
    a = capi.pnp_ransac(probs, sc["K"], n_hyp=128, seed=3, debug=True)
    b = capi.pnp_ransac(probs, sc["K"], n_hyp=128, seed=3, debug=True)
    for x, y in zip(a, b):
        same_bytes(x, y)


def test_invalid_arguments_are_refused(capi, scenes):
    sc = scenes[(64, 0.3, 3)][0]
    prob = [(sc["X"], sc["uv"])]
    K = sc["K"]

    def refused(**kw):
        Kx = kw.pop("K", K)
        with pytest.raises(capi.SfmbaError, match="rc=1:"):
            capi.pnp_ransac(prob, Kx, **kw)

    for n_hyp in (0, -1, 65537):
        refused(n_hyp=n_hyp)
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        refused(threshold_px=thr)
    for idx in (0, 4):
        for bad in (0.0, -2500.0, float("nan"), float("inf")):
            Kb = K.copy().reshape(9)
            Kb[idx] = bad
            refused(K=Kb.reshape(3, 3))
    refused(max_refine_iters=-1)
    # a decreasing prob_ptr, through the raw entry point
    L = capi.lib()
    ptr = np.array([0, 40, 20], np.int64)
    xyz, uv = np.ascontiguousarray(sc["X"]), np.ascontiguousarray(sc["uv"])
    K32 = np.ascontiguousarray(K, np.float32).reshape(9)
    pose, inl = np.zeros(24), np.zeros(64, np.uint8)
    res = (C.c_byte * 48)()
    fp = C.POINTER(C.c_float)
    rc = L.sfmba_pnp_ransac(C.c_int(0), C.c_int(2), ptr.ctypes.data_as(C.POINTER(C.c_int64)), xyz.ctypes.data_as(fp), uv.ctypes.data_as(fp),
                            K32.ctypes.data_as(fp), C.c_int(100), C.c_float(10.0), C.c_uint64(0), C.c_int(20),
                            pose.ctypes.data_as(C.POINTER(C.c_double)), inl.ctypes.data_as(C.POINTER(C.c_ubyte)), res, None, None)
    assert rc == 1
    assert capi.pnp_ransac(prob, K, n_hyp=65536, max_refine_iters=0)[0]["status"] == 0      # the largest n_hyp is accepted


# ---- 8. the shim's inlier-ratio gate ------------------------------------------------------------------------------------
def test_shim_gate(capfd):
    import sfm_toy_library_amd as sfm
    before = np.arange(12, dtype=np.float32).reshape(3, 4)
    sc = sfm.make_pnp_scene(300, 0.6, 10)
    capfd.readouterr()
    ok, pose = shim_pose(sc["K"], sc["X"], sc["uv"], before)
    err = capfd.readouterr().err
    assert not ok and np.array_equal(pose, before)
    m = re.search(r"Inliers ratio is too small: (\d+) / (\d+)", err)
    assert m and int(m.group(2)) == 300 and int(m.group(1)) < 150
    sc = sfm.make_pnp_scene(300, 0.3, 11)
    ok, pose = shim_pose(sc["K"], sc["X"], sc["uv"], before)
    assert ok
    assert np.abs(pose[:, :3] - sc["R"]).max() < 0.01 and np.abs(pose[:, 3] - sc["t"]).max() < 0.1


# ---- 9. a list past the score kernel's grid cap -------------------------------------------------------------------------
# k_pnp_score caps grid.y at PNP_MAX_CHUNK_BLOCKS; past PNP_MAX_CHUNK_BLOCKS * PNP_CHUNK points a block walks several chunks and
# reuses its LDS tile.  LONG_N: two blocks make a second trip, and the last chunk, reached on that trip, holds ONE point.
# 65 hypotheses: the second tile has one live lane.  The refinement's fixed-order sums then run over about 46 000 inliers.
MAX_CHUNK_BLOCKS = int(re.search(r"PNP_MAX_CHUNK_BLOCKS\s*=\s*(\d+)", open(os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "pnp_ransac.h")).read()).group(1))
FIRST_TRIP = MAX_CHUNK_BLOCKS * CHUNK
LONG_N = FIRST_TRIP + CHUNK + 1
LONG_SEED = 21
LONG_HYP = 65


@pytest.fixture(scope="module")
def long_scene():
    """(scene, the oracle's answer for seed 0): computed once, never modified.  The tail must matter: the oracle's winner has more
    inliers past the first trip than border points, so a count without them cannot pass."""
    import sfm_toy_library_amd as sfm
    sc = sfm.make_pnp_scene(LONG_N, 0.3, LONG_SEED)
    want = po.pnp_ransac(sc["X"], sc["uv"], sc["K"], n_hyp=LONG_HYP, threshold_px=THR, seed=0, max_refine_iters=0)
    assert want["status"] == 0
    tail, border = int(want["inlier"][FIRST_TRIP:].sum()), po.border_points(want["pose"], sc["X"], sc["uv"], sc["K"], THR)
    print("front_end_edges pnp long list: n %d, oracle winner %d with %d inliers, %d of them past the first trip, %d border points"
          % (LONG_N, want["best_hypothesis"], want["n_inliers"], tail, border))
    assert len(sc["X"]) == LONG_N == FIRST_TRIP + CHUNK + 1 and tail > border and tail > 0.5 * (LONG_N - FIRST_TRIP)
    return sc, want


@pytest.fixture(scope="module")
def long_run(capi, long_scene):
    sc, _ = long_scene
    return capi.pnp_ransac([(sc["X"], sc["uv"])], sc["K"], n_hyp=LONG_HYP, debug=True)[0]


def test_long_list_counts_against_fp64_recount(long_scene, long_run):
    sc, want = long_scene
    r = long_run
    X, uv, K = sc["X"], sc["uv"], sc["K"]
    counts = r["hyp_count"]
    assert r["status"] == 0 and len(counts) == LONG_HYP and len(r["inlier"]) == LONG_N
    worst = 0.0
    for h in np.flatnonzero(counts >= 0):
        recount = int(po.inlier_mask(r["hyp_pose"][h], X, uv, K, THR).sum())
        border = po.border_points(r["hyp_pose"][h], X, uv, K, THR)
        worst = max(worst, abs(int(counts[h]) - recount) / max(border, 1))
        assert abs(int(counts[h]) - recount) <= border, (h, counts[h], recount, border)
    print("front_end_edges pnp long list: worst |count - fp64 recount| / border count over %d valid hypotheses: %.3f" % ((counts >= 0).sum(), worst))
    assert (counts >= 0).sum() > LONG_HYP // 2
    assert r["best_hypothesis"] == int(np.argmax(counts))                                # the first maximum
    assert int(r["inlier"].sum()) == r["n_inliers"] == int(counts[r["best_hypothesis"]])
    assert r["n_inliers"] >= want["n_inliers"] - po.border_points(want["pose"], X, uv, K, THR)
    assert int(r["inlier"][FIRST_TRIP:].sum()) > 0.5 * (LONG_N - FIRST_TRIP)


def test_long_list_refinement_against_oracle(capi, long_scene, long_run):
    sc, _ = long_scene
    r = long_run
    X, uv, K = sc["X"].astype(np.float64), sc["uv"].astype(np.float64), sc["K"]
    start, mask = r["hyp_pose"][r["best_hypothesis"]], r["inlier"]
    pose, cost, iters, status = po.refine(start, X[mask], uv[mask], K, 20)
    print("front_end_edges pnp long list: refinement over %d inliers: |pose - oracle| %.2e, cost relative %.2e, iterations %d (oracle %d)"
          % (mask.sum(), np.abs(r["pose"] - pose).max(), abs(r["refine_cost"] - cost) / cost, r["refine_iters"], iters))
    assert status == 0 and r["status"] == 0 and mask.sum() > 40000
    assert 1 <= r["refine_iters"] <= 20 and r["refine_iters"] == iters
    assert np.abs(r["pose"] - pose).max() < 1e-8
    assert abs(r["refine_cost"] - cost) <= 1e-9 * cost


def test_long_list_in_a_mixed_batch(capi, scenes, long_scene):
    """grid.y is at its cap while three of the four problems have one chunk: 5, LONG_N, 300 and PNP_CHUNK points."""
    scs = [scenes[(5, 0.0, 2)][0], long_scene[0], scenes[(300, 0.45, 5)][0], scenes[(CHUNK, 0.3, 8)][0]]
    probs = [(s["X"], s["uv"]) for s in scs]
    assert [len(x) for x, _ in probs] == [5, LONG_N, 300, CHUNK]
    K, seed = scs[0]["K"], 41
    batch = capi.pnp_ransac(probs, K, n_hyp=LONG_HYP, seed=seed, debug=True)
    for p, prob in enumerate(probs):
        same_bytes(batch[p], capi.pnp_ransac([prob], K, n_hyp=LONG_HYP, seed=seed + p, debug=True)[0])
        assert batch[p]["status"] == 0


def test_long_list_two_calls_are_byte_equal(capi, long_scene, long_run):
    sc, _ = long_scene
    same_bytes(long_run, capi.pnp_ransac([(sc["X"], sc["uv"])], sc["K"], n_hyp=LONG_HYP, debug=True)[0])
