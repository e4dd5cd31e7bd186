"""The CPU restatement of the baseline-pose contract (tests/essential_oracle.py; include/sfmba.h, sfmba_essential_ransac) checked on
its own, without a GPU: the scene recipe, hand-built essential matrices and their four poses, the constraints every hypothesis must
satisfy, the device's own arithmetic (csrc/essential_math.h compiled for the host) held to the oracle hypothesis by hypothesis, and on
the scenes of tests/test_gpu_essential_ransac.py every condition that test imposes on the device.

Measured here (the figures the GPU test's bounds rest on; eleven scenes x 128 hypotheses, one planar, one at 4096 x 3072):
  oracle alone              det E and 2 E E^T E - tr(E E^T) E: 1.1e-15 at worst; Sampson distance at a hypothesis' own five points:
                            4.3e-11 px at worst; condition number of the eliminated block <= 5.7e6; 4.4 - 5.0 real solutions on
                            average, at most 6; 127 - 128 valid of 128.  Without the Newton polish of its solutions the oracle's
                            constraints were at 3.9e-10 and Horn's R orthonormal only to 2e-12.
  device arithmetic on the  same samples, same validity and the same number of real solutions on all 1408 hypotheses; E against the
  host against the oracle   oracle's: 3.0e-13 at worst of |E|_F = sqrt 2; its own five points: 1.7e-11 px at worst; constraints
                            8.9e-16.  (Before the device's Gauss-Newton polish: 1.2e-5 and 5e-6 on two hypotheses of the planar
                            scene -- the conditioning of the degree-10 polynomial's chart)
  the decision              residual in fp64, gradient sum in fp32: no decision differs from fp64 on any scene (0 of 998 144
                            evaluations by the host build, 0 by the numpy emulation; the GPU test allows the correspondences
                            within 5e-3 px of the threshold).  The all-fp32 form flipped none either, with a measured error of
                            7e-4 px at worst, but its worst-case bound is 8e-3 .. 1.5e-2 px on these scenes
  ill-conditioned           none on any scene (the rule: condition number > 1e10, selection gap < 1e-6, a solution within 1e-6 of
                            the real / complex decision, two real solutions within 1e-6)
  pose                      Horn's closed form against the SVD decomposition as a set of four: 1.0e-15; the device arithmetic's
                            candidates against the SVD's: 5.0e-16; the same candidate and the same in-front counts on every scene
  consensus                 at 128 hypotheses the winner keeps every planted good correspondence on the non-planar scenes (and
                            at most one clutter row before the pose, none after); rotation within 0.5 deg and translation within
                            0.8 deg of the planted pose; the top count is shared by 1 - 3 hypotheses on the scenes with >= 64
                            matches, by 64 and 128 on the two smallest, so the tie rule is exercised.  The planar scene's winner
                            is the plane's mirror solution: 225 inliers, 115 of them in front"""
import os
import re
import subprocess

import numpy as np
import pytest

import essential_oracle as eo
import pnp_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "essential_ransac.h")).read()
CHUNK = int(re.search(r"ESS_CHUNK\s*=\s*(\d+)", HDR).group(1))
SCENES = [(6, 0.0, 1), (7, 0.0, 2), (64, 0.3, 3), (65, 0.3, 4), (300, 0.45, 5), (2000, 0.3, 6),
          (CHUNK - 1, 0.3, 7), (CHUNK, 0.3, 8), (CHUNK + 1, 0.3, 9), (300, 0.3, 10, "planar"), (2000, 0.3, 6, (4096, 3072))]
THR = 1.0


def make_scene(sfm, key):
    kw = {}
    if len(key) > 3:
        kw = {"planar": True} if key[3] == "planar" else {"size": key[3]}
    return sfm.make_essential_scene(*key[:3], **kw)


@pytest.fixture(scope="module")
def solved(sfm):
    """scene key -> (scene, the oracle's answer at 128 hypotheses): computed once, never modified."""
    out = {}
    for key in SCENES:
        sc = make_scene(sfm, key)
        out[key] = (sc, eo.essential_ransac(sc["left"], sc["right"], sc["K"], n_hyp=128, threshold_px=THR))
    return out


def angle_deg(c):
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def constraint_residual(E):
    return max(abs(np.linalg.det(E)), np.abs(2.0 * E @ E.T @ E - np.trace(E @ E.T) * E).max())


def test_scene_generator_follows_its_recipe(sfm):
    a, b = sfm.make_essential_scene(300, 0.45, 5), sfm.make_essential_scene(300, 0.45, 5)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["left"].dtype == np.float32 and a["right"].dtype == np.float32 and a["left"].shape == (300, 2) and a["right"].shape == (300, 2)
    rng = np.random.default_rng(5)
    R = sfm.synthetic.rotvec_to_matrix(rng.normal(0, 0.1, 3))
    X = rng.uniform(-1, 1, (300, 3)) * [1.0, 0.7, 1.0] + [0.0, 0.0, 5.0]
    t = np.array([1.0, 0.1, 0.05]) / np.linalg.norm([1.0, 0.1, 0.05])
    assert np.array_equal(a["R"], R) and np.array_equal(a["t"], t)
    assert np.array_equal(a["K"], [[2500.0, 0, 512.0], [0, 2500.0, 384.0], [0, 0, 1]])
    good = ~a["bad"]
    assert 0.3 < a["bad"].mean() < 0.6
    # the planted E holds every good row at the reference's 1 px threshold: 0.2 px of noise per axis
    E = eo.cross_matrix(t) @ R
    d = eo.sampson_px(E, a["left"], a["right"], a["K"])
    assert d[good].max() < 1.0 and np.median(d[a["bad"]]) > 20.0
    proj = X[:, :2] / X[:, 2:3] * 2500.0 + [512.0, 384.0]
    assert np.abs(a["left"] - proj).max() < 1.2                               # 0.2 px Gaussian: 5 sigma and float32 rounding
    assert np.all((a["right"][a["bad"]] >= 0) & (a["right"][a["bad"]] <= [1024, 768]))
    # planar: the points lie on Z = 5 + 0.1 X
    pl = sfm.make_essential_scene(300, 0.3, 10, noise=0.0, planar=True)
    x = eo.normalise(pl["left"], pl["K"])
    Z = 5.0 / (1.0 - 0.1 * x[:, 0])                                          # Z = 5 + 0.1 x Z
    Y = np.concatenate([x * Z[:, None], Z[:, None]], axis=1) @ pl["R"].T + pl["t"]
    g = ~pl["bad"]
    assert np.abs(Y[g, :2] / Y[g, 2:3] * 2500.0 + [512.0, 384.0] - pl["right"][g]).max() < 1e-2
    big = sfm.make_essential_scene(300, 0.45, 5, size=(4096, 3072))
    assert big["left"].max() > 2500 and big["K"][0, 0] == 10000.0 and big["K"][0, 2] == 2048.0 and big["K"][1, 2] == 1536.0


def test_hand_checked_poses():
    # pure sideways translation, R = I: E = [t]x; t t^T = I - E E^T = diag(1, 0, 0); R(+t) = I and R(-t) = 2 t t^T - I
    t = np.array([1.0, 0.0, 0.0])
    E = eo.cross_matrix(t)
    assert np.array_equal(E, [[0, 0, 0], [0, 0, -1], [0, 1, 0]])
    twist = np.diag([1.0, -1.0, -1.0])
    want = [(np.eye(3), t), (twist, -t), (twist, t), (np.eye(3), -t)]
    for cands in (eo.horn_candidates(E), eo.svd_candidates(E)):
        for (R, tt), (Rw, tw) in zip(cands, want):
            assert np.abs(R - Rw).max() < 1e-15 and np.abs(tt - tw).max() < 1e-15
    # a quarter turn about the optical axis on top: E = [t]x R; cof(E) = t t^T R is no longer symmetric, so its transpose is caught
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    E = eo.cross_matrix(t) @ R
    assert np.array_equal(E, [[0, 0, 0], [0, 0, -1], [1, 0, 0]])
    Rt = np.diag([1.0, -1.0, -1.0]) @ R
    want = [(R, t), (Rt, -t), (Rt, t), (R, -t)]
    for cands in (eo.horn_candidates(E), eo.svd_candidates(E)):
        for (Rc, tt), (Rw, tw) in zip(cands, want):
            assert np.abs(Rc - Rw).max() < 1e-15 and np.abs(tt - tw).max() < 1e-15
    wrong = eo.horn_candidates(E, transposed_cofactor=True)
    assert np.abs(wrong[0][0] @ wrong[0][0].T - np.eye(3)).max() > 0.5         # the transposed cofactor gives no rotation at all
    assert np.abs(wrong[0][0] - R).max() > 0.5
    # depths: a point 4 in front of the left camera, the right camera one unit to the left of it (x' = x + t)
    x, xr = np.array([[0.25, 0.0]]), np.array([[0.5, 0.0]])
    lam, lamp, det = eo.depths(np.eye(3), t, x, xr)
    assert abs(lam[0] - 4.0) < 1e-12 and abs(lamp[0] - 4.0) < 1e-12 and det[0] > 0
    assert list(np.concatenate([eo.in_front(Rc, tc, x, xr) for Rc, tc in eo.horn_candidates(eo.cross_matrix(t))])) == [True, False, False, False]
    far = np.array([[0.25 + 1.0 / 60.0, 0.0]])                                 # depth 60: beyond the 50 of recoverPose
    assert not eo.in_front(np.eye(3), t, x, far)[0] and abs(eo.depths(np.eye(3), t, x, far)[0][0] - 60.0) < 1e-9
    # the Sampson decision: F = [t]x on unit intrinsics is the rectified pair, distance = |dy| / sqrt 2
    K = np.eye(3)
    left = np.array([[10.0, 5.0], [10.0, 5.0]])
    right = np.array([[20.0, 5.0 + 1.41], [20.0, 5.0 + 1.42]])
    assert list(eo.inlier_mask(eo.cross_matrix(t), left, right, K, 1.0)) == [True, False]
    assert list(eo.border_points(eo.cross_matrix(t), left, np.array([[20.0, 5.0 + 1.4142], [20.0, 5.0 + 1.43]]), K, 1.0)) == [True, False]


def test_sampler_and_degenerate_pairs(sfm):
    assert eo.sample(0, 0, 0, 5) is None
    s = eo.sample(7, 3, 99, 2000)
    assert s[:4] == pnp_oracle.sample(7, 3, 99, 2000) and len(set(s)) == 6     # the same stream, two entries further
    assert sorted(eo.sample(1, 0, 0, 6)) == [0, 1, 2, 3, 4, 5]
    K = sfm.make_essential_scene(6, 0.0, 1)["K"]
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    sc = sfm.make_essential_scene(64, 0.3, 3)
    s = np.arange(8.0)[:, None]
    line_l, line_r = np.array([[100.0, 200.0]]) + s * [[40.0, 20.0]], np.array([[150.0, 90.0]]) + s * s * [[8.0, 16.0]]
    same = np.zeros(8, int)
    for L, R, status in ((sc["left"][:0], sc["right"][:0], 1), (sc["left"][:5], sc["right"][:5], 1), (line_l, line_r, 2),
                         (sc["left"][same], sc["right"][same], 2)):
        r = eo.essential_ransac(L, R, K, n_hyp=64, seed=5)
        assert r["status"] == status and not r["E"].any() and np.array_equal(r["pose"], eye) and not r["inlier"].any()
        assert r["best_hypothesis"] == -1 and r["n_inliers"] == 0 and r["n_matches"] == len(L) and np.all(r["hyp_count"] == -1)
    r = eo.essential_ransac(sc["left"], sc["left"], K, n_hyp=64, seed=5)      # an image against itself: t = 0
    assert r["status"] in (2, 3) and not r["inlier"].any() and np.all(np.isfinite(r["E"]))
    # pair p of a batch with seed s draws what pair 0 draws with seed s + p
    a = eo.essential_ransac(sc["left"], sc["right"], K, n_hyp=16, seed=41, p=3)
    b = eo.essential_ransac(sc["left"], sc["right"], K, n_hyp=16, seed=44, p=0)
    assert np.array_equal(a["E"], b["E"]) and np.array_equal(a["hyp_count"], b["hyp_count"]) and np.array_equal(a["inlier"], b["inlier"])


def test_every_hypothesis_satisfies_its_constraints(solved):
    worst_c, worst_px, worst_cond = 0.0, 0.0, 0.0
    for key, (sc, r) in solved.items():
        L, R, K = sc["left"], sc["right"], sc["K"]
        nsol = r["hyp_nsol"][r["hyp_count"] >= 0]
        for s, E, ns, info in r["hyp"]:
            assert s is not None and len(set(s)) == 6
            if E is None:
                continue
            c, px = constraint_residual(E), eo.sampson_px(E, L[s[:5]], R[s[:5]], K).max()
            assert c < 1e-9 and px < 1e-6, (key, s, c, px)
            assert abs(np.linalg.norm(E) - np.sqrt(2.0)) < 1e-14 and E.ravel()[np.argmax(np.abs(E.ravel()))] > 0 and 1 <= ns <= 10
            worst_c, worst_px, worst_cond = max(worst_c, c), max(worst_px, px), max(worst_cond, info["cond"])
        print("scene %s: valid %d / 128, real solutions %.2f on average, at most %d" % (key, len(nsol), nsol.mean(), nsol.max()))
        assert len(nsol) >= 120
    print("oracle alone: constraints %.2e, own five points %.2e px, condition number <= %.2e" % (worst_c, worst_px, worst_cond))


def test_horn_closed_form_agrees_with_the_svd_as_a_set_of_four(solved):
    worst = 0.0
    for key, (sc, r) in solved.items():
        for _, E, _, _ in r["hyp"][:32]:
            if E is None:
                continue
            horn, svd = eo.horn_candidates(E), eo.svd_candidates(E)
            for R, t in horn:
                assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12 and abs(np.linalg.norm(t) - 1.0) < 1e-12
                d = min(max(np.abs(R - Rs).max(), np.abs(t - ts).max()) for Rs, ts in svd)
                assert d < 1e-12, (key, d)
                worst = max(worst, d)
            for (R, t), (Rs, ts) in zip(horn, svd):                            # and in the contract's order
                assert max(np.abs(R - Rs).max(), np.abs(t - ts).max()) < 1e-12
            assert np.abs(eo.cross_matrix(horn[0][1]) @ horn[0][0] - E).max() < 1e-12 and np.abs(eo.cross_matrix(horn[1][1]) @ horn[1][0] - E).max() < 1e-12
            assert np.abs(eo.cross_matrix(horn[2][1]) @ horn[2][0] + E).max() < 1e-12
    print("Horn's closed form against the SVD decomposition: %.2e" % worst)


def test_oracle_meets_the_conditions_of_the_gpu_test(solved):
    for key, (sc, r) in solved.items():
        L, R, K = sc["left"], sc["right"], sc["K"]
        flagged = np.array([eo.ill_conditioned(info) for _, _, _, info in r["hyp"]])
        for n_hyp in (1, 63, 64, 65, 100, 128):
            assert flagged[:n_hyp].sum() <= 0.02 * n_hyp, (key, n_hyp, flagged[:n_hyp].sum())
        counts = r["hyp_count"]
        for h, (s, E, ns, info) in enumerate(r["hyp"]):
            assert (E is None) == (counts[h] < 0)
            if E is not None:
                assert counts[h] == eo.inlier_mask(E, L, R, K, THR).sum()
        # winner rule, masks and counts
        best = r["best_hypothesis"]
        assert r["status"] == 0 and best == int(np.argmax(counts)) and r["n_matches"] == len(L)
        assert r["winner_mask"].sum() == r["n_inliers"] == counts[best] and np.array_equal(r["E"], r["hyp"][best][1])
        assert r["inlier"].sum() == r["n_pose_inliers"] <= r["n_inliers"] and not (r["inlier"] & ~r["winner_mask"]).any()
        # the device's decision against fp64, at every hypothesis
        flips = evals = 0
        for _, E, _, _ in r["hyp"]:
            if E is None:
                continue
            m32, m64 = eo.inlier_mask_device(E, L, R, K, THR), eo.inlier_mask(E, L, R, K, THR)
            assert not ((m32 != m64) & ~eo.border_points(E, L, R, K, THR)).any(), key
            flips += int((m32 != m64).sum())
            evals += len(L)
        # pose
        Rd, td = r["pose"][:, :3], r["pose"][:, 3]
        assert np.abs(Rd @ Rd.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rd) - 1.0) < 1e-12 and abs(np.linalg.norm(td) - 1.0) < 1e-12
        tR = eo.cross_matrix(td) @ Rd
        assert min(np.abs(tR - r["E"]).max(), np.abs(tR + r["E"]).max()) < 1e-12
        rp = eo.recover_pose(r["E"], L, R, K, r["winner_mask"], candidates=eo.horn_candidates)
        assert rp["pose_candidate"] == r["pose_candidate"] and np.array_equal(rp["front"], r["inlier"]) and not rp["border"].any()
        good = ~sc["bad"]
        ang_R, ang_t = angle_deg((np.trace(Rd.T @ sc["R"]) - 1.0) / 2.0), angle_deg(td @ sc["t"])
        ties = int((counts == counts.max()).sum())
        print("scene %s: winner %d with %d inliers (%d sharing the top count), candidate %d, %d in front, %d of %d planted good points kept, "
              "%d clutter rows kept, rotation %.3f deg, translation %.3f deg, fp32 flips %d of %d, flagged %d"
              % (key, best, r["n_inliers"], ties, r["pose_candidate"], r["n_pose_inliers"], int((r["inlier"] & good).sum()), int(good.sum()),
                 int((r["inlier"] & sc["bad"]).sum()), ang_R, ang_t, flips, evals, int(flagged.sum())))
        if len(L) >= 64 and "planar" not in key:
            assert ang_R < 2.0 and ang_t < 3.0, (key, ang_R, ang_t)
            assert (r["inlier"] & good).sum() >= 0.9 * good.sum()
        # 100 hypotheses are the first 100 of 128
        r100 = eo.essential_ransac(L, R, K, n_hyp=100, threshold_px=THR)
        assert np.array_equal(r100["hyp_count"], counts[:100])


def test_no_cpu_fallback_without_device(sfm):
    from sfm_toy_library_amd import capi
    import __graft_entry__ as ge
    ge.build_hip()
    assert "sfmba_essential_ransac" in capi.SYMBOLS and hasattr(capi.lib(), "sfmba_essential_ransac")
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    sc = sfm.make_essential_scene(64, 0.3, 3)
    pl, pr, q, t = eo.scene_arrays(sc, 3)
    with pytest.raises(capi.SfmbaError, match="no HIP device"):
        capi.essential_ransac([pl, pr], [(0, 1)], ([0, 64], q, t), sc["K"])
    with pytest.raises(capi.SfmbaError, match="rc=1:"):          # arguments are checked before the device is looked for
        capi.essential_ransac([pl, pr], [(0, 1)], ([0, 64], q, t), sc["K"], n_hyp=0)
    with pytest.raises(capi.SfmbaError, match="rc=1:.*fx and fy"):
        capi.essential_ransac([pl, pr], [(0, 1)], ([0, 64], q, t), np.diag([0.0, 2500.0, 1.0]))
    with pytest.raises(capi.SfmbaError, match="rc=1:.*outside its image"):
        capi.essential_ransac([pl, pr], [(0, 1)], ([0, 64], q + len(pl), t), sc["K"])


def test_cpp_shim_exports_the_reference_signatures():
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    so = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    syms = subprocess.check_output(["nm", "-C", so]).decode()
    assert (" T sfmtoylib::SfMStereoUtilities::findCameraMatricesFromMatch(sfmtoylib::Intrinsics const&, std::vector<cv::DMatch, std::allocator<cv::DMatch> > const&, "
            "sfmtoylib::Features const&, sfmtoylib::Features const&, std::vector<cv::DMatch, std::allocator<cv::DMatch> >&, cv::Matx<float, 3, 4>&, "
            "cv::Matx<float, 3, 4>&)") in syms
    assert " T sfmtoylib::SfMStereoUtilities::findCameraMatricesFromMatchBatch(sfmtoylib::Intrinsics const&, " in syms
    assert " T sfmba_shim_find_camera_matrices\n" in syms and " T sfmba_shim_find_camera_matrices_batch\n" in syms
    hdr = open(os.path.join(ROOT, "sfm-toy-library_amd", "host", "SfMStereoUtilities.h")).read()
    assert "stays on the" not in hdr and "findCameraMatricesFromMatchBatch" in hdr


def test_device_arithmetic_on_the_host_against_the_oracle(solved, tmp_path):
    """csrc/essential_math.h (what a lane of k_ess_hypotheses runs, the fp32 decision of k_ess_score / k_ess_select and the pose
    arithmetic of k_ess_select) compiled for the host: the same samples, the same valid hypotheses, the same number of real
    solutions, the Es, the counts and the pose the GPU test asks of the device, on the eleven scenes x 128 hypotheses."""
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path / "essential_math_host")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tools", "micro", "essential_math_host.hip")])
    worst_px, worst_rel, worst_c, worst_pose, flips, evals = 0.0, 0.0, 0.0, 0.0, 0, 0
    for key, (sc, r) in solved.items():
        L, R, K = sc["left"], sc["right"], sc["K"]
        path = tmp_path / "scene.txt"
        with open(path, "w") as f:
            f.write("%d 128 0 0 %r %r %r %r %r\n" % (len(L), THR, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])))
            for i in range(len(L)):
                f.write(" ".join(repr(float(v)) for v in (*L[i], *R[i])) + "\n")
        lines = subprocess.check_output([exe, str(path)]).decode().splitlines()
        assert len(lines) == 129
        left_out, scene_rel = 0, 0.0
        dev_counts = []
        for h, (s, E, nsol, info) in enumerate(r["hyp"]):
            t = lines[h].split()
            valid, ids, ns, D, count = t[0] == "1", [int(v) for v in t[1:7]], int(t[7]), np.array([float(v) for v in t[8:17]]).reshape(3, 3), int(t[17])
            dev_counts.append(count)
            assert ids == s, (key, h)
            if not valid:
                assert not D.any() and count == -1
            if eo.ill_conditioned(info):
                left_out += 1
                continue
            assert valid == (E is not None), (key, h, info)
            if not valid:
                continue
            assert ns == nsol, (key, h, ns, nsol)
            px, rel, c = eo.sampson_px(D, L[s[:5]], R[s[:5]], K).max(), np.abs(D - E).max(), constraint_residual(D)
            assert px < 1e-6 and rel <= 1e-6 * np.sqrt(2.0) and c < 1e-9, (key, h, px, rel, c)
            worst_px, worst_c, scene_rel = max(worst_px, px), max(worst_c, c), max(scene_rel, rel)
            m64 = eo.inlier_mask(D, L, R, K, THR)
            assert abs(count - int(m64.sum())) <= int(eo.border_points(D, L, R, K, THR).sum()), (key, h, count)
            flips += abs(count - int(m64.sum()))
            evals += len(L)
        assert left_out <= 0.02 * 128
        worst_rel = max(worst_rel, scene_rel)
        # the pose of the device arithmetic's own winner against the oracle's recoverPose on that E
        t = lines[128].split()
        assert t[0] == "pose"
        best, ok, cnt, cand, n_front = int(t[1]), int(t[2]), [int(v) for v in t[3:7]], int(t[7]), int(t[8])
        Rp, Rm, tt = (np.array([float(v) for v in t[9:18]]).reshape(3, 3), np.array([float(v) for v in t[18:27]]).reshape(3, 3),
                      np.array([float(v) for v in t[27:30]]))
        assert ok == 1 and best == int(np.argmax(dev_counts))
        D = np.array([float(v) for v in lines[best].split()[8:17]]).reshape(3, 3)
        svd = eo.svd_candidates(D)
        for (Rc, tc), (Rs, ts) in zip([(Rp, tt), (Rm, -tt), (Rm, tt), (Rp, -tt)], svd):
            d = max(np.abs(Rc - Rs).max(), np.abs(tc - ts).max())
            assert d < 1e-12, (key, d)
            worst_pose = max(worst_pose, d)
        mask = eo.inlier_mask(D, L, R, K, THR)
        rp = eo.recover_pose(D, L, R, K, mask)
        slack = int((eo.border_points(D, L, R, K, THR) | rp["border"]).sum())
        assert all(abs(a - b) <= slack for a, b in zip(cnt, rp["counts"])), (key, cnt, rp["counts"])
        assert cand == rp["pose_candidate"] and abs(n_front - rp["counts"][cand]) <= slack
        print("scene %s: E against the oracle's %.2e, winner %d, in-front counts %s (oracle %s)" % (key, scene_rel, best, cnt, list(rp["counts"])))
    print("device arithmetic on the host against the oracle: %.2e px at the sample points, %.2e between the Es, constraints %.2e, pose candidates "
          "against SVD %.2e; fp32 counts off by %d in %d evaluations" % (worst_px, worst_rel, worst_c, worst_pose, flips, evals))
