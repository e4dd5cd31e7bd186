"""The CPU restatement of the baseline-ranking contract (tests/homography_oracle.py; include/sfmba.h, sfmba_homography_ransac) checked
on its own, without a GPU: hand-computed homographies, the invalid quads, a numpy closed form and the device's own arithmetic
(csrc/homography_math.h compiled for the host) held to the SVD route, and on the scenes of tests/test_gpu_homography_ransac.py every
condition that test imposes on the device.

Measured here, with the oracle alone (the figures the GPU test's bounds rest on; ten scenes x 128 hypotheses, the tenth at
4096 x 3072):
  closed form against SVD   the device arithmetic on the host: 2.9e-10 px at worst at a hypothesis' own four sample points, 2.8e-12
                            of max|H| at worst between the two H; the numpy closed form of this file: 6.4e-10 px, 2.5e-12 (bounds
                            in the GPU test: 1e-6 px and 1e-6; a lost factor or a wrong determinant order is off by pixels)
  fp32 decision             the division-free fp32 form flipped no decision against fp64 on any scene (0 of 434 102 evaluations;
                            the GPU test allows the correspondences within 5e-3 px of the threshold)
  ill-conditioned           none: the determinant closest to the 1e-3 validity threshold is 8.7e-4 away (the rule starts at 1e-9)
  valid hypotheses          between 47 and 128 of 128 per scene
  consensus                 the winner holds every planted good correspondence on every scene at 100 hypotheses; the top count is
                            shared by at least 8 hypotheses on every scene, so the tie rule is exercised"""
import os
import re
import subprocess

import numpy as np
import pytest

import homography_oracle as ho
import pnp_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = int(re.search(r"HOM_CHUNK\s*=\s*(\d+)", open(os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "homography_ransac.h")).read()).group(1))
SCENES = [(4, 0.0, 1), (5, 0.0, 2), (64, 0.3, 3), (65, 0.3, 4), (300, 0.45, 5), (2000, 0.3, 6),
          (CHUNK - 1, 0.3, 7), (CHUNK, 0.3, 8), (CHUNK + 1, 0.3, 9)]
BIG = (2000, 0.3, 6, (4096, 3072))           # one scene repeated at a larger image, for the fp32 decision
THR = 10.0


@pytest.fixture(scope="module")
def solved(sfm):
    """scene key -> (scene, the oracle's answer at 128 hypotheses): computed once, never modified."""
    out = {}
    for key in SCENES + [BIG]:
        sc = sfm.make_homography_scene(*key[:3], **({"size": key[3]} if len(key) > 3 else {}))
        out[key] = (sc, ho.homography_ransac(sc["left"], sc["right"], n_hyp=128, threshold_px=THR))
    return out


def closed_form(l4, r4):
    """The contract's closed form in numpy: Hn = [b0 b1 b2] diag(dr_i / dl_i) adj([a0 a1 a2]) on the normalised points, de-normalised
    and scaled.  No validity test: the caller knows the quad is valid."""
    nl, cl, sl = ho.normalise(l4)
    nr, cr, sr = ho.normalise(r4)
    a = np.concatenate([nl, np.ones((4, 1))], axis=1)
    b = np.concatenate([nr, np.ones((4, 1))], axis=1)
    dl, dr = ho.triple_determinants(nl), ho.triple_determinants(nr)
    adj = np.stack([np.cross(a[1], a[2]), np.cross(a[2], a[0]), np.cross(a[0], a[1])])
    Hn = b[:3].T @ np.diag(dr[:3] / dl[:3]) @ adj
    Tl = np.array([[1 / sl, 0, -cl[0] / sl], [0, 1 / sl, -cl[1] / sl], [0, 0, 1]])
    Tri = np.array([[sr, 0, cr[0]], [0, sr, cr[1]], [0, 0, 1]])
    H = Tri @ Hn @ Tl
    return H / (H[2] @ np.array([cl[0], cl[1], 1.0]))


def test_scene_generator_follows_its_recipe(sfm):
    a, b = sfm.make_homography_scene(300, 0.45, 5), sfm.make_homography_scene(300, 0.45, 5)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["left"].dtype == np.float32 and a["right"].dtype == np.float32 and a["left"].shape == (300, 2) and a["right"].shape == (300, 2)
    rng = np.random.default_rng(5)
    th, sc = rng.normal(0, 0.05), 1.0 + rng.normal(0, 0.05)
    tr, pv = rng.normal(0, 30.0, 2), rng.normal(0, 2e-5, 2)
    want = np.array([[sc * np.cos(th), -sc * np.sin(th), tr[0]], [sc * np.sin(th), sc * np.cos(th), tr[1]], [pv[0], pv[1], 1.0]])
    assert np.array_equal(a["H"], want)
    assert np.all((a["left"] >= 0) & (a["left"] <= [1024, 768]))
    err, w = ho.transfer_errors(a["H"], a["left"], a["right"])
    good = ~a["bad"]
    assert np.all(w > 0) and err[good].max() < 3.5 and 0.3 < a["bad"].mean() < 0.6          # 0.5 px noise per axis; 45 % clutter
    assert np.all((a["right"][a["bad"]] >= 0) & (a["right"][a["bad"]] <= [1024, 768]))
    big = sfm.make_homography_scene(300, 0.45, 5, size=(4096, 3072))
    assert big["left"].max() > 2000 and np.all(big["left"] <= [4096, 3072])


def test_hand_checked_homographies():
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    H, info = ho.hypothesis(sq, sq)
    assert np.abs(H - np.eye(3)).max() < 1e-14
    # the unit square has four triangles of area 1/2: |d| = 1 / s^2 with s = 1/2, and both sides carry the same signs
    assert np.allclose(np.abs(info["dl"]), 4.0) and np.array_equal(np.sign(info["dl"]), np.sign(info["dr"]))
    H, _ = ho.hypothesis(sq * 100.0, sq * 100.0 + [7.0, -3.0])
    assert np.abs(H - np.array([[1, 0, 7], [0, 1, -3], [0, 0, 1.0]])).max() < 1e-12
    # the unit square under [[2,0,1],[0,3,2],[1,0,1]]: (0,0)->(1,2), (1,0)->(3,2)/2, (1,1)->(3,5)/2, (0,1)->(1,5); the third row at the
    # centre (1/2, 1/2) is 3/2, which the contract scales to 1
    quad = np.array([[1.0, 2.0], [1.5, 1.0], [1.5, 2.5], [1.0, 5.0]])
    H, _ = ho.hypothesis(sq, quad)
    assert np.abs(H - np.array([[2, 0, 1], [0, 3, 2], [1, 0, 1.0]]) / 1.5).max() < 1e-13
    assert np.abs(closed_form(sq, quad) - H).max() < 1e-13
    assert abs(H[2] @ [0.5, 0.5, 1.0] - 1.0) < 1e-15
    proj, w = ho.transfer(H, sq)
    assert np.abs(proj - quad).max() < 1e-13 and np.allclose(w, np.array([1, 2, 2, 1]) / 1.5)
    # the decision: a point 9.99 px off is in, 10.01 px off is out, and a point behind the line at infinity is out
    H = np.array([[1, 0, 0], [0, 1, 0], [-0.01, 0, 1.0]])
    left = np.array([[50.0, 0.0], [50.0, 0.0], [200.0, 0.0]])
    right = np.array([[100.0, 9.99], [100.0, 10.01], [-200.0, 0.0]])
    assert list(ho.inlier_mask(H, left, right, 10.0)) == [True, False, False]
    assert ho.border_points(H, left, np.array([[100.0, 10.004], [100.0, 10.006], [-200.0, 0.0]]), 10.0) == 1


def test_invalid_quads():
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    # three of the left points on a line: dl_3 = det[a0 a1 a2] = 0
    H, info = ho.hypothesis(np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [0.0, 1.0]]), sq)
    assert H is None and abs(info["dl"][3]) <= 1e-12 and np.all(np.abs(info["dl"][:3]) > 1e-3)
    H, _ = ho.hypothesis(sq, np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [0.0, 1.0]]))
    assert H is None
    # a bow-tie: two right points swapped, so two of the four triangles change their orientation
    H, info = ho.hypothesis(sq, sq[[0, 1, 3, 2]])
    assert H is None and np.all(np.abs(info["dr"]) > 1e-3) and sorted(np.sign(info["dl"] * info["dr"])) == [-1, -1, 1, 1]
    # a mirror image keeps ONE orientation (every product negative) and is valid
    H, info = ho.hypothesis(sq, sq * [-1.0, 1.0])
    assert H is not None and np.all(info["dl"] * info["dr"] < 0) and np.abs(H - np.diag([-1.0, 1.0, 1.0])).max() < 1e-14
    # four coinciding points have no scale; fewer than four correspondences have no sample
    H, info = ho.hypothesis(np.ones((4, 2)), sq)
    assert H is None and info["dl"] is None
    assert ho.sample(0, 0, 0, 3) is None and ho.sample(7, 3, 99, 2000) == pnp_oracle.sample(7, 3, 99, 2000) == [1597, 1342, 911, 1904]
    for l4, r4, status in ((sq[:0], sq[:0], 1), (sq[:3], sq[:3], 1), (np.array([[0.0, 0], [1, 1], [2, 2], [3, 3]]), sq, 2)):
        r = ho.homography_ransac(l4, r4, n_hyp=64)
        assert r["status"] == status and np.array_equal(r["H"], np.eye(3)) and not r["inlier"].any() and r["best_hypothesis"] == -1
        assert r["n_inliers"] == 0 and r["n_matches"] == len(l4) and np.all(r["hyp_count"] == -1)


def test_closed_form_agrees_with_the_svd_route(solved):
    worst_px, worst_rel = 0.0, 0.0
    for key, (sc, r) in solved.items():
        L, R = sc["left"].astype(np.float64), sc["right"].astype(np.float64)
        for s, H, info in r["hyp"]:
            if H is None:
                continue
            C = closed_form(L[s], R[s])
            rel = np.abs(C - H).max() / np.abs(H).max()
            err, w = ho.transfer_errors(C, L[s], R[s])
            assert rel < 1e-6 and err.max() < 1e-6 and np.all(w > 0), (key, s, rel, err)
            worst_px, worst_rel = max(worst_px, err.max()), max(worst_rel, rel)
    print("numpy closed form against SVD: %.2e px at the sample points, %.2e of max|H|" % (worst_px, worst_rel))


def test_oracle_meets_the_conditions_of_the_gpu_test(solved):
    closest = np.inf
    for key, (sc, r) in solved.items():
        L, R = sc["left"].astype(np.float64), sc["right"].astype(np.float64)
        left_out, worst = 0, 0.0
        for h, (s, H, info) in enumerate(r["hyp"]):
            assert s is not None and len(set(s)) == 4
            d = np.abs(np.concatenate([info["dl"], info["dr"]]))
            closest = min(closest, np.abs(d - ho.MIN_DET).min())
            if ho.ill_conditioned(info):
                left_out += 1
                continue
            assert (H is None) == (r["hyp_count"][h] < 0)
            if H is None:
                continue
            err, w = ho.transfer_errors(H, L[s], R[s])
            assert np.all(w > 0) and err.max() < 1e-6, (key, h, err)
            assert abs(H[2] @ [*L[s].mean(axis=0), 1.0] - 1.0) < 1e-12
            worst = max(worst, err.max())
            assert r["hyp_count"][h] == ho.inlier_mask(H, L, R, THR).sum()
        valid = int((r["hyp_count"] >= 0).sum())
        ties = int((r["hyp_count"] == r["hyp_count"].max()).sum())
        print("scene %s: valid %d / 128, worst own residual %.2e px, left out %d, hypotheses sharing the top count %d" % (key, valid, worst, left_out, ties))
        assert left_out <= 0.02 * 128
        assert 27 * 128 // 100 <= valid <= 128
        # winner rule, mask and counts
        assert r["status"] == 0 and r["best_hypothesis"] == int(np.argmax(r["hyp_count"])) and r["n_matches"] == len(L)
        assert r["inlier"].sum() == r["n_inliers"] == r["hyp_count"][r["best_hypothesis"]]
        assert np.array_equal(r["H"], r["hyp"][r["best_hypothesis"]][1])
        assert ties >= 2
        # consensus at 100 hypotheses, the number the GPU test scores
        r100 = ho.homography_ransac(L, R, n_hyp=100, threshold_px=THR)
        good = ~sc["bad"]
        assert (r100["inlier"] & good).sum() >= 0.98 * good.sum()
        assert np.array_equal(r100["hyp_count"], r["hyp_count"][:100])
    print("determinant closest to the validity threshold: %.2e away" % closest)
    assert closest > 1e-9


def test_oracle_batch_rule(solved):
    sc = solved[(64, 0.3, 3)][0]
    # pair p of a batch with seed s draws what pair 0 draws with seed s + p
    a = ho.homography_ransac(sc["left"], sc["right"], n_hyp=32, seed=41, p=3)
    b = ho.homography_ransac(sc["left"], sc["right"], n_hyp=32, seed=44, p=0)
    assert np.array_equal(a["H"], b["H"]) and np.array_equal(a["hyp_count"], b["hyp_count"])
    # repeated correspondences are legal: quads that pick the same point twice are invalid, the others are not
    idx = np.array([0, 0, 1, 1, 2, 3, 4, 5])
    r = ho.homography_ransac(sc["left"][idx], sc["right"][idx], n_hyp=64)
    assert r["status"] == 0 and np.all(np.isfinite(r["H"])) and (r["hyp_count"] < 0).any()


def test_no_cpu_fallback_without_device(sfm):
    from sfm_toy_library_amd import capi
    import __graft_entry__ as ge
    ge.build_hip()
    assert "sfmba_homography_ransac" in capi.SYMBOLS and hasattr(capi.lib(), "sfmba_homography_ransac")
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    sc = sfm.make_homography_scene(64, 0.3, 3)
    pl, pr, q, t = ho.scene_arrays(sc, 3)
    with pytest.raises(capi.SfmbaError, match="no HIP device"):
        capi.homography_ransac([pl, pr], [(0, 1)], ([0, 64], q, t))
    with pytest.raises(capi.SfmbaError, match="rc=1:"):          # arguments are checked before the device is looked for
        capi.homography_ransac([pl, pr], [(0, 1)], ([0, 64], q, t), n_hyp=0)
    with pytest.raises(capi.SfmbaError, match="rc=1:.*outside its image"):
        capi.homography_ransac([pl, pr], [(0, 1)], ([0, 64], q + len(pl), t))


def test_cpp_shim_exports_the_reference_signatures():
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    so = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    syms = subprocess.check_output(["nm", "-C", so]).decode()
    assert " T sfmtoylib::SfMStereoUtilities::findHomographyInliers(sfmtoylib::Features const&, sfmtoylib::Features const&, std::vector<cv::DMatch" in syms
    assert " T sfmtoylib::SfMFeatureMatching::sortViewsForBaseline(" in syms
    assert " T sfmba_shim_find_homography_inliers" in syms and " T sfmba_shim_sort_views_for_baseline" in syms
    hdr = open(os.path.join(ROOT, "sfm-toy-library_amd", "host", "SfMStereoUtilities.h")).read()
    assert "homography inliers, essential-matrix pose" not in hdr


def test_device_arithmetic_on_the_host_against_the_oracle(solved, tmp_path):
    """csrc/homography_math.h (what a lane of k_hom_hypotheses runs, and the fp32 decision of k_hom_score / k_hom_select) compiled
    for the host: the same samples, the same valid hypotheses, the Hs and the counts the GPU test asks of the device, on the ten
    scenes x 128 hypotheses."""
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path / "homography_math_host")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tools", "micro", "homography_math_host.hip")])
    worst_px, worst_rel, flips, evals = 0.0, 0.0, 0, 0
    for key, (sc, r) in solved.items():
        L, R = sc["left"].astype(np.float64), sc["right"].astype(np.float64)
        path = tmp_path / "scene.txt"
        with open(path, "w") as f:
            f.write("%d 128 0 0 %r\n" % (len(L), THR))
            for i in range(len(L)):
                f.write(" ".join(repr(float(v)) for v in (*L[i], *R[i])) + "\n")
        lines = subprocess.check_output([exe, str(path)]).decode().splitlines()
        assert len(lines) == 128
        for h, (s, H, info) in enumerate(r["hyp"]):
            t = lines[h].split()
            valid, ids, D, count = t[0] == "1", [int(v) for v in t[1:5]], np.array([float(v) for v in t[5:14]]).reshape(3, 3), int(t[14])
            assert ids == s, (key, h)
            if ho.ill_conditioned(info):
                continue
            assert valid == (H is not None), (key, h, info)
            if not valid:
                assert not D.any() and count == -1
                continue
            err, w = ho.transfer_errors(D, L[s], R[s])
            rel = np.abs(D - H).max() / np.abs(H).max()
            assert np.all(w > 0) and err.max() < 1e-6 and rel < 1e-6, (key, h, err, rel)
            worst_px, worst_rel = max(worst_px, err.max()), max(worst_rel, rel)
            want = int(ho.inlier_mask(D, L, R, THR).sum())
            assert abs(count - want) <= ho.border_points(D, L, R, THR), (key, h, count, want)
            flips += abs(count - want)
            evals += len(L)
    print("device arithmetic on the host against SVD: %.2e px at the sample points, %.2e of max|H|; fp32 counts off by %d in %d evaluations"
          % (worst_px, worst_rel, flips, evals))
