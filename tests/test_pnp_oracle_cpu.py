"""The CPU restatement of the pose contract (tests/pnp_oracle.py; include/sfmba.h, sfmba_pnp_ransac) checked on its own, without a
GPU: it recovers the reference's known answer (find_camera_pose_from_2d3d_match, SfMUnitTests.cpp:194-216, inputs in
tests/golden/stereo_kat.json), its refinement agrees with scipy, and on the scenes of tests/test_gpu_pnp_ransac.py it meets every
condition that test imposes on the device.

Measured here, with the oracle alone (the figures the GPU test's bounds rest on):
  known answer          R to 3.8e-8, t to 2.4e-6 at hypothesis 0; all 128 hypotheses valid
  P3P residual          worst reprojection of a hypothesis' own three sample points over the six scenes x 128: 1.3e-6 px
                        (bound in the GPU test: 1e-3 px; a wrong root is off by pixels)
  ill-conditioned       none over the six scenes (closest pair of fourth-point errors: 0.23 px; the rule starts at 0.01 px)
  valid hypotheses      at least 125 of 128 per scene
  consensus             the winner holds every planted inlier on all six scenes at 100 hypotheses
  refinement            Gauss-Newton and scipy.optimize.least_squares agree to 4.2e-14 or better, in 4 - 5 steps"""
import json
import os
import subprocess

import numpy as np
import pytest

import pnp_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [(4, 0.0, 1), (5, 0.0, 2), (64, 0.3, 3), (65, 0.3, 4), (300, 0.45, 5), (2000, 0.3, 6)]
THR = 10.0


@pytest.fixture(scope="module")
def solved(sfm):
    """scene key -> (scene, the oracle's answer at 128 hypotheses): computed once, never modified."""
    out = {}
    for n, frac, seed in SCENES:
        sc = sfm.make_pnp_scene(n, frac, seed)
        out[(n, frac, seed)] = (sc, po.pnp_ransac(sc["X"], sc["uv"], sc["K"], n_hyp=128, threshold_px=THR))
    return out


def test_scene_generator_follows_its_recipe(sfm):
    a, b = sfm.make_pnp_scene(300, 0.45, 5), sfm.make_pnp_scene(300, 0.45, 5)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["X"].dtype == np.float32 and a["uv"].dtype == np.float32 and a["X"].shape == (300, 3) and a["uv"].shape == (300, 2)
    assert np.array_equal(a["K"], [[2500, 0, 512], [0, 2500, 384], [0, 0, 1]]) and np.array_equal(a["t"], [0.1, -0.2, 5.0])
    rng = np.random.default_rng(5)
    assert np.allclose(a["R"], sfm.synthetic.rotvec_to_matrix(rng.normal(0, 0.2, 3)), atol=0, rtol=0)
    pose = np.concatenate([a["R"], a["t"][:, None]], axis=1)
    err, z = po.pixel_errors(pose, a["X"], a["uv"], a["K"])
    good = ~a["bad"]
    assert np.all(z > 0) and err[good].max() < 3.5 and 0.3 < a["bad"].mean() < 0.6          # 0.5 px noise per axis; 45 % clutter
    assert np.all((a["uv"][a["bad"]] >= 0) & (a["uv"][a["bad"]] <= [1024, 768]))


def test_sampler_hand_computed():
    # splitmix64 seeded with 0: its first two published outputs
    assert po.mix(0) == 0xE220A8397B1DCDAF and po.mix(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    # (seed 0, p 0, h 0) over 12 points: key = mix(0); draws k = 0.. are mix(key ^ k) mod 12 = 3, 10, 1, 5
    key = 0xE220A8397B1DCDAF
    assert [po.mix(key ^ k) % 12 for k in range(4)] == [3, 10, 1, 5]
    assert po.sample(0, 0, 0, 12) == [3, 10, 1, 5]
    # (seed 7, p 3, h 99) over 2000 points: key = mix(10), draws mix(key ^ (99 << 8 | k)) mod 2000
    key = po.mix(10)
    assert [po.mix(key ^ ((99 << 8) | k)) % 2000 for k in range(4)] == [1597, 1342, 911, 1904]
    assert po.sample(7, 3, 99, 2000) == [1597, 1342, 911, 1904]
    # repeated draws are skipped, the order of first appearance is kept, and too few points or draws give no sample
    s = po.sample(1, 0, 5, 4)
    assert sorted(s) == [0, 1, 2, 3]
    draws = [po.mix(po.mix(1) ^ ((5 << 8) | k)) % 4 for k in range(64)]
    assert s == list(dict.fromkeys(draws))[:4]
    assert po.sample(0, 0, 0, 3) is None


def test_known_answer_of_the_reference():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "stereo_kat.json")))
    K, P, uv, X = np.array(d["K"]), np.array(d["P_left"]), np.array(d["left"]), np.array(d["points3d"])
    r = po.pnp_ransac(X, uv, K, n_hyp=128, threshold_px=THR)
    assert r["status"] == 0 and r["n_inliers"] == 12 and r["inlier"].all()
    dR, dt = np.abs(r["pose"][:, :3] - P[:, :3]).max(), np.abs(r["pose"][:, 3] - P[:, 3]).max()
    print("known answer: dR %.2e dt %.2e best %d valid %d" % (dR, dt, r["best_hypothesis"], (r["hyp_count"] >= 0).sum()))
    assert dR < 0.01 and dt < 0.1                              # the reference test's own tolerances
    assert (r["hyp_count"] >= 0).all()


def _left_jacobian_so3(w):
    """d exp([w]x) = exp([J_l(w) dw]x) exp([w]x)."""
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-8:
        return np.eye(3) + 0.5 * W + W @ W / 6.0
    return np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W


def _scipy_refine(start, X, uv, K):
    """MINPACK's Levenberg-Marquardt on d = (rotation vector applied on the left of the start's R, translation offset), with the
    analytic Jacobian (a finite-difference one stops at ~1e-7)."""
    from scipy.optimize import least_squares
    R0, t0 = start[:, :3], start[:, 3]

    def pose_of(d):
        return np.concatenate([po._exp_so3(d[:3]) @ R0, (t0 + d[3:])[:, None]], axis=1)

    def jac(d):
        J = po.jacobian(pose_of(d), X, K).copy()
        J[:, :3] = J[:, :3] @ _left_jacobian_so3(d[:3])
        return J

    sol = least_squares(lambda d: po.residuals(pose_of(d), X, uv, K), np.zeros(6), jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return pose_of(sol.x)


def test_refinement_agrees_with_scipy(solved):
    # Both minimise the same sum of squares from the same start; what separates them is the conditioning of the 6 x 6 normal
    # matrix times the fp64 rounding of the residuals (~1e6 x 1e-16 = 1e-10).  1e-9 per entry is ten times that and ten times under
    # the 1e-8 the device is held to.
    for key, (sc, r) in solved.items():
        X, uv, K = sc["X"].astype(np.float64), sc["uv"].astype(np.float64), sc["K"]
        mask, start = r["inlier"], r["hyp"][r["best_hypothesis"]][1]
        pose, cost, iters, status = po.refine(start, X[mask], uv[mask], K, 20)
        ref = _scipy_refine(start, X[mask], uv[mask], K)
        print("refine %s: |GN - scipy| %.2e in %d steps, cost %.6g" % (key, np.abs(pose - ref).max(), iters, cost))
        assert status == 0 and 1 <= iters < 20
        assert np.abs(pose - ref).max() < 1e-9
        assert cost <= po.cost(start, X[mask], uv[mask], K)
        assert np.array_equal(pose, r["pose"]) and cost == r["refine_cost"] and iters == r["refine_iters"]
        # the Jacobian against central differences of the residual
        J = po.jacobian(start, X[mask], K)
        for j in range(6):
            d = np.zeros(6)
            d[j] = 1e-6
            plus = np.concatenate([po._exp_so3(d[:3]) @ start[:, :3], (start[:, 3] + d[3:])[:, None]], axis=1)
            minus = np.concatenate([po._exp_so3(-d[:3]) @ start[:, :3], (start[:, 3] - d[3:])[:, None]], axis=1)
            num = (po.residuals(plus, X[mask], uv[mask], K) - po.residuals(minus, X[mask], uv[mask], K)) / 2e-6
            assert np.abs(num - J[:, j]).max() < 1e-4 * max(1.0, np.abs(J[:, j]).max())


def test_oracle_meets_the_conditions_of_the_gpu_test(solved):
    for key, (sc, r) in solved.items():
        X, uv, K = sc["X"].astype(np.float64), sc["uv"].astype(np.float64), sc["K"]
        left_out, worst, gap = 0, 0.0, np.inf
        for h, (s, pose, info) in enumerate(r["hyp"]):
            assert s is not None and len(set(s)) == 4
            if po.ill_conditioned(info):
                left_out += 1
                continue
            assert (pose is None) == (r["hyp_count"][h] < 0)
            if pose is None:
                continue
            R = pose[:, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1.0) < 1e-9
            err, z = po.pixel_errors(pose, X[s], uv[s], K)
            assert np.all(z > 0) and err[:3].max() < 1e-3 and err[3] <= info["e4"][0] + 1e-3
            worst = max(worst, err[:3].max())
            if len(info["e4"]) > 1:
                gap = min(gap, info["e4"][1] - info["e4"][0])
            assert r["hyp_count"][h] == po.inlier_mask(pose, X, uv, K, THR).sum()
        print("scene %s: valid %d / 128, worst own residual %.2e px, closest fourth-point pair %.3g px, left out %d" %
              (key, (r["hyp_count"] >= 0).sum(), worst, gap, left_out))
        assert left_out <= 0.02 * 128
        assert (r["hyp_count"] >= 0).sum() >= 120
        # winner rule, mask and counts
        assert r["status"] == 0 and r["best_hypothesis"] == int(np.argmax(r["hyp_count"]))
        assert r["inlier"].sum() == r["n_inliers"] == r["hyp_count"][r["best_hypothesis"]]
        # consensus at the 100 hypotheses the shim asks for
        r100 = po.pnp_ransac(X, uv, K, n_hyp=100, threshold_px=THR)
        good = ~sc["bad"]
        assert (r100["inlier"] & good).sum() == good.sum()
        assert np.abs(r100["pose"][:, :3] - sc["R"]).max() < 0.01 and np.abs(r100["pose"][:, 3] - sc["t"]).max() < 0.1
        assert 1 <= r100["refine_iters"] < 20
        off = po.pnp_ransac(X, uv, K, n_hyp=100, threshold_px=THR, max_refine_iters=0)
        assert off["refine_iters"] == 0 and np.array_equal(off["pose"], off["hyp"][off["best_hypothesis"]][1])


def test_oracle_batch_and_degenerate_problems(solved):
    sc = solved[(64, 0.3, 3)][0]
    X, uv, K = sc["X"], sc["uv"], sc["K"]
    # problem p of a batch with seed s draws what problem 0 draws with seed s + p
    a, b = po.pnp_ransac(X, uv, K, n_hyp=32, seed=41, p=3), po.pnp_ransac(X, uv, K, n_hyp=32, seed=44, p=0)
    assert np.array_equal(a["pose"], b["pose"]) and np.array_equal(a["hyp_count"], b["hyp_count"])
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    for Xd, ud, status in ((X[:0], uv[:0], 1), (X[:3], uv[:3], 1), (X[[0, 0, 1, 1]], uv[[0, 2, 1, 3]], 2)):
        r = po.pnp_ransac(Xd, ud, K, n_hyp=64)
        assert r["status"] == status and np.array_equal(r["pose"], ident) and not r["inlier"].any() and r["best_hypothesis"] == -1
    t = np.linspace(-1, 1, 40)
    Xl = (np.array([0.1, 0.2, 0.3]) + t[:, None] * np.array([1.0, 0.5, -0.25])).astype(np.float32)
    ul, _ = po.project(np.concatenate([sc["R"], sc["t"][:, None]], axis=1), Xl, K)
    r = po.pnp_ransac(Xl, ul.astype(np.float32), K, n_hyp=100)
    assert r["status"] in (0, 2, 3) and np.all(np.isfinite(r["pose"]))


def test_no_cpu_fallback_without_device(sfm):
    from sfm_toy_library_amd import capi
    import __graft_entry__ as ge
    ge.build_hip()
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    sc = sfm.make_pnp_scene(64, 0.3, 3)
    with pytest.raises(capi.SfmbaError, match="no HIP device"):
        capi.pnp_ransac([(sc["X"], sc["uv"])], sc["K"])
    with pytest.raises(capi.SfmbaError, match="rc=1:"):          # arguments are checked before the device is looked for
        capi.pnp_ransac([(sc["X"], sc["uv"])], sc["K"], n_hyp=0)


def test_cpp_shim_exports_the_reference_signature():
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    so = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    syms = subprocess.check_output(["nm", "-C", so]).decode()
    assert "sfmtoylib::SfMStereoUtilities::findCameraPoseFrom2D3DMatch(" in syms
    assert "sfmtoylib::Image2D3DMatch const&, cv::Matx<float, 3, 4>&)" in syms
    assert " T sfmba_shim_find_camera_pose" in syms


def test_device_arithmetic_on_the_host_against_the_oracle(solved, tmp_path):
    """csrc/pnp_math.h (what a lane of k_pnp_hypotheses runs) compiled for the host: the same samples, the same valid
    hypotheses, and conditions (a) - (c) of the GPU test, on the six scenes x 128 hypotheses."""
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path / "pnp_math_host")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tools", "micro", "pnp_math_host.hip")])
    for key, (sc, r) in solved.items():
        X, uv, K = sc["X"].astype(np.float64), sc["uv"].astype(np.float64), sc["K"]
        path = tmp_path / "scene.txt"
        with open(path, "w") as f:
            f.write("%d 128 0 0 %r %r %r %r\n" % (len(X), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])))
            for i in range(len(X)):
                f.write(" ".join(repr(float(v)) for v in (*X[i], *uv[i])) + "\n")
        lines = subprocess.check_output([exe, str(path)]).decode().splitlines()
        assert len(lines) == 128
        for h, (s, pose, info) in enumerate(r["hyp"]):
            t = lines[h].split()
            valid, ids, P = t[0] == "1", [int(v) for v in t[1:5]], np.array([float(v) for v in t[5:]]).reshape(3, 4)
            assert ids == s, (key, h)
            if po.ill_conditioned(info):
                continue
            assert valid == (pose is not None), (key, h, info)
            if not valid:
                assert not P.any()
                continue
            R = P[:, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1.0) < 1e-9
            err, z = po.pixel_errors(P, X[s], uv[s], K)
            assert np.all(z > 0) and err[:3].max() < 1e-3 and err[3] <= info["e4"][0] + 1e-3, (key, h, err, info)
