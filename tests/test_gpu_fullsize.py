"""GPU tests at sizes the oracle cannot cover in seconds, and ragged visibility.

* ragged: points seen by 1 .. 150 cameras (a point with more than 64 observations is swept by its wave in several
  rounds; a point with ONE observation has a rank-2 V block that only the LM damping makes invertible) -- trajectory
  identical to the oracle (fp64).
* BASELINE config 3 (200 cams / 100k pts / 1M obs): size-independent properties -- PCG and the exact Cholesky path reach
  the same cost, the residual vector re-evaluated at the solution reproduces the reported cost, a solve restarted from
  the solution stops after one iteration at the same cost (idempotence), F32J vs F64 within the 1e-4 px bar, the
  device-built pair lists give a symmetric reduced matrix whose blocks match a brute-force numpy rebuild on sampled
  camera pairs.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sfm():
    import sfm_toy_library_amd as m
    return m


@pytest.fixture(scope="module")
def capi(sfm):
    from sfm_toy_library_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle_py
    return oracle_py


def rms(cost, n_obs):
    return float(np.sqrt(2.0 * cost / n_obs))


def test_ragged_visibility_matches_oracle(capi, sfm, oracle):
    rng = np.random.default_rng(4242)
    base = sfm.make_problem("cfg2", n_cam=160, n_pt=300, views=(1, 150), seed=4242)
    # make sure the extremes are present: first point 1 observation, second 150
    counts = np.bincount(base.obs_pt, minlength=base.n_pt)
    assert counts.max() > 64 and counts.min() >= 1
    keep = np.ones(base.n_obs, dtype=bool)
    first = np.flatnonzero(base.obs_pt == 0)
    keep[first[1:]] = False
    prob = sfm.BAProblem(base.cam6, base.pt3, base.focal, base.obs_cam[keep], base.obs_pt[keep], base.obs_xy[keep])
    assert np.bincount(prob.obs_pt)[0] == 1
    cam_o, pt_o, f_o, s_o, tr_o = oracle.solve(prob, sfm.SfmbaOptions.defaults(max_seconds=0.0))
    for linear, tol in ((0, 0.0), (1, 1e-13)):
        cam, pt, f, s, tr = capi.solve(prob, capi.default_options(max_seconds=0.0, linear_solver=linear, pcg_tolerance=tol or 1e-6, pcg_anchored=0))
        assert s["termination_name"] == s_o["termination_name"]
        assert s["iterations"] == s_o["iterations"]
        assert abs(s["final_cost"] - s_o["final_cost"]) <= 1e-6 * s_o["final_cost"]
        assert len(tr) == len(tr_o)
        for a, b in zip(tr, tr_o):
            assert a["step_is_successful"] == b["step_is_successful"]
            assert np.isclose(a["cost"], b["cost"], rtol=1e-6)
        assert np.allclose(pt, pt_o, rtol=0, atol=1e-5)
        assert np.allclose(cam, cam_o, rtol=0, atol=1e-6)


@pytest.fixture(scope="module")
def cfg3(sfm):
    return sfm.make_problem("cfg3")


def test_cfg3_pcg_and_cholesky_agree_and_cost_is_reproducible(capi, sfm, cfg3):
    res = {}
    for linear in (0, 1):
        with capi.Problem(cfg3, precision=1) as P:
            s, tr = P.solve(capi.default_options(max_seconds=0.0, precision=1, linear_solver=linear))
            assert s["termination_name"] == "CONVERGENCE"
            r, cost = P.eval_residuals()
            # checksum of the residual vector at the returned parameters == the cost the solver reported
            assert np.isclose(0.5 * float(np.dot(r.ravel(), r.ravel())), s["final_cost"], rtol=1e-12)
            assert np.isclose(cost, s["final_cost"], rtol=1e-12)
            # idempotence: restarted from its own solution the solver stops at once, at the same cost
            cam, pt, f = P.get_params()
            P.set_params(cam, pt, f)
            s2, _ = P.solve(capi.default_options(max_seconds=0.0, precision=1, linear_solver=linear))
            assert s2["termination_name"] == "CONVERGENCE" and s2["iterations"] <= 1
            assert abs(s2["final_cost"] - s["final_cost"]) <= 1e-6 * s["final_cost"]
            res[linear] = s
    assert res[0]["iterations"] == res[1]["iterations"]
    assert abs(res[0]["final_cost"] - res[1]["final_cost"]) <= 1e-8 * res[0]["final_cost"]
    # noise is 0.5 px per coordinate: RMS over both coordinates ~ 0.5*sqrt(2) * sqrt(dof fraction)
    assert 0.6 < rms(res[1]["final_cost"], cfg3.n_obs) < 0.72


def test_cfg3_f32_jacobians_within_rms_bar(capi, sfm, cfg3):
    out = []
    for precision in (0, 1):
        with capi.Problem(cfg3, precision=precision) as P:
            s, _ = P.solve(capi.default_options(max_seconds=0.0, precision=precision, linear_solver=1))
            assert s["termination_name"] == "CONVERGENCE"
            out.append(s)
    assert out[0]["iterations"] == out[1]["iterations"]
    assert abs(rms(out[0]["final_cost"], cfg3.n_obs) - rms(out[1]["final_cost"], cfg3.n_obs)) < 1e-4     # BASELINE bar


def test_cfg3_reduced_system_blocks_against_bruteforce(capi, sfm, cfg3):
    """S = U - sum_points W_a V^-1 W_b^T rebuilt in numpy for a few camera pairs from the device Jacobian blocks."""
    with capi.Problem(cfg3, precision=0) as P:
        radius = 1e4
        S, rhs, scale = P.build_reduced(radius)
        jc, jp, jf = P.eval_jacobian()
    d = 6 * cfg3.n_cam + 1
    assert S.shape == (d, d)
    assert np.abs(S - S.T).max() <= 1e-12 * np.abs(S).max()
    sc = scale[:6 * cfg3.n_cam].reshape(-1, 6)          # Jacobi column scales of the camera parameters
    oc, op = cfg3.obs_cam, cfg3.obs_pt
    col2 = np.zeros((cfg3.n_pt, 3))
    np.add.at(col2, op, np.einsum("nri,nri->ni", jp, jp))
    sp = 1.0 / (1.0 + np.sqrt(col2))                      # ... and of the points (1 / (1 + ||column||))
    Jp = jp.reshape(-1, 2, 3) * sp[op][:, None, :]
    Jc = jc.reshape(-1, 2, 6) * sc[oc][:, None, :]
    V = np.zeros((cfg3.n_pt, 3, 3))
    np.add.at(V, op, np.einsum("nri,nrj->nij", Jp, Jp))
    dg = np.clip(np.einsum("nii->ni", V), 1e-6, 1e32) / radius
    V[:, [0, 1, 2], [0, 1, 2]] += dg
    Vinv = np.linalg.inv(V)
    rng = np.random.default_rng(7)
    for _ in range(6):
        ja, jb = sorted(rng.choice(cfg3.n_cam, size=2, replace=False))
        ia, ib = np.flatnonzero(oc == ja), np.flatnonzero(oc == jb)
        common, xa, xb = np.intersect1d(op[ia], op[ib], return_indices=True)
        qa, qb = ia[xa], ib[xb]
        Wa = np.einsum("nri,nrj->nij", Jc[qa], Jp[qa])          # 6x3 per shared point
        Wb = np.einsum("nri,nrj->nij", Jc[qb], Jp[qb])
        blk = -np.einsum("nij,njk,nlk->il", Wa, Vinv[common], Wb)
        got = S[6 * ja:6 * ja + 6, 6 * jb:6 * jb + 6]
        assert np.abs(got - blk).max() <= 1e-9 * max(1.0, np.abs(blk).max())


def test_one_shot_calls_recycle_device_memory(capi, sfm):
    """adjustBundle() re-creates the problem on every call (SfM.cpp:464-466): repeated one-shot solves must give
    identical results when their device arrays are carved out of recycled (dirty) arena chunks."""
    prob = sfm.make_problem("cfg2")
    capi.release_cache()
    ref = capi.solve(prob, capi.default_options(max_seconds=0.0, precision=1, linear_solver=1))
    other = sfm.make_problem("crazyhorse_like")
    for _ in range(3):
        capi.solve(other, capi.default_options(max_seconds=0.0))          # dirties the cached chunks with another problem
        again = capi.solve(prob, capi.default_options(max_seconds=0.0, precision=1, linear_solver=1))
        # (fp64 atomics make the summation order, hence the last bits, run-dependent; the truncated CG solve carries such a
        # perturbation into the parameters at the level of its own accuracy, ~1e-7: see DESIGN.md, CG stopping rule)
        assert again[3]["iterations"] == ref[3]["iterations"]
        assert abs(again[3]["final_cost"] - ref[3]["final_cost"]) <= 1e-11 * ref[3]["final_cost"]
        assert np.allclose(again[0], ref[0], rtol=0, atol=2e-7) and np.allclose(again[1], ref[1], rtol=0, atol=2e-7)
    assert capi.release_cache() > 0
    assert capi.release_cache() == 0


def test_streaming_cg_path_with_fp32_matrix(capi, sfm, monkeypatch):
    """d > 1280 (here 230 cameras, d = 1381): the CG matvec streams the preconditioned matrix from HBM; in fp32-Jacobian
    mode that matrix is stored in fp32.  Against the exact Cholesky solve and against fp64 storage."""
    prob = sfm.make_problem("cfg3", n_cam=230, n_pt=6000, seed=77)
    ref = capi.solve(prob, capi.default_options(max_seconds=0.0, precision=1, linear_solver=0))
    out = {}
    for mode in ("0", "1"):
        out[mode] = capi.solve(prob, capi.default_options(max_seconds=0.0, precision=1, linear_solver=1, pcg_f32_matrix=1 if mode == "1" else -1))
    for mode in ("0", "1"):
        r = out[mode]
        assert r[3]["termination_name"] == ref[3]["termination_name"] == "CONVERGENCE"
        assert r[3]["iterations"] == ref[3]["iterations"]
        assert abs(r[3]["final_cost"] - ref[3]["final_cost"]) <= 1e-9 * ref[3]["final_cost"]
        assert np.abs(r[0] - ref[0]).max() < 2e-6 and np.abs(r[1] - ref[1]).max() < 2e-6
    assert abs(out["0"][3]["linear_iters"] - out["1"][3]["linear_iters"]) <= 3


def test_gauge_coarse_space_cuts_cg_iterations_and_gauge_drift(capi, sfm, cfg3, monkeypatch):
    """Two-level preconditioner (8 analytic gauge vectors as a coarse space, pcg_common.h): same LM trajectory, at most
    10 CG iterations per LM iteration at cfg 3 (was 17-20), and the truncation error no longer sits in the gauge directions:
    parameters within 5e-8 of the exact Cholesky solve (plain block-Jacobi at the same tolerance: 2e-7)."""
    ref = capi.solve(cfg3, capi.default_options(max_seconds=0.0, precision=1, linear_solver=0))
    res = {}
    for coarse in ("0", "1"):
        res[coarse] = capi.solve(cfg3, capi.default_options(max_seconds=0.0, precision=1, linear_solver=1, pcg_coarse_space=1 if coarse == "1" else -1))
    for coarse in ("0", "1"):
        r = res[coarse]
        assert r[3]["termination_name"] == "CONVERGENCE" and r[3]["iterations"] == ref[3]["iterations"]
        assert abs(r[3]["final_cost"] - ref[3]["final_cost"]) <= 1e-10 * ref[3]["final_cost"]
    its0, its1 = res["0"][3]["linear_iters"], res["1"][3]["linear_iters"]
    assert its1 <= 10 * res["1"][3]["iterations"] and its1 < 0.6 * its0, (its0, its1)
    drift1 = max(np.abs(res["1"][0] - ref[0]).max(), np.abs(res["1"][1] - ref[1]).max())
    drift0 = max(np.abs(res["0"][0] - ref[0]).max(), np.abs(res["0"][1] - ref[1]).max())
    assert drift1 < 5e-8 and drift1 < drift0, (drift0, drift1)


def test_coarse_space_with_degenerate_camera_sets(capi, sfm, oracle, monkeypatch):
    """Fewer cameras than gauge freedoms / tiny systems: dependent gauge vectors are dropped, the solve is unaffected."""
    for name, kw in (("tiny", {}), ("cfg2", dict(n_cam=2, n_pt=300, views=2, seed=5)), ("cfg2", dict(n_cam=3, n_pt=300, views=3, seed=6))):
        prob = sfm.make_problem(name, **kw)
        want = oracle.solve(prob, sfm.SfmbaOptions.defaults(max_seconds=0.0))
        got = capi.solve(prob, capi.default_options(max_seconds=0.0, linear_solver=1, pcg_tolerance=1e-12, pcg_anchored=0))
        assert got[3]["termination_name"] == want[3]["termination_name"]
        assert got[3]["iterations"] == want[3]["iterations"]
        assert abs(got[3]["final_cost"] - want[3]["final_cost"]) <= 1e-8 * max(want[3]["final_cost"], 1e-30)


def test_deterministic_mode_is_bitwise_reproducible(capi, sfm, cfg3, monkeypatch):
    """SFMBA_DETERMINISTIC=1 (a determinism bound): every accumulator has a single writer per launch or a fixed
    summation order, so two solves of the same problem -- resident re-solves and freshly built problems alike -- agree in
    every bit of every parameter and of the per-iteration trace.  The default mode (fp64 atomics into 64 slots) agrees with
    it to rounding."""
    monkeypatch.setenv("SFMBA_DETERMINISTIC", "1")
    opt = capi.default_options(max_seconds=0.0, precision=1, linear_solver=1)
    runs = []
    for fresh in range(2):
        with capi.Problem(cfg3, precision=1) as P:
            for rep in range(2):
                P.reset()
                s, tr = P.solve(opt)
                runs.append((P.get_params(), s, tr))
    (cam0, pt0, f0), s0, tr0 = runs[0]
    for (cam, pt, f), s, tr in runs[1:]:
        assert np.array_equal(cam, cam0) and np.array_equal(pt, pt0) and f == f0
        assert s["final_cost"] == s0["final_cost"] and s["linear_iters"] == s0["linear_iters"]
        assert [r["cost"] for r in tr] == [r["cost"] for r in tr0]
        assert [r["trust_region_radius"] for r in tr] == [r["trust_region_radius"] for r in tr0]
    monkeypatch.setenv("SFMBA_DETERMINISTIC", "0")
    ref = capi.solve(cfg3, opt)
    assert ref[3]["iterations"] == s0["iterations"] and abs(ref[3]["final_cost"] - s0["final_cost"]) <= 1e-11 * s0["final_cost"]
    assert np.allclose(ref[0], cam0, rtol=0, atol=1e-7) and np.allclose(ref[1], pt0, rtol=0, atol=1e-7)
    # ... and the exact (Cholesky, fp64) configuration on a small problem, one-shot calls
    monkeypatch.setenv("SFMBA_DETERMINISTIC", "1")
    small = sfm.make_problem("cfg2")
    a = capi.solve(small, capi.default_options(max_seconds=0.0))
    b = capi.solve(small, capi.default_options(max_seconds=0.0))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3]["final_cost"] == b[3]["final_cost"]


def test_early_linearisation_launch_changes_nothing(capi, sfm, cfg3, monkeypatch):
    """run_solve enqueues the next linearisation's first kernel before it waits for the control kernel's verdict (the kernel checks
    the LM state itself).  Same kernels in the same order either way: the trajectory must not depend on the switch, also when the
    iteration limit cuts the solve short (no early launch is allowed past the limit) and when CG batches come up short (the early
    kernel must stand down while the iteration waits for more CG)."""
    for okw in (dict(), dict(max_iters=2), dict(pcg_max_iters=200, pcg_tolerance=1e-13, pcg_anchored=0)):
        out = {}
        for flag in ("1", "0"):
            out[flag] = capi.solve(cfg3, capi.default_options(max_seconds=0.0, linear_solver=1, precision=1, early_linearise=1 if flag == "1" else -1, **okw))
        (cam_a, pt_a, f_a, a, tr_a), (cam_b, pt_b, f_b, b, tr_b) = out["1"], out["0"]
        assert a["termination_name"] == b["termination_name"] and a["iterations"] == b["iterations"]
        assert abs(a["final_cost"] - b["final_cost"]) <= 1e-9 * b["final_cost"]
        assert [r["step_is_successful"] for r in tr_a] == [r["step_is_successful"] for r in tr_b]
        assert np.abs(cam_a - cam_b).max() < 1e-6 and np.abs(pt_a - pt_b).max() < 1e-6


def test_deferred_reset_is_seen_by_every_entry_point(capi, sfm):
    """sfmba_problem_reset() enqueues nothing: the next solve's first kernel restores the initial parameters, and every other entry
    point that looks at the parameters flushes the reset first."""
    prob = sfm.make_problem("small")
    opt = capi.default_options(max_seconds=0.0)
    with capi.Problem(prob) as P:
        r0, c0 = P.eval_residuals()
        s1, _ = P.solve(opt)
        cam1, pt1, f1 = P.get_params()
        assert s1["termination_name"] == "CONVERGENCE" and np.abs(pt1 - prob.pt3).max() > 0
        P.reset()
        cam, pt, f = P.get_params()                               # reset, then a read
        assert np.array_equal(cam, prob.cam6) and np.array_equal(pt, prob.pt3) and f == prob.focal
        P.solve(opt); P.reset()
        r, c = P.eval_residuals()                                 # reset, then an evaluation
        assert abs(c - c0) <= 1e-12 * c0 and np.array_equal(r, r0)     # (the cost is a sum of atomics: last bits vary)
        P.solve(opt); P.reset()
        s2, _ = P.solve(opt)                                      # reset, then a solve (restored inside its first kernel)
        cam2, pt2, f2 = P.get_params()
        assert s2["iterations"] == s1["iterations"] and abs(s2["final_cost"] - s1["final_cost"]) <= 1e-12 * s1["final_cost"]
        assert np.allclose(cam2, cam1, atol=1e-9) and np.allclose(pt2, pt1, atol=1e-9)
        P.reset(); P.set_params(cam1, pt1, f1)                    # reset, then new parameters: the reset must not come back
        cam, pt, f = P.get_params()
        assert np.array_equal(cam, cam1) and np.array_equal(pt, pt1) and f == f1
        s3, _ = P.solve(opt)
        assert s3["iterations"] <= 1 or s3["final_cost"] <= s1["final_cost"] * (1 + 1e-9)


def test_pair_pass_carries_long_blocks_in_fp64(capi, sfm):
    """Three cameras that all see all 30 000 points: every off-diagonal block of the reduced system is the sum of 30 000 pair terms
    (470 rounds of the wave-per-block pair pass).  In fp32-Jacobian mode the lane-local sums are flushed into fp64 every 64
    rounds, so the block must agree with the all-fp64 one to fp32 ROUND-OFF of its terms, not to a random walk of 470 of them."""
    prob = sfm.make_problem("cfg2", n_cam=3, n_pt=30000, views=(3, 3), seed=11)
    out = {}
    for prec in (0, 1):
        with capi.Problem(prob, precision=prec) as P:
            S, rhs, scale = P.build_reduced(1e4, capi.default_options(precision=prec))
            out[prec] = S
    blk64, blk32 = out[0][0:6, 6:12], out[1][0:6, 6:12]
    assert np.abs(blk64).max() > 0
    assert np.abs(blk32 - blk64).max() <= 3e-6 * np.abs(blk64).max()
