"""The step check of tests/linear_step_check.py has teeth: on oracle systems at d = 61, 253 and 1285 the exact step passes every bar,
and each planted error of the kind a reduced-system kernel could make -- while whole solves still converge -- is rejected."""
import numpy as np
import pytest

import linear_step_check as lsc

SIZES = (10, 42, 214)       # d = 61, 253, 1285
TOL = 1e-10


@pytest.fixture(scope="module", params=SIZES, ids=lambda n: "d%d" % (6 * n + 1))
def case(request, oracle, sfm):
    n = request.param
    prob = sfm.make_problem("small", n_cam=n, n_pt=15 * n, views=(2, 8), seed=4200 + n)
    step = oracle.lm_step(prob, 10.0)
    assert step["info"] == 0
    return prob, step, lsc.System(step["S"], step["rhs"])


def _rejected_by_cg(sys_, z, k=50):
    rho, bar = lsc.check_cg(sys_, z, TOL, k)
    return rho > bar


def _rejected_by_cholesky(sys_, z):
    r, bar = lsc.check_cholesky(sys_, z)
    return r > bar


def test_exact_step_passes(case):
    prob, step, sys_ = case
    z = step["z"]
    rho, bar = lsc.check_cg(sys_, z, TOL, 0)
    assert rho <= bar, (rho, bar)
    r, cbar = lsc.check_cholesky(sys_, z)
    assert r <= cbar, (r, cbar)
    err, sbar = lsc.check_step(sys_, z, z, cbar, 0.0)
    assert err == 0.0 and sbar > 0.0
    zc, k = lsc.numpy_pcg(sys_, TOL)
    rho, bar = lsc.check_cg(sys_, zc, TOL, k)
    assert rho <= bar, (rho, bar, k)
    err, sbar = lsc.check_step(sys_, zc, z, bar, 0.0)
    assert err <= sbar, (err, sbar)


def _solve(S, rhs):
    return np.linalg.solve(S, rhs)


def test_zeroed_off_diagonal_block_is_rejected(case):
    prob, step, sys_ = case
    S = step["S"].copy()
    nc = (sys_.d - 1) // 6
    # the first non-empty off-diagonal block of the last camera's block row
    i = nc - 1
    j = next(c for c in range(nc - 1) if np.abs(S[6 * i:6 * i + 6, 6 * c:6 * c + 6]).max() > 0.0)
    S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = 0.0
    S[6 * j:6 * j + 6, 6 * i:6 * i + 6] = 0.0
    z = _solve(S, step["rhs"])
    assert _rejected_by_cg(sys_, z) and _rejected_by_cholesky(sys_, z)


def test_dropped_last_strip_upper_part_is_rejected(case):
    prob, step, sys_ = case
    d = sys_.d
    r0 = 32 * ((d - 1) // 32)
    S = step["S"].copy()
    for r in range(r0, d):
        S[r, r + 1:] = 0.0           # the upper triangle of the last 32-row strip (a mis-masked diagonal tile) ...
        S[r + 1:, r] = 0.0           # ... and what a symmetric product mirrors from it
    z = _solve(S, step["rhs"])
    assert _rejected_by_cg(sys_, z) and _rejected_by_cholesky(sys_, z)


def test_cg_stopped_early_is_rejected(case):
    prob, step, sys_ = case
    z, k = lsc.numpy_pcg(sys_, 30 * TOL)
    rho, bar = lsc.check_cg(sys_, z, TOL, k)
    assert rho > bar, (rho, bar, k)


def test_focal_component_off_is_rejected(case):
    prob, step, sys_ = case
    z = step["z"].copy()
    z[-1] *= 1.0 + 1e-6
    assert _rejected_by_cg(sys_, z) and _rejected_by_cholesky(sys_, z)


def test_wrong_back_transform_is_rejected(case):
    prob, step, sys_ = case
    xt = sys_.xt(step["z"])
    # B^-1 x~ instead of B^-T x~: the transposed factor of k_cam_update's z = Linv^T x~
    z = lsc.apply_binv(sys_.L, sys_.lf, xt)
    assert _rejected_by_cg(sys_, z) and _rejected_by_cholesky(sys_, z)


def test_point_step_from_a_perturbed_z_is_rejected(case, oracle):
    prob, step, sys_ = case
    nobs = np.bincount(prob.obs_pt, minlength=prob.n_pt)
    ratio, _ = lsc.check_points(step["dpt"], step["dpt"], step["vcond"], step["dmag"], nobs, prob.pt3)
    assert ratio == 0.0
    rng = np.random.default_rng(7)
    zp = step["z"] * (1.0 + 1e-6 * rng.standard_normal(step["z"].shape))
    bad = oracle.lm_step(prob, 10.0, z=zp)["dpt"]
    ratio, i = lsc.check_points(bad, step["dpt"], step["vcond"], step["dmag"], nobs, prob.pt3)
    assert ratio > 1.0, (ratio, i)
