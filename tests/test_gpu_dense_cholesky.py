"""The exact dense solve (csrc/dense_cholesky.hip + chol_tile.h) held to LAPACK in each of its three forms (-m gpu): the info value at
every position a report can come from, the tile edges with the unreported pivot of the augmented row on both sides of zero, the
backward error against dpotrf / dpotrs on the same system, and the storage contract.  Everything goes through
capi.dense_spd_solve(A, b, method=0); the cases and their references are tests/dense_spd_cases.py, proved on the CPU by
tests/test_dense_spd_cases_cpu.py (which also checks that every table entry is a test id here).

The accuracy bar, eta_device <= 16 max(eta_lapack, u) with u = 1.1e-16 and eta the normwise backward error: both are O(u) backward-stable
algorithms that differ in summation order and blocking, which moves the constant, not the order.  Measured on an MI355X: at most 4.05 x
(profiles/dense_cholesky_forms.txt).  What the bar does NOT see is one lost Newton step on the reciprocal of the pivot chain (chol_tile.h,
SFMBA_CT_NEWTON=1): a build with it passes every case here, worst ratio 2.91, case by case indistinguishable from the shipped build.  One
step leaves the square of the estimate's error, at most 2.5e-15 and of one sign, on each 1 / pivot; the factor is then that of A - sum_j e_j^2
l_j l_j^T (trailing parts), a perturbation nearly parallel to A whose residual is nearly parallel to b: eta moves by about
mean(e_j^2) ||b|| / (||A|| ||x|| + ||b||), a few u at the very most, which is where the shipped build already is.  No factor separates the two."""
import numpy as np
import pytest

import dense_spd_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return c


def _solve(capi, A, b):
    """One call; A and b must come back untouched."""
    A0, b0 = A.copy(), b.copy()
    x, info, _ = capi.dense_spd_solve(A, b, method=0)
    assert np.array_equal(A, A0, equal_nan=True) and np.array_equal(b, b0)
    return x, info


# ---------------------------------------------------------------------------------------------
# C1: info
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.INFO_CASES, ids=dc.info_id)
def test_info_position(capi, case):
    """*info = the order of the first leading minor that is not positive definite, which is dpotrf's: from every 16-column panel position,
    from tiles after the first, from the last (partial) panel, in each form; with a negative diagonal entry (D) and with a positive one
    whose pivot fails only after the updates of the earlier block columns (S).  x is unspecified then."""
    n, p, kind = case
    B, _ = dc.info_matrix(n, p, kind)
    expected = dc.lapack_info(B)
    assert expected == p
    x, info = _solve(capi, B, dc.info_rhs(n))
    print("C1 %-16s %-5s info %d (dpotrf %d)" % (dc.info_id(case), dc.form_of(n), info, expected))
    assert info == expected


@pytest.mark.parametrize("case", dc.TWO_FAILURE_CASES, ids=lambda c: "n%d-p%d-p%d" % c)
def test_info_first_failure_wins(capi, case):
    n, p1, p2 = case
    B = dc.two_failure_matrix(n, p1, p2)
    expected = dc.lapack_info(B)
    assert expected == p1
    x, info = _solve(capi, B, dc.info_rhs(n))
    assert info == expected


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("case", dc.NONFINITE_CASES, ids=lambda c: "n%d-p%d" % c)
def test_info_nonfinite_diagonal(capi, case, value):
    """A NaN on the diagonal at p fails minor p: the rule of reference LAPACK (dpotf2 tests ajj <= 0 or disnan(ajj)).  +inf fails it by the
    project's own rule, not LAPACK's: chol_tile.h asks for a pivot that is "positive and finite", rank_one_sweep for dj <= 1.7e308.  The
    expected value is p as the long-double Cholesky and the CPU restatement give it (test_dense_spd_cases_cpu.py); scipy's dpotrf is not
    asked, optimised LAPACK builds drop the disnan test."""
    n, p = case
    x, info = _solve(capi, dc.nonfinite_matrix(n, p, value), dc.info_rhs(n))
    assert info == p


# ---------------------------------------------------------------------------------------------
# C3: backward error per form against LAPACK on the same system
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.ACCURACY_CASES, ids=dc.accuracy_id)
def test_backward_error_matches_lapack(capi, case):
    A, b, normA = dc.accuracy_system(*case)
    x_ref, info_ref, eta_ref = dc.lapack_solve(A, b, normA)
    assert info_ref == 0
    x, info = _solve(capi, A, b)
    assert info == 0
    e = dc.eta(A, b, x, normA)
    print("C3 n=%-5d %-5s %-8s kappa=%.0e eta_lapack=%.2e eta_device=%.2e ratio=%.2f" %
          (case[1], dc.form_of(case[1]), case[0], case[2], eta_ref, e, e / max(eta_ref, dc.U)))
    assert e <= dc.eta_bar(eta_ref), (e, eta_ref)


# ---------------------------------------------------------------------------------------------
# C2: tile edges, the augmented pivot 1 - |L^-1 b|^2 positive, negative and hugely negative
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", dc.EDGE_GROUPS, ids=lambda g: g[0])
def test_tile_edges_and_augmented_pivot(capi, group):
    """The right-hand side rides along as row d of the matrix; its pivot is not one of the matrix and must neither be reported nor
    disturb the solution when it is negative (|L^-1 b|^2 ~ 15 scale^2 here)."""
    worst = (0.0, None)
    failures = []
    for n in group[1]:
        A, b1, normA = dc.edge_system(n)
        Al = A.astype(np.longdouble)
        for scale in dc.EDGE_SCALES:
            b = scale * b1
            x_ref, info_ref, eta_ref = dc.lapack_solve(A, b, normA)
            assert info_ref == 0
            x, info = _solve(capi, A, b)
            e = dc.eta(Al, b, x, normA) if info == 0 and np.all(np.isfinite(x)) else np.inf
            ratio = e / max(eta_ref, dc.U)
            worst = max(worst, (ratio, (n, scale)))
            if info != 0 or not e <= dc.eta_bar(eta_ref):
                failures.append((n, scale, info, e, eta_ref))
    print("C2 %-14s worst eta_device / max(eta_lapack, u) = %.2f at n, scale = %s" % (group[0], worst[0], worst[1]))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------
# C4: storage contract
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 200, 2600])
def test_only_the_upper_triangle_is_read_and_the_result_is_reproducible(capi, n):
    """include/sfmba.h: A is symmetric, row-major, and only its upper triangle is read.  Each tile has one writer and no sum goes through an
    atomic, so the same input gives the same bits, and so does a copy whose strict lower triangle is NaN."""
    A, b, _ = dc.edge_system(n)
    x1, info1 = _solve(capi, A, b)
    x2, info2 = _solve(capi, A, b)
    assert info1 == 0 and info2 == 0
    assert np.array_equal(x1, x2), np.abs(x1 - x2).max()
    An = A.copy()
    An[np.tril_indices(n, -1)] = np.nan
    x3, info3 = _solve(capi, An, b)
    assert info3 == 0
    assert np.array_equal(x1, x3), np.abs(x1 - x3).max()
