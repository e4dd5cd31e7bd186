"""The case tables of tests/dense_spd_cases.py are what they claim to be, checked without a GPU: every info case fails exactly where it
is declared to (LAPACK, an independent long-double Cholesky, and the project's own CPU restatement agree), every accuracy case is
solvable by LAPACK at rounding level, and tests/test_gpu_dense_cholesky.py is parametrised over exactly the tables: every entry is a
test id there (that the bodies drop nothing is for the reader to see: they hold no branch on a case)."""
import numpy as np
import pytest

import dense_spd_cases as dc

LONG_DOUBLE_MAX = 640       # first_bad_minor is O(n^3) in software long double


@pytest.mark.parametrize("case", dc.INFO_CASES, ids=dc.info_id)
def test_info_case_fails_where_declared(oracle, case):
    n, p, kind = case
    B, frac = dc.info_matrix(n, p, kind)       # asserts the side of frac itself; once more, explicitly:
    assert (frac >= 0.25) if kind == "S" else (frac < 0)
    assert dc.form_of(n) == ("small" if n <= 63 else "fused" if n <= 2559 else "panel")
    assert dc.lapack_info(B) == p
    if n <= LONG_DOUBLE_MAX:
        assert dc.first_bad_minor(B) == p
    x, info = oracle.dense_spd_solve(B, dc.info_rhs(n))
    assert info == p


def test_info_cases_cover_both_kinds_in_every_form():
    kinds = {(dc.form_of(n), kind) for n, p, kind in dc.INFO_CASES}
    assert kinds == {(f, k) for f in ("small", "fused", "panel") for k in "SD"}
    # a negative diagonal beyond the first tile, in both multi-tile forms
    assert (640, 65, "D") in dc.INFO_CASES and (2560, 65, "D") in dc.INFO_CASES


@pytest.mark.parametrize("case", dc.TWO_FAILURE_CASES, ids=lambda c: "n%d-p%d-p%d" % c)
def test_two_failures_first_wins(oracle, case):
    n, p1, p2 = case
    B = dc.two_failure_matrix(n, p1, p2)
    only2, _ = dc.break_minor(dc.base_matrix(n), p2)
    assert dc.lapack_info(only2) == p2          # the later failure is a failure on its own
    assert dc.lapack_info(B) == p1
    if n <= LONG_DOUBLE_MAX:
        assert dc.first_bad_minor(B) == p1
    assert oracle.dense_spd_solve(B, dc.info_rhs(n))[1] == p1


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("case", dc.NONFINITE_CASES, ids=lambda c: "n%d-p%d" % c)
def test_nonfinite_diagonal(oracle, case, value):
    """A pivot that is not a positive finite number fails the minor: reference LAPACK's rule for NaN (dpotf2: ajj <= 0 or disnan(ajj)), the
    project's own for +inf.  The LAPACK behind scipy is not consulted: optimised builds replace dpotrf by a kernel without the disnan test
    and return 0 here.  The long-double Cholesky and the project's CPU restatement state the rule."""
    n, p = case
    B = dc.nonfinite_matrix(n, p, value)
    if n <= LONG_DOUBLE_MAX:
        assert dc.first_bad_minor(B) == p
    assert oracle.dense_spd_solve(B, dc.info_rhs(n))[1] == p


@pytest.mark.parametrize("case", dc.ACCURACY_CASES, ids=dc.accuracy_id)
def test_accuracy_case_is_solved_by_lapack_at_rounding_level(case):
    A, b, normA = dc.accuracy_system(*case)
    x, info, e = dc.lapack_solve(A, b, normA)
    assert info == 0
    print("eta_lapack %-22s %.2e" % (dc.accuracy_id(case), e))
    assert e <= 4 * dc.U, e         # a backward-stable solve; measured 2e-17 .. 1.5e-16


def test_spectrum_class_has_the_condition_it_is_named_for():
    for kappa in (1e4, 1e8, 1e11):
        ev = np.linalg.eigvalsh(dc.spectrum_spd(129, kappa, 3))
        assert abs(ev[-1] - 1.0) < 1e-12 and abs(ev[0] * kappa - 1.0) < 1e-3


def test_graded_class_condition_of_the_unscaled_matrix():
    n, kappa = 129, 1e8
    rng = np.random.default_rng(5)
    G = rng.normal(size=(n, 16))            # graded_spd's first draw
    lam1 = np.linalg.eigvalsh(G.T @ G / 16).max()
    ev = np.linalg.eigvalsh(G @ G.T / 16 + lam1 / (kappa - 1) * np.eye(n))
    assert abs(ev[-1] / ev[0] / kappa - 1.0) < 1e-3
    A = dc.graded_spd(n, kappa, 5)
    assert np.array_equal(A, A.T)
    dg = np.sqrt(np.diag(A))
    assert dg.max() / dg.min() > 1e3        # graded over (nearly) four decades


def test_edge_system_norm_and_augmented_pivot():
    """||A||_2 from the Gram matrix is the norm, and b^T A^-1 b at scale 1 is above 1: the augmented pivot 1 - |L^-1 b|^2 is negative at
    scales 1 and 1e6, positive at 1e-6."""
    for n in (5, 63, 200, 1281):
        A, b, normA = dc.edge_system(n)
        assert abs(normA / np.abs(np.linalg.eigvalsh(A)).max() - 1.0) < 1e-12
        q = b @ np.linalg.solve(A, b)
        assert q > (1.5 if n > 5 else 0.0) and q * 1e-12 < 1e-9, (n, q)
    sizes = [n for _, g in dc.EDGE_GROUPS for n in g]
    assert len(sizes) == len(set(sizes)) and {1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 640, 2559, 2560, 2561, 2624, 3000} <= set(sizes)


# ---------------------------------------------------------------------------------------------
# the GPU file runs every entry
# ---------------------------------------------------------------------------------------------
def _param_values(fn, argname):
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize" and m.args[0] == argname:
            return list(m.args[1])
    raise AssertionError("%s is not parametrised over %r" % (fn.__name__, argname))


def test_gpu_file_runs_every_table_entry():
    import test_gpu_dense_cholesky as g
    assert _param_values(g.test_info_position, "case") == dc.INFO_CASES
    assert _param_values(g.test_info_first_failure_wins, "case") == dc.TWO_FAILURE_CASES
    assert _param_values(g.test_info_nonfinite_diagonal, "case") == dc.NONFINITE_CASES
    assert _param_values(g.test_backward_error_matches_lapack, "case") == dc.ACCURACY_CASES
    assert _param_values(g.test_tile_edges_and_augmented_pivot, "group") == dc.EDGE_GROUPS
    assert len(set(map(dc.info_id, dc.INFO_CASES))) == len(dc.INFO_CASES) == 30
    assert len(set(map(dc.accuracy_id, dc.ACCURACY_CASES))) == len(dc.ACCURACY_CASES) == 24
