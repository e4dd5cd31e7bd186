"""tests/trace_row_check.py against the oracle itself (no GPU): the restatement reproduces the oracle's own trace rows, every case meets the
conditions the GPU test relies on, and the checker has teeth.

Restatement.  The oracle's trajectory is walked row by row (one thread: its runs then repeat bit for bit); the step of an ACCEPTED row is
the difference of the parameters the oracle returns, so the row is restated exactly and has to agree at the figures measured when the
checker was written, times ten: step norm 1.3e-10, cost change 2e-11, rho 3.4e-11, gradient maximum 1.1e-9, all relative.  Two kinds of
row need more room, and get it from what the number formats say, not from what they measured:
  * a cost change that is 1e-7 of the cost (the function-tolerance row of `ten`) cancels: it is held at the checker's own bar for a
    cost change, 1e-12 (cost_prev + cost_trial), and its rho is reported, not held;
  * the trial point of a row the oracle did NOT accept is not returned; it is rebuilt with oracle.lm_step, which repeats the solve's
    internal step to the conditioning of its reduced system (the step norm agrees inside its 1.3e-10).  A trial point that is off by
    eps = 1.3e-10 |s| moves the trial cost by at most |gradient(x_trial)|_2 eps: that is added to the cost-change bar of such rows."""
import numpy as np
import pytest

import trace_row_check as trc

CASES = ("ten", "rejected", "cams_1", "cams_2", "cams_65", "cams_401", "implicit_dup", "no_jacobi", "scaled_200", "point_max")
STEP_REL, CC_REL, RHO_REL, GMAX_REL = 1.3e-10, 2e-11, 3.4e-11, 1.1e-9

_walks = {}


def walk(sfm, oracle, case):
    if case not in _walks:
        _walks[case] = trc.oracle_walk(sfm, oracle, case)
    return _walks[case]


def _gradient_norm(lin):
    return float(np.sqrt((lin.g[0] ** 2).sum() + (lin.g[1] ** 2).sum() + lin.g[2] ** 2))


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_oracles_rows(sfm, oracle, case):
    prob, okw, first, last = trc.case_problem(sfm, oracle, case)
    row0, lin0, rows = walk(sfm, oracle, case)
    g0 = lin0.gradient_max(trc.TAU[0])
    report = ["%s row 0: cost %.2e gradient %.2e (maximum in the %s block)" % (case, abs(row0["cost"] - float(lin0.cost)) / row0["cost"],
                                                                               abs(row0["gradient_max_norm"] - g0["value"]) / g0["value"], g0["block"])]
    checks = [("row 0 cost", abs(row0["cost"] - float(lin0.cost)), trc.COST_REL * row0["cost"]),
              ("row 0 gradient", abs(row0["gradient_max_norm"] - g0["value"]), GMAX_REL * g0["value"])]
    held = []
    prev_gmax = row0["gradient_max_norm"]
    for row, lin, x_trial, summ in rows:
        k = row["iteration"]
        ref = trc.RowReference(oracle, lin, x_trial, 0)
        accepted = bool(row["step_is_successful"])
        lin_t = trc.Linearisation(oracle, prob, x_trial)
        cc_bar = max(CC_REL * abs(float(ref.cost_change)), float(ref.cost_change_bar))
        if not accepted:
            cc_bar += _gradient_norm(lin_t) * STEP_REL * float(ref.step_norm)
        checks.append(("row %d step_norm" % k, abs(row["step_norm"] - float(ref.step_norm)), STEP_REL * float(ref.step_norm)))
        checks.append(("row %d cost_change" % k, abs(row["cost_change"] - float(ref.cost_change)), cc_bar))
        tolerance_row = summ["termination_name"] == "CONVERGENCE" and not accepted
        if tolerance_row:
            assert row["relative_decrease"] == 0.0 and row["gradient_max_norm"] == prev_gmax, row
        else:
            name = "row %d rho" % k + ("" if ref.held and accepted else " (not held)")
            checks.append((name, abs(row["relative_decrease"] - float(ref.rho)), RHO_REL * abs(float(ref.rho))))
        if ref.held:
            held.append(k)
        if accepted:
            gm = lin_t.gradient_max(trc.TAU[0])
            checks.append(("row %d gradient" % k, abs(row["gradient_max_norm"] - gm["value"]), GMAX_REL * gm["value"]))
            prev_gmax = row["gradient_max_norm"]
        else:
            assert row["gradient_max_norm"] == prev_gmax, "a row that was not accepted reports the previous gradient"
    for name, m, bar in checks:
        report.append("  %-28s %.3e / %.3e = %.3f" % (name, m, bar, m / bar))
    report.append("  rows whose rho is held in fp64: %s" % held)
    print("\n".join(report))
    for name, m, bar in checks:
        if trc.is_held(name):
            assert m <= bar, "\n".join(report)
    # every row declared "held" has a fp64 rho bar <= 1e-6 |rho|
    assert set(trc.MUST_HOLD[case]) <= set(held), (case, held)
    assert all(first <= k <= last for k in trc.MUST_HOLD[case])


def test_the_rejected_case_has_rows_the_radius_depends_on(sfm, oracle):
    """within the rows used: at least three accepted rows with rho < 0.9 (below the saturation of the radius update at 0.937) and at least
    one valid unsuccessful row"""
    _, _, rows = walk(sfm, oracle, "rejected")
    assert len(rows) == trc.REJECTED_ROWS
    low = [r["iteration"] for r, _, _, _ in rows if r["step_is_successful"] and r["relative_decrease"] < 0.9]
    rejected = [r["iteration"] for r, _, _, _ in rows if r["step_is_valid"] and not r["step_is_successful"]]
    print("accepted with rho < 0.9:", low, "rejected:", rejected)
    assert len(low) >= 3 and len(rejected) >= 1
    assert rows[-1][3]["termination_name"] == "NO_CONVERGENCE"
    assert sum(k in trc.MUST_HOLD["rejected"] for k in low) >= 3


def test_point_max_has_its_gradient_maximum_in_the_point_block(sfm, oracle):
    row0, lin0, rows = walk(sfm, oracle, "point_max")
    g = lin0.gradient_max(trc.TAU[0])
    print(g["block"], g["index"], g["per_block"])
    assert g["block"] == "points" and g["index"] // 3 == 0
    # ... by a margin no bar of the GPU test reaches, and the focal block is nowhere near (no start was found where the focal entry leads)
    assert g["per_block"]["points"][0] > 2.0 * g["per_block"]["cameras"][0] > 2.0 * g["per_block"]["focal"][0]
    assert row0["gradient_max_norm"] == pytest.approx(g["value"], rel=GMAX_REL)


def test_cams_401_is_past_the_trial_pose_threshold():
    assert 401 >= trc.trial_pose_min_cams()


@pytest.mark.parametrize("case", ("ten", "rejected"))
def test_the_checker_has_teeth(sfm, oracle, case):
    """the oracle's own row against the restatement with one term removed: each comes out at more than 100 x its bar"""
    _, _, rows = walk(sfm, oracle, case)
    row, lin, x_trial, _ = rows[0]
    good = dict((n, (m, b)) for n, m, b in trc.compare_row(row, trc.RowReference(oracle, lin, x_trial, 0)))
    assert all(m <= b for m, b in good.values()), good
    no_focal = dict((n, (m, b)) for n, m, b in trc.compare_row(row, trc.RowReference(oracle, lin, x_trial, 0, drop="focal_step")))
    no_point = dict((n, (m, b)) for n, m, b in trc.compare_row(row, trc.RowReference(oracle, lin, x_trial, 0, drop="point_term")))
    print("focal entry left out of step_norm: %.3e / %.3e" % no_focal["step_norm"])
    print("point term left out of J s: model %.3e / %.3e, rho %.3e / %.3e" % (no_point["model"] + no_point["relative_decrease"]))
    assert no_focal["step_norm"][0] > 100.0 * no_focal["step_norm"][1]
    assert no_point["model"][0] > 100.0 * no_point["model"][1]
    assert no_point["relative_decrease"][0] > 100.0 * no_point["relative_decrease"][1]


def test_the_gradient_check_has_teeth(sfm, oracle):
    """point_max: the gradient taken over the cameras only misses the oracle's row 0 by more than 100 x the bar"""
    row0, lin0, _ = walk(sfm, oracle, "point_max")
    _, m, bar = trc.compare_gradient(row0["gradient_max_norm"], lin0.gradient_max(trc.TAU[0]))
    assert m <= bar
    _, m, bar = trc.compare_gradient(row0["gradient_max_norm"], lin0.gradient_max(trc.TAU[0], blocks=("cameras", "focal")))
    print("cameras only: %.3e / %.3e" % (m, bar))
    assert m > 100.0 * bar
