"""Every numeric column of the LM trace (sfmba_iteration), row by row, against the long-double restatement of tests/trace_row_check.py (-m gpu).

The trace is public API -- the library's stand-in for ceres::IterationSummary -- and its columns decide every exit and every trust-region
update, but only `cost` and `trust_region_radius` were compared with anything, and the radius does not stand in for rho: its update
saturates at x3 for rho > 0.937, which is every accepted row of the suite's usual problems.  Here a row is held AT THE DEVICE'S OWN STEP, so
no trajectory has to match an oracle solve, in either precision.  Per case and configuration, for k = 1 .. K: reset, step probe on,
solve(max_iters = k), then the trace, get_params and the probe.  Row k is held with x_prev = the parameters after the run to k - 1 (the
caller's input for k = 1) and x_trial = get_params after an accepted step, x_prev - scale z / - dpt from the probe otherwise; on accepted
rows the probe's reconstruction also has to equal get_params to 8 ulp, which pins the convention (not on the matrix-free handle, where
build_reduced, the source of `scale`, is refused: its one row is an accepted one).  Runs with K > 1 are on
SFMBA_CREATE_DETERMINISTIC handles, whose runs repeat bit for bit (rows 0 .. k - 1 of the run to k ARE the run to k - 1: asserted), so
x_prev is exactly the point row k was linearised at; plain handles are held at row 1.  A row that ends the run on a tolerance follows
Ceres' order: the columns computed before the exit are held, the rest are exactly 0, the gradient is the previous row's.

gradient_max_norm of a row is taken at the point the row REPORTS: the accepted point, also when the run ends on the iteration limit with
that row -- every run here does, which is what showed that the last row of such a run carried the previous point's gradient.

The routes: k_cam_update's partial sums per 64-camera workgroup (cams_1, cams_2, cams_65: the lone group, and a second workgroup with ONE
camera), the F32J unsharded route whose camera share of the model cost change is g . z (every F32J configuration), k_point_update's
closed form with G summed in the precision of the blocks, the trial pose from the parameters (cams_401: 401 >= SFMBA_TRIAL_POSE_MIN_CAMS,
asserted), the deterministic slot sums, the matrix-free handle (implicit_dup), no Jacobi scaling, translations of ~1e3 in the fp32 camera
record (scaled_200), and a gradient maximum in the POINT block (point_max).  No start was found where the focal entry is the gradient
maximum (with only the focal perturbed the camera block still leads 6.3e5 to 3.5e3): the focal gradient is reached through `model`,
`step_norm` and the right-hand side only.

Bars: trace_row_check's docstring; none is fitted.  The cost of rows k >= 1 is held at 1e-12 of itself plus the rounding of its fp64 residuals
(trace_row_check.cost_rounding); the ratio to 1e-12 alone is printed beside it.  rho is held where its bar is <= 1e-6 |rho| in fp64 (1e-3 |rho| in F32J) and printed
otherwise; trace_row_check.MUST_HOLD names the rows that have to be held in fp64.  Every test prints measured / bar per column and row
before it asserts, and leaves its worst ratios in WORST (tools/trace_columns_record.py writes them to profiles/trace_columns.txt)."""
import numpy as np
import pytest

import trace_row_check as trc

pytestmark = pytest.mark.gpu

F64, F32J = 0, 1
CHOL, PCG, AUTO = 0, 1, 2
DET, NO_PAIRS = 1, 4

# (case, precision, linear solver, create flags); a handle without SFMBA_CREATE_DETERMINISTIC is held at row 1 only
CONFIGS = []
for _p in (F64, F32J):
    for _l in (CHOL, PCG, AUTO):
        CONFIGS += [("ten", _p, _l, DET), ("ten", _p, _l, 0)]
    for _l in (CHOL, AUTO):
        CONFIGS.append(("rejected", _p, _l, DET))
    for _n in (1, 2, 65):
        for _l in (CHOL, PCG):
            CONFIGS.append(("cams_%d" % _n, _p, _l, DET))
    for _l in (PCG, AUTO):
        CONFIGS.append(("cams_401", _p, _l, 0))
    CONFIGS += [("implicit_dup", _p, AUTO, NO_PAIRS), ("implicit_dup", _p, AUTO, NO_PAIRS | DET)]
    CONFIGS.append(("point_max", _p, AUTO, DET))
CONFIGS += [("no_jacobi", F64, AUTO, DET), ("scaled_200", F32J, AUTO, 0)]

WORST = {}          # (case, column, precision) -> worst measured / bar


def _id(c):
    return "%s-%s-%s-%s" % (c[0], ("f64", "f32j")[c[1]], ("chol", "pcg", "auto")[c[2]], {0: "plain", 1: "det", 4: "nopairs", 5: "nopairs_det"}[c[3]])


@pytest.fixture(scope="module")
def capi(oracle):
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    oracle.set_num_threads(min(oracle.num_threads(), 16))
    return c


_lin_cache, _f32_obs = {}, {}


def _as_the_precision_sees_it(prob, case, precision):
    """SFMBA_PRECISION_F32J is defined with fp32 observation coordinates (include/sfmba.h; the reference's are cv::Point2f): the problem the
    mode solves, and the reference restates, has them rounded.  The synthetic problems' coordinates are fp32 values already; the doubled
    observations of implicit_dup (+ 0.25 px) are not all."""
    if precision == F64:
        return prob
    if case not in _f32_obs:
        q = prob.copy()
        q.obs_xy = prob.obs_xy.astype(np.float32).astype(np.float64)
        _f32_obs[case] = q
    return _f32_obs[case]


def _linearisation(oracle, prob, case, x):
    """the reference at a point, shared by the configurations that stand at the same point (all of them at the start)"""
    key = (case, id(prob), x[0].tobytes(), x[1].tobytes(), x[2])
    if key not in _lin_cache:
        _lin_cache[key] = trc.Linearisation(oracle, prob, x)
    return _lin_cache[key]


def _ulps(got, want, ref):
    got, want, ref = (np.asarray(a, dtype=np.float64).ravel() for a in (got, want, ref))
    return float((np.abs(got - want) / np.spacing(np.maximum(np.abs(ref), np.abs(want)))).max()) if got.size else 0.0


@pytest.mark.parametrize("config", CONFIGS, ids=_id)
def test_trace_columns(capi, sfm, oracle, config):
    case, precision, linear, flags = config
    prob, okw, _, last = trc.case_problem(sfm, oracle, case)
    ref_prob = _as_the_precision_sees_it(prob, case, precision)
    if not flags & DET:
        last = 1                # a plain handle does not repeat itself bit for bit: row 1 only
    if case == "cams_401":
        assert prob.n_cam >= trc.trial_pose_min_cams()
    tau = trc.TAU[precision]
    act = np.unique(prob.obs_cam)
    assert len(act) == prob.n_cam
    opt = lambda k: capi.default_options(max_seconds=0.0, precision=precision, linear_solver=linear, max_iters=k, **okw)
    report, checks = ["%s" % _id(config)], []

    def note(row, column, m, bar):
        checks.append(("row %d %s" % (row, column), m, bar))
        key = (case, column, ("fp64", "F32J")[precision])
        WORST[key] = max(WORST.get(key, 0.0), m / bar if bar > 0 else np.inf)

    with capi.Problem(prob, precision=precision, flags=flags) as P:
        scale = None
        if not flags & NO_PAIRS:
            scale = P.build_reduced(opt(1).initial_radius, opt(1))[2]
        x_prev = trc.params_of(prob)
        lin = _linearisation(oracle, ref_prob, case, x_prev)
        prev_rows, prev_gmax, held = None, None, []
        for k in range(1, last + 1):
            P.reset()
            P.set_step_probe(True)
            summ, tr = P.solve(opt(k))
            x_now = P.get_params()
            z, dpt, info = P.step_probe()
            assert len(tr) == k + 1 and info["family"] != 0, (summ, len(tr))
            if prev_rows is not None:
                assert tr[:k] == prev_rows, "the run to max_iters = %d is not the run to %d plus one row:\n%s\n%s" % (k, k - 1, tr[:k], prev_rows)
            if k == 1:
                # row 0: the initial evaluation
                g0 = lin.gradient_max(tau)
                note(0, "cost", abs(tr[0]["cost"] - float(lin.cost)), trc.COST_REL * float(lin.cost))
                _, m, bar = trc.compare_gradient(tr[0]["gradient_max_norm"], g0)
                note(0, "gradient_max_norm", m, bar)
                report.append("  row 0: the gradient maximum is in the %s block" % g0["block"])
                if case == "point_max":
                    assert g0["block"] == "points"
                prev_gmax = tr[0]["gradient_max_norm"]
                assert tr[0]["trust_region_radius"] == opt(1).initial_radius and summ["initial_cost"] == tr[0]["cost"]
            row = tr[k]
            assert row["iteration"] == k and row["step_is_valid"] == 1, row
            accepted = bool(row["step_is_successful"])
            rebuilt = trc.trial_from_step(prob, x_prev, scale, z, dpt) if scale is not None else None
            if accepted:
                x_trial = x_now
                if rebuilt is not None:
                    note(k, "probe: cameras (ulp)", _ulps(x_now[0], rebuilt[0], x_prev[0]), 8.0)
                    note(k, "probe: points (ulp)", _ulps(x_now[1], rebuilt[1], x_prev[1]), 8.0)
                    note(k, "probe: focal (ulp)", _ulps(x_now[2], rebuilt[2], x_prev[2]), 8.0)
            else:
                assert rebuilt is not None, "a step that was not accepted on a handle without build_reduced: no scale to rebuild the trial point from"
                x_trial = rebuilt
                assert all(np.array_equal(a, b) for a, b in zip(x_now[:2], x_prev[:2])) and x_now[2] == x_prev[2], "parameters moved without an accepted step"
            ref = trc.RowReference(oracle, lin, x_trial, precision)
            ended = summ["termination_name"] == "CONVERGENCE" and not accepted       # a tolerance ended the run on this row
            message = summ["message"]
            cols = dict((c, (m, b)) for c, m, b in trc.compare_row(row, ref))
            note(k, "step_norm", *cols["step_norm"])
            if ended and message.startswith("Parameter tolerance"):
                assert row["cost_change"] == 0.0 and row["relative_decrease"] == 0.0 and row["cost"] == tr[k - 1]["cost"], row
            else:
                note(k, "cost_change", *cols["cost_change"])
                if ended:
                    assert message.startswith("Function tolerance") or message.startswith("Minimum trust region radius"), summ
                if ended and message.startswith("Function tolerance"):
                    assert row["relative_decrease"] == 0.0 and row["cost"] == tr[k - 1]["cost"], row
                else:
                    note(k, "model", *cols["model"])
                    rho = [c for c in cols if c.startswith("relative_decrease")][0]
                    note(k, rho, *cols[rho])
                    if trc.is_held(rho):
                        held.append(k)
                    # the cost the row reports is the trial cost, formed directly from the trial residuals (also on a rejected row)
                    note(k, "cost", abs(row["cost"] - float(ref.cost_trial)), float(ref.cost_trial_bar))
                    note(k, "cost / (1e-12 cost) (not held)", abs(row["cost"] - float(ref.cost_trial)), trc.COST_REL * float(ref.cost_trial))
                    # the radius follows from the row's own rho (Ceres' update; exact in the device's own arithmetic up to the cube)
                    r0 = tr[k - 1]["trust_region_radius"]
                    if accepted:
                        want = min(opt(k).max_radius, r0 / max(1.0 / 3.0, 1.0 - (2.0 * row["relative_decrease"] - 1.0) ** 3))
                        note(k, "radius from rho", abs(row["trust_region_radius"] - want), 8.0 * np.spacing(want))
            if accepted:
                x_prev = x_now
                lin = _linearisation(oracle, ref_prob, case, x_prev)
                _, m, bar = trc.compare_gradient(row["gradient_max_norm"], lin.gradient_max(tau))
                note(k, "gradient_max_norm", m, bar)
                prev_gmax = row["gradient_max_norm"]
                assert summ["jacobian_evals"] == 1 + summ["successful_steps"], summ       # (as the oracle counts: one per point it stood at)
            else:
                assert row["gradient_max_norm"] == prev_gmax, "a row that was not accepted reports the previous row's gradient"
            at_minimum = summ["termination_name"] == "CONVERGENCE" and accepted      # the gradient tolerance, met at the accepted point
            if at_minimum:
                assert message.startswith("Gradient tolerance") and row["gradient_max_norm"] <= opt(k).gradient_tolerance, summ
            elif not ended:
                assert summ["termination_name"] == "NO_CONVERGENCE" and message.startswith("Maximum number of iterations"), summ
            prev_rows = tr
            if ended or at_minimum:
                break
    for name, m, bar in checks:
        report.append("  %-40s %.3e / %.3e = %.3g" % (name, m, bar, m / bar if bar > 0 else np.inf))
    report.append("  rows whose rho is held: %s" % held)
    print("\n".join(report))
    for name, m, bar in checks:
        if trc.is_held(name):
            assert m <= bar, "\n".join(report)
    if precision == F64:
        must = [k for k in trc.MUST_HOLD[case] if k <= last]
        assert set(must) <= set(held), "rows %s have to be held for rho, held: %s\n%s" % (must, held, "\n".join(report))
