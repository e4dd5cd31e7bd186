"""The linearisation of a handle that GREW through sfmba_problem_append, held to the oracle after every step (-m gpu).

tests/test_gpu_append.py registers the cameras in index order and looks at residuals and the end of an LM solve only; LM reaches the
same minimum with any reasonable descent direction (tests/test_gpu_linear_step.py), so a wrongly rebuilt structure can hide there.
Here every growth sequence of tests/append_cases.py -- cameras and points registered out of order, sort-key widths, chunk lengths, the
sort switch, the threaded host loop, duplicates, an append without observations -- is compared after EVERY step with the oracle on
step_problem(case, k): sizes, residuals in caller order, the Jacobian blocks per observation, and the reduced system S / rhs / scale
in the order include/sfmba.h states (active cameras by ascending caller index, focal last), plus a freshly created handle on the
same list.  The tolerances are the project's own for fresh handles: tests/test_gpu_parity.py (residuals, Jacobian blocks, reduced
system), tests/test_gpu_append.py (solve parity), tests/test_gpu_linear_step.py (one LM step with the step probe).  One figure is
measured instead (append_cases.MEASURED_TOL): where the only point has a single view the ORACLE is 7e-9 off, and that step is also
held to the same formulas in long double at the project's 1e-10.

Every step prints its worst deviation / tolerance ratios (appended and fresh handle against the oracle) before it asserts."""
import numpy as np
import pytest

import append_cases as ac
import linear_step_check as lsc

pytestmark = pytest.mark.gpu

F64, F32J = 0, 1
CHOL = 0
RADIUS = 1e4

_refs = {}


@pytest.fixture(scope="module")
def capi(oracle):
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    oracle.set_num_threads(min(oracle.num_threads(), 16))
    return c


def _ref(oracle, name, k, jac=False):
    """The oracle on step_problem(case, k): computed once per module, shared, never modified."""
    key = (name, k)
    if key not in _refs:
        sub = ac.step_problem(ac.make_case(name), k)
        r = dict(sub=sub, act=np.unique(sub.obs_cam))
        r["res"], r["cost"] = oracle.eval_residuals(sub)
        r["S"], r["rhs"], r["scale"], r["info"] = oracle.build_reduced(sub, RADIUS)
        _refs[key] = r
    r = _refs[key]
    if jac and "jc" not in r:
        _, r["jc"], r["jp"], r["jf"] = oracle.eval_jacobian(r["sub"])
    return r


def _grow(capi, name, precision=F64, flags=0):
    """Yields (k, handle) after create (k = 0) and after every append of the case; closes the handle at the end."""
    case = ac.make_case(name)
    P = capi.Problem(ac.step_problem(case, 0), precision=precision, flags=flags)
    try:
        yield 0, P
        for k in range(1, case.n_steps):
            P.append(*ac.step_new(case, k))
            yield k, P
    finally:
        P.close()


def _grown(capi, name, precision=F64, flags=0):
    """The handle after the last step (the caller closes it)."""
    case = ac.make_case(name)
    P = capi.Problem(ac.step_problem(case, 0), precision=precision, flags=flags)
    for k in range(1, case.n_steps):
        P.append(*ac.step_new(case, k))
    return P


def _reduced_tol(n_active, precision):
    """tests/test_gpu_parity.py::test_reduced_system_matches_oracle: 1e-10 up to 10 cameras (tiny, small), 1e-9 above (cfg2), 2e-4 in F32J."""
    return 2e-4 if precision == F32J else (1e-10 if n_active <= 10 else 1e-9)


def _close_ratio(a, b, rtol, atol):
    """max |a - b| / (atol + rtol |b|): <= 1 is np.allclose(a, b, rtol, atol)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b)))) if a.size else 0.0


def _max_ratio(a, b, tol):
    """|a - b|_max / (tol |b|_max)."""
    return float(np.abs(a - b).max() / (tol * np.abs(b).max()))


def _linearise(P, with_jac):
    out = dict(n_obs=P.n_obs, dim=P.reduced_dim)
    out["res"], out["cost"] = P.eval_residuals()
    if with_jac:
        out["jc"], out["jp"], out["jf"] = P.eval_jacobian()
    out["S"], out["rhs"], out["scale"] = P.build_reduced(RADIUS)
    return out


def _ratios(got, ref, precision, with_jac, measured=None):
    """name -> deviation / tolerance of one handle against the oracle (the figures of tests/test_gpu_parity.py; `measured`: the
    entry of ac.MEASURED_TOL for this step, fp64)."""
    tol = _reduced_tol(len(ref["act"]), precision)
    tol_s, tol_rhs = (max(tol, measured["S"]), max(tol, measured["rhs"])) if measured else (tol, tol)
    out = {"res": _close_ratio(got["res"], ref["res"], 1e-11, 1e-9),
           "cost": abs(got["cost"] - ref["cost"]) / (1e-12 * abs(ref["cost"])) if ref["cost"] else abs(got["cost"]),
           "S": _max_ratio(got["S"], ref["S"], tol_s), "rhs": _max_ratio(got["rhs"], ref["rhs"], tol_rhs),
           "scale": _close_ratio(got["scale"], ref["scale"], max(tol, 1e-12), 1e-8)}
    if with_jac:
        s = max(np.abs(ref["jc"]).max(), 1.0)
        rt, at = (1e-9, 1e-9 * s) if precision == F64 else (2e-4, 2e-5 * s)
        out["jc"] = _close_ratio(got["jc"], ref["jc"], rt, at)
        out["jp"] = _close_ratio(got["jp"], ref["jp"], rt, at)
        out["jf"] = _close_ratio(got["jf"], ref["jf"], 1e-12, 1e-12) if precision == F64 else _close_ratio(got["jf"], ref["jf"], rt, at)
    return out


def _check_step(capi, oracle, name, k, P, precision, with_jac):
    ref = _ref(oracle, name, k, jac=with_jac)
    sub = ref["sub"]
    assert P.n_obs == sub.n_obs and P.reduced_dim == 6 * len(ref["act"]) + 1
    app = _linearise(P, with_jac)
    with capi.Problem(sub, precision=precision) as Q:
        assert Q.reduced_dim == P.reduced_dim
        fresh = _linearise(Q, with_jac)
    measured = ac.MEASURED_TOL.get((name, k))
    ra, rf = _ratios(app, ref, precision, with_jac, measured), _ratios(fresh, ref, precision, with_jac, measured)
    tol = _reduced_tol(len(ref["act"]), precision)
    if name == "grow_from_one" and k in ac.SINGLE_VIEW_INFO and precision == F64:
        # a point with a single view: the oracle's fp64 inverse of its block is the weaker side (ac.MEASURED_TOL), so these steps are
        # ALSO held to the same formulas in long double, at the project's tolerance
        if "ld" not in ref:
            ref["ld"] = ac.reduced_longdouble(sub, ref["res"], ref["jc"], ref["jp"], ref["jf"], RADIUS)
        Sl, rl = (a.astype(np.float64) for a in ref["ld"][:2])
        for r, got in ((ra, app), (rf, fresh)):
            r["S_longdouble"], r["rhs_longdouble"] = _max_ratio(got["S"], Sl, tol), _max_ratio(got["rhs"], rl, tol)
    # appended against fresh, device against device, to the same tolerances (it does not stand in for the oracle check)
    rd = {"res": _close_ratio(app["res"], fresh["res"], 1e-11, 1e-9), "S": _max_ratio(app["S"], fresh["S"], tol),
          "rhs": _max_ratio(app["rhs"], fresh["rhs"], tol)}
    line = "%s precision=%d step %d (%d obs, %d cameras, oracle info %d): deviation / tolerance" % (name, precision, k, sub.n_obs, len(ref["act"]), ref["info"])
    for what, r in (("appended vs oracle", ra), ("fresh vs oracle", rf), ("appended vs fresh", rd)):
        line += "\n    %-19s " % what + "  ".join("%s %.3g" % kv for kv in r.items())
    print(line)
    assert np.allclose(app["S"], app["S"].T), line
    for what, r in (("appended vs oracle", ra), ("fresh vs oracle", rf), ("appended vs fresh", rd)):
        for key, v in r.items():
            assert v <= 1.0, "%s: %s\n%s" % (what, key, line)


LINEARISATION = [(name, F64) for name in ac.CASES] + [(name, F32J) for name in ac.F32J_CASES]


@pytest.mark.parametrize("name,precision", LINEARISATION)
def test_appended_handle_linearises_like_the_oracle(capi, oracle, name, precision):
    steps = ac.checked_steps(name)
    with_jac = name not in ac.LAST_STEP_ONLY
    for k, P in _grow(capi, name, precision):
        if k in steps:
            _check_step(capi, oracle, name, k, P, precision, with_jac)


@pytest.mark.parametrize("name", ac.LM_STEP_CASES)
def test_lm_step_of_an_appended_handle(capi, sfm, oracle, name):
    """One LM step (Cholesky, fp64) on a handle that reached its state BY APPENDS, held as tests/test_gpu_linear_step.py holds a fresh one."""
    case = ac.make_case(name)
    sub = ac.step_problem(case, case.n_steps - 1)
    act = np.unique(sub.obs_cam)
    opt = capi.default_options(max_iters=1, initial_radius=RADIUS, max_seconds=0.0, precision=F64, linear_solver=CHOL)
    P = _grown(capi, name)
    try:
        red = P.build_reduced(RADIUS, opt)
        P.reset()
        P.set_step_probe(True)
        summ, _ = P.solve(opt)
        z, dpt, info = P.step_probe()
        cam, pt, f = P.get_params()
    finally:
        P.close()
    o = oracle.lm_step(sub, RADIUS)
    assert o["info"] == 0
    family = "CHOL_SMALL" if len(act) <= 10 else "CHOL_FUSED"
    report = ["%s: family %s cg_iters %d fallback %d" % (name, info["family_name"], info["cg_iters"], info["cholesky_fallback"])]
    assert (info["family_name"], info["f32_matrix"], info["coarse_vectors"], info["cholesky_fallback"]) == (family, 0, 0, 0), report
    assert np.all(np.isfinite(z)) and z.shape == o["z"].shape
    sys_o = lsc.System(o["S"], o["rhs"])
    sys_d = lsc.System(red[0], red[1], ref=sys_o)
    report.append("delta %.3e kappa~ %.3e" % (sys_d.delta, sys_o.kappa))
    # (the bars below grow with delta, the device's own distance from the oracle's matrix: hold that first, to the reduced-system tolerance)
    tol = _reduced_tol(len(act), F64)
    ratios = [("S vs oracle / tolerance", _max_ratio(red[0], o["S"], tol), 1.0), ("rhs vs oracle / tolerance", _max_ratio(red[1], o["rhs"], tol), 1.0)]
    ratios.append(("device S",) + lsc.check_cholesky(sys_d, z))
    m, bar = lsc.check_cg(sys_o, z, 0.0, 0, lsc.U64, sys_d.delta)
    ratios.append(("oracle S", m, bar))
    ratios.append(("step vs oracle",) + lsc.check_step(sys_o, z, o["z"], bar, sys_d.delta))
    ob = oracle.lm_step(sub, RADIUS, z=z)
    nobs = np.bincount(sub.obs_pt, minlength=sub.n_pt)
    pr, i = lsc.check_points(dpt, ob["dpt"], ob["vcond"], ob["dmag"], nobs, sub.pt3, lsc.U64)
    ratios.append(("points (worst %d)" % i, pr, 1.0))
    # the trial cameras after the accepted step, in CALLER order: x0 - scale z (scale: the device's own Jacobi scaling)
    want_ok = oracle.solve(sub, sfm.SfmbaOptions.defaults(max_iters=1, max_seconds=0.0))[3]["successful_steps"]
    assert summ["successful_steps"] == want_ok == 1, report
    nc = 6 * len(act)
    want = sub.cam6[act].ravel() - red[2][:nc] * z[:nc]
    got = cam[act].ravel()
    ulps = np.abs(got - want) / np.spacing(np.maximum(np.abs(sub.cam6[act].ravel()), np.abs(want)))
    ratios.append(("cameras x0 - scale z (ulp / 8)", float(ulps.max()), 8.0))
    for what, m, bar in ratios:
        report.append("  %-30s %.3e / %.3e = %.3f" % (what, m, bar, m / bar if bar > 0 else np.inf))
    print("\n".join(report))
    for what, m, bar in ratios:
        assert m <= bar, "\n".join(report)
    inactive = np.setdiff1d(np.arange(sub.n_cam), act)
    assert np.array_equal(cam[inactive], sub.cam6[inactive])


def test_view_order_solve_matches_the_oracle(capi, sfm, oracle):
    """After the last out-of-order append: the whole LM solve, to the figures of tests/test_gpu_append.py."""
    case = ac.make_case("view_order")
    sub = ac.step_problem(case, case.n_steps - 1)
    want = oracle.solve(sub, sfm.SfmbaOptions.defaults(max_seconds=0.0))
    P = _grown(capi, "view_order")
    try:
        s, _ = P.solve(capi.default_options(max_seconds=0.0))
        cam, pt, f = P.get_params()
    finally:
        P.close()
    assert s["termination_name"] == want[3]["termination_name"] == "CONVERGENCE"
    assert s["iterations"] == want[3]["iterations"], (s["iterations"], want[3]["iterations"])
    assert abs(s["final_cost"] - want[3]["final_cost"]) <= 1e-9 * want[3]["final_cost"]
    assert np.abs(cam - want[0]).max() <= 1e-7 and np.abs(pt - want[1]).max() <= 1e-7


def test_view_order_parameter_round_trip(capi, oracle):
    case = ac.make_case("view_order")
    sub = ac.step_problem(case, case.n_steps - 1)
    act_c, act_p = np.unique(sub.obs_cam), np.unique(sub.obs_pt)
    rng = np.random.default_rng(77)
    cam = sub.cam6 + rng.normal(0.0, 1e-3, sub.cam6.shape)
    pt = sub.pt3 + rng.normal(0.0, 1e-3, sub.pt3.shape)
    f = sub.focal * 1.001
    P = _grown(capi, "view_order")
    try:
        P.set_params(cam, pt, f)
        cam2, pt2, f2 = P.get_params()
        res, cost = P.eval_residuals()
    finally:
        P.close()
    assert f2 == f and np.array_equal(cam2[act_c], cam[act_c]) and np.array_equal(pt2[act_p], pt[act_p])
    # (what is not observed is not on the device: get_params leaves the caller's entries as they are)
    assert np.array_equal(np.delete(cam2, act_c, axis=0), np.delete(sub.cam6, act_c, axis=0))
    assert np.array_equal(np.delete(pt2, act_p, axis=0), np.delete(sub.pt3, act_p, axis=0))
    res_o, cost_o = oracle.eval_residuals(sub, cam, pt, f)
    assert np.allclose(res, res_o, rtol=1e-11, atol=1e-9) and np.isclose(cost, cost_o, rtol=1e-12)


def test_append_without_observations_replaces_the_parameters(capi, oracle):
    case = ac.make_case("no_new_obs")
    old, new = ac.step_problem(case, 0), ac.step_problem(case, 1)
    res_old, _ = oracle.eval_residuals(old)
    res_new, cost_new = oracle.eval_residuals(new)
    assert np.abs(res_new - res_old).max() > 1.0            # (the changed parameters move the residuals by pixels)
    with capi.Problem(old) as P:
        P.append(*ac.step_new(case, 1))
        assert P.n_obs == new.n_obs and P.reduced_dim == 6 * len(np.unique(new.obs_cam)) + 1
        res, cost = P.eval_residuals()
        assert np.allclose(res, res_new, rtol=1e-11, atol=1e-9) and np.isclose(cost, cost_new, rtol=1e-12)
        cam, pt, f = P.get_params()
        assert np.array_equal(cam, new.cam6) and np.array_equal(pt, new.pt3) and f == new.focal
        s, _ = P.solve(capi.default_options(max_seconds=0.0))
        assert s["termination_name"] == "CONVERGENCE" and np.isclose(s["initial_cost"], cost_new, rtol=1e-12)
        assert s["final_cost"] < 0.5 * cost_new
        P.reset()                                           # back to the APPEND's parameters, not the create's
        res, cost = P.eval_residuals()
        assert np.allclose(res, res_new, rtol=1e-11, atol=1e-9) and np.isclose(cost, cost_new, rtol=1e-12)
        cam, pt, f = P.get_params()
        assert np.array_equal(cam, new.cam6) and np.array_equal(pt, new.pt3) and f == new.focal
    # the same append onto an empty handle: it stays empty
    from sfm_toy_library_amd.synthetic import BAProblem
    empty = BAProblem(old.cam6, old.pt3, old.focal, old.obs_cam[:0], old.obs_pt[:0], old.obs_xy[:0])
    with capi.Problem(empty) as P:
        assert P.reduced_dim == 0
        P.append(*ac.step_new(case, 1))                     # (raises on any rc but SFMBA_OK)
        assert P.reduced_dim == 0 and P.n_obs == 0
        res, cost = P.eval_residuals()
        assert cost == 0.0 and res.size == 0
        cam, pt, f = P.get_params()
        assert f == new.focal and np.array_equal(cam, new.cam6)


def test_deterministic_flag_is_kept_across_appends(capi, sfm, oracle):
    case = ac.make_case("view_order")
    k = case.n_steps - 1
    ref = _ref(oracle, "view_order", k)
    opt = capi.default_options(max_seconds=0.0)
    P = _grown(capi, "view_order", flags=sfm.CREATE_DETERMINISTIC)
    try:
        runs = []
        for _ in range(2):
            P.reset()
            s, tr = P.solve(opt)
            runs.append((s, [r["cost"] for r in tr], P.get_params()))
        P.reset()
        S, rhs, scale = P.build_reduced(RADIUS)
    finally:
        P.close()
    (s1, t1, p1), (s2, t2, p2) = runs
    assert s1["termination_name"] == "CONVERGENCE" and s1["iterations"] == s2["iterations"]
    assert s1["initial_cost"] == s2["initial_cost"] and s1["final_cost"] == s2["final_cost"] and t1 == t2
    assert np.array_equal(p1[0], p2[0]) and np.array_equal(p1[1], p2[1]) and p1[2] == p2[2]
    tol = _reduced_tol(len(ref["act"]), F64)
    print("deterministic view_order: S %.3g rhs %.3g of the tolerance" % (_max_ratio(S, ref["S"], tol), _max_ratio(rhs, ref["rhs"], tol)))
    assert np.allclose(S, S.T) and np.allclose(scale, ref["scale"], rtol=max(tol, 1e-12))
    assert _max_ratio(S, ref["S"], tol) <= 1.0 and _max_ratio(rhs, ref["rhs"], tol) <= 1.0
