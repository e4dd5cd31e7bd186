"""The small kernels between the big passes of an LM iteration (-m gpu): k_cam_update (a group of four lanes per camera, 64 cameras per
workgroup, every lane storing its share of the trial camera's tables; the sums of a workgroup taken from one value per camera), k_finalize
(the LM state read once in front of the first store) and the branches of k_lm_control behind them.  Every result is held to the oracle's
summary, trace and parameters, in both precisions and with the three solver settings.

Bars (none of them new):
  fp64      termination, iteration count and accept / reject sequence identical; initial cost 1e-12; final cost 1e-9 (+ 1e-14 of the initial
            cost: the rounding floor of an exactly satisfiable problem); parameters 1e-6, focal 1e-6 relative (test_gpu_edge_cases.py:
            test_degenerate_shapes_follow_the_oracle, all three solvers; the one- and two-camera problems here are that test's own);
            per-iteration cost 1e-7 and radius 1e-4 with the exact solvers (test_gpu_parity.py: test_solve_matches_oracle_fp64), 1e-6 and
            1e-3 with the CG (test_gpu_rejections.py); a solve cut short by an iteration limit ends ON such a row and is held to its bar
  F32J      the result: the oracle's termination type, final RMS within 1e-4 px (BASELINE's bar for fp32 Jacobians) and, for a solve that ran
            to convergence, final cost 1e-5 (test_gpu_parity.py: test_solve_f32_jacobians_within_rms_bar).  The trajectory, on problems that
            determine their parameters (seven cameras and more here; include/sfmba.h: "LM iterations and termination type: identical"):
            iteration count and accept / reject sequence identical, every row's cost within the same 1e-4 px of RMS (fp32 Jacobian blocks
            move a step by ~1e-6 of its length: far from the minimum that is more than 1e-5 of the cost the step arrives at), radius 1e-3,
            parameters at the SFMBA_F32J_BUDGET_* of include/sfmba.h.  With one or two views, and from the far start of the rejected-step
            case, scale and pose are held by the damping alone / the path is long: there the result alone is held (the bar tests/fuzz_parity.py
            puts on fp32 runs), and the test asks that the branch it is about was taken."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
COMBOS = [(p, l) for p in (0, 1) for l in (0, 1, 2)]          # precision (fp64, F32J) x linear solver (factorisation, CG, AUTO)


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return c


@pytest.fixture(scope="module")
def budget():
    h = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    return {k: float(v) for k, v in re.findall(r"#define\s+SFMBA_F32J_BUDGET_(\w+)\s+([0-9.eE+-]+)", h)}


_oracle_cache = {}


def oracle_solve(sfm, oracle, key, prob, **kw):
    """the oracle's solve of a case, computed once for all precision / solver combinations"""
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.solve(prob, sfm.SfmbaOptions.defaults(max_seconds=0.0, **kw))
    return _oracle_cache[key]


def hold_to_oracle(got, want, prob, precision, linear, budget, params=True, converged=True, trajectory=True):
    """converged: the oracle's run ended by a tolerance of the default options (the final-cost bars are stated for such runs; a run that was
    cut short is held to the per-iteration bars instead).  trajectory = False (F32J only): termination and final result alone."""
    cam, pt, f, s, tr = got
    cam_o, pt_o, f_o, s_o, tr_o = want
    rms = lambda c: np.sqrt(2.0 * c / prob.n_obs)
    assert s["termination_name"] == s_o["termination_name"], (s, s_o)
    assert np.isclose(s["initial_cost"], s_o["initial_cost"], rtol=1e-12)
    assert trajectory or precision == 1
    if trajectory:
        assert s["iterations"] == s_o["iterations"], (s, s_o)
        assert len(tr) == len(tr_o)
        assert [r["step_is_successful"] for r in tr] == [r["step_is_successful"] for r in tr_o]
        assert [r["step_is_valid"] for r in tr[1:]] == [r["step_is_valid"] for r in tr_o[1:]]
    floor = 1e-14 * s_o["initial_cost"]
    if precision == 0:
        cost_tr, radius_tr = (1e-7, 1e-4) if linear != 1 else (1e-6, 1e-3)
        assert abs(s["final_cost"] - s_o["final_cost"]) <= (1e-9 if converged else cost_tr) * s_o["final_cost"] + floor
        for a, b in zip(tr, tr_o):
            assert abs(a["cost"] - b["cost"]) <= cost_tr * b["cost"] + floor, (a, b)
            assert np.isclose(a["trust_region_radius"], b["trust_region_radius"], rtol=radius_tr), (a, b)
    else:
        if converged:
            assert abs(s["final_cost"] - s_o["final_cost"]) <= 1e-5 * s_o["final_cost"] + floor
        assert abs(rms(s["final_cost"]) - rms(s_o["final_cost"])) < 1e-4
        if trajectory:
            for a, b in zip(tr, tr_o):
                assert abs(rms(a["cost"]) - rms(b["cost"])) < 1e-4, (a, b)
                assert np.isclose(a["trust_region_radius"], b["trust_region_radius"], rtol=1e-3), (a, b)
    if not params:
        return
    if precision == 0:
        assert np.abs(cam - cam_o).max() < 1e-6 and np.abs(pt - pt_o).max() < 1e-6 and abs(f - f_o) < 1e-6 * abs(f_o)
    else:
        scale = max(1.0, float(np.abs(cam_o[:, 3:]).max()))
        assert np.abs(cam[:, :3] - cam_o[:, :3]).max() <= budget["ROTATION"]
        assert np.abs(cam[:, 3:] - cam_o[:, 3:]).max() / scale <= budget["TRANSLATION"]
        assert abs(f - f_o) <= budget["FOCAL_REL"] * abs(f_o)
        assert np.quantile(np.linalg.norm(pt - pt_o, axis=1), 0.999) / scale <= budget["POINT_P999"]


# ---------------------------------------------------------------------------------------------
# camera counts across the edges of the lane groups (4 lanes), the waves (16 cameras) and the workgroups (64 cameras) of k_cam_update
# ---------------------------------------------------------------------------------------------
CAMERA_CASES = {1: dict(n_pt=200, views=1, seed=101), 2: dict(n_pt=150, views=2, seed=102),        # (test_gpu_edge_cases.py's one and two views)
                7: dict(n_pt=300, views=4, seed=307), 31: dict(n_pt=400, views=5, seed=331), 32: dict(n_pt=400, views=5, seed=332),
                33: dict(n_pt=400, views=5, seed=333), 65: dict(n_pt=500, views=6, seed=365)}


@pytest.mark.parametrize("precision,linear", COMBOS)
@pytest.mark.parametrize("n_cam", sorted(CAMERA_CASES))
def test_camera_counts_across_group_wave_and_workgroup_edges(capi, sfm, oracle, budget, n_cam, precision, linear):
    """1, 2, 7, 31, 32, 33, 65 cameras: a lone group, a partial wave, the last camera of a wave's neighbour, one and two workgroups (the
    second with ONE camera: 255 idle lanes whose zeros go through the sums).  Camera 0 of every synthetic problem starts at w = 0 exactly: the
    first-order branch of the camera table (CT_SMALL) at the linearisation point of the first iteration, beside cameras on the full branch
    in the same wave."""
    prob = sfm.make_problem("cfg2", n_cam=n_cam, **CAMERA_CASES[n_cam])
    assert np.all(prob.cam6[0, :3] == 0.0) and (n_cam == 1 or np.all(np.abs(prob.cam6[1:, :3]).sum(axis=1) > 1e-3))
    want = oracle_solve(sfm, oracle, ("cams", n_cam), prob)
    assert want[3]["termination_name"] == "CONVERGENCE" and want[3]["iterations"] >= 2
    got = capi.solve(prob, capi.default_options(max_seconds=0.0, precision=precision, linear_solver=linear))
    hold_to_oracle(got, want, prob, precision, linear, budget, params=(precision == 0 or n_cam >= 7), trajectory=(precision == 0 or n_cam >= 7))


# ---------------------------------------------------------------------------------------------
# the branches of k_lm_control
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ten(sfm):
    return sfm.make_problem("cfg2", n_cam=10, n_pt=600, views=4, seed=4711)


@pytest.fixture(scope="module")
def ten_trace(sfm, oracle, ten):
    """the oracle's trajectory on `ten` with every tolerance off: the tolerances of the termination cases are put BETWEEN two of its rows"""
    tr = oracle.solve(ten, sfm.SfmbaOptions.defaults(max_seconds=0.0, max_iters=6, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0))[4]
    assert len(tr) == 7 and all(r["step_is_successful"] for r in tr[1:4])
    return tr


@pytest.mark.parametrize("precision,linear", COMBOS)
def test_accepted_steps(capi, sfm, oracle, budget, ten, precision, linear):
    want = oracle_solve(sfm, oracle, "accepted", ten)
    assert all(r["step_is_successful"] for r in want[4][1:3])
    hold_to_oracle(capi.solve(ten, capi.default_options(max_seconds=0.0, precision=precision, linear_solver=linear)), want, ten, precision, linear, budget)


@pytest.mark.parametrize("precision,linear", COMBOS)
def test_rejected_steps(capi, sfm, oracle, budget, precision, linear):
    """a start far from the minimum (tests/golden/small_rejected.sfmba, test_gpu_rejections.py) and a trust region that starts large:
    steps are rejected, the radius shrinks by the growing decrease factor, the linearisation is re-used at the same point"""
    prob = sfm.load_problem(os.path.join(GOLD, "small_rejected.sfmba"))
    want = oracle_solve(sfm, oracle, "rejected", prob, initial_radius=1e4)
    assert any(r["step_is_valid"] and not r["step_is_successful"] for r in want[4][1:-1]), "the oracle rejects no step here"
    opt = capi.default_options(max_seconds=0.0, precision=precision, linear_solver=linear, initial_radius=1e4)
    if linear == 1:
        opt.pcg_tolerance, opt.pcg_anchored = 1e-13, 0          # (as test_gpu_rejections.py runs the CG on this start)
    got = capi.solve(prob, opt)
    assert any(r["step_is_valid"] and not r["step_is_successful"] for r in got[4][1:-1]), "no step was rejected"
    # (no parameters: tracks of two views with a short baseline leave single points of this scene loose along their rays, and the test this
    # start comes from holds the trajectory and the cost, not them)
    hold_to_oracle(got, want, prob, precision, linear, budget, params=False, trajectory=(precision == 0))


def _invalid_case(sfm):
    """test_gpu_edge_cases.py: test_a_failed_factorisation_does_not_poison_the_handle -- fp32 Jacobians and the factorisation on a barely
    determined problem: the trust region grows until the reduced matrix stops being positive definite in fp32"""
    prob = sfm.make_problem("cfg2", n_cam=31, n_pt=200, views=2, seed=1053981787, noise_px=2.0).copy()
    idx = [201, 171, 380, 308, 48, 20, 146, 260]
    delta = [[-63.13321304321289, -150.52149963378906], [-51.15266418457031, 137.68687438964844], [133.22479248046875, -60.34691619873047],
             [-139.6809844970703, 11.003218650817871], [-96.08357238769531, 22.575063705444336], [61.0911865234375, 3.1266109943389893],
             [-121.2233657836914, 102.10670471191406], [-89.97096252441406, 50.266456604003906]]
    prob.obs_xy[idx] += np.asarray(delta)
    return prob


def test_invalid_steps_shrink_the_radius_by_eight_and_end_the_solve_when_consecutive(capi, sfm):
    """An INVALID step (the factorisation failed): no trial point is looked at, the radius goes down by F32J's factor of 8 (exactly: a power
    of two), the iteration counts as unsuccessful and the solve goes on; with max_consecutive_invalid_steps = 1 the first one ends it:
    FAILURE, at the cost of the last accepted point.  The oracle (fp64) meets no invalid step on this problem, so the bar is the rule
    itself, and for the whole solve the one of the test this problem comes from (CONVERGENCE, 2e-3 of the fp64 cost)."""
    prob = _invalid_case(sfm)
    ref = capi.solve(prob, capi.default_options(max_seconds=0.0, precision=0, linear_solver=0))[3]
    cam, pt, f, s, tr = capi.solve(prob, capi.default_options(max_seconds=0.0, precision=1, linear_solver=0))
    invalid = [r["iteration"] for r in tr[1:] if not r["step_is_valid"]]
    assert invalid, "no invalid step: the branch was not taken"
    for k in invalid:
        assert tr[k]["trust_region_radius"] == tr[k - 1]["trust_region_radius"] / 8.0 and not tr[k]["step_is_successful"]
        assert tr[k]["step_norm"] == 0.0 and tr[k]["cost_change"] == 0.0 and tr[k]["relative_decrease"] == 0.0
    assert s["termination_name"] == "CONVERGENCE" and abs(s["final_cost"] - ref["final_cost"]) < 2e-3 * ref["final_cost"]
    assert s["unsuccessful_steps"] >= len(invalid) and s["successful_steps"] == sum(r["step_is_successful"] for r in tr)
    s1, tr1 = capi.solve(prob, capi.default_options(max_seconds=0.0, precision=1, linear_solver=0, max_consecutive_invalid_steps=1))[3:]
    assert s1["termination_name"] == "FAILURE", s1
    assert not tr1[-1]["step_is_valid"] and all(r["step_is_valid"] for r in tr1[1:-1]) and s1["iterations"] == len(tr1) - 1
    assert s1["final_cost"] == tr1[-1]["cost"] and "consecutive invalid steps" in s1["message"]


def _between(a, b):
    assert a > b > 0.0
    return float(np.sqrt(a * b))


@pytest.mark.parametrize("precision,linear", COMBOS)
@pytest.mark.parametrize("which", ["gradient", "parameter", "function", "min_radius"])
def test_termination_by_each_tolerance(capi, sfm, oracle, budget, ten, ten_trace, which, precision, linear):
    """Each tolerance on its own (the others zero), put at the geometric mean of the oracle's values in two successive iterations, so that
    the iteration it ends the solve in does not hang on the last digits; the minimum radius is reached through two rejected steps."""
    tr = ten_trace
    off = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0, max_iters=6)
    if which == "gradient":
        kw, at = dict(off, gradient_tolerance=_between(tr[1]["gradient_max_norm"], tr[2]["gradient_max_norm"])), 2
    elif which == "parameter":
        x_norm = float(np.sqrt((ten.cam6 ** 2).sum() + (ten.pt3 ** 2).sum() + ten.focal ** 2))
        kw, at = dict(off, parameter_tolerance=_between(tr[2]["step_norm"], tr[3]["step_norm"]) / x_norm), 3
    elif which == "function":
        kw, at = dict(off, function_tolerance=_between(abs(tr[2]["cost_change"]) / tr[1]["cost"], abs(tr[3]["cost_change"]) / tr[2]["cost"])), 3
    else:
        # no step is good enough (rho ~ 1 < 2): rejected at the same point twice, the radius 1e4 -> 5e3 -> 1.25e3 by the growing decrease factor
        kw, at = dict(off, min_relative_decrease=2.0, min_radius=2e3), 2
    want = oracle_solve(sfm, oracle, ("term", which), ten, **kw)
    assert (want[3]["termination_name"], want[3]["iterations"]) == ("CONVERGENCE", at), (which, want[3])
    got = capi.solve(ten, capi.default_options(max_seconds=0.0, precision=precision, linear_solver=linear, **kw))
    hold_to_oracle(got, want, ten, precision, linear, budget, converged=False, params=(which != "gradient"))      # (parameters: of converged runs, or where no step was taken)
    assert got[3]["message"].startswith({"gradient": "Gradient tolerance", "parameter": "Parameter tolerance", "function": "Function tolerance",
                                         "min_radius": "Minimum trust region radius"}[which]), got[3]["message"]


@pytest.mark.parametrize("precision,linear", COMBOS)
@pytest.mark.parametrize("max_iters", [0, 1, 2])
def test_iteration_limits(capi, sfm, oracle, budget, ten, max_iters, precision, linear):
    want = oracle_solve(sfm, oracle, ("max_iters", max_iters), ten, max_iters=max_iters)
    assert (want[3]["termination_name"], want[3]["iterations"]) == ("NO_CONVERGENCE", max_iters)
    got = capi.solve(ten, capi.default_options(max_seconds=0.0, precision=precision, linear_solver=linear, max_iters=max_iters))
    hold_to_oracle(got, want, ten, precision, linear, budget, converged=False, params=(max_iters == 0))
    if max_iters == 0:
        assert got[3]["final_cost"] == got[3]["initial_cost"] and np.array_equal(got[0], ten.cam6) and np.array_equal(got[1], ten.pt3) and got[2] == ten.focal


@pytest.mark.parametrize("precision", [0, 1])
def test_a_too_short_cg_batch_is_reported_and_made_up_for(capi, sfm, oracle, ten, precision):
    """pcg_max_iters = 3: the gated kernels behind the CG batch find it unfinished -- k_cam_update returns before its barrier, k_lm_control
    posts -2 and touches nothing but the retry mark and the launch count -- and run again once the cap is spent and the step is forced (test_gpu_random.py:
    test_truncated_linear_solves_still_converge, its bars): inexact steps, the same minimum."""
    want = oracle_solve(sfm, oracle, "accepted", ten)[3]
    s, tr = capi.solve(ten, capi.default_options(max_seconds=0.0, precision=precision, linear_solver=1, pcg_max_iters=3, max_iters=50))[3:]
    assert s["termination_name"] == "CONVERGENCE" and s["iterations"] >= want["iterations"]
    assert s["linear_iters"] == 3 * s["iterations"]
    assert abs(s["final_cost"] - want["final_cost"]) <= 1e-5 * want["final_cost"]
    assert [r["iteration"] for r in tr] == list(range(s["iterations"] + 1))          # one row per LM iteration: a -2 post writes none


# ---------------------------------------------------------------------------------------------
# a deterministic handle repeats itself bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,linear", COMBOS)
def test_deterministic_handle_is_bitwise_repeatable(capi, sfm, precision, linear):
    """solve / reset / solve on a handle with ordered sums (SFMBA_CREATE_DETERMINISTIC), 65 cameras (two workgroups of k_cam_update, each
    with its own slot): the summary (read from the mirrored LM state), every trace row and every parameter repeat exactly."""
    prob = sfm.make_problem("cfg2", n_cam=65, **CAMERA_CASES[65])
    opt = capi.default_options(max_seconds=0.0, precision=precision, linear_solver=linear)
    with capi.Problem(prob, precision=precision, flags=sfm.CREATE_DETERMINISTIC) as P:
        s1, tr1 = P.solve(opt)
        p1 = P.get_params()
        P.reset()
        s2, tr2 = P.solve(opt)
        p2 = P.get_params()
    assert s1["termination_name"] == "CONVERGENCE" and s1["iterations"] >= 2
    skip = ("seconds", "setup_seconds")
    assert {k: v for k, v in s1.items() if k not in skip} == {k: v for k, v in s2.items() if k not in skip}
    assert tr1 == tr2
    assert np.array_equal(p1[0], p2[0]) and np.array_equal(p1[1], p2[1]) and p1[2] == p2[2]
