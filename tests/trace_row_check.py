"""A long-double restatement of one row of the LM trace (sfmba_iteration) -- TEST INFRASTRUCTURE ONLY (numpy and the oracle bindings).

Given the linearisation point x_prev and the trial point x_trial that a solver itself used, every numeric column of the row is a closed
formula of the oracle's residuals and Jet Jacobian blocks (oracle.eval_residuals, oracle.eval_jacobian), evaluated in np.longdouble:

    s            = x_trial - x_prev                      (cameras, points, focal; unscaled)
    step_norm    = |s|_2
    cost_change  = cost(x_prev) - cost(x_trial)
    model        = -(J s)^T (r + J s / 2)                (J, r at x_prev)
    rho          = cost_change / model
    gradient_max = max |J^T r| over ALL parameters at the point the row reports
                   (x_trial after an accepted step, otherwise the previous row's)

No oracle solve and no matching trajectory is needed: a row is held at the solver's OWN step.  The convention of include/sfmba.h:
trial cameras = x0 - scale * z, trial points = x0 - dpt.

Bars (u = 2^-53; tau = the Jacobian-block figure of tests/test_gpu_parity.py: 1e-9 in fp64, 2e-4 with fp32 Jacobian blocks):
    cost               row 0: 1e-12 relative.  Row k >= 1 (the trial cost, 0.5 sum r^2 formed directly): 1e-12 cost_trial + cost_rounding(),
                       the rounding of fp64 residuals that are differences of pixel coordinates (derived there; 1e-12 alone asks more
                       digits of the last rows of an exactly satisfiable problem than fp64 residuals have: measured 6.5 x it on cams_1 row 2)
    cost_change        1e-12 (cost_prev + cost_trial)                    the trial residuals are fp64 in both precisions
    step_norm          relative (n_par + 16) u + 2 u |x| / |s|           the reference is the actual parameter difference, as Ceres forms it
    model              tau sum_obs |J||s| (|r| + |J||s|), element-wise absolute values; F32J adds ceil(track / 4) 2^-24 of a point's share
                       of that sum (a lane's own fp32 sum of at most that many products)
    relative_decrease  |rho| (bar_cc / |cost_change| + bar_model / |model|)
    gradient_max_norm  tau (|J|^T |r|) at the reference's arg-max entry; entries within that bar of the maximum count as ties
A row is HELD for rho only if its rho bar is <= 1e-6 |rho| in fp64 (1e-3 |rho| in F32J): a row whose cost change cancels to 1e-7 of the
cost is reported, not held.  MUST_HOLD fixes which rows of each case have to be held, so that a bar cannot go vacuous unnoticed
(tests/test_trace_row_check_cpu.py checks it on the oracle's own trajectory)."""
import os

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
U32 = 2.0 ** -24
TAU = {0: 1e-9, 1: 2e-4}
HELD_RHO = {0: 1e-6, 1: 1e-3}
COST_REL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

REJECTED_ROWS = 7          # tests/golden/small_rejected.sfmba at radius 1e4: rows 1 - 6 accepted (rho 0.93, 0.91, 0.77, 0.62, 0.42, 0.0039), row 7 rejected (rho -0.43)
# rows of each case whose rho has to be HELD in fp64 (checked on the oracle's trajectory by the CPU test, asked of the device by the GPU test)
MUST_HOLD = {"ten": (1, 2), "rejected": (1, 2, 3, 4, 5), "cams_1": (1, 2), "cams_2": (1, 2), "cams_65": (1, 2), "cams_401": (1,),
             "implicit_dup": (1,), "no_jacobi": (1, 2), "scaled_200": (1,), "point_max": (1,)}


def trial_pose_min_cams():
    """SFMBA_TRIAL_POSE_MIN_CAMS, read from the source: at and above it k_point_update<float> takes the trial pose from the parameters"""
    import re
    src = open(os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "ba_step.hip")).read()
    return int(re.search(r"#define\s+SFMBA_TRIAL_POSE_MIN_CAMS\s+(\d+)", src).group(1))


# ---------------------------------------------------------------------------------------------
# the cases (problem, options of the solve, rows)
# ---------------------------------------------------------------------------------------------
def dup_problem(sfm):
    """the "dup" problem of tests/test_gpu_linear_step.py: 40 cameras, 1500 points, every 9th observation doubled"""
    prob = sfm.make_problem("small", seed=7040, n_cam=40, n_pt=1500, views=(2, 8))
    extra = np.arange(0, prob.n_obs, 9)
    return sfm.BAProblem(prob.cam6, prob.pt3, prob.focal, np.concatenate([prob.obs_cam, prob.obs_cam[extra]]),
                         np.concatenate([prob.obs_pt, prob.obs_pt[extra]]), np.concatenate([prob.obs_xy, prob.obs_xy[extra] + 0.25]))


def scaled(prob, s):
    """tests/test_gpu_f32j_budget.py: the same scene in units s times smaller"""
    q = prob.copy()
    q.pt3 = q.pt3 * s
    q.cam6 = q.cam6.copy()
    q.cam6[:, 3:] *= s
    return q


POINT_MAX_SHIFT = 0.5


def point_max_problem(sfm, oracle):
    """`ten` with point 0 seen by ALL ten cameras (the missing observations are its projections in the true scene), solved by the oracle, then
    that one point displaced: the largest gradient entry is then one of the point's (asserted by the CPU test)"""
    ten = sfm.make_problem("cfg2", n_cam=10, n_pt=600, views=4, seed=4711)
    seen = set(ten.obs_cam[ten.obs_pt == 0].tolist())
    add = np.array([j for j in range(ten.n_cam) if j not in seen], dtype=ten.obs_cam.dtype)
    from sfm_toy_library_amd.synthetic import project
    xy, _ = project(ten.cam6_true, ten.pt3_true, ten.focal_true, add, np.zeros(len(add), dtype=ten.obs_pt.dtype))
    prob = sfm.BAProblem(ten.cam6, ten.pt3, ten.focal, np.concatenate([ten.obs_cam, add]), np.concatenate([ten.obs_pt, np.zeros(len(add), dtype=ten.obs_pt.dtype)]),
                         np.concatenate([ten.obs_xy, np.asarray(xy, dtype=np.float32).astype(np.float64).reshape(-1, 2)]))      # (fp32 values, as every observation of the suite)
    cam, pt, f, s, _ = oracle.solve(prob, sfm.SfmbaOptions.defaults(max_seconds=0.0))
    assert s["termination_name"] == "CONVERGENCE"
    pt = pt.copy()
    pt[0] += POINT_MAX_SHIFT
    return sfm.BAProblem(cam, pt, f, prob.obs_cam, prob.obs_pt, prob.obs_xy)


_problems = {}


def case_problem(sfm, oracle, case):
    """(problem, options of the solve, first row, last row)"""
    if case not in _problems:
        from test_gpu_serial_kernels import CAMERA_CASES
        if case == "ten":
            v = sfm.make_problem("cfg2", n_cam=10, n_pt=600, views=4, seed=4711), {}, 1, 3
        elif case == "rejected":
            v = sfm.load_problem(os.path.join(GOLD, "small_rejected.sfmba")), dict(initial_radius=1e4), 1, REJECTED_ROWS
        elif case.startswith("cams_") and int(case[5:]) in CAMERA_CASES:
            n = int(case[5:])
            v = sfm.make_problem("cfg2", n_cam=n, **CAMERA_CASES[n]), {}, 1, 2
        elif case == "cams_401":
            v = sfm.make_problem("small", n_cam=401, n_pt=3000, views=(2, 6)), {}, 1, 1
        elif case == "implicit_dup":
            v = dup_problem(sfm), {}, 1, 1
        elif case == "no_jacobi":
            v = sfm.make_problem("tiny"), dict(jacobi_scaling=0), 1, 2
        elif case == "scaled_200":
            v = scaled(sfm.make_problem("cfg2"), 200.0), {}, 1, 1
        elif case == "point_max":
            v = point_max_problem(sfm, oracle), {}, 0, 1
        else:
            raise KeyError(case)
        _problems[case] = v
    return _problems[case]


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
def params_of(prob):
    return np.array(prob.cam6, dtype=np.float64), np.array(prob.pt3, dtype=np.float64), float(prob.focal)


def _scatter(n, idx, val):
    out = np.zeros((n,) + val.shape[1:], dtype=LD)
    np.add.at(out, idx, val)
    return out


class Linearisation:
    """residuals, Jacobian blocks and the gradient J^T r at x, in long double; A = |J|^T |r| (the size of the terms behind each gradient entry)"""

    def __init__(self, oracle, prob, x):
        self.prob, self.x = prob, x
        r, jc, jp, jf = oracle.eval_jacobian(prob, cam6=x[0], pt3=x[1], focal=x[2])
        self.r, self.jc, self.jp, self.jf = r.astype(LD), jc.astype(LD), jp.astype(LD), jf.astype(LD)
        self.cost = 0.5 * (self.r * self.r).sum()
        r_ = self.r[:, :, None]
        oc, op = np.asarray(prob.obs_cam), np.asarray(prob.obs_pt)
        self.g = (_scatter(prob.n_cam, oc, (self.jc * r_).sum(axis=1)), _scatter(prob.n_pt, op, (self.jp * r_).sum(axis=1)), (self.jf * self.r).sum())
        a_ = np.abs(r_)
        self.A = (_scatter(prob.n_cam, oc, (np.abs(self.jc) * a_).sum(axis=1)), _scatter(prob.n_pt, op, (np.abs(self.jp) * a_).sum(axis=1)),
                  (np.abs(self.jf) * np.abs(self.r)).sum())

    def gradient_max(self, tau, blocks=("cameras", "points", "focal")):
        """dict: value (max |g| over the named blocks), per-block maxima with their arg-max, block of the maximum, the bar and the tied values"""
        entries = []        # (|g|, A, block, index)
        per_block = {}
        for name, g, A in (("cameras", self.g[0], self.A[0]), ("points", self.g[1], self.A[1]), ("focal", np.array([self.g[2]]), np.array([self.A[2]]))):
            ga, Aa = np.abs(np.asarray(g, dtype=LD)).ravel(), np.asarray(A, dtype=LD).ravel()
            k = int(np.argmax(ga)) if ga.size else 0
            per_block[name] = (float(ga[k]) if ga.size else 0.0, k)
            if name in blocks and ga.size:
                entries.append((ga, Aa, name))
        best = max(entries, key=lambda e: e[0].max())
        k = int(np.argmax(best[0]))
        value, bar = best[0][k], tau * best[1][k]
        ties, tie_bar = [], bar
        for ga, Aa, name in entries:
            m = ga >= value - bar
            ties.extend(float(v) for v in ga[m])
            if m.any():
                tie_bar = max(tie_bar, tau * Aa[m].max())
        return dict(value=float(value), block=best[2], index=k, per_block=per_block, bar=float(tie_bar), ties=ties)


def residuals_at(oracle, prob, x):
    r, _ = oracle.eval_residuals(prob, cam6=x[0], pt3=x[1], focal=x[2])
    return r.astype(LD)


def cost_at(oracle, prob, x):
    r = residuals_at(oracle, prob, x)
    return 0.5 * (r * r).sum()


def cost_rounding(prob, x, r):
    """What fp64 residuals can leave in a cost, from how a residual is formed (k_point_update's trial sweep and the oracle alike):
    p = R X + t, r = f p_xy / p_z - obs, cost = sum r^2 / 2.  With a = |R||X| + |t| (the size of the terms behind p), an entry of p is off by
    at most 8 u a (four roundings of the three-term dot product and the sum with t, four more for the entries of R out of Rodrigues'
    formula), so r_x by  u [ 8 (f / |p_z|) (a_x + |x_p| a_z) + 2 |f x_p| + |r_x| ]  (the quotient, the product with f, the difference), and
    the cost by sum |r| dr.  Twice: the device's residuals and the reference's -- the oracle evaluates in fp64 too, only the sums here are
    long double.  A worst-case bound: 4e-12 .. 6e-12 of the cost where |r| is a fraction of a pixel (ten, cams_401, scaled_200), 1e-14
    of it far from the minimum (rejected), and 5e-10 of it where the residuals are 1e-6 of the coordinates they are the difference of
    (cams_1 row 2, an exactly satisfiable problem at a cost of 1.5e-4).  It does not depend on the cost the solve started from."""
    from sfm_toy_library_amd.synthetic import rotvec_to_matrix
    cam, pt, f = np.asarray(x[0], dtype=np.float64), np.asarray(x[1], dtype=np.float64), abs(float(x[2]))
    oc, op = np.asarray(prob.obs_cam), np.asarray(prob.obs_pt)
    R = rotvec_to_matrix(cam[:, :3])[oc]
    X = pt[op]
    p = np.einsum("nij,nj->ni", R, X) + cam[oc, 3:]
    a = np.einsum("nij,nj->ni", np.abs(R), np.abs(X)) + np.abs(cam[oc, 3:])
    ra = np.abs(np.asarray(r, dtype=np.float64))
    dr = [U * (8.0 * (f / np.abs(p[:, 2])) * (a[:, c] + np.abs(p[:, c] / p[:, 2]) * a[:, 2]) + 2.0 * np.abs(f * p[:, c] / p[:, 2]) + ra[:, c]) for c in (0, 1)]
    return 2.0 * float((ra[:, 0] * dr[0] + ra[:, 1] * dr[1]).sum())


class RowReference:
    """Every column of the row whose step went from x_prev (linearised: `lin`) to x_trial, with its bar.
    drop: the teeth check's switch -- "focal_step" leaves the focal entry out of step_norm, "point_term" the point term out of J s."""

    def __init__(self, oracle, lin, x_trial, precision, drop=None):
        prob, x_prev = lin.prob, lin.x
        tau = TAU[precision]
        sc = (np.asarray(x_trial[0], dtype=LD) - np.asarray(x_prev[0], dtype=LD))
        sp = (np.asarray(x_trial[1], dtype=LD) - np.asarray(x_prev[1], dtype=LD))
        sf = LD(x_trial[2]) - LD(x_prev[2])
        oc, op = np.asarray(prob.obs_cam), np.asarray(prob.obs_pt)
        used_c, used_p = np.zeros(prob.n_cam, bool), np.zeros(prob.n_pt, bool)
        used_c[oc] = True
        used_p[op] = True
        n_par = 6 * int(used_c.sum()) + 3 * int(used_p.sum()) + 1
        s2 = (sc[used_c] ** 2).sum() + (sp[used_p] ** 2).sum() + (sf * sf if drop != "focal_step" else LD(0))
        x2 = (np.asarray(x_prev[0], dtype=LD)[used_c] ** 2).sum() + (np.asarray(x_prev[1], dtype=LD)[used_p] ** 2).sum() + LD(x_prev[2]) ** 2
        self.step_norm = np.sqrt(s2)
        self.step_norm_bar = self.step_norm * ((n_par + 16) * U + 2.0 * U * np.sqrt(x2) / self.step_norm)
        self.cost_prev = lin.cost
        r_trial = residuals_at(oracle, prob, x_trial)
        self.cost_trial = 0.5 * (r_trial * r_trial).sum()
        self.cost_trial_bar = COST_REL * self.cost_trial + cost_rounding(prob, x_trial, r_trial)
        self.cost_change = self.cost_prev - self.cost_trial
        self.cost_change_bar = COST_REL * (self.cost_prev + self.cost_trial)
        # J s per observation and the size of its terms
        js_c = (lin.jc * sc[oc][:, None, :]).sum(axis=2)
        js_p = (lin.jp * sp[op][:, None, :]).sum(axis=2)
        js_f = lin.jf * sf
        js = js_c + js_f + (js_p if drop != "point_term" else 0)
        ajs = (np.abs(lin.jc) * np.abs(sc[oc])[:, None, :]).sum(axis=2) + (np.abs(lin.jp) * np.abs(sp[op])[:, None, :]).sum(axis=2) + np.abs(lin.jf) * abs(sf)
        self.model = -(js * (lin.r + 0.5 * js)).sum()
        size = (ajs * (np.abs(lin.r) + ajs)).sum(axis=1)
        self.model_bar = tau * size.sum()
        if precision == 1:
            track = np.bincount(op, minlength=prob.n_pt)
            self.model_bar += (np.ceil(track[op] / 4.0) * U32 * size).sum()
        self.rho = self.cost_change / self.model
        self.rho_bar = abs(self.rho) * (self.cost_change_bar / abs(self.cost_change) + self.model_bar / abs(self.model))
        self.held = bool(self.rho_bar <= HELD_RHO[precision] * abs(self.rho))


def compare_row(row, ref):
    """[(column, measured, bar)] of a trace row (dict) against a RowReference.  The model is read back as cost_change / relative_decrease."""
    out = [("step_norm", float(abs(LD(row["step_norm"]) - ref.step_norm)), float(ref.step_norm_bar)),
           ("cost_change", float(abs(LD(row["cost_change"]) - ref.cost_change)), float(ref.cost_change_bar))]
    if row["relative_decrease"] != 0.0:
        model = LD(row["cost_change"]) / LD(row["relative_decrease"])
        out.append(("model", float(abs(model - ref.model)), float(ref.model_bar)))
    else:
        out.append(("model", np.inf, float(ref.model_bar)))
    out.append(("relative_decrease" if ref.held else "relative_decrease (not held)", float(abs(LD(row["relative_decrease"]) - ref.rho)), float(ref.rho_bar)))
    return out


def compare_gradient(value, gm):
    """(column, measured, bar): the nearest of the tied entries"""
    return ("gradient_max_norm", min(abs(value - t) for t in gm["ties"]), gm["bar"])


def is_held(name):
    return not name.endswith("(not held)")


# ---------------------------------------------------------------------------------------------
# the oracle's own trajectory, row by row (the CPU test; the GPU test walks the device's in the same way)
# ---------------------------------------------------------------------------------------------
def trial_from_step(prob, x_prev, scale, z, dpt):
    """include/sfmba.h: trial cameras = x0 - scale * z (active cameras in ascending order, the focal last), trial points = x0 - dpt"""
    act = np.unique(prob.obs_cam)
    nc = 6 * len(act)
    cam = np.array(x_prev[0], dtype=np.float64)
    cam[act] = (cam[act].ravel() - scale[:nc] * z[:nc]).reshape(-1, 6)
    return cam, np.asarray(x_prev[1], dtype=np.float64) - dpt, float(x_prev[2] - scale[nc] * z[nc])


def oracle_walk(sfm, oracle, case, last=None):
    """(the oracle's row 0, the linearisation at the start, [(oracle row k, Linearisation at x_prev, x_trial, summary of the run that ends on row k)]
    for k = 1 .. last).  On ONE thread: the oracle sums with OpenMP, and only then is the run to max_iters = k the run to k - 1 plus one row."""
    threads = oracle.num_threads()
    oracle.set_num_threads(1)
    try:
        return _oracle_walk(sfm, oracle, case, last)
    finally:
        oracle.set_num_threads(threads)


def _oracle_walk(sfm, oracle, case, last):
    prob, okw, first, k_last = case_problem(sfm, oracle, case)
    last = k_last if last is None else last
    x, lin0 = params_of(prob), None
    rows, out = None, []
    lin = Linearisation(oracle, prob, x)
    lin0 = lin
    for k in range(1, last + 1):
        opt = sfm.SfmbaOptions.defaults(max_seconds=0.0, max_iters=k, **okw)
        cam, pt, f, summ, tr = oracle.solve(prob, opt)
        assert len(tr) == k + 1 and (rows is None or tr[:k] == rows), "the oracle does not repeat itself"
        row = tr[k]
        if row["step_is_successful"]:
            x_trial = (cam, pt, f)
        else:
            st = oracle.lm_step(prob, tr[k - 1]["trust_region_radius"], opt, cam6=x[0], pt3=x[1], focal=x[2])
            assert st["info"] == 0
            x_trial = trial_from_step(prob, x, st["scale"], st["z"], st["dpt"])
        out.append((row, lin, x_trial, summ))
        rows = tr
        if row["step_is_successful"]:
            x = x_trial
            lin = Linearisation(oracle, prob, x)
    return rows[0] if rows else None, lin0, out
