"""The linear solve of ONE LM step, per reduced-system solver family, held to a direct reference (tests/linear_step_check.py).

Whole-solve parity cannot see a step that is merely less accurate than the CG tolerance promises (LM reaches the same minimum with any
reasonable descent direction), so every case here opens a fresh handle, enables the step probe (sfmba_problem_set_step_probe), runs ONE
LM iteration and checks what the back-substitution consumed: the family that produced z (a moved selection threshold fails here instead
of silently turning the case into another family's), the residual of z in the block-Jacobi transformed system against the device's own
reduced matrix (build_reduced of the same handle) and, in fp64, against the oracle's with the step itself compared to the oracle's exact
step; the point step against the oracle's back-substitution of the device's z; and the trial cameras against x0 - scale z."""
import numpy as np
import pytest

import linear_step_check as lsc

pytestmark = pytest.mark.gpu

F64, F32J = 0, 1
CHOL, PCG, AUTO = 0, 1, 2


def _sg_vectors(n_cam):
    return 7 * min(max(n_cam // 25, 8), 20) + 1


# name: (make_problem kwargs, precision, create flags, options, expected (family, f32_matrix, coarse_vectors), radii, kind)
CASES = {
    "chol_small_1": (dict(n_cam=1, n_pt=60, views=(1, 1)), F64, 0, dict(linear_solver=CHOL), ("CHOL_SMALL", 0, 0), (1e4, 10.0), "plain"),
    "chol_small_10": (dict(n_cam=10, n_pt=300), F64, 0, dict(linear_solver=CHOL), ("CHOL_SMALL", 0, 0), (1e4, 10.0), "plain"),
    "chol_fused_11": (dict(n_cam=11, n_pt=330), F64, 0, dict(linear_solver=CHOL), ("CHOL_FUSED", 0, 0), (1e4,), "plain"),
    "chol_fused_42": (dict(n_cam=42, n_pt=1000), F64, 0, dict(linear_solver=CHOL), ("CHOL_FUSED", 0, 0), (1e4, 10.0), "plain"),
    "chol_fused_426": (dict(n_cam=426, n_pt=5000), F64, 0, dict(linear_solver=CHOL), ("CHOL_FUSED", 0, 0), (1e4,), "plain"),
    "chol_panel_427": (dict(n_cam=427, n_pt=5000), F64, 0, dict(linear_solver=CHOL), ("CHOL_PANEL", 0, 0), (1e4,), "plain"),
    "fast_coarse": (dict(n_cam=213, n_pt=3000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10), ("PCG_FAST", 0, 8), (1e4, 10.0), "plain"),
    "fast_plain": (dict(n_cam=213, n_pt=3000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10, pcg_coarse_space=-1), ("PCG_FAST", 0, 0), (1e4,), "plain"),
    "fast_f32j": (dict(n_cam=213, n_pt=3000), F32J, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10), ("PCG_FAST", 0, 8), (1e4,), "plain"),
    "fast_auto": (dict(n_cam=213, n_pt=3000), F64, 0, dict(linear_solver=AUTO), ("PCG_FAST", 0, 8), (1e4,), "plain"),
    "segments_32": (dict(name="banded_small", n_cam=32, n_pt=2000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10, pcg_coarse_space=2), ("PCG_SEGMENTS", 0, 57), (1e4,), "plain"),
    "segments_213": (dict(n_cam=213, n_pt=3000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10, pcg_coarse_space=2), ("PCG_SEGMENTS", 0, 57), (1e4,), "plain"),
    "symmetric_214": (dict(n_cam=214, n_pt=3000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10), ("PCG_SYMMETRIC", 0, 8), (1e4, 10.0), "plain"),
    "symmetric_300": (dict(n_cam=300, n_pt=4000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10), ("PCG_SYMMETRIC", 0, 8), (1e4,), "plain"),
    "symmetric_f32m": (dict(n_cam=214, n_pt=3000), F32J, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10), ("PCG_SYMMETRIC", 1, 8), (1e4,), "plain"),
    "symmetric_f32j_f64m": (dict(n_cam=300, n_pt=4000), F32J, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10, pcg_f32_matrix=-1), ("PCG_SYMMETRIC", 0, 8), (1e4,), "plain"),
    "streaming_214": (dict(n_cam=214, n_pt=3000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10, pcg_symmetric=-1), ("PCG_STREAMING", 0, 8), (1e4,), "plain"),
    "streaming_det": (dict(n_cam=214, n_pt=3000), F64, 1, dict(linear_solver=PCG, pcg_tolerance=1e-10), ("PCG_STREAMING", 0, 8), (1e4,), "plain"),
    "sg_sparse_240": (dict(name="banded_small", n_cam=240, n_pt=6000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10), ("PCG_SEGMENTS_STREAMING_SPARSE", 0, _sg_vectors(240)), (1e4,), "plain"),
    "sg_sparse_520": (dict(name="banded_small", n_cam=520, n_pt=12000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10), ("PCG_SEGMENTS_STREAMING_SPARSE", 0, _sg_vectors(520)), (1e4,), "plain"),
    "sg_dense_214": (dict(n_cam=214, n_pt=3000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10, pcg_coarse_space=2), ("PCG_SEGMENTS_STREAMING", 0, _sg_vectors(214)), (1e4,), "plain"),
    "implicit_f64": (dict(n_cam=40, n_pt=1500), F64, 4, dict(linear_solver=PCG, pcg_tolerance=1e-10), ("IMPLICIT", 0, 8), (1e4,), "dup"),
    "implicit_f32j": (dict(n_cam=40, n_pt=1500), F32J, 4, dict(linear_solver=PCG, pcg_tolerance=1e-10), ("IMPLICIT", 0, 8), (1e4,), "dup"),
    "implicit_det": (dict(n_cam=40, n_pt=1500), F64, 5, dict(linear_solver=PCG, pcg_tolerance=1e-10), ("IMPLICIT", 0, 8), (1e4,), "dup"),
    "dist_blocks": (dict(n_cam=60, n_pt=2000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10, shard_distributed_cg=1), ("DIST_BLOCKS", 0, 8), (1e4,), "shard"),
    "dist_rows": (dict(n_cam=60, n_pt=2000), F64, 0, dict(linear_solver=PCG, pcg_tolerance=1e-10, shard_distributed_cg=3), ("DIST_ROWS", 0, 8), (1e4,), "row"),
    "auto_fallback": (dict(n_cam=214, n_pt=3000), F64, 0, dict(linear_solver=AUTO, pcg_max_iters=2), ("CHOL_FUSED", 0, 0), (1e4,), "plain"),
}

_cache = {}


@pytest.fixture(scope="module")
def capi(oracle):
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    n = oracle.num_threads()
    oracle.set_num_threads(min(n, 16))
    return c


def _problem(sfm, kw, kind):
    key = (tuple(sorted(kw.items())), kind)
    if key not in _cache:
        kw = dict(kw)
        name = kw.pop("name", "small")
        if name != "banded_small":
            kw.setdefault("views", (2, 8))
        prob = sfm.make_problem(name, seed=7000 + kw["n_cam"], **kw)
        if kind == "dup":
            # duplicate (camera, point) observations: the implicit product's own pair terms
            extra = np.arange(0, prob.n_obs, 9)
            prob = sfm.BAProblem(prob.cam6, prob.pt3, prob.focal, np.concatenate([prob.obs_cam, prob.obs_cam[extra]]),
                                 np.concatenate([prob.obs_pt, prob.obs_pt[extra]]), np.concatenate([prob.obs_xy, prob.obs_xy[extra] + 0.25]))
        _cache[key] = prob
    return _cache[key]


def _oracle_step(oracle, prob, radius, z=None):
    key = (id(prob), radius)
    if z is None:
        if key not in _cache:
            _cache[key] = oracle.lm_step(prob, radius)
        return _cache[key]
    return oracle.lm_step(prob, radius, z=z)


def _run(capi, sfm, prob, precision, flags, opt, kind):
    """(z, dpt, info, summary, cam, pt, f, device S / rhs / scale or None)."""
    from sfm_toy_library_amd import sharded
    if kind in ("shard", "row"):
        cls = sharded.HipRowShardBackend if kind == "row" else sharded.HipShardBackend
        b = cls(prob, 0, 1, device=0, precision=precision)
        try:
            b.set_step_probe(True)
            summ = sharded.solve_sharded_native(b, opt)
            z, dpt, info = b.step_probe()
            cam, pt, f = b.get_params() if hasattr(b, "get_params") else (None, None, None)
        finally:
            b.close()
        with capi.Problem(prob, precision=precision) as P:
            red = P.build_reduced(opt.initial_radius, opt)
        return z, dpt, info, summ, cam, pt, f, red
    with capi.Problem(prob, precision=precision, flags=flags) as P:
        red = None
        if not flags & sfm.CREATE_NO_PAIR_LIST:
            red = P.build_reduced(opt.initial_radius, opt)
            P.reset()
        P.set_step_probe(True)
        summ, _ = P.solve(opt)
        z, dpt, info = P.step_probe()
        cam, pt, f = P.get_params()
    return z, dpt, info, summ, cam, pt, f, red


@pytest.mark.parametrize("name", list(CASES))
def test_linear_step(capi, sfm, oracle, name):
    kw, precision, flags, okw, (family, f32m, ncoarse), radii, kind = CASES[name]
    prob = _problem(sfm, kw, kind)
    f32 = precision == F32J
    for radius in radii:
        opt = capi.default_options(max_iters=1, initial_radius=radius, max_seconds=0.0, precision=precision, **okw)
        z, dpt, info, summ, cam, pt, f, red = _run(capi, sfm, prob, precision, flags, opt, kind)
        o = _oracle_step(oracle, prob, radius)
        assert o["info"] == 0
        report = ["%s r=%g: family %s f32_matrix %d coarse %d cg_iters %d fallback %d" % (name, radius, info["family_name"], info["f32_matrix"],
                                                                                          info["coarse_vectors"], info["cg_iters"], info["cholesky_fallback"])]
        assert (info["family_name"], info["f32_matrix"], info["coarse_vectors"]) == (family, f32m, ncoarse), report
        assert info["cholesky_fallback"] == (1 if name == "auto_fallback" else 0), report
        assert np.all(np.isfinite(z)) and z.shape == o["z"].shape
        sys_o = lsc.System(o["S"], o["rhs"])
        cholesky = family.startswith("CHOL")
        tol = 1e-12 if okw.get("linear_solver") == AUTO else okw.get("pcg_tolerance", 1e-8)
        k = info["cg_iters"]
        u_mat = lsc.U32 if f32m else lsc.U64
        ratios = []
        if red is not None:
            sys_d = lsc.System(red[0], red[1], ref=sys_o)
            report.append("delta %.3e kappa~ %.3e" % (sys_d.delta, sys_o.kappa))
            if cholesky:
                m, bar = lsc.check_cholesky(sys_d, z)
            else:
                m, bar = lsc.check_cg(sys_d, z, tol, k, u_mat)
            ratios.append(("device S", m, bar))
            delta = sys_d.delta
        else:
            delta = 0.0
        if not f32:
            # against the oracle's system, and the step against the oracle's exact step
            if cholesky:
                # (against another matrix the Cholesky's backward error is delta itself: the transformed residual, as for the CG, at k = 0)
                m, bar = lsc.check_cg(sys_o, z, 0.0, 0, lsc.U64, delta)
            else:
                m, bar = lsc.check_cg(sys_o, z, tol, k, u_mat, delta)
            ratios.append(("oracle S", m, bar))
            e, ebar = lsc.check_step(sys_o, z, o["z"], bar, delta)
            ratios.append(("step vs oracle", e, ebar))
        # the point step: the oracle's back-substitution of the device's own z
        ob = _oracle_step(oracle, prob, radius, z=z)
        nobs = np.bincount(prob.obs_pt, minlength=prob.n_pt)
        pr, i = lsc.check_points(dpt, ob["dpt"], ob["vcond"], ob["dmag"], nobs, prob.pt3, lsc.U64 + (lsc.U32 if f32 else 0.0))
        ratios.append(("points (worst %d)" % i, pr, 1.0))
        # the trial cameras after an accepted step: x0 - scale z (scale: the device's own Jacobi scaling)
        if cam is not None and summ["successful_steps"] == 1 and red is not None:
            act = np.unique(prob.obs_cam)
            nc = 6 * len(act)
            want = prob.cam6[act].ravel() - red[2][:nc] * z[:nc]
            got = cam[act].ravel()
            ulps = np.abs(got - want) / np.spacing(np.maximum(np.abs(prob.cam6[act].ravel()), np.abs(want)))
            ratios.append(("cameras x0 - scale z (ulp / 8)", float(ulps.max()), 8.0))
        for what, m, bar in ratios:
            report.append("  %-30s %.3e / %.3e = %.3f" % (what, m, bar, m / bar if bar > 0 else np.inf))
        print("\n".join(report))
        for what, m, bar in ratios:
            assert m <= bar, "\n".join(report)
