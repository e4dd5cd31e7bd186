"""Every reduced-system CG family at every size class against the numpy restatement of the method (-m gpu): tests/cg_family_cases.py holds the table,
the systems, the long-double reference and the bars; tests/test_cg_family_cases_cpu.py proves on the CPU that the inputs are what they claim and
that the bars catch a planted defect.  The device side is sfmba_dense_pcg_probe: the library's own transform, path choice and family launches on a
matrix and coarse vectors handed in from here.

Per case, three probe calls (each uploads the matrix once and runs its right-hand sides one after another on one workspace):
    reuse    b, the zero vector, b2                               (max_iters 200 each)
    forced   b2 -- that system solved alone --, then b stopped after 1, 2, 3 iterations
    poison   b, then b stopped after 1, 2, 3 iterations, with NaN in everything the kernels promise not to multiply
and six verdicts: (1) routing, (2) true residual, (3) iterations, (4) forced iterates, (5) poison, (6) reuse.  One `cgfam` line per case goes to
stdout before anything is asserted: routing, iterations device / reference, every measured / bar ratio (profiles/cg_families.txt is those lines)."""
import numpy as np
import pytest

import cg_family_cases as cf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


@pytest.mark.parametrize("case", cf.CASES, ids=cf.case_id)
def test_family_matches_the_reference_cg(capi, case):
    nc, variant, expect = case
    sym, f32, coarse, seg = cf.VARIANTS[variant]
    s = cf.system(nc)
    flags = (capi.PCG_PROBE_SYMMETRIC if sym else 0) | (capi.PCG_PROBE_F32_MATRIX if f32 else 0) | (capi.PCG_PROBE_SEGMENTS if seg else 0)
    Wt = cf.probe_vectors(s, variant)
    k_ref, k_ref_ld, _ = cf.reference(nc, variant, 0)
    k2_ref = cf.reference(nc, variant, 1)[0]
    full, forced = cf.MAX_ITERS, list(cf.FORCED)
    zero = np.zeros(s.d)

    X, info, it, path = capi.dense_pcg_probe(s.S, [s.rhs, zero, s.rhs2], Wt, flags, cf.TOL, [full] * 3)
    Xf, info_f, it_f, path_f = capi.dense_pcg_probe(s.S, [s.rhs2, s.rhs, s.rhs, s.rhs], Wt, flags, cf.TOL, [full] + forced)
    Xp, info_p, it_p, path_p = capi.dense_pcg_probe(s.S, [s.rhs] * 4, Wt, flags | capi.PCG_PROBE_POISON, cf.TOL, [full] + forced)

    routes = [(p["family_name"], p["f32_matrix"], p["coarse_vectors"]) for p in (path, path_f, path_p)]
    finite = bool(np.all(np.isfinite(Xp)))
    rr = cf.residual_ratios(s, nc, variant, [X[0], X[2], Xf[0], Xp[0]], [s.rhs, s.rhs2, s.rhs2, s.rhs], [it[0], it[2], it_f[0], it_p[0]])
    fr = cf.forced_ratios(s, nc, variant, Xf[1:4])
    fp = cf.forced_ratios(s, nc, variant, Xp[1:4])
    print("cgfam %-12s d %4d  %-22s f32 %d cv %3d  iters %2d/%2d (ld %2d) poison %2d  b2 %2d/%2d alone %2d  rho %.1e %.1e %.1e poison %.1e  forced %s  poison %s" % (
        cf.case_id(case), s.d, routes[0][0], routes[0][1], routes[0][2], it[0], k_ref, k_ref_ld, it_p[0], it[2], k2_ref, it_f[0], rr[0], rr[1], rr[2], rr[3],
        " ".join("%.1e" % v for v in fr), " ".join("%.1e" % v for v in fp)), flush=True)

    # (1) routing: what the table says, on every call
    assert routes == [expect] * 3
    assert info == info_f == info_p == 0
    # (2) true residual of every full solve, in long double against the matrix that was handed in
    assert max(rr) <= 1.0, rr
    # (3) iterations against the float64 restatement (its long-double twin is within 1: the CPU test)
    assert abs(int(it[0]) - k_ref) <= 2 and abs(int(it_f[0]) - k2_ref) <= 2
    # (4) the iterates after 1, 2, 3 iterations against the long-double restatement's
    assert list(it_f[1:]) == forced and max(fr) <= 1.0, (list(it_f), fr)
    # (5) with the poison in place: the same routing (above), residual (above), iterations and iterates, and nothing but finite numbers
    assert finite
    assert abs(int(it_p[0]) - k_ref) <= 2 and list(it_p[1:]) == forced and max(fp) <= 1.0, (list(it_p), fp)
    # (6) reuse of the workspace: the zero right-hand side costs nothing and returns zero, the solve behind it is the solve alone
    assert it[1] == 0 and not np.any(X[1])
    assert abs(int(it[2]) - int(it_f[0])) <= 1
