"""A/B of the segmented coarse space (pcg_segments.hip, pcg_segments_streaming.hip) on banded problems: CG iterations, result, time per solve with SFMBA_PCG_SEGMENTS=0 / 1.
    python tools/segments_check.py [workload ...]      (runs on the GPU box)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sfm_toy_library_amd as sfm
from sfm_toy_library_amd import capi

cases = sys.argv[1:] or ["banded_small", "banded60", "cfg3_banded", "cfg3"]
for name in cases:
    prob = sfm.make_problem("cfg3_banded", n_cam=60, n_pt=8000) if name == "banded60" else sfm.make_problem(name)
    for prec in (0, 1):
        res = {}
        for seg in ("0", "1"):
            os.environ["SFMBA_PCG_SEGMENTS"] = seg
            with capi.Problem(prob, precision=prec) as P:
                opt = capi.default_options(max_seconds=0.0, precision=prec, linear_solver=1)
                s, tr = P.solve(opt)
                cam, pt, f = P.get_params()
                t = []
                for _ in range(5):
                    P.reset(); t0 = time.perf_counter(); s2, _ = P.solve(opt); t.append(time.perf_counter() - t0)
                res[seg] = (s, tr, cam, pt, f, min(t))
        a, b = res["0"], res["1"]
        print("%-12s prec %d: d = %d  LM its %d / %d  CG iterations per LM iteration %s / %s" % (
            name, prec, 6 * prob.n_cam + 1, a[0]["iterations"], b[0]["iterations"],
            [r["linear_iters"] for r in a[1][1:]], [r["linear_iters"] for r in b[1][1:]]))
        print("             final cost %.12e / %.12e  max |dcam| %.2e  |df| %.2e  solve %.3f / %.3f ms  -> %.0f / %.0f LM it/s" % (
            a[0]["final_cost"], b[0]["final_cost"], np.abs(a[2] - b[2]).max(), abs(a[4] - b[4]), 1e3 * a[5], 1e3 * b[5],
            a[0]["iterations"] / a[5], b[0]["iterations"] / b[5]))
