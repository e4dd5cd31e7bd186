"""Pose measurement (sfmba_pnp_ransac): one JSON line per shape.

  (a) 1 view x 2000 points x 100 hypotheses      (the reference's shape: one solvePnPRansac call, iterationsCount = 100)
  (b) 49 views x 5000 points x 1024 hypotheses   (every not-yet-registered view of a 50-image set posed in one call)

Per shape: the HIP-event times of the call's phases (SFMBA_PNP_TIMING: upload, the three kernels, download; median over --reps
calls after --warmup), the end-to-end call time and projections/s = problems x hypotheses x points over the kernel time (the
score kernel does that many; the hypothesis and refinement kernels are inside the same events).  Every repetition is compared
byte for byte with the first.  Kernel by kernel: run this under rocprofv3 --kernel-trace --stats, in a run of its own.
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"a": (1, 2000, 100), "b": (49, 5000, 1024)}


def timed_call(capi, probs, K, n_hyp):
    """(result, {phase: ms}, wall ms) of one call with SFMBA_PNP_TIMING on; the library's stderr line is captured."""
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            res = capi.pnp_ransac(probs, K, n_hyp=n_hyp)
            wall = 1e3 * (time.perf_counter() - t0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    m = re.findall(r"\[sfmba pnp\] upload_ms (\S+) kernels_ms (\S+) download_ms (\S+)", text)
    if not m:
        raise RuntimeError("no timing line from the library: %r" % text)
    up, kern, down = m[-1]
    return res, dict(upload_ms=float(up), kernels_ms=float(kern), download_ms=float(down)), wall


def same(a, b):
    return all(x["pose"].tobytes() == y["pose"].tobytes() and x["inlier"].tobytes() == y["inlier"].tobytes() and
               x["n_inliers"] == y["n_inliers"] and x["refine_cost"] == y["refine_cost"] for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_PNP_TIMING"] = "1"
    import sfm_toy_library_amd as sfm
    from sfm_toy_library_amd import capi
    assert capi.device_count() >= 1
    for name in args.shapes.split(","):
        n_prob, n_pts, n_hyp = SHAPES[name]
        scenes = [sfm.make_pnp_scene(n_pts, 0.3, 2024 + p) for p in range(n_prob)]
        probs = [(s["X"], s["uv"]) for s in scenes]
        K = scenes[0]["K"]
        for _ in range(args.warmup):
            timed_call(capi, probs, K, n_hyp)
        phases, walls, first = [], [], None
        for _ in range(args.reps):
            res, ph, wall = timed_call(capi, probs, K, n_hyp)
            if first is None:
                first = res
            else:
                assert same(first, res), "two calls differ"
            phases.append(ph)
            walls.append(wall)
        med = {k: float(np.median([p[k] for p in phases])) for k in ("upload_ms", "kernels_ms", "download_ms")}
        proj = float(n_prob) * n_pts * n_hyp
        held = [int((r["inlier"] & ~s["bad"]).sum()) == int((~s["bad"]).sum()) for r, s in zip(first, scenes)]
        print(json.dumps(dict(
            shape=name, problems=n_prob, points=n_pts, hypotheses=n_hyp, projections=proj, reps=args.reps,
            kernels_us=round(1e3 * med["kernels_ms"], 1), upload_us=round(1e3 * med["upload_ms"], 1),
            download_us=round(1e3 * med["download_ms"], 1), call_ms=round(float(np.median(walls)), 3),
            call_ms_min=round(float(np.min(walls)), 3), projections_per_s=float("%.4g" % (proj / (med["kernels_ms"] * 1e-3))),
            status_ok=all(r["status"] == 0 for r in first), refine_iters_max=max(r["refine_iters"] for r in first),
            every_planted_inlier_held=all(held))), flush=True)


if __name__ == "__main__":
    main()
