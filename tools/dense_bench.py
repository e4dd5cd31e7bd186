"""Dense-stereo measurement (sfmba_depth_sweep, sfmba_depth_fuse): one JSON line per workload.

  (a) one 1024 x 768 job with 2 sources at D = 64, r = 3 (smoothed noise on a plane, tests/depth_cases.py, focal 2500)
  (b) the four 640 x 480 corner views of tests/sfm_scene.py in one call, true poses, every view against its two nearest
  (c) the fuse of (b)'s depth maps, every view checked against its sources

Per workload: the HIP-event times of the call's phases (SFMBA_DEPTH_TIMING; median over --reps calls after --warmup) and the
end-to-end call time.  For the sweep, the window operations -- one per reference pixel that takes part, plane, source and window
pixel, counted here from the images -- against the kernel time.  Every repetition is compared byte for byte with the first.
These are first measurements with nothing to compare against; nothing is gated on them.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SWEEP = ("upload_ms", "gray_ms", "sweep_ms", "download_ms")
FUSE = ("upload_ms", "flag_ms", "scan_ms", "emit_ms", "download_ms")
PARAMS = dict(n_planes=64, radius=3, min_std=2, min_score=0.6, min_sources=1)


def timed(call, tag, phases):
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            res = call()
            wall = 1e3 * (time.perf_counter() - t0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    m = re.findall(r"\[sfmba " + tag + r"\] " + " ".join(k + r" (\S+)" for k in phases), text)
    if not m:
        raise RuntimeError("no timing line from the library: %r" % text)
    return res, dict(zip(phases, map(float, m[-1]))), wall


def measure(call, tag, phases, same, reps, warmup):
    for _ in range(warmup):
        timed(call, tag, phases)
    rows, walls, first = [], [], None
    for _ in range(reps):
        res, ph, wall = timed(call, tag, phases)
        if first is None:
            first = res
        else:
            assert same(first, res), "two calls differ"
        rows.append(ph)
        walls.append(wall)
    med = {k: float(np.median([r[k] for r in rows])) for k in phases}
    return first, med, float(np.median(walls)), float(np.min(walls))


def window_ops(images, jobs, prm):
    import depth_oracle as do
    n = (2 * prm["radius"] + 1) ** 2
    total = 0
    for ref, srcs, _, _ in jobs:
        part = do._reference(do.gray(images[ref]), prm["radius"], prm["min_std"], do.box_integral)[4]
        total += int(part.sum()) * prm["n_planes"] * len(srcs) * n
    return total


def sweep_line(capi, name, images, K, P, jobs, args):
    same = lambda a, b: all(x[i].tobytes() == y[i].tobytes() for x, y in zip(a, b) for i in range(3))
    res, med, call, call_min = measure(lambda: capi.depth_sweep(images, K, P, jobs, **PARAMS), "depth_sweep", SWEEP, same, args.reps, args.warmup)
    ops = window_ops(images, jobs, PARAMS)
    out = dict(workload=name, jobs=len(jobs), sizes=sorted({images[j[0]].shape[::-1] for j in jobs}), sources=[len(j[1]) for j in jobs], reps=args.reps,
               accepted=[int((r[0] > 0).sum()) for r in res], **PARAMS)
    for k in SWEEP:
        out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
    out.update(call_ms=round(call, 3), call_ms_min=round(call_min, 3), window_ops=ops,
               window_Gops_per_s=float("%.4g" % (ops / (med["sweep_ms"] * 1e-3) / 1e9)))
    print(json.dumps(out), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b,c")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_DEPTH_TIMING"] = "1"
    from sfm_toy_library_amd import capi
    import depth_cases as dc
    import sfm_scene
    assert capi.device_count() >= 1
    todo = args.workloads.split(",")
    if "a" in todo:
        images, K, P = dc.scene((1024, 768), 2, focal=2500.0, scale=250.0)
        sweep_line(capi, "a", images, K, P, [(0, [1, 2], dc.Z_NEAR, dc.Z_FAR)], args)
    if "b" in todo or "c" in todo:
        sc = sfm_scene.make_corner(seed=0)
        images, K = sc["images"], sc["K"].astype(np.float32)
        P = np.concatenate([sc["R"], sc["t"][:, :, None]], axis=2).astype(np.float32)
        jobs = [(0, [1, 2], 8.5, 12.0), (1, [0, 2], 8.5, 12.0), (2, [1, 3], 8.5, 12.0), (3, [2, 1], 8.5, 12.0)]
        if "b" in todo:
            res = sweep_line(capi, "b", images, K, P, jobs, args)
        else:
            res = capi.depth_sweep(images, K, P, jobs, **PARAMS)
        if "c" in todo:
            maps, checks = [r[0] for r in res], [j[1] for j in jobs]
            same = lambda a, b: all(a[k].tobytes() == b[k].tobytes() for k in a)
            n = int(capi.depth_fuse(images, K, P, maps, checks)["pt_ptr"][-1])
            cloud, med, call, call_min = measure(lambda: capi.depth_fuse(images, K, P, maps, checks, cap=n), "depth_fuse", FUSE, same, args.reps, args.warmup)
            out = dict(workload="c", images=len(images), pixels_with_depth=int(sum((m > 0).sum() for m in maps)), points=int(cloud["pt_ptr"][-1]),
                       rel_tol=0.01, min_consistent=1, reps=args.reps)
            for k in FUSE:
                out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
            out.update(kernels_us=round(1e3 * (med["flag_ms"] + med["scan_ms"] + med["emit_ms"]), 1), call_ms=round(call, 3), call_ms_min=round(call_min, 3))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
