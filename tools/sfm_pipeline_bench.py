"""Where the time of sfmtoylib::SfM::runSfM goes, and what batching the per-view triangulation saves (needs the MI355X).

  (1) runSfM on the "box" recipe of tests/sfm_scene.py at 6 and at 20 views (setFeatures: no extraction): the wall time of every stage
      as the class itself clocks it (SFMBA_SFM_TIMING, host clocks around stages that end in a device synchronise).  Each size runs
      in a fresh process, twice; the SECOND run is reported (the first pays the HIP context and the code objects).
  (2) the triangulation step of ONE added view -- the 19 pairs (good view, view 19) of the 20-view scene under the planted poses -- as
      one sfmba_triangulate_pairs call and as 19 sfmba_triangulate calls with the host alignment in front of each: the median wall
      time of --reps alternating repetitions after --warmup, and a byte comparison of the two results.

Nothing is gated on these times: the pipeline has no earlier version to be compared with.  One JSON line per measurement.

    python tools/sfm_pipeline_bench.py [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sfm_loop  # noqa: E402
import sfm_scene  # noqa: E402


def stage_times(n_views, tmp):
    scene = sfm_scene.make_box(seed=0, n_views=n_views)
    src = os.path.join(tmp, "box%d_in.npz" % n_views)
    np.savez(src, **sfm_loop.features_input(scene["views"], *scene["size"]))
    env = {k: v for k, v in os.environ.items() if not k.startswith("SFMBA_")}
    env.update(SFMBA_SFM_TIMING="1")
    outs = [os.path.join(tmp, "box%d_out%d.npz" % (n_views, k)) for k in range(2)]
    t0 = time.perf_counter()
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sfm_loop.py"), "class", src, outs[0], src, outs[1]], env=env, timeout=600,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    if done.returncode != 0:
        raise SystemExit("runSfM at %d views ended with %d:\n%s" % (n_views, done.returncode, done.stderr.decode()[-2000:]))
    lines = [l for l in done.stderr.decode().splitlines() if l.startswith("[sfmba sfm]")]
    if len(lines) != 2:
        raise SystemExit("expected two timing lines, got %d" % len(lines))
    res = dict(np.load(outs[1]))
    row = dict(measurement="runSfM stages, second run of a process", views=n_views, key_points=int(sum(len(v["xy"]) for v in scene["views"])),
               good_views=int(res["good"].sum()), cloud_points=int(len(res["xyz"])), process_wall_s=round(wall, 3))
    for name, ms in re.findall(r"(\w+)_ms ([0-9.]+)", lines[1]):
        row[name + "_ms"] = float(ms)
    row["total_ms"] = round(sum(v for k, v in row.items() if k.endswith("_ms")), 3)
    return row


def triangulation_step(n_views, reps, warmup):
    from sfm_toy_library_amd import capi
    scene = sfm_scene.make_box(seed=0, n_views=n_views)
    pts = [v["xy"] for v in scene["views"]]
    new = n_views - 1
    pairs = [(g, new) for g in range(new)]
    m = capi.match_features([v["desc"] for v in scene["views"]], pairs)
    _, _, ptr, q, t, _ = m
    P = np.concatenate([scene["R"], scene["t"][:, :, None]], axis=2).astype(np.float32)
    Pl, Pr = P[[g for g, _ in pairs]], P[[new] * len(pairs)]
    K = scene["K"].astype(np.float32)

    def batched():
        return capi.triangulate_pairs(pts, pairs, m, K, Pl, Pr)

    def singles():
        out = []
        for p, (l, r) in enumerate(pairs):
            a, b = int(ptr[p]), int(ptr[p + 1])
            out.append(capi.triangulate(K, Pl[p], Pr[p], pts[l][q[a:b]], pts[r][t[a:b]]))      # the host alignment, then one call
        return out

    for _ in range(warmup):
        batched(); singles()
    tb, ts = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); rb = batched(); t1 = time.perf_counter(); rs = singles(); t2 = time.perf_counter()
        tb.append(t1 - t0); ts.append(t2 - t1)
    same = all(rb["points3d"][ptr[p]:ptr[p + 1]].tobytes() == rs[p][0].tobytes() and np.array_equal(rb["keep"][ptr[p]:ptr[p + 1]], rs[p][1])
               for p in range(len(pairs)))
    return dict(measurement="triangulation step of one added view", pairs=len(pairs), matches=int(ptr[-1]), kept=int(rb["keep"].sum()),
                batched_call_ms=round(1e3 * float(np.median(tb)), 4), single_calls_ms=round(1e3 * float(np.median(ts)), 4),
                batched_min_ms=round(1e3 * min(tb), 4), single_min_ms=round(1e3 * min(ts), 4), reps=reps, same_bytes=bool(same))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        for n in (6, 20):
            print(json.dumps(stage_times(n, tmp)), flush=True)
    print(json.dumps(triangulation_step(20, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
