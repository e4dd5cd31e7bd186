"""Feature-extraction measurement (sfmba_orb_extract): one JSON line per shape.

  (a) 1 image  of 1024 x 768 at the reference's parameters (5000 features, 1.2, 8 levels, FAST threshold 20)
  (b) 7 images of 1024 x 768, one call

Per shape: the HIP-event times of the call's phases (SFMBA_ORB_TIMING, summed over the levels: upload, gray + resample, score,
flags + scan + compaction, response, the sort passes, smoothing, orientation + descriptor, pack + download; median over --reps
calls after --warmup) and the end-to-end call time.  For the two stencil kernels, the bytes each must move (every level read once
and written once: score map or smoothed level) against the time it took.  Every repetition is compared byte for byte with the
first.  The images are renderings of one synthetic scene (sfm_toy_library_amd.synthetic.render_orb_view) from different views.
"""
import argparse
import json
import math
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"a": 1, "b": 7}
W, H = 1024, 768
PHASES = ("upload_ms", "pyramid_ms", "score_ms", "candidates_ms", "response_ms", "select_ms", "smooth_ms", "describe_ms", "download_ms")


def timed_call(capi, imgs):
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            res = capi.orb_extract(imgs)
            wall = 1e3 * (time.perf_counter() - t0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    m = re.findall(r"\[sfmba orb\] " + " ".join(k + r" (\S+)" for k in PHASES), text)
    if not m:
        raise RuntimeError("no timing line from the library: %r" % text)
    return res, dict(zip(PHASES, map(float, m[-1]))), wall


def level_pixels(w, h, scale=float(np.float32(1.2)), n_levels=8):
    s, out = 1.0, []
    for _ in range(n_levels):
        wl, hl = int(math.floor(w / s + 0.5)), int(math.floor(h / s + 0.5))
        if wl > 62 and hl > 62:
            out.append(wl * hl)
        s *= scale
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_ORB_TIMING"] = "1"
    import sfm_toy_library_amd as sfm
    from sfm_toy_library_amd import capi
    assert capi.device_count() >= 1
    scene = sfm.make_orb_scene(1)
    views = [(0.0, 1.0, 0.0, 0.0), (0.1, 1.0, 40.0, 0.0), (0.2, 1.1, 0.0, 30.0), (0.3, 1.0, -40.0, 10.0), (0.4, 0.9, 20.0, -30.0),
             (0.5, 1.2, 0.0, 0.0), (0.6, 1.0, 60.0, 60.0)]
    rendered = [sfm.render_orb_view(scene, W, H, *v) for v in views]
    for name in args.shapes.split(","):
        imgs = rendered[:SHAPES[name]]
        for _ in range(args.warmup):
            timed_call(capi, imgs)
        phases, walls, first = [], [], None
        for _ in range(args.reps):
            res, ph, wall = timed_call(capi, imgs)
            if first is None:
                first = res
            else:
                assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(first, res)), "two calls differ"
            phases.append(ph)
            walls.append(wall)
        med = {k: float(np.median([p[k] for p in phases])) for k in PHASES}
        stencil_bytes = 2.0 * sum(level_pixels(W, H)) * len(imgs)          # a level read once, its map written once
        out = dict(shape=name, images=len(imgs), width=W, height=H, reps=args.reps, key_points=[len(r[0]) for r in first])
        for k in PHASES:
            out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
        out["kernels_us"] = round(1e3 * sum(med[k] for k in PHASES[1:8]), 1)
        out["call_ms"] = round(float(np.median(walls)), 3)
        out["call_ms_min"] = round(float(np.min(walls)), 3)
        out["stencil_bytes"] = stencil_bytes
        out["score_GBps"] = float("%.4g" % (stencil_bytes / (med["score_ms"] * 1e-3) / 1e9))
        out["smooth_GBps"] = float("%.4g" % (stencil_bytes / (med["smooth_ms"] * 1e-3) / 1e9))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
