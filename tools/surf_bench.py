"""Float-descriptor extraction measurement (sfmba_surf_extract): one JSON line per shape.

  (a) 1 image  of 1024 x 768 at the class's parameters (5000 features, 4 octaves, threshold 100, oriented)
  (b) 7 images of 1024 x 768, one call

Per shape: the HIP-event times of the call's phases (SFMBA_SURF_TIMING, summed over the octaves: upload, gray + integral image,
response, candidates, the count read-back + sort passes, orientation + descriptor, download; median over --reps calls after
--warmup) and the end-to-end call time.  For the response kernel, the bytes it writes (8 per sample it computes, as the library
counts them) plus the integral image read once, against the time it took.  Every repetition is compared byte for byte with the
first.  The images are renderings of one synthetic scene (sfm_toy_library_amd.synthetic.render_orb_view) from different views.
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

SHAPES = {"a": 1, "b": 7}
W, H = 1024, 768
PHASES = ("upload_ms", "integral_ms", "response_ms", "candidates_ms", "select_ms", "describe_ms", "download_ms")


def timed_call(capi, imgs):
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            res = capi.surf_extract(imgs)
            wall = 1e3 * (time.perf_counter() - t0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    m = re.findall(r"\[sfmba surf\] " + " ".join(k + r" (\S+)" for k in PHASES) + r" groups (\d+) response_bytes (\d+)", text)
    if not m:
        raise RuntimeError("no timing line from the library: %r" % text)
    return res, dict(zip(PHASES, map(float, m[-1][:len(PHASES)]))), wall, float(m[-1][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_SURF_TIMING"] = "1"
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
        phases, walls, first, written = [], [], None, 0.0
        for _ in range(args.reps):
            res, ph, wall, written = timed_call(capi, imgs)
            if first is None:
                first = res
            else:
                assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(first, res)), "two calls differ"
            phases.append(ph)
            walls.append(wall)
        med = {k: float(np.median([p[k] for p in phases])) for k in PHASES}
        read = 4.0 * (W + 1) * (H + 1) * len(imgs)                          # the integral image, read at least once
        out = dict(shape=name, images=len(imgs), width=W, height=H, reps=args.reps, key_points=[len(r[0]) for r in first])
        for k in PHASES:
            out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
        out["kernels_us"] = round(1e3 * sum(med[k] for k in PHASES[1:6]), 1)
        out["call_ms"] = round(float(np.median(walls)), 3)
        out["call_ms_min"] = round(float(np.min(walls)), 3)
        out["response_bytes_written"] = written
        out["response_bytes_read"] = read
        out["response_GBps"] = float("%.4g" % ((written + read) / (med["response_ms"] * 1e-3) / 1e9))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
