"""Optical-flow matcher measurement (sfmba_flow_track, sfmba_flow_match): one JSON line per workload; --out FILE also appends the
lines to FILE (profiles/flow_track.txt holds them with what they say).

  (a) a frame sequence: 7 renderings of one synthetic scene (sfm_toy_library_amd.synthetic.render_orb_view) at 1024 x 768, the view
      moved by (3.3, -2.6) px from frame to frame; the key points are sfmba_orb_extract's (5000 per image); the 6 consecutive pairs
      in ONE sfmba_flow_track call and ONE sfmba_flow_match call with the defaults (L = 4, r = 7, max_iters 20, min_eig 1; 12, 2, 0.7)
  (b) the same pair list through the ORB-descriptor matcher (sfmba_match_features), for comparison

Per workload: the HIP-event times of the call's phases (SFMBA_FLOW_TIMING / SFMBA_MATCH_TIMING; median over --reps calls after
--warmup) and the end-to-end call time.  For the tracker, the samples it takes -- per (point, level) the (2r+3)^2 template, n per
iteration and n for err, counted here from the debug arrays -- against the kernel time.  Every repetition is compared byte for byte
with the first.  These are first measurements with nothing to compare against; nothing is gated on them.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dense_bench import measure          # noqa: E402  (the stderr-capturing timer of the dense unit's bench)

TRACK = ("upload_ms", "gray_ms", "pyramid_ms", "track_ms", "download_ms")
MATCH = ("upload_ms", "near_ms", "compact_ms", "download_ms")
ORB = ("upload_ms", "top2_ms", "compact_ms", "download_ms")
PARAMS = dict(n_levels=4, radius=7, max_iters=20, min_eig=1.0)
SNAP = dict(max_err=12.0, radius=2.0, ratio=0.7)
W, H, FRAMES, STEP = 1024, 768, 7, (3.3, -2.6)


def samples_taken(debug_out, radius):
    n, side = (2 * radius + 1) ** 2, (2 * radius + 3) ** 2
    total = 0
    for nxt, status, err, G, state in debug_out:
        total += state.shape[0] * state.shape[1] * side + int(state[:, :, 1].sum()) * n + int(state[:, 0, 0].sum()) * n
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    os.environ["SFMBA_FLOW_TIMING"] = "1"
    os.environ["SFMBA_MATCH_TIMING"] = "1"
    import sfm_toy_library_amd as sfm
    from sfm_toy_library_amd import capi
    assert capi.device_count() >= 1
    scene = sfm.make_orb_scene(1)
    images = [sfm.render_orb_view(scene, W, H, 0.0, 1.0, -k * STEP[0], -k * STEP[1]) for k in range(FRAMES)]
    feats = capi.orb_extract(images)
    kps = [np.stack([f[0]["x"], f[0]["y"]], axis=1).astype(np.float32) for f in feats]
    descs = [f[1] for f in feats]
    pairs = [(i, i + 1) for i in range(FRAMES - 1)]
    points = [kps[i] for i, _ in pairs]
    lines = []

    def emit(out):
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)

    same3 = lambda a, b: all(x[i].tobytes() == y[i].tobytes() for x, y in zip(a, b) for i in range(3))
    tracked, med, call, call_min = measure(lambda: capi.flow_track(images, pairs, points, **PARAMS), "flow_track", TRACK + ("groups",), same3,
                                           args.reps, args.warmup)
    dbg, _ = capi.flow_track(images, pairs, points, debug=True, **PARAMS)
    n_samples = samples_taken(dbg, PARAMS["radius"])
    moved = np.concatenate([t[0] - p for t, p in zip(tracked, points)])
    ok = np.concatenate([(t[1] == 1) & (t[2] < SNAP["max_err"]) for t in tracked])
    out = dict(workload="a:track", pairs=len(pairs), size=[W, H], points=[len(p) for p in points], reps=args.reps, **PARAMS)
    for k in TRACK:
        out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
    out.update(call_ms=round(call, 3), call_ms_min=round(call_min, 3), eligible=int(ok.sum()),
               within_quarter_px_of_the_step=int((np.abs(moved[ok] - np.asarray(STEP, np.float32)).max(axis=1) <= 0.25).sum()),
               iterations_level0_mean=float("%.4g" % np.mean([d[4][:, 0, 1].mean() for d in dbg])), samples=n_samples,
               Gsamples_per_s=float("%.4g" % (n_samples / (med["track_ms"] * 1e-3) / 1e9)))
    emit(out)

    same4 = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    res, med, call, call_min = measure(lambda: capi.flow_match(kps, pairs, tracked, **SNAP), "flow_match", MATCH, same4, args.reps, args.warmup)
    out = dict(workload="a:match", pairs=len(pairs), queries=int(sum(len(p) for p in points)), matches=np.diff(res[0]).tolist(), reps=args.reps, **SNAP)
    for k in MATCH:
        out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
    out.update(kernels_us=round(1e3 * (med["near_ms"] + med["compact_ms"]), 1), call_ms=round(call, 3), call_ms_min=round(call_min, 3))
    emit(out)

    same6 = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    res, med, call, call_min = measure(lambda: capi.match_features(descs, pairs), "match", ORB + ("batches",), same6, args.reps, args.warmup)
    out = dict(workload="b:descriptors", pairs=len(pairs), queries=int(sum(len(p) for p in points)), matches=np.diff(res[2]).tolist(), reps=args.reps)
    for k in ORB:
        out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
    out.update(kernels_us=round(1e3 * (med["top2_ms"] + med["compact_ms"]), 1), call_ms=round(call, 3), call_ms_min=round(call_min, 3))
    emit(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
