"""Baseline-ranking measurement (sfmba_homography_ransac): one JSON line per shape.

  (a) 21 pairs x 1000 matches x 2000 hypotheses     (crazyhorse-like: every pair of 7 images, cv::findHomography's default maxIters)
  (b) 1225 pairs x 1000 matches x 2000 hypotheses   (every pair of 50 images in one call)

Per shape: the HIP-event times of the call's phases (SFMBA_HOMOGRAPHY_TIMING: upload, k_hom_hypotheses, k_hom_score, k_hom_select,
download; median over --reps calls after --warmup), the end-to-end call time and evaluations/s = pairs x hypotheses x matches over
the time of k_hom_score alone.  Every repetition is compared byte for byte with the first.  The pairs reach the device as a match
matrix does: every image holds the key points of all its pairs, shuffled, and the match lists index into them.
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

SHAPES = {"a": (7, 1000, 2000), "b": (50, 1000, 2000)}       # images (all pairs i < j), matches per pair, hypotheses
PHASES = ("upload_ms", "hypotheses_ms", "score_ms", "select_ms", "download_ms")


def make_batch(sfm, n_img, n_match, seed):
    """(pts_per_image, pairs, (pair_ptr, query_idx, train_idx), scenes): one planted homography per pair, 30 % clutter."""
    rng = np.random.default_rng(seed)
    blocks = [[] for _ in range(n_img)]
    pairs, scenes = [], []
    for i in range(n_img):
        for j in range(i + 1, n_img):
            sc = sfm.make_homography_scene(n_match, 0.3, seed + 1 + len(pairs))
            pairs.append((i, j))
            scenes.append(sc)
            blocks[i].append((len(pairs) - 1, 0, sc["left"]))
            blocks[j].append((len(pairs) - 1, 1, sc["right"]))
    pts, where = [], {}
    for i in range(n_img):
        allp = np.concatenate([b[2] for b in blocks[i]])
        perm = rng.permutation(len(allp))                     # key point k of the concatenation sits at row inv[k]
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        pts.append(np.ascontiguousarray(allp[perm]))
        at = 0
        for p, side, b in blocks[i]:
            where[(p, side)] = inv[at:at + len(b)].astype(np.int32)
            at += len(b)
    ptr = np.arange(len(pairs) + 1, dtype=np.int64) * n_match
    q = np.concatenate([where[(p, 0)] for p in range(len(pairs))])
    t = np.concatenate([where[(p, 1)] for p in range(len(pairs))])
    return pts, pairs, (ptr, q, t), scenes


def timed_call(capi, args, n_hyp):
    """(result, {phase: ms}, wall ms) of one call with SFMBA_HOMOGRAPHY_TIMING on; the library's stderr line is captured."""
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            res = capi.homography_ransac(*args, n_hyp=n_hyp)
            wall = 1e3 * (time.perf_counter() - t0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    m = re.findall(r"\[sfmba homography\] " + " ".join(k + r" (\S+)" for k in PHASES), text)
    if not m:
        raise RuntimeError("no timing line from the library: %r" % text)
    return res, dict(zip(PHASES, map(float, m[-1]))), wall


def same(a, b):
    return all(x["H"].tobytes() == y["H"].tobytes() and x["inlier"].tobytes() == y["inlier"].tobytes() and
               x["n_inliers"] == y["n_inliers"] and x["best_hypothesis"] == y["best_hypothesis"] for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_HOMOGRAPHY_TIMING"] = "1"
    import sfm_toy_library_amd as sfm
    from sfm_toy_library_amd import capi
    assert capi.device_count() >= 1
    for name in args.shapes.split(","):
        n_img, n_match, n_hyp = SHAPES[name]
        pts, pairs, matches, scenes = make_batch(sfm, n_img, n_match, 3000)
        call = (pts, pairs, matches)
        for _ in range(args.warmup):
            timed_call(capi, call, n_hyp)
        phases, walls, first = [], [], None
        for _ in range(args.reps):
            res, ph, wall = timed_call(capi, call, n_hyp)
            if first is None:
                first = res
            else:
                assert same(first, res), "two calls differ"
            phases.append(ph)
            walls.append(wall)
        med = {k: float(np.median([p[k] for p in phases])) for k in PHASES}
        evals = float(len(pairs)) * n_match * n_hyp
        held = [int((r["inlier"] & ~s["bad"]).sum()) >= 0.98 * int((~s["bad"]).sum()) for r, s in zip(first, scenes)]
        print(json.dumps(dict(
            shape=name, pairs=len(pairs), matches=n_match, hypotheses=n_hyp, evaluations=evals, reps=args.reps,
            hypotheses_us=round(1e3 * med["hypotheses_ms"], 1), score_us=round(1e3 * med["score_ms"], 1),
            select_us=round(1e3 * med["select_ms"], 1), kernels_us=round(1e3 * (med["hypotheses_ms"] + med["score_ms"] + med["select_ms"]), 1),
            upload_us=round(1e3 * med["upload_ms"], 1), download_us=round(1e3 * med["download_ms"], 1),
            call_ms=round(float(np.median(walls)), 3), call_ms_min=round(float(np.min(walls)), 3),
            score_evaluations_per_s=float("%.4g" % (evals / (med["score_ms"] * 1e-3))),
            status_ok=all(r["status"] == 0 for r in first), inlier_ratio_min=round(min(r["n_inliers"] / r["n_matches"] for r in first), 3),
            planted_inliers_held=all(held))), flush=True)


if __name__ == "__main__":
    main()
