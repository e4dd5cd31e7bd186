"""Baseline-pose measurement (sfmba_essential_ransac): one JSON line per shape.

  (a) 1 pair x 2000 matches x 1000 hypotheses      (one call of findCameraMatricesFromMatch; cv::findEssentialMat's maxIters)
  (b) 199 pairs x 2000 matches x 1000 hypotheses   (the pairs (good view, new view) when the 200th view is added, in one call)

Per shape: the HIP-event times of the call's phases (SFMBA_ESSENTIAL_TIMING: upload, k_ess_hypotheses, k_ess_score, k_ess_select,
download; median over --reps calls after --warmup), the end-to-end call time and evaluations/s = pairs x hypotheses x matches over
the time of k_ess_score alone.  Every repetition is compared byte for byte with the first.  The pairs reach the device as a match
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

SHAPES = {"a": (2, 2000, 1000), "b": (200, 2000, 1000)}       # images (every earlier image against the last), matches per pair, hypotheses
PHASES = ("upload_ms", "hypotheses_ms", "score_ms", "select_ms", "download_ms")


def make_batch(sfm, n_img, n_match, seed):
    """(pts_per_image, pairs, (pair_ptr, query_idx, train_idx), scenes): one planted relative pose per pair, 30 % clutter."""
    rng = np.random.default_rng(seed)
    blocks = [[] for _ in range(n_img)]
    pairs, scenes = [], []
    for i in range(n_img - 1):
        sc = sfm.make_essential_scene(n_match, 0.3, seed + 1 + i)
        pairs.append((i, n_img - 1))
        scenes.append(sc)
        blocks[i].append((i, 0, sc["left"]))
        blocks[n_img - 1].append((i, 1, sc["right"]))
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


def timed_call(capi, args, K, n_hyp):
    """(result, {phase: ms}, wall ms) of one call with SFMBA_ESSENTIAL_TIMING on; the library's stderr line is captured."""
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            res = capi.essential_ransac(*args, K, n_hyp=n_hyp, threshold_px=1.0)
            wall = 1e3 * (time.perf_counter() - t0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    m = re.findall(r"\[sfmba essential\] " + " ".join(k + r" (\S+)" for k in PHASES), text)
    if not m:
        raise RuntimeError("no timing line from the library: %r" % text)
    return res, dict(zip(PHASES, map(float, m[-1]))), wall


def same(a, b):
    return all(x["E"].tobytes() == y["E"].tobytes() and x["pose"].tobytes() == y["pose"].tobytes() and x["inlier"].tobytes() == y["inlier"].tobytes() and
               x["n_inliers"] == y["n_inliers"] and x["best_hypothesis"] == y["best_hypothesis"] for x, y in zip(a, b))


def angle_deg(c):
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_ESSENTIAL_TIMING"] = "1"
    import sfm_toy_library_amd as sfm
    from sfm_toy_library_amd import capi
    assert capi.device_count() >= 1
    for name in args.shapes.split(","):
        n_img, n_match, n_hyp = SHAPES[name]
        pts, pairs, matches, scenes = make_batch(sfm, n_img, n_match, 4000)
        call = (pts, pairs, matches)
        K = scenes[0]["K"]
        for _ in range(args.warmup):
            timed_call(capi, call, K, n_hyp)
        phases, walls, first = [], [], None
        for _ in range(args.reps):
            res, ph, wall = timed_call(capi, call, K, n_hyp)
            if first is None:
                first = res
            else:
                assert same(first, res), "two calls differ"
            phases.append(ph)
            walls.append(wall)
        med = {k: float(np.median([p[k] for p in phases])) for k in PHASES}
        evals = float(len(pairs)) * n_match * n_hyp
        held = [int((r["inlier"] & ~s["bad"]).sum()) / max(int((~s["bad"]).sum()), 1) for r, s in zip(first, scenes)]
        rot = [angle_deg((np.trace(r["pose"][:, :3].T @ s["R"]) - 1.0) / 2.0) for r, s in zip(first, scenes)]
        tra = [angle_deg(r["pose"][:, 3] @ s["t"]) for r, s in zip(first, scenes)]
        print(json.dumps(dict(
            shape=name, pairs=len(pairs), matches=n_match, hypotheses=n_hyp, evaluations=evals, reps=args.reps,
            hypotheses_us=round(1e3 * med["hypotheses_ms"], 1), score_us=round(1e3 * med["score_ms"], 1),
            select_us=round(1e3 * med["select_ms"], 1), kernels_us=round(1e3 * (med["hypotheses_ms"] + med["score_ms"] + med["select_ms"]), 1),
            upload_us=round(1e3 * med["upload_ms"], 1), download_us=round(1e3 * med["download_ms"], 1),
            call_ms=round(float(np.median(walls)), 3), call_ms_min=round(float(np.min(walls)), 3),
            score_evaluations_per_s=float("%.4g" % (evals / (med["score_ms"] * 1e-3))),
            hypotheses_per_s=float("%.4g" % (len(pairs) * n_hyp / (med["hypotheses_ms"] * 1e-3))),
            status_ok=all(r["status"] == 0 for r in first), planted_inliers_held_min=round(min(held), 4),
            rotation_deg_max=round(max(rot), 3), translation_deg_max=round(max(tra), 3))), flush=True)


if __name__ == "__main__":
    main()
