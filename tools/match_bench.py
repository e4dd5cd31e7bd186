"""Feature-matcher measurement (sfmba_match_features): one JSON line per shape.

  (a) 7 images x 5000 x 32 B, all 21 pairs   (the Crazy Horse shape)
  (b) 50 images x 5000 x 32 B, all 1225 pairs

Per shape: the HIP-event times of the call's phases (SFMBA_MATCH_TIMING: upload, top-2 + merge kernels, compaction, download;
median over --reps calls after --warmup), the end-to-end call time, distances/s over the top-2 kernels, and the fraction of the
VALU-issue ceiling 256 CUs x 4 SIMD x 32 lanes x 2.4 GHz / 20 VALU instructions per distance = 3.93e12 distances/s (the clock is the
2.4 GHz peak engine clock; the clock under load is lower, so the fraction is a lower bound on the fraction of the issue rate
at the real clock).  --check compares every call of (a) with the oracle of tests/match_oracle.py (slow: ~40 s).
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

CEILING = 256 * 4 * 32 * 2.4e9 / 20
SHAPES = {"a": (7, 5000, 32), "b": (50, 5000, 32)}


def timed_call(capi, descs):
    """(result, {phase: ms}, wall ms) of one call with SFMBA_MATCH_TIMING on; the library's stderr line is captured."""
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            res = capi.match_features(descs)
            wall = 1e3 * (time.perf_counter() - t0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    m = re.findall(r"\[sfmba match\] upload_ms (\S+) top2_ms (\S+) compact_ms (\S+) download_ms (\S+) batches (\d+)", text)
    if not m:
        raise RuntimeError("no timing line from the library: %r" % text)
    up, top2, comp, down, batches = m[-1]
    return res, dict(upload_ms=float(up), top2_ms=float(top2), compact_ms=float(comp), download_ms=float(down), batches=int(batches)), wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    os.environ["SFMBA_MATCH_TIMING"] = "1"
    import sfm_toy_library_amd as sfm
    from sfm_toy_library_amd import capi
    assert capi.device_count() >= 1
    for name in args.shapes.split(","):
        n_img, n_rows, nbytes = SHAPES[name]
        descs = sfm.make_descriptors(n_img, n_rows, nbytes, seed=2024, extras=False)
        n_pairs = n_img * (n_img - 1) // 2
        n_dist = float(n_pairs) * n_rows * n_rows
        for _ in range(args.warmup):
            timed_call(capi, descs)
        phases, walls, first = [], [], None
        for _ in range(args.reps):
            res, ph, wall = timed_call(capi, descs)
            if first is None:
                first = res
            else:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(first, res)), "two calls differ"
            phases.append(ph)
            walls.append(wall)
        med = {k: float(np.median([p[k] for p in phases])) for k in ("upload_ms", "top2_ms", "compact_ms", "download_ms")}
        checked = None
        if args.check and name == "a":
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import match_oracle as mo
            want = mo.match_features(descs, knn=mo.knn_keys)
            pl, pr, ptr, q, t, d = first
            got = [((int(pl[p]), int(pr[p])), list(zip(q[ptr[p]:ptr[p + 1]].tolist(), t[ptr[p]:ptr[p + 1]].tolist(),
                                                       d[ptr[p]:ptr[p + 1]].tolist()))) for p in range(len(pl))]
            checked = got == want
        rate = n_dist / (med["top2_ms"] * 1e-3)
        print(json.dumps(dict(
            shape=name, images=n_img, rows=n_rows, desc_bytes=nbytes, pairs=n_pairs, distances=n_dist, matches=int(first[2][-1]),
            batches=phases[0]["batches"], reps=args.reps, kernel_us=round(1e3 * med["top2_ms"], 1),
            compact_us=round(1e3 * med["compact_ms"], 1), upload_us=round(1e3 * med["upload_ms"], 1),
            download_us=round(1e3 * med["download_ms"], 1), call_ms=round(float(np.median(walls)), 3),
            call_ms_min=round(float(np.min(walls)), 3), distances_per_s=float("%.4g" % rate),
            valu_ceiling_per_s=float("%.4g" % CEILING), fraction_of_ceiling_at_2_4GHz=round(rate / CEILING, 4),
            oracle_exact=checked)), flush=True)


if __name__ == "__main__":
    main()
