"""Float-matcher measurement (sfmba_match_features_l2): one JSON line per shape.

  (a) 7 images x 5000 x 128 floats, all 21 pairs   (the Crazy Horse shape with SIFT-length rows)
  (b) 50 images x 5000 x 128 floats, all 1225 pairs
  (c) 7 images x 5000 x 256 floats, all 21 pairs

Per shape: the HIP-event times of the call's phases (SFMBA_MATCH_TIMING: upload, top-2 + merge kernels, compaction, download;
median over --reps calls after --warmup), the end-to-end call time, subtract-fma pairs/s over the top-2 kernels (one pair = one
column of one (query, train) distance), and the share of the packed-fp32 issue ceiling: the fp32 vector rate is 64 FLOP per clock
and SIMD, i.e. 32 packed element operations, a subtract-fma pair is two of them (half a v_pk_add_f32 and half a v_pk_fma_f32), so
256 CUs x 4 SIMDs x 16 pairs x 2.4 GHz = 3.93e13 pairs/s.  The clock is the 2.4 GHz peak engine clock; the clock under load is
lower, so the share is a lower bound on the share of the issue rate at the real clock.  --check compares the first three pairs of
(a) with the oracle of tests/match_l2_oracle.py.
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

CEILING = 256 * 4 * 16 * 2.4e9
SHAPES = {"a": (7, 5000, 128), "b": (50, 5000, 128), "c": (7, 5000, 256)}


def make_rows(n_img, n_rows, dims, seed=2024):
    """SIFT-like rows (integers 0..255 as float32): every image shows about 60 % of a common pool of rows, each copy disturbed."""
    rng = np.random.default_rng(seed)
    pool = np.minimum(255, np.floor(rng.exponential(30.0, (2 * n_rows, dims)))).astype(np.float32)
    out = []
    for _ in range(n_img):
        rows = pool[rng.choice(len(pool), n_rows, replace=False)] + rng.integers(-3, 4, (n_rows, dims)).astype(np.float32)
        out.append(np.ascontiguousarray(np.clip(rows, 0, 255), np.float32))
    return out


def timed_call(capi, descs):
    """(result, {phase: ms}, wall ms) of one call with SFMBA_MATCH_TIMING on; the library's stderr line is captured."""
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            res = capi.match_features_l2(descs)
            wall = 1e3 * (time.perf_counter() - t0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    m = re.findall(r"\[sfmba match_l2\] upload_ms (\S+) top2_ms (\S+) compact_ms (\S+) download_ms (\S+) batches (\d+)", text)
    if not m:
        raise RuntimeError("no timing line from the library: %r" % text)
    up, top2, comp, down, batches = m[-1]
    return res, dict(upload_ms=float(up), top2_ms=float(top2), compact_ms=float(comp), download_ms=float(down), batches=int(batches)), wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    os.environ["SFMBA_MATCH_TIMING"] = "1"
    from sfm_toy_library_amd import capi
    assert capi.device_count() >= 1
    for name in args.shapes.split(","):
        n_img, n_rows, dims = SHAPES[name]
        descs = make_rows(n_img, n_rows, dims)
        n_pairs = n_img * (n_img - 1) // 2
        n_fma = float(n_pairs) * n_rows * n_rows * dims
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
            import match_l2_oracle as lo
            pl, pr, ptr, q, t, d = first
            db = d.view(np.uint32)
            checked = True
            for p in range(3):
                want = lo.match_pair(descs[pl[p]], descs[pr[p]])
                got = list(zip(q[ptr[p]:ptr[p + 1]].tolist(), t[ptr[p]:ptr[p + 1]].tolist(), db[ptr[p]:ptr[p + 1]].tolist()))
                checked = checked and got == want
        rate = n_fma / (med["top2_ms"] * 1e-3)
        print(json.dumps(dict(
            shape=name, images=n_img, rows=n_rows, dims=dims, pairs=n_pairs, sub_fma_pairs=n_fma, matches=int(first[2][-1]),
            batches=phases[0]["batches"], reps=args.reps, kernel_us=round(1e3 * med["top2_ms"], 1),
            compact_us=round(1e3 * med["compact_ms"], 1), upload_us=round(1e3 * med["upload_ms"], 1),
            download_us=round(1e3 * med["download_ms"], 1), call_ms=round(float(np.median(walls)), 3),
            call_ms_min=round(float(np.min(walls)), 3), sub_fma_pairs_per_s=float("%.4g" % rate),
            packed_fp32_ceiling_per_s=float("%.4g" % CEILING), share_of_ceiling_at_2_4GHz=round(rate / CEILING, 4),
            oracle_exact=checked)), flush=True)


if __name__ == "__main__":
    main()
