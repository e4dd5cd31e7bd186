"""Seam-levelling measurement (sfmba_mesh_texture_adjust): one JSON line per workload and area floor.

  corner      the four rendered 640 x 480 corner views of tests/sfm_scene.py through SfM::runSfM, densify and meshDenseCloud at
              resolution 256 (the mesh of tools/texture_bench.py)
  crazyhorse  the seven Crazy Horse photographs at 512 x 384 (tests/golden/crazyhorse_half) through the same steps

Per workload, on the mesh the class made and with the host rules of host/SfM.h, at min_area 0 and at the default floor: the HIP-event
times of the phases of one sfmba_mesh_texture_adjust call at sfmtoy's defaults (K = 4, 4 rings, penalty 256, at most 100 relaxation passes; 16 levelling
passes, seam weight 16, sample radius 1; SFMBA_MESH_TEXTURE_TIMING; median over --reps calls after --warmup) -- keys, sort, nodes, colours,
the passes, the statistics and the levelled raster -- the time per pass, its end-to-end time against the sfmba_mesh_texture_smooth call
IN THE SAME RUN, the nodes, the seam vertices, the spread before and after and the clamped texels.  Every repetition is compared byte for
byte with the first.  First measurements of untuned defaults; nothing is gated on them, and there is no earlier time for this path.
"""
import argparse
import glob
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

TEXTURE = ("upload_ms", "check_ms", "views_ms", "raster_ms", "download_ms")
LEVEL = ("keys_ms", "sort_ms", "nodes_ms", "colours_ms", "passes_ms", "stats_ms")
STATS = ("nodes", "blind", "seam_vertices", "spread_before", "spread_after", "max_offset", "n_clamped", "n_passes")
K, RINGS, PENALTY, PASSES, RADIUS, WEIGHT, LEVEL_PASSES = 4, 4, 256, 100, 1, 16, 16


def timed(call, patterns):
    """(result, one dict of phases per pattern, wall ms) of one call: the library prints one line per pattern"""
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
    out = []
    for head, phases in patterns:
        m = re.findall(re.escape(head) + " " + " ".join(k + r" (\S+)" for k in phases), text)
        if not m:
            raise RuntimeError("no timing line from the library: %r" % text)
        out.append(dict(zip(phases, map(float, m[-1]))))
    return res, out, wall


def workload(capi, name, images, args):
    import texture_pipeline_run as run
    cls = run.run_class_texture(dict(images=images))
    xyz, bgr, tri = cls["mesh_xyz"], cls["mesh_bgr"], cls["mesh_tri"]
    nt = len(tri)
    occl_tol, floor, B = run.host_rules(cls, nt)
    maps = [m if has else None for m, has in zip(cls["depth"], cls["has_map"])]
    same = lambda a, b: all((a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    for min_area in (0, floor):
        shared = (xyz, bgr, tri, list(images), cls["K"], cls["poses"], maps, occl_tol, min_area, 6, B, K, RINGS, PENALTY, PASSES)
        smooth = lambda: capi.mesh_texture_smooth(*shared)
        adjust = lambda: capi.mesh_texture_adjust(*shared, RADIUS, WEIGHT, LEVEL_PASSES)
        smooth_lines = [("[sfmba mesh_texture_smooth]", TEXTURE)]
        adjust_lines = [("[sfmba mesh_texture_adjust]", TEXTURE), ("[sfmba mesh_texture_adjust level]", LEVEL)]
        for _ in range(args.warmup):
            timed(smooth, smooth_lines)
            timed(adjust, adjust_lines)
        srows = [timed(smooth, smooth_lines) for _ in range(args.reps)]
        rows = [timed(adjust, adjust_lines) for _ in range(args.reps)]
        for r in rows[1:]:
            assert same(rows[0][0], r[0]), "two calls differ"
        for k in ("uv", "view", "score", "stats"):
            assert np.asarray(rows[0][0][k]).tobytes() == np.asarray(srows[0][0][k]).tobytes(), k
        st = rows[0][0]["level_stats"]
        tex = {k: float(np.median([r[1][0][k] for r in rows])) for k in TEXTURE}
        lev = {k: float(np.median([r[1][1][k] for r in rows])) for k in LEVEL}
        out = dict(workload=name, views=len(images), triangles=nt, min_area=int(min_area), candidates=K, rings=RINGS, penalty=PENALTY, max_passes=PASSES,
                   sample_radius=RADIUS, seam_weight=WEIGHT, level_passes=LEVEL_PASSES, reps=args.reps, **{k: int(v) for k, v in zip(STATS, st.tolist())})
        out.update(spread_ratio=round(st[4] / max(st[3], 1), 4), texels_changed=int((rows[0][0]["atlas"] != srows[0][0]["atlas"]).any(axis=2).sum()))
        for k in LEVEL:
            out[k.replace("_ms", "_us")] = round(1e3 * lev[k], 1)
        out.update(pass_us=round(1e3 * lev["passes_ms"] / LEVEL_PASSES, 2), raster_us=round(1e3 * tex["raster_ms"], 1),
                   smooth_raster_us=round(1e3 * float(np.median([r[1][0]["raster_ms"] for r in srows])), 1),
                   call_ms=round(float(np.median([r[2] for r in rows])), 3), call_ms_min=round(float(np.min([r[2] for r in rows])), 3),
                   smooth_call_ms=round(float(np.median([r[2] for r in srows])), 3), smooth_call_ms_min=round(float(np.min([r[2] for r in srows])), 3))
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="corner,crazyhorse")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_MESH_TEXTURE_TIMING"] = "1"
    os.environ.setdefault("SFMBA_DETERMINISTIC", "1")
    from sfm_toy_library_amd import capi
    assert capi.device_count() >= 1
    todo = args.workloads.split(",")
    if "corner" in todo:
        import sfm_scene
        workload(capi, "corner", np.stack(sfm_scene.make_corner(seed=0)["images"]), args)
    if "crazyhorse" in todo:
        files = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "crazyhorse_half", "*.JPG")))]
        info, images = capi.jpeg_decode(files)
        assert len(images) == 7 and all(im is not None for im in images)
        workload(capi, "crazyhorse", np.stack(images), args)


if __name__ == "__main__":
    main()
