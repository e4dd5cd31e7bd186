"""Label-smoothing measurement (sfmba_mesh_texture_smooth): one JSON line per workload and area floor.

  corner      the four rendered 640 x 480 corner views of tests/sfm_scene.py through SfM::runSfM, densify and meshDenseCloud at
              resolution 256 (the mesh of tools/texture_bench.py)
  crazyhorse  the seven Crazy Horse photographs at 512 x 384 (tests/golden/crazyhorse_half) through the same steps

Per workload, on the mesh the class made and with the host rules of host/SfM.h, at min_area 0 and at the default floor: the HIP-event
times of the phases of one sfmba_mesh_texture_smooth call at sfmtoy's --texture-smooth defaults (K = 4, 4 rings, penalty 256, at most 100
passes; SFMBA_MESH_TEXTURE_TIMING; median over --reps calls after --warmup) -- candidates, keys, sort, link, the ring passes, the start,
the gain passes, the move passes, the statistics, and the raster -- its end-to-end time against the plain sfmba_mesh_texture call IN THE
SAME RUN, and the eight statistics as shares of the mesh's linked pairs.  Every repetition is compared byte for byte with the first.
First measurements; nothing is gated on them.
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

from dense_bench import measure  # noqa: E402

TEXTURE = ("upload_ms", "check_ms", "views_ms", "raster_ms", "download_ms")
LABELS = ("upload_ms", "candidates_ms", "keys_ms", "sort_ms", "link_ms", "rings_ms", "start_ms", "gain_ms", "move_ms", "stats_ms", "download_ms")
STATS = ("energy_start", "energy_end", "diff_rank0", "diff_start", "diff_end", "frontier", "moves", "n_passes")
K, RINGS, PENALTY, PASSES = 4, 4, 256, 100


def timed_smooth(call):
    """(result, the label phases, the texture phases, wall ms) of one call: the library prints one line of each"""
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
    for phases in (LABELS, TEXTURE):
        m = re.findall(r"\[sfmba mesh_texture_smooth\] " + " ".join(k + r" (\S+)" for k in phases), text)
        if not m:
            raise RuntimeError("no timing line from the library: %r" % text)
        out.append(dict(zip(phases, map(float, m[-1]))))
    return res, out[0], out[1], wall


def workload(capi, name, images, args):
    import texture_pipeline_run as run
    cls = run.run_class_texture(dict(images=images))
    xyz, bgr, tri = cls["mesh_xyz"], cls["mesh_bgr"], cls["mesh_tri"]
    nt = len(tri)
    occl_tol, floor, B = run.host_rules(cls, nt)
    maps = [m if has else None for m, has in zip(cls["depth"], cls["has_map"])]
    same = lambda a, b: all((a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    adj = capi.mesh_adjacency(tri)
    pairs = adj["n_pairs"]
    for min_area in (0, floor):
        plain = lambda: capi.mesh_texture(xyz, bgr, tri, list(images), cls["K"], cls["poses"], maps, occl_tol, min_area, 6, B)
        smooth = lambda: capi.mesh_texture_smooth(xyz, bgr, tri, list(images), cls["K"], cls["poses"], maps, occl_tol, min_area, 6, B, K, RINGS, PENALTY,
                                                  PASSES)
        _, pmed, pwall, pwall_min = measure(plain, "mesh_texture", TEXTURE, same, args.reps, args.warmup)
        for _ in range(args.warmup):
            timed_smooth(smooth)
        rows = [timed_smooth(smooth) for _ in range(args.reps)]
        for r in rows[1:]:
            assert same(rows[0][0], r[0]), "two calls differ"
        st = rows[0][0]["stats"]
        lab = {k: float(np.median([r[1][k] for r in rows])) for k in LABELS}
        tex = {k: float(np.median([r[2][k] for r in rows])) for k in TEXTURE}
        walls = [r[3] for r in rows]
        out = dict(workload=name, views=len(images), triangles=nt, linked_pairs=pairs, open_edges=adj["n_open_edges"],
                   nonmanifold_edges=adj["n_nonmanifold_edges"], min_area=int(min_area), candidates=K, rings=RINGS, penalty=PENALTY, max_passes=PASSES,
                   reps=args.reps, **{k: int(v) for k, v in zip(STATS, st.tolist())})
        out.update(diff_rank0_share=round(st[2] / max(pairs, 1), 4), diff_start_share=round(st[3] / max(pairs, 1), 4),
                   diff_end_share=round(st[4] / max(pairs, 1), 4), frontier_share=round(st[5] / max(pairs, 1), 4))
        for k in LABELS[1:-1]:
            out[k.replace("_ms", "_us")] = round(1e3 * lab[k], 1)
        passes_run = max(int(st[7]) + 1, 1)
        out.update(ring_pass_us=round(1e3 * lab["rings_ms"] / RINGS, 1), raster_us=round(1e3 * tex["raster_ms"], 1),
                   plain_views_us=round(1e3 * pmed["views_ms"], 1), plain_raster_us=round(1e3 * pmed["raster_ms"], 1), passes_with_moves=int(st[7]),
                   passes_run_at_least=passes_run, call_ms=round(float(np.median(walls)), 3), call_ms_min=round(float(np.min(walls)), 3),
                   plain_call_ms=round(pwall, 3), plain_call_ms_min=round(pwall_min, 3))
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
