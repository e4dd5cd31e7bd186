"""Mesh measurement (sfmba_tsdf_mesh, sfmba_tsdf_integrate, sfmba_tsdf_extract): one JSON line per workload.

  corner      the four rendered 640 x 480 corner views of tests/sfm_scene.py through SfM::runSfM, densify and meshDenseCloud at
              resolution 256
  crazyhorse  the seven Crazy Horse photographs at 512 x 384 (tests/golden/crazyhorse_half) through the same three steps

Per workload, on the depth maps and the grid the class made: the HIP-event times of the phases of one sfmba_tsdf_mesh call
(SFMBA_MESH_TIMING; median over --reps calls after --warmup, the capacities given so that a call is ONE call), its end-to-end time, which
phase dominates the kernel time, the vertices, the triangles and the share of edges that lie on a boundary, and the integrate kernel's
rate in (voxel, view) pairs per second.  Beside them the end-to-end time of the two-call form (integrate, then extract, the grid
crossing the host twice).  Every repetition is compared byte for byte with the first, and the one-call form with the two-call form.
These are first measurements; nothing is gated on them.
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dense_bench import measure  # noqa: E402

PHASES = ("upload_ms", "integrate_ms", "check_ms", "count_ms", "scan_ms", "flags_ms", "emit_ms", "vertices_ms", "download_ms")
KERNELS = ("integrate_ms", "count_ms", "scan_ms", "flags_ms", "emit_ms", "vertices_ms")


def workload(capi, name, images, args):
    import mesh_oracle as mo
    import mesh_pipeline_run as run
    cls = run.run_class_mesh(dict(images=images, resolution=args.resolution))
    K, P = cls["K"].reshape(3, 3), cls["poses"].reshape(-1, 3, 4)
    maps = [d if has else None for d, has in zip(cls["depth"], cls["has_map"])]
    dims, voxel, trunc = tuple(int(v) for v in cls["dims"]), float(cls["voxel"]), float(cls["trunc"])
    nv, nt = len(cls["mesh_xyz"]), len(cls["mesh_tri"])
    same = lambda a, b: all((a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    call = lambda: capi.tsdf_mesh(list(images), K, P, maps, cls["origin"], voxel, dims, trunc, want_vkey=False, vcap=nv, tcap=nt)
    mesh, med, wall, wall_min = measure(call, "tsdf_mesh", PHASES, same, args.reps, args.warmup)
    assert mesh["xyz"].tobytes() == cls["mesh_xyz"].tobytes() and mesh["tri"].tobytes() == cls["mesh_tri"].tobytes()
    two = []
    for _ in range(max(args.reps // 2, 1)):
        t0 = time.perf_counter()
        g = capi.tsdf_integrate(list(images), K, P, maps, cls["origin"], voxel, dims, trunc)
        m2 = capi.tsdf_extract(cls["origin"], voxel, g["sum"], g["weight"], g["csum"], g["cweight"], want_vkey=False, vcap=nv, tcap=nt)
        two.append(1e3 * (time.perf_counter() - t0))
        assert m2["xyz"].tobytes() == mesh["xyz"].tobytes() and m2["bgr"].tobytes() == mesh["bgr"].tobytes() and m2["tri"].tobytes() == mesh["tri"].tobytes()
    closed, euler, boundary, n_edges = mo.topology(mesh["tri"])
    kernel_ms = sum(med[k] for k in KERNELS)
    n_maps, voxels = int(cls["has_map"].sum()), dims[0] * dims[1] * dims[2]
    top = max(KERNELS, key=lambda k: med[k])
    h, w = cls["depth"].shape[1:]
    out = dict(workload=name, views=len(images), maps=n_maps, size=[int(w), int(h)], grid=list(dims), voxels=voxels, voxel=float("%.6g" % voxel),
               trunc=float("%.6g" % trunc), vertices=nv, triangles=nt, edges=n_edges, boundary_edges=boundary,
               boundary_share=round(boundary / max(n_edges, 1), 4), euler=euler, defined_share=round(float((g["weight"] > 0).mean()), 4), reps=args.reps)
    for k in PHASES:
        out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
    out.update(kernels_us=round(1e3 * kernel_ms, 1), dominant=top.replace("_ms", ""), dominant_share=round(med[top] / kernel_ms, 3),
               call_ms=round(wall, 3), call_ms_min=round(wall_min, 3), two_calls_ms=round(float(np.median(two)), 3),
               pairs=voxels * n_maps, integrate_Gpairs_per_s=float("%.4g" % (voxels * n_maps / (med["integrate_ms"] * 1e-3) / 1e9)))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="corner,crazyhorse")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_MESH_TIMING"] = "1"
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
