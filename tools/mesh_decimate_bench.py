"""Mesh-decimation measurement (sfmba_mesh_decimate): one JSON line per workload and cell size.

  corner      the four rendered 640 x 480 corner views of tests/sfm_scene.py through SfM::runSfM, densify and meshDenseCloud at
              resolution 256
  crazyhorse  the seven Crazy Horse photographs at 512 x 384 (tests/golden/crazyhorse_half) through the same steps

Per workload, on the mesh the class made and with the host rules of host/SfM.h, at cells of 1, 2 and 4 voxels with the quadric
placement and reg 1024: the HIP-event times of the phases of one sfmba_mesh_decimate call (SFMBA_MESH_DECIMATE_TIMING; median over
--reps calls after --warmup, the capacities given so that a call is ONE call) and its end-to-end time, beside the end-to-end times of
the sfmba_tsdf_mesh and sfmba_mesh_clean calls of the same run; the triangles in and out, the four stats and the share of boundary and
of non-manifold edges; and what the decimation is for: the share of triangles that get a view at the default area floor, the atlas
size and the time of one sfmba_mesh_texture_adjust call, each on the mesh and on the decimated mesh.  Every repetition is compared byte
for byte with the first.  These are first measurements; nothing is gated on them, and there is no earlier time to compare with.
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

PHASES = ("upload_ms", "keys_ms", "sort_ms", "runs_ms", "members_ms", "quadrics_ms", "solve_ms", "map_ms", "dedup_ms", "compact_ms", "emit_ms", "download_ms")
KERNELS = PHASES[1:-1]


def wall_ms(call, reps):
    out, times = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, float(np.median(times))


def texture_line(capi, cls, images, maps, xyz, bgr, tri, reps):
    """share of triangles with a view and the atlas at the class's rules; the time of one levelled texturing call"""
    from texture_pipeline_run import host_rules
    occl_tol, min_area, B = host_rules(cls, len(tri))
    plain = capi.mesh_texture(xyz, bgr, tri, images, cls["K"], cls["poses"], maps, occl_tol, min_area, 6, B)
    _, adjust_ms = wall_ms(lambda: capi.mesh_texture_adjust(xyz, bgr, tri, images, cls["K"], cls["poses"], maps, occl_tol, min_area, 6, B), reps)
    return dict(triangles=len(tri), with_view=int(plain["n_textured"]), view_share=round(plain["n_textured"] / max(len(tri), 1), 4),
                atlas=[int(plain["atlas"].shape[1]), int(plain["atlas"].shape[0])], texture_adjust_call_ms=round(adjust_ms, 2))


def workload(capi, name, images, args):
    import decimate_oracle as do
    import decimate_pipeline_run as run
    inp = dict(images=images)
    cls = run.run_class_decimate(inp)
    xyz, bgr, tri = cls["mesh_xyz"], cls["mesh_bgr"], cls["mesh_tri"]
    views = list(images)
    maps = [m if has else None for m, has in zip(cls["depth"], cls["has_map"])]
    quantum = float(np.float32(cls["voxel"]) / np.float32(1024.0))
    few = max(args.reps // 3, 1)
    _, tsdf_ms = wall_ms(lambda: capi.tsdf_mesh(views, cls["K"], cls["poses"], maps, cls["origin"], float(cls["voxel"]), [int(d) for d in cls["dims"]],
                                                float(cls["trunc"]), vcap=len(xyz), tcap=len(tri)), few)
    _, clean_ms = wall_ms(lambda: capi.mesh_clean(xyz, bgr, tri, cls["origin"], quantum, max(1, len(tri) // 1000), False, 10, 0.5, -0.53,
                                                  vcap=len(xyz), tcap=len(tri)), few)
    before = texture_line(capi, cls, views, maps, xyz, bgr, tri, few)
    b0 = do.edge_counts(tri)
    same = lambda a, b: all((a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    for cell_voxels in (1, 2, 4):
        cell = cell_voxels * 1024
        sizes = capi.mesh_decimate(xyz, bgr, tri, cls["origin"], quantum, cell, 1, 1024)
        kv, kt = len(sizes["xyz"]), len(sizes["tri"])
        call = lambda: capi.mesh_decimate(xyz, bgr, tri, cls["origin"], quantum, cell, 1, 1024, vcap=kv, tcap=kt)
        got, med, wall, wall_min = measure(call, "mesh_decimate", PHASES, same, args.reps, args.warmup)
        if cell_voxels == 2:
            assert got["xyz"].tobytes() == cls["decimated_xyz"].tobytes() and got["tri"].tobytes() == cls["decimated_tri"].tobytes()
        b1 = do.edge_counts(got["tri"])
        kernel_ms = sum(med[k] for k in KERNELS)
        top = max(KERNELS, key=lambda k: med[k])
        out = dict(workload=name, views=len(images), cell_voxels=cell_voxels, placement="quadric", reg=1024, vertices=len(xyz), triangles=len(tri),
                   vertices_out=kv, triangles_out=kt, clusters=got["stats"][0], collapsed=got["stats"][1], duplicates=got["stats"][2],
                   took_the_mean=got["stats"][3], boundary_share_before=round(b0[0] / max(b0[2], 1), 4), boundary_share_after=round(b1[0] / max(b1[2], 1), 4),
                   non_manifold_edges_before=b0[1], non_manifold_edges_after=b1[1], reps=args.reps)
        for k in PHASES:
            out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
        out.update(kernels_us=round(1e3 * kernel_ms, 1), dominant=top.replace("_ms", ""), dominant_share=round(med[top] / kernel_ms, 3),
                   call_ms=round(wall, 3), call_ms_min=round(wall_min, 3), tsdf_mesh_call_ms=round(tsdf_ms, 2), mesh_clean_call_ms=round(clean_ms, 2),
                   quadric_accumulation="int64 atomics (a lane per triangle, ten adds per distinct cluster)", texture_before=before,
                   texture_after=texture_line(capi, cls, views, maps, got["xyz"], got["bgr"], got["tri"], few))
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="corner,crazyhorse")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_MESH_DECIMATE_TIMING"] = "1"
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
