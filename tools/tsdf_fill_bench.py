"""Hole-filling measurement (sfmba_tsdf_mesh_fill, sfmba_tsdf_fill): one JSON line per workload.

  corner      the four rendered 640 x 480 corner views of tests/sfm_scene.py through SfM::runSfM, densify and meshDenseCloud at
              resolution 256
  crazyhorse  the seven Crazy Horse photographs at 512 x 384 (tests/golden/crazyhorse_half) through the same three steps

Per workload, on the depth maps and the grid the class made, with --passes passes at --neighbours (8 and 2): the HIP-event times of the
phases of one sfmba_tsdf_mesh_fill call (SFMBA_MESH_TIMING; median over --reps calls after --warmup, the capacities given so that a call is
ONE call); the fill phase (quantise, the passes, write-back) as a whole and per pass, the latter as the difference between --passes
passes and one pass over --passes - 1; the same against the bytes a dense pass moves at most (one 8-byte read and one 8-byte write per
vertex; an observed vertex is not written and an unknown one reads its six neighbours out of cache); beside them the integrate and
extract phases of the same call, the call with 0 passes and sfmba_tsdf_mesh on the same inputs (alternating, so that the difference is
the new call's fixed cost); the vertices filled, the triangles with a filled vertex, and the share of boundary edges before and after,
also after sfmba_mesh_clean with the class's defaults.  Every repetition is compared byte for byte with the first, the 0-pass call with
sfmba_tsdf_mesh, and the one-call form with integrate, fill, extract.  These are first measurements; nothing is gated on them.
"""
import argparse
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dense_bench import measure  # noqa: E402

MESH = ("upload_ms", "integrate_ms", "check_ms", "count_ms", "scan_ms", "flags_ms", "emit_ms", "vertices_ms", "download_ms")
FILL = ("upload_ms", "integrate_ms", "check_ms", "fill_ms", "count_ms", "scan_ms", "flags_ms", "emit_ms", "vertices_ms", "download_ms")
EXTRACT = ("count_ms", "scan_ms", "flags_ms", "emit_ms", "vertices_ms")


def boundary_share(tri):
    e = np.sort(np.asarray(tri, np.int64).reshape(-1, 3)[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    _, n = np.unique(e[:, 0] * (int(e.max()) + 1) + e[:, 1], return_counts=True)
    return int((n == 1).sum()), len(n)


def cleaned(capi, m, origin, voxel):
    return capi.mesh_clean(m["xyz"], m["bgr"], m["tri"], origin, voxel / 1024.0, min_triangles=max(1, len(m["tri"]) // 1000))


def workload(capi, name, images, args):
    import mesh_pipeline_run as run
    cls = run.run_class_mesh(dict(images=images, resolution=args.resolution))
    K, P = cls["K"].reshape(3, 3), cls["poses"].reshape(-1, 3, 4)
    maps = [d if has else None for d, has in zip(cls["depth"], cls["has_map"])]
    dims, voxel, trunc = tuple(int(v) for v in cls["dims"]), float(cls["voxel"]), float(cls["trunc"])
    views = (list(images), K, P, maps, cls["origin"], voxel, dims, trunc)
    same = lambda a, b: all((a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    nv0, nt0 = len(cls["mesh_xyz"]), len(cls["mesh_tri"])
    full = capi.tsdf_mesh_fill(*views, fill_iterations=args.passes, min_neighbours=args.neighbours)
    nv, nt = len(full["xyz"]), len(full["tri"])
    one = capi.tsdf_mesh_fill(*views, fill_iterations=1, min_neighbours=args.neighbours)

    def fill_call(passes, v, t):
        return lambda: capi.tsdf_mesh_fill(*views, fill_iterations=passes, min_neighbours=args.neighbours, want_vkey=False, vcap=v, tcap=t)
    # alternate the three forms whose difference is reported
    plain, zero = [], []
    for _ in range(2):
        m0, med0, wall0, _ = measure(lambda: capi.tsdf_mesh(*views, want_vkey=False, vcap=nv0, tcap=nt0), "tsdf_mesh", MESH, same, args.reps, args.warmup)
        z, medz, wallz, _ = measure(fill_call(0, nv0, nt0), "tsdf_mesh_fill", FILL, same, args.reps, args.warmup)
        plain.append((med0, wall0))
        zero.append((medz, wallz))
    for k in ("xyz", "bgr", "tri"):
        assert m0[k].tobytes() == z[k].tobytes() == cls["mesh_" + k].tobytes(), k
    assert not z["vfilled"].any()
    m8, med8, wall8, _ = measure(fill_call(args.passes, nv, nt), "tsdf_mesh_fill", FILL, same, args.reps, args.warmup)
    _, med1, _, _ = measure(fill_call(1, len(one["xyz"]), len(one["tri"])), "tsdf_mesh_fill", FILL, same, args.reps, args.warmup)
    # the one-call form against integrate, fill, extract through the host
    g = capi.tsdf_integrate(*views)
    f = capi.tsdf_fill(g["sum"], g["weight"], g["csum"], g["cweight"], iterations=args.passes, min_neighbours=args.neighbours)
    three = capi.tsdf_extract(cls["origin"], voxel, f["sum"], f["weight"], f["csum"], f["cweight"])
    for k in ("xyz", "bgr", "tri"):
        assert three[k].tobytes() == m8[k].tobytes() == full[k].tobytes(), k

    voxels = dims[0] * dims[1] * dims[2]
    per_pass_ms = (med8["fill_ms"] - med1["fill_ms"]) / max(args.passes - 1, 1)
    dense_bytes = 16 * voxels
    b0, b8 = boundary_share(m0["tri"]), boundary_share(full["tri"])
    c0, c8 = boundary_share(cleaned(capi, m0, cls["origin"], voxel)["tri"]), boundary_share(cleaned(capi, full, cls["origin"], voxel)["tri"])
    out = dict(workload=name, views=len(images), grid=list(dims), voxels=voxels, passes=args.passes, min_neighbours=args.neighbours, reps=args.reps,
               observed_share=round(float((f["state"] == 0).mean()), 4), filled_grid_vertices=f["n_filled"],
               still_unknown_share=round(float((f["state"] == 255).mean()), 4),
               vertices=[nv0, nv], triangles=[nt0, nt], vertices_filled=int(full["vfilled"].sum()),
               triangles_with_a_filled_vertex=int(full["vfilled"][full["tri"]].any(axis=1).sum()),
               boundary_share=[round(b0[0] / max(b0[1], 1), 4), round(b8[0] / max(b8[1], 1), 4)],
               boundary_share_after_clean=[round(c0[0] / max(c0[1], 1), 4), round(c8[0] / max(c8[1], 1), 4)],
               fill_us=round(1e3 * med8["fill_ms"], 1), fill_one_pass_us=round(1e3 * med1["fill_ms"], 1), per_pass_us=round(1e3 * per_pass_ms, 2),
               dense_pass_bytes=dense_bytes, per_pass_TB_per_s=float("%.4g" % (dense_bytes / (per_pass_ms * 1e-3) / 1e12)) if per_pass_ms > 0 else None,
               integrate_us=round(1e3 * med8["integrate_ms"], 1), extract_us=round(1e3 * sum(med8[k] for k in EXTRACT), 1),
               upload_us=round(1e3 * med8["upload_ms"], 1), download_us=round(1e3 * med8["download_ms"], 1), call_ms=round(wall8, 3),
               tsdf_mesh_call_ms=[round(w, 3) for _, w in plain], zero_pass_call_ms=[round(w, 3) for _, w in zero],
               tsdf_mesh_kernels_us=[round(1e3 * (m["integrate_ms"] + sum(m[k] for k in EXTRACT)), 1) for m, _ in plain],
               zero_pass_kernels_us=[round(1e3 * (m["integrate_ms"] + m["fill_ms"] + sum(m[k] for k in EXTRACT)), 1) for m, _ in zero])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="corner,crazyhorse")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--neighbours", type=int, default=2)
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
