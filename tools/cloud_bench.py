"""Voxel-merge measurement (sfmba_depth_normals, sfmba_cloud_merge): one JSON line per workload.

  corner      the four rendered 640 x 480 corner views of tests/sfm_scene.py through SfM::runSfM and densify: about 6e5 dense points
  crazyhorse  the seven Crazy Horse photographs at 512 x 384 (tests/golden/crazyhorse_half) through the same two steps

Per workload, on the dense cloud the class made and at the class's auto voxel: the HIP-event times of the merge's phases
(SFMBA_CLOUD_TIMING; median over --reps calls after --warmup), the end-to-end time of a merge call and of the normals call, the sort's
share of the kernel time, and the bytes the reduction has to move -- per valid point its sorted index (4), position (12), colour (3)
and normal (12), per voxel two run starts' worth of 4 bytes and the nine 8-byte sums written -- against the time of its two kernels.
Beside them the time of the sfmba_depth_fuse call that produced the input (same images, poses, maps and check lists, measured the same
way): whether the merge costs less than the stage before it is the only comparison there is.  Every repetition is compared byte for
byte with the first.  These are first measurements; nothing is gated on them.
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

MERGE = ("upload_ms", "quantise_ms", "sort_ms", "runs_ms", "reduce_ms", "compact_ms", "finalise_ms", "download_ms")
NORMALS = ("upload_ms", "kernel_ms", "download_ms")
FUSE = ("upload_ms", "flag_ms", "scan_ms", "emit_ms", "download_ms")


def workload(capi, name, images, args):
    import cloud_pipeline_run as run
    cls = run.run_class_merged(dict(images=images))
    K, P = cls["K"].reshape(3, 3), cls["poses"].reshape(-1, 3, 4)
    maps = [d if has else None for d, has in zip(cls["depth"], cls["has_map"])]
    same = lambda a, b: all((a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    same_list = lambda a, b: all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))

    # the stage before: the fuse call that made this cloud
    checks = [[] for _ in maps]
    for j, ref in enumerate(cls["job_ref"]):
        checks[int(ref)] = [int(s) for s in cls["job_src"][cls["job_src_ptr"][j]:cls["job_src_ptr"][j + 1]]]
    os.environ["SFMBA_DEPTH_TIMING"] = "1"
    n_dense = len(cls["dense_xyz"])
    fused, fuse_med, fuse_call, fuse_min = measure(lambda: capi.depth_fuse(list(images), K, P, maps, checks, cap=n_dense), "depth_fuse", FUSE, same,
                                                   args.reps, args.warmup)
    assert fused["xyz"].tobytes() == cls["dense_xyz"].tobytes()

    normal_maps, n_med, n_call, n_min = measure(lambda: capi.depth_normals(K, P, maps, max_rel_step=0.05), "depth_normals", NORMALS, same_list,
                                                args.reps, args.warmup)
    h, w = cls["depth"].shape[1:]
    stack = np.stack([np.zeros((h, w, 3), np.float32) if m is None else m for m in normal_maps]).reshape(len(maps), h * w, 3)
    gathered = np.ascontiguousarray(stack[cls["dense_view"], cls["dense_pixel"]])
    voxel, m = float(cls["voxel_used"]), len(cls["merged_xyz"])
    merged, med, call, call_min = measure(lambda: capi.cloud_merge(cls["dense_xyz"], cls["dense_bgr"], gathered, voxel=voxel, cap=m, want_voxel_of=False),
                                          "cloud_merge", MERGE, same, args.reps, args.warmup)
    assert merged["xyz"].tobytes() == cls["merged_xyz"].tobytes() and merged["normal"].tobytes() == cls["merged_normal"].tobytes()
    n_valid = n_dense - merged["n_skipped"]
    kernels = ("quantise_ms", "sort_ms", "runs_ms", "reduce_ms", "compact_ms", "finalise_ms")
    kernel_ms = sum(med[k] for k in kernels)
    reduce_bytes = n_valid * (4 + 12 + 3 + 12) + m * (8 + 9 * 8)
    out = dict(workload=name, views=len(images), size=[int(w), int(h)], dense_points=n_dense, voxel=float("%.6g" % voxel), merged_points=m,
               ratio=round(n_dense / m, 3), counts_1_2_3_4plus=np.bincount(np.minimum(merged["count"], 4), minlength=5)[1:].tolist(),
               longest_run=int(merged["count"].max()), merged_with_normal=round(float((merged["normal"] != 0).any(axis=1).mean()), 4), reps=args.reps)
    for k in MERGE:
        out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
    out.update(kernels_us=round(1e3 * kernel_ms, 1), sort_share=round(med["sort_ms"] / kernel_ms, 3), call_ms=round(call, 3), call_ms_min=round(call_min, 3),
               reduce_bytes=int(reduce_bytes), reduce_GB_per_s=float("%.4g" % (reduce_bytes / (med["reduce_ms"] * 1e-3) / 1e9)),
               normals_kernel_us=round(1e3 * n_med["kernel_ms"], 1), normals_call_ms=round(n_call, 3),
               fuse_kernels_us=round(1e3 * (fuse_med["flag_ms"] + fuse_med["scan_ms"] + fuse_med["emit_ms"]), 1), fuse_call_ms=round(fuse_call, 3),
               fuse_call_ms_min=round(fuse_min, 3))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="corner,crazyhorse")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_CLOUD_TIMING"] = "1"
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
