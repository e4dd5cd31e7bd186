"""sfmtoylib::SfM::runSfM, densify and mergeDenseCloud, as a program -- TEST INFRASTRUCTURE ONLY.

    python tests/cloud_pipeline_run.py class INPUT.npz OUTPUT.npz [PLY_PREFIX]
    python tests/cloud_pipeline_run.py capi  INPUT.npz CLASS.npz OUTPUT.npz

INPUT.npz holds images [v, h, w] or [v, h, w, 3] and, optionally, voxel (0 = auto), min_count and max_rel_step.  `class`: the three
steps in one call (sfmba_shim_run_sfm_merged), the four PLY files written if a prefix is given.  OUTPUT.npz: poses, K, densify's jobs
(job_ref, job_src_ptr, job_src, z_near, z_far), has_map, depth [v, h, w], the dense cloud as it stands after the merge (dense_xyz,
dense_bgr, dense_view, dense_pixel, dense_unchanged), the merged cloud (merged_xyz, merged_bgr, merged_normal, merged_count, merged_first), voxel_used and
n_skipped.  `capi`: sfmba_depth_normals over the class's depth maps, the gather of every dense point's normal through dense_view /
dense_pixel, and sfmba_cloud_merge at voxel_used, through the ctypes binding; OUTPUT.npz: the merged cloud under the same names.
tests/test_gpu_cloud_pipeline.py starts it as a fresh process with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0."""
import ctypes as C
import sys

import numpy as np

from sfm_loop import ROOT, _a, _p, bp, fp, ip, lib, lp


def settings(inp):
    return float(inp.get("voxel", 0.0)), int(inp.get("min_count", 1)), float(inp.get("max_rel_step", 0.05))


def run_class_merged(inp, ply_prefix=None, debug_level=4):
    images = _a(inp["images"], np.uint8)
    n, h, w = images.shape[:3]
    channels = 3 if images.ndim == 4 else 1
    voxel, min_count, max_rel_step = settings(inp)
    img_ptr = np.arange(n + 1, dtype=np.int64) * h * w * channels
    wd, ht = np.full(n, w, np.int32), np.full(n, h, np.int32)
    poses, K = np.zeros((n, 12), np.float32), np.zeros(9, np.float32)
    zn, zf, has_map = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    job_ref, job_src_ptr, job_src = np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros(4 * n, np.int32)
    depth = np.zeros((n, h, w), np.float32)
    cap = n * h * w
    dxyz, dbgr, dview, dpix = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.uint8), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    mxyz, mbgr, mnrm = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.uint8), np.zeros((cap, 3), np.float32)
    mcount, mfirst = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    n_jobs, unchanged, n_dense, n_merged, n_skipped, used = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_float(0)
    code = lib().sfmba_shim_run_sfm_merged(C.c_int(n), C.c_int(channels), _p(img_ptr, lp), _p(images, bp), _p(wd, ip), _p(ht, ip), C.c_int(debug_level),
                                           C.c_float(voxel), C.c_int(min_count), C.c_float(max_rel_step), ply_prefix.encode() if ply_prefix else None,
                                           _p(poses, fp), _p(K, fp), C.byref(n_jobs), _p(job_ref, ip), _p(job_src_ptr, lp), _p(job_src, ip),
                                           _p(zn, fp), _p(zf, fp), _p(has_map, bp), _p(depth, fp), C.c_int64(cap), C.byref(n_dense), _p(dxyz, fp), _p(dbgr, bp), _p(dview, ip), _p(dpix, ip),
                                           C.byref(unchanged), C.byref(n_merged), _p(mxyz, fp), _p(mbgr, bp), _p(mnrm, fp), _p(mcount, ip),
                                           _p(mfirst, ip), C.byref(used), C.byref(n_skipped))
    assert code == 0, "sfmba_shim_run_sfm_merged returned %d" % code
    nj, nd, nm = n_jobs.value, n_dense.value, n_merged.value
    return dict(poses=poses, K=K, job_ref=job_ref[:nj], job_src_ptr=job_src_ptr[:nj + 1], job_src=job_src[:int(job_src_ptr[nj])],
                z_near=zn[:nj], z_far=zf[:nj], has_map=has_map.astype(bool), depth=depth, dense_xyz=dxyz[:nd], dense_bgr=dbgr[:nd],
                dense_view=dview[:nd], dense_pixel=dpix[:nd], dense_unchanged=unchanged.value, merged_xyz=mxyz[:nm], merged_bgr=mbgr[:nm],
                merged_normal=mnrm[:nm], merged_count=mcount[:nm], merged_first=mfirst[:nm], voxel_used=np.float32(used.value),
                n_skipped=n_skipped.value)


def run_capi(inp, cls):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from sfm_toy_library_amd import capi
    _, min_count, max_rel_step = settings(inp)
    maps = [d if has else None for d, has in zip(cls["depth"], cls["has_map"])]
    normal_maps = capi.depth_normals(cls["K"].reshape(3, 3), cls["poses"].reshape(-1, 3, 4), maps, max_rel_step=max_rel_step)
    h, w = cls["depth"].shape[1:]
    stack = np.stack([np.zeros((h, w, 3), np.float32) if m is None else m for m in normal_maps]).reshape(len(maps), h * w, 3)
    gathered = stack[cls["dense_view"], cls["dense_pixel"]]
    out = capi.cloud_merge(cls["dense_xyz"], cls["dense_bgr"], gathered, voxel=float(cls["voxel_used"]), min_count=min_count)
    return dict(merged_xyz=out["xyz"], merged_bgr=out["bgr"], merged_normal=out["normal"], merged_count=out["count"], merged_first=out["first"],
                n_skipped=out["n_skipped"], normals_with_a_value=float(np.mean([(m != 0).any(-1).mean() for m in normal_maps if m is not None])))


if __name__ == "__main__":
    mode, src = sys.argv[1:3]
    inp = dict(np.load(src))
    if mode == "class":
        np.savez(sys.argv[3], **run_class_merged(inp, ply_prefix=sys.argv[4] if len(sys.argv) > 4 else None))
    else:
        np.savez(sys.argv[4], **run_capi(inp, dict(np.load(sys.argv[3]))))
