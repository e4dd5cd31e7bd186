"""sfmtoylib::SfM::runSfM followed by SfM::densify, as a program -- TEST INFRASTRUCTURE ONLY.

    python tests/depth_pipeline_run.py class INPUT.npz OUTPUT.npz [PLY_PREFIX]
    python tests/depth_pipeline_run.py capi  INPUT.npz CLASS.npz OUTPUT.npz

INPUT.npz holds images [v, h, w] or [v, h, w, 3].  `class`: setImages, runSfM and densify() in one call (sfmba_shim_run_sfm_dense),
the three PLY files written if a prefix is given.  OUTPUT.npz: the dict of tests/sfm_loop.py's run_class plus the jobs densify made
(job_ref, job_src_ptr, job_src, z_near, z_far), has_map, depth [v, h, w] and the dense cloud (dense_xyz, dense_bgr, dense_view,
dense_pixel).  `capi`: the two C-ABI calls (sfmba_depth_sweep, sfmba_depth_fuse) through the ctypes binding with the class's poses,
K, jobs and the default parameters; OUTPUT.npz: depth [v, h, w] and the cloud under the same names.
tests/test_gpu_depth_pipeline.py starts it as a fresh process with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0."""
import ctypes as C
import sys

import numpy as np

from sfm_loop import ROOT, _a, _p, bp, fp, ip, lib, lp

FEATURES_ORB = 0


def run_class_dense(inp, ply_prefix=None, debug_level=4):
    images = _a(inp["images"], np.uint8)
    n, h, w = images.shape[:3]
    channels = 3 if images.ndim == 4 else 1
    img_ptr = np.arange(n + 1, dtype=np.int64) * h * w * channels
    wd, ht = np.full(n, w, np.int32), np.full(n, h, np.int32)
    cap_pts = 8 * 5000 * n
    cap_views = cap_pts * n
    poses, K = np.zeros((n, 12), np.float32), np.zeros(9, np.float32)
    done, good = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    n_added, n_pts, n_jobs, n_dense = C.c_int(0), C.c_int64(0), C.c_int(0), C.c_int64(0)
    av, ap, ac = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.int64)
    xyz, view_ptr = np.zeros((cap_pts, 3), np.float32), np.zeros(cap_pts + 1, np.int64)
    vi, fi = np.zeros(cap_views, np.int32), np.zeros(cap_views, np.int32)
    job_ref, job_src_ptr, job_src = np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros(4 * n, np.int32)
    zn, zf, has_map = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    depth = np.zeros((n, h, w), np.float32)
    cap_dense = n * h * w
    dxyz, dbgr = np.zeros((cap_dense, 3), np.float32), np.zeros((cap_dense, 3), np.uint8)
    dview, dpix = np.zeros(cap_dense, np.int32), np.zeros(cap_dense, np.int32)
    code = lib().sfmba_shim_run_sfm_dense(C.c_int(FEATURES_ORB), C.c_float(20.0), C.c_int(n), C.c_int(channels), _p(img_ptr, lp), _p(images, bp),
                                          _p(wd, ip), _p(ht, ip), C.c_int(debug_level), _p(poses, fp), _p(K, fp), _p(done, bp), _p(good, bp),
                                          C.byref(n_added), _p(av, ip), _p(ap, bp), _p(ac, lp), C.c_int64(cap_pts), C.c_int64(cap_views),
                                          C.byref(n_pts), _p(xyz, fp), _p(view_ptr, lp), _p(vi, ip), _p(fi, ip),
                                          ply_prefix.encode() if ply_prefix else None, C.byref(n_jobs), _p(job_ref, ip), _p(job_src_ptr, lp),
                                          _p(job_src, ip), _p(zn, fp), _p(zf, fp), _p(has_map, bp), _p(depth, fp), C.c_int64(cap_dense),
                                          C.byref(n_dense), _p(dxyz, fp), _p(dbgr, bp), _p(dview, ip), _p(dpix, ip))
    assert code in (0, 1), "sfmba_shim_run_sfm_dense returned %d" % code
    na, npt, nj, nd = n_added.value, n_pts.value, n_jobs.value, n_dense.value
    nv = int(view_ptr[npt])
    return dict(code=code, poses=poses[:n], K=K, done=done[:n].astype(bool), good=good[:n].astype(bool), added_view=av[:na], added_posed=ap[:na].astype(bool),
                added_cloud=ac[:na], xyz=xyz[:npt], view_ptr=view_ptr[:npt + 1], view_idx=vi[:nv], feat_idx=fi[:nv],
                job_ref=job_ref[:nj], job_src_ptr=job_src_ptr[:nj + 1], job_src=job_src[:int(job_src_ptr[nj])], z_near=zn[:nj], z_far=zf[:nj],
                has_map=has_map.astype(bool), depth=depth, dense_xyz=dxyz[:nd], dense_bgr=dbgr[:nd], dense_view=dview[:nd], dense_pixel=dpix[:nd])


def jobs_of(cls):
    ptr = cls["job_src_ptr"]
    return [(int(r), [int(s) for s in cls["job_src"][ptr[j]:ptr[j + 1]]], float(cls["z_near"][j]), float(cls["z_far"][j]))
            for j, r in enumerate(cls["job_ref"])]


def run_capi(inp, cls):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from sfm_toy_library_amd import capi
    images = list(_a(inp["images"], np.uint8))
    jobs = jobs_of(cls)
    K, P = cls["K"].reshape(3, 3), cls["poses"].reshape(-1, 3, 4)
    maps, checks = [None] * len(images), [[] for _ in images]
    for (ref, srcs, _, _), (d, _, _) in zip(jobs, capi.depth_sweep(images, K, P, jobs)):     # the binding's defaults are the class's
        maps[ref], checks[ref] = d, srcs
    cloud = capi.depth_fuse(images, K, P, maps, checks)
    depth = np.stack([np.zeros(images[0].shape[:2], np.float32) if m is None else m for m in maps])
    return dict(depth=depth, dense_xyz=cloud["xyz"], dense_bgr=cloud["bgr"], dense_view=cloud["src_image"], dense_pixel=cloud["src_pixel"])


if __name__ == "__main__":
    mode, src = sys.argv[1:3]
    inp = dict(np.load(src))
    if mode == "class":
        np.savez(sys.argv[3], **run_class_dense(inp, ply_prefix=sys.argv[4] if len(sys.argv) > 4 else None))
    else:
        np.savez(sys.argv[4], **run_capi(inp, dict(np.load(sys.argv[3]))))
