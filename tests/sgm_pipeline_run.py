"""sfmtoylib::SfM::runSfM followed by SfM::densify with DenseParams::sgm, as a program -- TEST INFRASTRUCTURE ONLY.

    python tests/sgm_pipeline_run.py class SGM INPUT.npz OUTPUT.npz [PLY_PREFIX]
    python tests/sgm_pipeline_run.py capi  INPUT.npz CLASS.npz OUTPUT.npz

SGM is "off" or "sgm,p1,p2,paths,invalid_cost,uniqueness" as six integers.  `class`: setImages, runSfM, densify(params) and
meshDenseCloud at resolution 64 in one call (sfmba_shim_run_sfm_dense_sgm); OUTPUT.npz: the dict of tests/depth_pipeline_run.py's
run_class_dense plus n_triangles.  `capi`: with the class's poses, K and jobs, sfmba_depth_sweep + sfmba_depth_fuse (OUTPUT keys
depth, dense_*) and sfmba_depth_sweep_sgm with SGM_SET + sfmba_depth_fuse (sgm_depth, sgm_dense_*).
tests/test_gpu_sgm_pipeline.py starts it as a fresh process with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0."""
import ctypes as C
import sys

import numpy as np

import depth_pipeline_run as dpr
from sfm_loop import ROOT, _a, _p, bp, fp, ip, lib, lp

SGM_SET = dict(p1=6, p2=48, n_paths=4, invalid_cost=100, uniqueness=7)       # not the defaults: every field has to arrive
MESH_RESOLUTION = 64


def sgm_text(on=True):
    return ",".join(str(v) for v in [1 if on else 0] + [SGM_SET[k] for k in ("p1", "p2", "n_paths", "invalid_cost", "uniqueness")])


def run_class_sgm(inp, sgm, ply_prefix=None, debug_level=4):
    images = _a(inp["images"], np.uint8)
    n, h, w = images.shape[:3]
    channels = 3 if images.ndim == 4 else 1
    img_ptr = np.arange(n + 1, dtype=np.int64) * h * w * channels
    wd, ht = np.full(n, w, np.int32), np.full(n, h, np.int32)
    cap_pts = 8 * 5000 * n
    cap_views = cap_pts * n
    poses, K = np.zeros((n, 12), np.float32), np.zeros(9, np.float32)
    done, good = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    n_added, n_pts, n_jobs, n_dense, n_tri = C.c_int(0), C.c_int64(0), C.c_int(0), C.c_int64(0), C.c_int64(0)
    av, ap, ac = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.int64)
    xyz, view_ptr = np.zeros((cap_pts, 3), np.float32), np.zeros(cap_pts + 1, np.int64)
    vi, fi = np.zeros(cap_views, np.int32), np.zeros(cap_views, np.int32)
    job_ref, job_src_ptr, job_src = np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros(4 * n, np.int32)
    zn, zf, has_map = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    depth = np.zeros((n, h, w), np.float32)
    cap_dense = n * h * w
    dxyz, dbgr = np.zeros((cap_dense, 3), np.float32), np.zeros((cap_dense, 3), np.uint8)
    dview, dpix = np.zeros(cap_dense, np.int32), np.zeros(cap_dense, np.int32)
    sgm = np.asarray(sgm, np.int32)
    code = lib().sfmba_shim_run_sfm_dense_sgm(_p(sgm, ip), C.c_int(MESH_RESOLUTION), C.byref(n_tri), C.c_int(dpr.FEATURES_ORB), C.c_float(20.0), C.c_int(n),
                                              C.c_int(channels), _p(img_ptr, lp), _p(images, bp), _p(wd, ip), _p(ht, ip), C.c_int(debug_level),
                                              _p(poses, fp), _p(K, fp), _p(done, bp), _p(good, bp), C.byref(n_added), _p(av, ip), _p(ap, bp),
                                              _p(ac, lp), C.c_int64(cap_pts), C.c_int64(cap_views), C.byref(n_pts), _p(xyz, fp), _p(view_ptr, lp),
                                              _p(vi, ip), _p(fi, ip), ply_prefix.encode() if ply_prefix else None, C.byref(n_jobs), _p(job_ref, ip),
                                              _p(job_src_ptr, lp), _p(job_src, ip), _p(zn, fp), _p(zf, fp), _p(has_map, bp), _p(depth, fp),
                                              C.c_int64(cap_dense), C.byref(n_dense), _p(dxyz, fp), _p(dbgr, bp), _p(dview, ip), _p(dpix, ip))
    assert code in (0, 1), "sfmba_shim_run_sfm_dense_sgm returned %d" % code
    na, npt, nj, nd = n_added.value, n_pts.value, n_jobs.value, n_dense.value
    nv = int(view_ptr[npt])
    return dict(code=code, poses=poses[:n], K=K, done=done[:n].astype(bool), good=good[:n].astype(bool), added_view=av[:na], added_posed=ap[:na].astype(bool),
                added_cloud=ac[:na], xyz=xyz[:npt], view_ptr=view_ptr[:npt + 1], view_idx=vi[:nv], feat_idx=fi[:nv],
                job_ref=job_ref[:nj], job_src_ptr=job_src_ptr[:nj + 1], job_src=job_src[:int(job_src_ptr[nj])], z_near=zn[:nj], z_far=zf[:nj],
                has_map=has_map.astype(bool), depth=depth, dense_xyz=dxyz[:nd], dense_bgr=dbgr[:nd], dense_view=dview[:nd], dense_pixel=dpix[:nd],
                n_triangles=np.int64(n_tri.value))


def run_capi(inp, cls):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from sfm_toy_library_amd import capi
    images = list(_a(inp["images"], np.uint8))
    jobs = dpr.jobs_of(cls)
    K, P = cls["K"].reshape(3, 3), cls["poses"].reshape(-1, 3, 4)
    out = {}
    for prefix, results in (("", capi.depth_sweep(images, K, P, jobs)), ("sgm_", capi.depth_sweep_sgm(images, K, P, jobs, **SGM_SET))):
        maps, checks = [None] * len(images), [[] for _ in images]
        for (ref, srcs, _, _), (d, _, _) in zip(jobs, results):
            maps[ref], checks[ref] = d, srcs
        cloud = capi.depth_fuse(images, K, P, maps, checks)
        out[prefix + "depth"] = np.stack([np.zeros(images[0].shape[:2], np.float32) if m is None else m for m in maps])
        for k, f in (("dense_xyz", "xyz"), ("dense_bgr", "bgr"), ("dense_view", "src_image"), ("dense_pixel", "src_pixel")):
            out[prefix + k] = cloud[f]
    return out


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "class":
        sgm = [0, 8, 64, 8, 127, 5] if sys.argv[2] == "off" else [int(v) for v in sys.argv[2].split(",")]
        np.savez(sys.argv[4], **run_class_sgm(dict(np.load(sys.argv[3])), sgm, ply_prefix=sys.argv[5] if len(sys.argv) > 5 else None))
    else:
        np.savez(sys.argv[4], **run_capi(dict(np.load(sys.argv[2])), dict(np.load(sys.argv[3]))))
