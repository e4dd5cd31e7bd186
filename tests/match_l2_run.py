"""sfmtoylib::SfM::runSfM from features with FLOAT descriptors (sfmba_shim_run_sfm_f32) as a program -- TEST INFRASTRUCTURE ONLY.

    python tests/match_l2_run.py INPUT.npz OUTPUT.npz

INPUT.npz holds kp_ptr / kp_xy / desc [..][dims] float32 / cols / rows / merge_distance; OUTPUT.npz the dict of tests/sfm_loop.py's
run_class.  tests/test_gpu_match_l2_pipeline.py starts it as a fresh process with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0."""
import ctypes as C
import sys

import numpy as np

from sfm_loop import _a, _p, bp, fp, ip, lib, lp


def run_class_f32(inp, debug_level=4):
    kp_ptr, kp_xy, desc = _a(inp["kp_ptr"], np.int64), _a(inp["kp_xy"], np.float32), _a(inp["desc"], np.float32)
    n, cols, rows, dims = len(kp_ptr) - 1, int(inp["cols"]), int(inp["rows"]), desc.shape[1]
    cap_pts = 8 * max(len(kp_xy), 1)
    m = max(n, 1)
    cap_views = cap_pts * m
    poses, K = np.zeros((m, 12), np.float32), np.zeros(9, np.float32)
    done, good = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    n_added, n_pts = C.c_int(0), C.c_int64(0)
    av, ap, ac = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(m, np.int64)
    xyz, view_ptr = np.zeros((cap_pts, 3), np.float32), np.zeros(cap_pts + 1, np.int64)
    vi, fi = np.zeros(cap_views, np.int32), np.zeros(cap_views, np.int32)
    code = lib().sfmba_shim_run_sfm_f32(C.c_int(n), _p(kp_ptr, lp), _p(kp_xy, fp), _p(desc, fp), C.c_int(dims), C.c_float(float(inp["merge_distance"])),
                                        C.c_int(cols), C.c_int(rows), C.c_int(debug_level), _p(poses, fp), _p(K, fp), _p(done, bp), _p(good, bp),
                                        C.byref(n_added), _p(av, ip), _p(ap, bp), _p(ac, lp), C.c_int64(cap_pts), C.c_int64(cap_views), C.byref(n_pts),
                                        _p(xyz, fp), _p(view_ptr, lp), _p(vi, ip), _p(fi, ip))
    assert code in (0, 1), "sfmba_shim_run_sfm_f32 returned %d" % code
    na, npt = n_added.value, n_pts.value
    nv = int(view_ptr[npt])
    return dict(code=code, poses=poses[:n], K=K, done=done[:n].astype(bool), good=good[:n].astype(bool), added_view=av[:na], added_posed=ap[:na].astype(bool),
                added_cloud=ac[:na], xyz=xyz[:npt], view_ptr=view_ptr[:npt + 1], view_idx=vi[:nv], feat_idx=fi[:nv])


if __name__ == "__main__":
    np.savez(sys.argv[2], **run_class_f32(dict(np.load(sys.argv[1]))))
