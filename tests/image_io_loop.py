"""sfmtoylib::SfM started from a DIRECTORY (setImagesDirectory with a downscale factor, then runSfM) through the shim harness -- TEST
INFRASTRUCTURE ONLY, the companion of tests/sfm_loop.py, whose result dict and npz layout it shares.

As a program (a fresh process per run, which the tests start with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0):
    python tests/image_io_loop.py class [--ply PREFIX] DIRECTORY FACTOR OUTPUT.npz      one SfM(FACTOR) object: directory -> runSfM
    python tests/image_io_loop.py pixels DIRECTORY FACTOR OUTPUT.npz                    images [v,h,w(,3)] as setImagesDirectory leaves them
"""
import ctypes as C
import sys

import numpy as np

import sfm_loop
from sfm_loop import _p, bp, fp, ip, lp

MAX_VIEWS = 64


def read_pixels(directory, factor, cap=256 << 20):
    """The images of SfM(factor).setImagesDirectory(directory) as one array [v,h,w] or [v,h,w,3]; None when the call fails."""
    w, h, ch = np.zeros(MAX_VIEWS, np.int32), np.zeros(MAX_VIEWS, np.int32), C.c_int(0)
    px = np.zeros(cap, np.uint8)
    n = sfm_loop.lib().sfmba_shim_read_images_directory_scaled(directory.encode(), C.c_float(factor), C.c_int(MAX_VIEWS), C.c_int64(cap), _p(w, ip),
                                                               _p(h, ip), C.byref(ch), _p(px, bp))
    if n < 0:
        return None
    assert n > 0 and np.all(w[:n] == w[0]) and np.all(h[:n] == h[0]), "the views of a run are of one size"
    shape = (n, int(h[0]), int(w[0])) + ((3,) if ch.value == 3 else ())
    return px[:int(np.prod(shape))].reshape(shape).copy()


def run_class_directory(directory, factor, ply_prefix=None, debug_level=4):
    m = MAX_VIEWS
    cap_pts = 8 * 5000 * 8
    cap_views = cap_pts * 8
    poses, K = np.zeros((m, 12), np.float32), np.zeros(9, np.float32)
    done, good = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    n_views, n_added, n_pts = C.c_int(0), C.c_int(0), C.c_int64(0)
    av, ap, ac = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(m, np.int64)
    xyz, view_ptr = np.zeros((cap_pts, 3), np.float32), np.zeros(cap_pts + 1, np.int64)
    vi, fi = np.zeros(cap_views, np.int32), np.zeros(cap_views, np.int32)
    code = sfm_loop.lib().sfmba_shim_run_sfm_directory(directory.encode(), C.c_float(factor), C.c_int(debug_level), C.c_int(m), C.byref(n_views),
                                                       _p(poses, fp), _p(K, fp), _p(done, bp), _p(good, bp), C.byref(n_added), _p(av, ip), _p(ap, bp),
                                                       _p(ac, lp), C.c_int64(cap_pts), C.c_int64(cap_views), C.byref(n_pts), _p(xyz, fp),
                                                       _p(view_ptr, lp), _p(vi, ip), _p(fi, ip), ply_prefix.encode() if ply_prefix else None)
    assert code in (0, 1), "sfmba_shim_run_sfm_directory returned %d" % code
    n, na, npt = n_views.value, n_added.value, n_pts.value
    nv = int(view_ptr[npt])
    return dict(code=code, poses=poses[:n], K=K, done=done[:n].astype(bool), good=good[:n].astype(bool), added_view=av[:na], added_posed=ap[:na].astype(bool),
                added_cloud=ac[:na], xyz=xyz[:npt], view_ptr=view_ptr[:npt + 1], view_idx=vi[:nv], feat_idx=fi[:nv])


def figures(res, feats):
    """(views registered, cloud size, RMS reprojection px) of a finished run."""
    if int(res["code"]) != 0 or len(res["xyz"]) == 0:
        return int(res["good"].sum()) if "good" in res else 0, 0, float("nan")
    K = res["K"].reshape(3, 3).astype(np.float64)
    pt = np.repeat(np.arange(len(res["xyz"])), np.diff(res["view_ptr"]))
    P = res["poses"].reshape(-1, 3, 4).astype(np.float64)[res["view_idx"]]
    X = res["xyz"].astype(np.float64)[pt]
    pc = np.einsum("nij,nj->ni", P[:, :, :3], X) + P[:, :, 3]
    uv = pc[:, :2] / pc[:, 2:3] * np.array([K[0, 0], K[1, 1]]) + K[:2, 2]
    obs = feats["kp_xy"][feats["kp_ptr"][res["view_idx"]] + res["feat_idx"]].astype(np.float64)
    return int(res["good"].sum()), len(res["xyz"]), float(np.sqrt(((uv - obs) ** 2).sum(axis=1).mean()))


def main(argv):
    args = list(argv[1:])
    ply = None
    if "--ply" in args:
        at = args.index("--ply")
        ply = args[at + 1]
        del args[at:at + 2]
    mode, directory, factor, out = args[0], args[1], float(args[2]), args[3]
    if mode == "class":
        np.savez(out, **run_class_directory(directory, factor, ply_prefix=ply))
    else:
        images = read_pixels(directory, factor)
        np.savez(out, images=images if images is not None else np.zeros(0, np.uint8), ok=images is not None)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
