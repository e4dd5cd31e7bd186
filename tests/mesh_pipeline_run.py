"""sfmtoylib::SfM::runSfM, densify and meshDenseCloud, as a program -- TEST INFRASTRUCTURE ONLY.

    python tests/mesh_pipeline_run.py class INPUT.npz OUTPUT.npz [PLY_PREFIX]
    python tests/mesh_pipeline_run.py capi  INPUT.npz CLASS.npz OUTPUT.npz
    python tests/mesh_pipeline_run.py refuse INPUT.npz OUTPUT.npz

INPUT.npz holds images [v, h, w] or [v, h, w, 3] and, optionally, voxel (0 = from resolution), resolution, trunc_voxels and min_weight.
`class`: the three steps in one call (sfmba_shim_run_sfm_mesh), <prefix>_mesh.ply written if a prefix is given.  OUTPUT.npz: poses, K,
has_map, depth [v, h, w] and dense_xyz as they stand after the mesh call, unchanged, the grid the class chose (origin, voxel, trunc,
dims) and the mesh (mesh_xyz, mesh_bgr, mesh_tri).  `capi`: sfmba_tsdf_mesh through the ctypes binding with the class's images, poses,
depth maps and grid; OUTPUT.npz: the mesh under the same names.  `refuse`: meshDenseCloud without a densify (no device involved);
OUTPUT.npz: code.  tests/test_gpu_mesh_pipeline.py starts it as a fresh process with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0."""
import ctypes as C
import sys

import numpy as np

from sfm_loop import ROOT, _a, _p, bp, fp, ip, lib, lp


def settings(inp):
    return float(inp.get("voxel", 0.0)), int(inp.get("resolution", 256)), float(inp.get("trunc_voxels", 4.0)), int(inp.get("min_weight", 1))


def run_class_mesh(inp, ply_prefix=None, debug_level=4, what=0):
    images = _a(inp["images"], np.uint8)
    n, h, w = images.shape[:3]
    channels = 3 if images.ndim == 4 else 1
    voxel, resolution, trunc_voxels, min_weight = settings(inp)
    img_ptr = np.arange(n + 1, dtype=np.int64) * h * w * channels
    wd, ht = np.full(n, w, np.int32), np.full(n, h, np.int32)
    poses, K, has_map = np.zeros((n, 12), np.float32), np.zeros(9, np.float32), np.zeros(n, np.uint8)
    depth = np.zeros((n, h, w), np.float32)
    cap = n * h * w
    vcap, tcap = 4 * cap, 8 * cap
    dxyz, grid = np.zeros((cap, 3), np.float32), np.zeros(8, np.float32)
    mxyz, mbgr, mtri = np.zeros((vcap, 3), np.float32), np.zeros((vcap, 3), np.uint8), np.zeros((tcap, 3), np.int32)
    unchanged, n_dense, nv, nt = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    code = lib().sfmba_shim_run_sfm_mesh(C.c_int(what), C.c_int(n), C.c_int(channels), _p(img_ptr, lp), _p(images, bp), _p(wd, ip), _p(ht, ip),
                                         C.c_int(debug_level), C.c_float(voxel), C.c_int(resolution), C.c_float(trunc_voxels), C.c_int(min_weight),
                                         ply_prefix.encode() if ply_prefix else None, _p(poses, fp), _p(K, fp), _p(has_map, bp), _p(depth, fp),
                                         C.c_int64(cap), C.byref(n_dense), _p(dxyz, fp), C.byref(unchanged), _p(grid, fp), C.c_int64(vcap),
                                         C.c_int64(tcap), C.byref(nv), C.byref(nt), _p(mxyz, fp), _p(mbgr, bp), _p(mtri, ip))
    if what:
        return dict(code=code)
    assert code == 0, "sfmba_shim_run_sfm_mesh returned %d" % code
    return dict(poses=poses, K=K, has_map=has_map.astype(bool), depth=depth, dense_xyz=dxyz[:n_dense.value], unchanged=unchanged.value,
                origin=grid[:3].copy(), voxel=grid[3], trunc=grid[4], dims=grid[5:].astype(np.int32), mesh_xyz=mxyz[:nv.value],
                mesh_bgr=mbgr[:nv.value], mesh_tri=mtri[:nt.value])


def run_capi(inp, cls):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from sfm_toy_library_amd import capi
    maps = [d if has else None for d, has in zip(cls["depth"], cls["has_map"])]
    out = capi.tsdf_mesh(list(inp["images"]), cls["K"].reshape(3, 3), cls["poses"].reshape(-1, 3, 4), maps, cls["origin"], float(cls["voxel"]),
                         tuple(int(v) for v in cls["dims"]), float(cls["trunc"]), min_weight=settings(inp)[3])
    return dict(mesh_xyz=out["xyz"], mesh_bgr=out["bgr"], mesh_tri=out["tri"], mesh_vkey=out["vkey"])


if __name__ == "__main__":
    mode, src = sys.argv[1:3]
    inp = dict(np.load(src))
    if mode == "class":
        np.savez(sys.argv[3], **run_class_mesh(inp, ply_prefix=sys.argv[4] if len(sys.argv) > 4 else None))
    elif mode == "refuse":
        np.savez(sys.argv[3], **run_class_mesh(inp, what=1))
    else:
        np.savez(sys.argv[4], **run_capi(inp, dict(np.load(sys.argv[3]))))
