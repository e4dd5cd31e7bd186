"""sfmtoylib::SfM::runSfM, densify and meshDenseCloud with and without the hole filling, as a program -- TEST INFRASTRUCTURE ONLY.

    python tests/tsdf_fill_pipeline_run.py class INPUT.npz OUTPUT.npz [PLY_PREFIX]
    python tests/tsdf_fill_pipeline_run.py capi  INPUT.npz CLASS.npz OUTPUT.npz
    python tests/tsdf_fill_pipeline_run.py refuse INPUT.npz OUTPUT.npz

INPUT.npz holds images [v, h, w] or [v, h, w, 3] and, optionally, resolution, min_weight, fill_iterations and fill_min_neighbours.
`class`: everything in one call (sfmba_shim_run_sfm_mesh_fill): meshDenseCloud with fillIterations 0, then with the fill, then cleanMesh;
<prefix>_mesh.ply of the filled mesh written if a prefix is given.  OUTPUT.npz: poses, K, has_map, depth and dense_xyz as they stand
after the mesh calls, unchanged, the grid of either call (origin, voxel, trunc, dims; *0 for the call without the fill), the two meshes
(mesh0_* and mesh_*, mesh_filled), filled0_size, filled_size and clean_code.  `capi`: sfmba_tsdf_mesh and sfmba_tsdf_mesh_fill through
the ctypes binding with the class's images, poses, depth maps and grid; OUTPUT.npz: the meshes under the same names, mesh_vkey and
mesh_filled.  `refuse`: meshDenseCloud with fill parameters out of range (no device involved); OUTPUT.npz: code.
tests/test_gpu_tsdf_fill_pipeline.py starts it as a fresh process with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0."""
import ctypes as C
import sys

import numpy as np

from sfm_loop import ROOT, _a, _p, bp, fp, ip, lib, lp


def settings(inp):
    return int(inp.get("resolution", 64)), int(inp.get("min_weight", 1)), int(inp.get("fill_iterations", 3)), int(inp.get("fill_min_neighbours", 2))


def run_class(inp, ply_prefix=None, debug_level=4, what=0):
    images = _a(inp["images"], np.uint8)
    n, h, w = images.shape[:3]
    channels = 3 if images.ndim == 4 else 1
    resolution, min_weight, passes, k = settings(inp)
    img_ptr = np.arange(n + 1, dtype=np.int64) * h * w * channels
    wd, ht = np.full(n, w, np.int32), np.full(n, h, np.int32)
    poses, K, has_map = np.zeros((n, 12), np.float32), np.zeros(9, np.float32), np.zeros(n, np.uint8)
    depth = np.zeros((n, h, w), np.float32)
    cap = n * h * w
    vcap, tcap = cap, 2 * cap
    dxyz, grid = np.zeros((cap, 3), np.float32), np.zeros(16, np.float32)
    m0 = [np.zeros((vcap, 3), np.float32), np.zeros((vcap, 3), np.uint8), np.zeros((tcap, 3), np.int32)]
    m1 = [np.zeros((vcap, 3), np.float32), np.zeros((vcap, 3), np.uint8), np.zeros((tcap, 3), np.int32)]
    filled = np.zeros(vcap, np.uint8)
    unchanged, clean_code = C.c_int(0), C.c_int(0)
    n_dense, nv0, nt0, nv, nt, f0, f1 = (C.c_int64(0) for _ in range(7))
    code = lib().sfmba_shim_run_sfm_mesh_fill(C.c_int(what), C.c_int(n), C.c_int(channels), _p(img_ptr, lp), _p(images, bp), _p(wd, ip), _p(ht, ip),
                                              C.c_int(debug_level), C.c_int(resolution), C.c_int(min_weight), C.c_int(passes), C.c_int(k),
                                              ply_prefix.encode() if ply_prefix else None, _p(poses, fp), _p(K, fp), _p(has_map, bp), _p(depth, fp),
                                              C.c_int64(cap), C.byref(n_dense), _p(dxyz, fp), C.byref(unchanged), _p(grid, fp), C.c_int64(vcap),
                                              C.c_int64(tcap), C.byref(nv0), C.byref(nt0), _p(m0[0], fp), _p(m0[1], bp), _p(m0[2], ip), C.byref(f0),
                                              C.byref(nv), C.byref(nt), _p(m1[0], fp), _p(m1[1], bp), _p(m1[2], ip), _p(filled, bp), C.byref(f1),
                                              C.byref(clean_code))
    if what:
        return dict(code=code)
    assert code == 0, "sfmba_shim_run_sfm_mesh_fill returned %d" % code
    return dict(poses=poses, K=K, has_map=has_map.astype(bool), depth=depth, dense_xyz=dxyz[:n_dense.value], unchanged=unchanged.value,
                origin0=grid[:3].copy(), voxel0=grid[3], trunc0=grid[4], dims0=grid[5:8].astype(np.int32),
                origin=grid[8:11].copy(), voxel=grid[11], trunc=grid[12], dims=grid[13:].astype(np.int32),
                mesh0_xyz=m0[0][:nv0.value], mesh0_bgr=m0[1][:nv0.value], mesh0_tri=m0[2][:nt0.value], filled0_size=f0.value,
                mesh_xyz=m1[0][:nv.value], mesh_bgr=m1[1][:nv.value], mesh_tri=m1[2][:nt.value], mesh_filled=filled[:max(f1.value, 0)],
                filled_size=f1.value, clean_code=clean_code.value)


def run_capi(inp, cls):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from sfm_toy_library_amd import capi
    _, min_weight, passes, k = settings(inp)
    maps = [d if has else None for d, has in zip(cls["depth"], cls["has_map"])]
    args = (list(inp["images"]), cls["K"].reshape(3, 3), cls["poses"].reshape(-1, 3, 4), maps, cls["origin"], float(cls["voxel"]),
            tuple(int(v) for v in cls["dims"]), float(cls["trunc"]))
    plain = capi.tsdf_mesh(*args, min_weight=min_weight)
    out = capi.tsdf_mesh_fill(*args, min_weight=min_weight, fill_iterations=passes, min_neighbours=k)
    return dict(mesh0_xyz=plain["xyz"], mesh0_bgr=plain["bgr"], mesh0_tri=plain["tri"], mesh_xyz=out["xyz"], mesh_bgr=out["bgr"], mesh_tri=out["tri"],
                mesh_vkey=out["vkey"], mesh_filled=out["vfilled"])


if __name__ == "__main__":
    mode, src = sys.argv[1:3]
    inp = dict(np.load(src))
    if mode == "class":
        np.savez(sys.argv[3], **run_class(inp, ply_prefix=sys.argv[4] if len(sys.argv) > 4 else None))
    elif mode == "refuse":
        np.savez(sys.argv[3], **run_class(inp, what=1))
    else:
        np.savez(sys.argv[4], **run_capi(inp, dict(np.load(sys.argv[3]))))
