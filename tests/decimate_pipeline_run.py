"""sfmtoylib::SfM::runSfM, densify, meshDenseCloud, textureMesh, decimateMesh, textureMesh, cleanMesh and decimateMesh again, as a
program -- TEST INFRASTRUCTURE ONLY.

    python tests/decimate_pipeline_run.py class INPUT.npz OUTPUT.npz [PLY_PREFIX]
    python tests/decimate_pipeline_run.py capi  INPUT.npz CLASS.npz OUTPUT.npz
    python tests/decimate_pipeline_run.py refuse INPUT.npz OUTPUT.npz

INPUT.npz holds images [v, h, w] or [v, h, w, 3] and, optionally, cell_voxels, placement, reg and patch.  `class`: the steps in one
call (sfmba_shim_run_sfm_mesh_decimate), <prefix>_mesh_decimated.ply of the decimated mesh written if a prefix is given.  OUTPUT.npz:
unchanged, K, poses, has_map, depth, the grid the class chose (origin, voxel, trunc, dims), four meshes (mesh_*, clean_*, decimated_* made from the
mesh, decimated_clean_* made from the clean mesh: xyz, bgr, normal, tri) and per textured mesh (raw_* on the mesh before decimateMesh,
coarse_* on the decimated mesh) atlas, uv, view, textured, same_source.  `capi`: sfmba_mesh_decimate, sfmba_mesh_smooth and
sfmba_mesh_texture through the ctypes binding with the class's meshes and the host rules of host/SfM.h; OUTPUT.npz: the same names.
`refuse`: decimateMesh without a meshDenseCloud (no device involved); OUTPUT.npz: code.  tests/test_gpu_mesh_decimate_pipeline.py starts
it as a fresh process with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0."""
import ctypes as C
import sys

import numpy as np

from sfm_loop import ROOT, _a, _p, bp, fp, ip, lib, lp
from texture_pipeline_run import host_rules as texture_rules

MESHES = ("mesh", "clean", "decimated", "decimated_clean")


def settings(inp):
    return float(inp.get("cell_voxels", 2.0)), int(inp.get("placement", 1)), int(inp.get("reg", 1024)), int(inp.get("patch", 6))


def run_class_decimate(inp, ply_prefix=None, debug_level=4, what=0):
    images = _a(inp["images"], np.uint8)
    n, h, w = images.shape[:3]
    channels = 3 if images.ndim == 4 else 1
    cell_voxels, placement, reg, patch = settings(inp)
    img_ptr = np.arange(n + 1, dtype=np.int64) * h * w * channels
    wd, ht = np.full(n, w, np.int32), np.full(n, h, np.int32)
    cap = n * h * w
    vcap, tcap = 4 * cap, 8 * cap
    acap = 3 * (tcap // 2 + 4 * int(np.sqrt(tcap)) + 64) * (patch + 1) * patch        # the atlas of tcap triangles, and a row and a column to spare
    poses, K, has_map, depth = np.zeros((n, 12), np.float32), np.zeros(9, np.float32), np.zeros(n, np.uint8), np.zeros(cap, np.float32)
    grid, counts = np.zeros(8, np.float32), np.zeros(8, np.int64)
    xyz, bgr, nrm, tri = np.zeros((4, vcap, 3), np.float32), np.zeros((4, vcap, 3), np.uint8), np.zeros((4, vcap, 3), np.float32), np.zeros((4, tcap, 3), np.int32)
    wh, atlas, uv, view = np.zeros(4, np.int32), np.zeros((2, acap), np.uint8), np.zeros((2, tcap, 6), np.float32), np.zeros((2, tcap), np.int32)
    textured, same_source = np.zeros(2, np.int64), np.zeros(2, np.int32)
    unchanged = C.c_int(0)
    code = lib().sfmba_shim_run_sfm_mesh_decimate(C.c_int(what), C.c_int(n), C.c_int(channels), _p(img_ptr, lp), _p(images, bp), _p(wd, ip), _p(ht, ip),
                                                  C.c_int(debug_level), C.c_float(cell_voxels), C.c_int(placement), C.c_int(reg), C.c_int(patch),
                                                  ply_prefix.encode() if ply_prefix else None, _p(poses, fp), _p(K, fp), _p(has_map, bp), _p(depth, fp),
                                                  _p(grid, fp), C.byref(unchanged), C.c_int64(vcap), C.c_int64(tcap), _p(counts, lp), _p(xyz, fp),
                                                  _p(bgr, bp), _p(nrm, fp), _p(tri, ip), C.c_int64(acap), _p(wh, ip), _p(atlas, bp), _p(uv, fp),
                                                  _p(view, ip), _p(textured, lp), _p(same_source, ip))
    if what:
        return dict(code=code)
    assert code == 0, "sfmba_shim_run_sfm_mesh_decimate returned %d" % code
    out = dict(unchanged=unchanged.value, K=K.reshape(3, 3), poses=poses.reshape(n, 3, 4), has_map=has_map, depth=depth.reshape(n, h, w), origin=grid[:3].copy(),
               voxel=grid[3], trunc=grid[4], dims=grid[5:].astype(np.int32), patch=patch)
    for k, name in enumerate(MESHES):
        nv, nt = int(counts[2 * k]), int(counts[2 * k + 1])
        out.update({name + "_xyz": xyz[k, :nv].copy(), name + "_bgr": bgr[k, :nv].copy(), name + "_normal": nrm[k, :nv].copy(), name + "_tri": tri[k, :nt].copy()})
    for k, (name, mesh) in enumerate((("raw", "mesh"), ("coarse", "decimated"))):
        W, H, nt = int(wh[2 * k]), int(wh[2 * k + 1]), len(out[mesh + "_tri"])
        out.update({name + "_atlas": atlas[k, :3 * W * H].reshape(H, W, 3).copy(), name + "_uv": uv[k, :nt].reshape(-1, 3, 2).copy(),
                    name + "_view": view[k, :nt].copy(), name + "_textured": int(textured[k]), name + "_same_source": int(same_source[k])})
    return out


def host_rules(inp, cls):
    """(quantum, cell) as the top of host/SfM.h states them"""
    quantum = np.float32(cls["voxel"]) / np.float32(1024.0)
    return float(quantum), int(np.floor(settings(inp)[0] * 1024.0 + 0.5))


def run_capi(inp, cls):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from sfm_toy_library_amd import capi
    _, placement, reg, _ = settings(inp)
    quantum, cell = host_rules(inp, cls)
    out = {}
    for name, source in (("decimated", "mesh"), ("decimated_clean", "clean")):
        got = capi.mesh_decimate(cls[source + "_xyz"], cls[source + "_bgr"], cls[source + "_tri"], cls["origin"], quantum, cell, placement, reg)
        nrm = capi.mesh_smooth(got["xyz"], got["tri"], cls["origin"], quantum, 0)
        assert got["xyz"].tobytes() == nrm["xyz"].tobytes()
        out.update({name + "_xyz": got["xyz"], name + "_bgr": got["bgr"], name + "_normal": nrm["normal"], name + "_tri": got["tri"],
                    name + "_stats": np.asarray(got["stats"], np.int64)})
    images = list(_a(inp["images"], np.uint8))
    maps = [m if has else None for m, has in zip(cls["depth"], cls["has_map"])]
    for name, mesh in (("raw", "mesh"), ("coarse", "decimated")):
        xyz, bgr, tri = cls[mesh + "_xyz"], cls[mesh + "_bgr"], cls[mesh + "_tri"]
        occl_tol, min_area, B = texture_rules(cls, len(tri))
        got = capi.mesh_texture(xyz, bgr, tri, images, cls["K"], cls["poses"], maps, occl_tol, min_area, int(cls["patch"]), B)
        out.update({name + "_atlas": got["atlas"], name + "_uv": got["uv"], name + "_view": got["view"], name + "_textured": got["n_textured"]})
    return out


if __name__ == "__main__":
    mode, src = sys.argv[1:3]
    inp = dict(np.load(src))
    if mode == "class":
        np.savez(sys.argv[3], **run_class_decimate(inp, ply_prefix=sys.argv[4] if len(sys.argv) > 4 else None))
    elif mode == "refuse":
        np.savez(sys.argv[3], **run_class_decimate(inp, what=1))
    else:
        np.savez(sys.argv[4], **run_capi(inp, dict(np.load(sys.argv[3]))))
