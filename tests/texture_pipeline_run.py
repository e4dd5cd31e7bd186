"""sfmtoylib::SfM::runSfM, densify, meshDenseCloud, textureMesh, cleanMesh and textureMesh again, as a program -- TEST INFRASTRUCTURE ONLY.

    python tests/texture_pipeline_run.py class INPUT.npz OUTPUT.npz [OBJ_PREFIX]
    python tests/texture_pipeline_run.py capi  INPUT.npz CLASS.npz OUTPUT.npz
    python tests/texture_pipeline_run.py refuse INPUT.npz OUTPUT.npz

INPUT.npz holds images [v, h, w] or [v, h, w, 3] and, optionally, patch.  `class`: the steps in one call (sfmba_shim_run_sfm_texture),
<prefix>_textured.{obj,mtl,png} of the mesh and <prefix>_clean_textured.{obj,mtl,png} of the clean mesh written if a prefix is given.
OUTPUT.npz: unchanged, K, poses, has_map, depth, voxel, the mesh and the clean mesh (mesh_* / clean_*: xyz, bgr, tri) and per textured
mesh (raw_* on the mesh, cleaned_* on the clean mesh) atlas, uv, view, textured, same_source.  `capi`: sfmba_mesh_texture through the
ctypes binding with the class's meshes and the host rules of host/SfM.h; OUTPUT.npz: the same raw_* / cleaned_* names, and the PNG files
of PREFIX (stored in CLASS.npz as obj_prefix) decoded by sfmba_png_decode as raw_png / cleaned_png.  `refuse`: textureMesh without a
meshDenseCloud (no device involved); OUTPUT.npz: code.  tests/test_gpu_texture_pipeline.py starts it as a fresh process with
SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0."""
import ctypes as C
import sys

import numpy as np

from sfm_loop import ROOT, _a, _p, bp, fp, ip, lib, lp


def run_class_texture(inp, obj_prefix=None, debug_level=4, what=0):
    images = _a(inp["images"], np.uint8)
    n, h, w = images.shape[:3]
    channels = 3 if images.ndim == 4 else 1
    patch = int(inp.get("patch", 6))
    img_ptr = np.arange(n + 1, dtype=np.int64) * h * w * channels
    wd, ht = np.full(n, w, np.int32), np.full(n, h, np.int32)
    cap = n * h * w
    vcap, tcap = 4 * cap, 8 * cap
    acap = 3 * (tcap // 2 + 4 * int(np.sqrt(tcap)) + 64) * (patch + 1) * patch        # the atlas of tcap triangles, and a row and a column to spare
    poses, K, has_map, depth = np.zeros((n, 12), np.float32), np.zeros(9, np.float32), np.zeros(n, np.uint8), np.zeros(cap, np.float32)
    mxyz, mbgr, mtri = np.zeros((vcap, 3), np.float32), np.zeros((vcap, 3), np.uint8), np.zeros((tcap, 3), np.int32)
    cxyz, cbgr, ctri = np.zeros((vcap, 3), np.float32), np.zeros((vcap, 3), np.uint8), np.zeros((tcap, 3), np.int32)
    wh, atlas, uv, view = np.zeros(4, np.int32), np.zeros((2, acap), np.uint8), np.zeros((2, tcap, 6), np.float32), np.zeros((2, tcap), np.int32)
    textured, same_source = np.zeros(2, np.int64), np.zeros(2, np.int32)
    voxel, unchanged, nv, nt, cv, ct = C.c_float(0), C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    code = lib().sfmba_shim_run_sfm_texture(C.c_int(what), C.c_int(n), C.c_int(channels), _p(img_ptr, lp), _p(images, bp), _p(wd, ip), _p(ht, ip),
                                            C.c_int(debug_level), C.c_int(patch), obj_prefix.encode() if obj_prefix else None, _p(poses, fp), _p(K, fp),
                                            _p(has_map, bp), _p(depth, fp), C.byref(voxel), C.byref(unchanged), C.c_int64(vcap), C.c_int64(tcap),
                                            C.byref(nv), C.byref(nt), _p(mxyz, fp), _p(mbgr, bp), _p(mtri, ip), C.byref(cv), C.byref(ct), _p(cxyz, fp),
                                            _p(cbgr, bp), _p(ctri, ip), C.c_int64(acap), _p(wh, ip), _p(atlas, bp), _p(uv, fp), _p(view, ip),
                                            _p(textured, lp), _p(same_source, ip))
    if what:
        return dict(code=code)
    assert code == 0, "sfmba_shim_run_sfm_texture returned %d" % code
    counts = (nt.value, ct.value)
    out = dict(unchanged=unchanged.value, K=K.reshape(3, 3), poses=poses.reshape(n, 3, 4), has_map=has_map, depth=depth.reshape(n, h, w), voxel=voxel.value,
               patch=patch, mesh_xyz=mxyz[:nv.value], mesh_bgr=mbgr[:nv.value], mesh_tri=mtri[:nt.value], clean_xyz=cxyz[:cv.value],
               clean_bgr=cbgr[:cv.value], clean_tri=ctri[:ct.value], obj_prefix=obj_prefix or "")
    for k, name in enumerate(("raw", "cleaned")):
        W, H = int(wh[2 * k]), int(wh[2 * k + 1])
        out.update({name + "_atlas": atlas[k, :3 * W * H].reshape(H, W, 3).copy(), name + "_uv": uv[k, :counts[k]].reshape(-1, 3, 2).copy(),
                    name + "_view": view[k, :counts[k]].copy(), name + "_textured": int(textured[k]), name + "_same_source": int(same_source[k])})
    return out


def host_rules(cls, n_triangles):
    """(occl_tol, min_area, blocks_per_row) as the top of host/SfM.h states them, at the defaults of TextureParams"""
    occl_tol = float(np.float32(2.0) * np.float32(cls["voxel"]))
    blocks, B = (n_triangles + 1) // 2, 1
    while B * B < blocks:
        B += 1
    return occl_tol, int(round(2 * 256 * 0.5)), B


def run_capi(inp, cls):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from sfm_toy_library_amd import capi
    images = list(_a(inp["images"], np.uint8))
    maps = [m if has else None for m, has in zip(cls["depth"], cls["has_map"])]
    out = {}
    for name, mesh in (("raw", "mesh"), ("cleaned", "clean")):
        xyz, bgr, tri = cls[mesh + "_xyz"], cls[mesh + "_bgr"], cls[mesh + "_tri"]
        occl_tol, min_area, B = host_rules(cls, len(tri))
        got = capi.mesh_texture(xyz, bgr, tri, images, cls["K"], cls["poses"], maps, occl_tol, min_area, int(cls["patch"]), B)
        out.update({name + "_atlas": got["atlas"], name + "_uv": got["uv"], name + "_view": got["view"], name + "_textured": got["n_textured"]})
    prefix = str(cls["obj_prefix"])
    if prefix:
        files = [open(prefix + suffix + "_textured.png", "rb").read() for suffix in ("", "_clean")]
        infos, decoded = capi.png_decode(files)                    # B, G, R, as the atlas
        out["png_status"] = np.asarray([i["status"] for i in infos])
        assert not out["png_status"].any(), infos
        out["raw_png"], out["cleaned_png"] = decoded
    return out


if __name__ == "__main__":
    mode, src = sys.argv[1:3]
    inp = dict(np.load(src))
    if mode == "class":
        np.savez(sys.argv[3], **run_class_texture(inp, obj_prefix=sys.argv[4] if len(sys.argv) > 4 else None))
    elif mode == "refuse":
        np.savez(sys.argv[3], **run_class_texture(inp, what=1))
    else:
        np.savez(sys.argv[4], **run_capi(inp, dict(np.load(sys.argv[3]))))
