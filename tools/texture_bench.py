"""Texturing measurement (sfmba_mesh_texture): one JSON line per workload.

  corner      the four rendered 640 x 480 corner views of tests/sfm_scene.py through SfM::runSfM, densify and meshDenseCloud at
              resolution 256, then textureMesh with its defaults (S = 6)
  crazyhorse  the seven Crazy Horse photographs at 512 x 384 (tests/golden/crazyhorse_half) through the same steps

Per workload, on the mesh the class made and with the host rules of host/SfM.h: the HIP-event times of the phases of one
sfmba_mesh_texture call (SFMBA_MESH_TEXTURE_TIMING; median over --reps calls after --warmup), its end-to-end time, the atlas size, the
texels per second of the raster kernel, and that rate set against two ceilings BY THIS TOOL'S OWN ARITHMETIC (stated in the code): the
rate at which a plain copy of the atlas would run, and the rate at which the fp64 instructions of a texel can issue.  Also the share of
textured triangles and of adjacent triangle pairs with different views.  Every repetition is compared byte for byte with the first and
with the class's textured mesh.  These are first measurements; nothing is gated on them.
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

PHASES = ("upload_ms", "check_ms", "views_ms", "raster_ms", "download_ms")
KERNELS = ("check_ms", "views_ms", "raster_ms")

# The ceilings.  COPY: a streaming float4 copy on this part is taken at 6.29 TB/s of reads plus writes (79 % of the 8 TB/s on the data
# sheet; NOT measured by this tool); a copy of the atlas reads and writes 3 bytes per texel.  FP64: 256 CUs x 4 SIMDs x 16 fp64 lanes per clock
# x 2.4 GHz = 39.3e12 fp64 instructions per second (an fma counts once).  A texel issues, by our count of texture_math.h: the blend
# 9 mul + 6 add + 3 div and 4 conversions, the camera point 9 mul + 9 add, the image point 2 mul + 2 add + 2 div, the NaN tests and the
# clamps 8, the fixed point 2 mul + 2 add + 2 floor + 2 conversions: 49 plain instructions and 5 divisions.  A correctly rounded fp64
# division is a sequence of about 10 instructions (scale, reciprocal, Newton steps in fma, fix-up), so a texel is about 99 fp64
# instructions.  The integer work (the two divisions by run-time values that split the texel index, the sample's products) issues on the
# same VALU and is NOT in this count: the ceiling is an upper bound.
COPY_BYTES_PER_S = 6.29e12
FP64_INSTR_PER_S = 256 * 4 * 16 * 2.4e9
FP64_INSTR_PER_TEXEL = 49 + 5 * 10


def workload(capi, name, images, args):
    import texture_oracle as to
    import texture_pipeline_run as run
    inp = dict(images=images)
    cls = run.run_class_texture(inp)
    xyz, bgr, tri = cls["mesh_xyz"], cls["mesh_bgr"], cls["mesh_tri"]
    nv, nt = len(xyz), len(tri)
    occl_tol, min_area, B = run.host_rules(cls, nt)
    maps = [m if has else None for m, has in zip(cls["depth"], cls["has_map"])]
    same = lambda a, b: all((a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    call = lambda: capi.mesh_texture(xyz, bgr, tri, list(images), cls["K"], cls["poses"], maps, occl_tol, min_area, 6, B)
    got, med, wall, wall_min = measure(call, "mesh_texture", PHASES, same, args.reps, args.warmup)
    for k in ("atlas", "uv", "view"):
        assert got[k].tobytes() == cls["raw_" + k].tobytes(), k
    H, W = got["atlas"].shape[:2]
    owned = nt * 6 * 7 // 2
    raster_s = med["raster_ms"] * 1e-3
    pairs, changes = to.view_changes(tri, got["view"])
    # the same call without the area floor (min_area 0): what the floor of half a square pixel leaves to the vertex colours
    os.environ.pop("SFMBA_MESH_TEXTURE_TIMING", None)
    free = capi.mesh_texture(xyz, bgr, tri, list(images), cls["K"], cls["poses"], maps, occl_tol, 0, 6, B)
    os.environ["SFMBA_MESH_TEXTURE_TIMING"] = "1"
    _, free_changes = to.view_changes(tri, free["view"])
    copy_rate, fp64_rate = COPY_BYTES_PER_S / 6.0, FP64_INSTR_PER_S / FP64_INSTR_PER_TEXEL
    out = dict(workload=name, views=len(images), image=list(images[0].shape[1::-1]), vertices=nv, triangles=nt, patch=6, blocks_per_row=B, atlas=[W, H],
               atlas_MB=round(3 * W * H / 1e6, 2), texels=W * H, owned_texels=owned, textured=got["n_textured"],
               textured_share=round(got["n_textured"] / float(max(nt, 1)), 4), adjacent_pairs=pairs, view_change_share=round(changes / float(max(pairs, 1)), 4),
               textured_share_without_floor=round(free["n_textured"] / float(max(nt, 1)), 4),
               view_change_share_without_floor=round(free_changes / float(max(pairs, 1)), 4), reps=args.reps)
    for k in PHASES:
        out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
    out.update(kernels_us=round(1e3 * sum(med[k] for k in KERNELS), 1), call_ms=round(wall, 3), call_ms_min=round(wall_min, 3),
               raster_Gtexels_per_s=float("%.4g" % (W * H / raster_s / 1e9)), copy_ceiling_Gtexels_per_s=float("%.4g" % (copy_rate / 1e9)),
               fp64_ceiling_Gtexels_per_s=float("%.4g" % (fp64_rate / 1e9)), share_of_copy_ceiling=round(W * H / raster_s / copy_rate, 4),
               share_of_fp64_ceiling=round(owned / raster_s / fp64_rate, 4), views_Mtriangle_views_per_s=float("%.4g" % (nt * len(images) / (med["views_ms"] * 1e-3) / 1e6)))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="corner,crazyhorse")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_MESH_TEXTURE_TIMING"] = "1"
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
