"""Mesh-cleaning measurement (sfmba_mesh_clean, sfmba_mesh_components, sfmba_mesh_filter, sfmba_mesh_smooth): one JSON line per workload.

  corner      the four rendered 640 x 480 corner views of tests/sfm_scene.py through SfM::runSfM, densify and meshDenseCloud at
              resolution 256, then cleanMesh with its defaults
  crazyhorse  the seven Crazy Horse photographs at 512 x 384 (tests/golden/crazyhorse_half) through the same steps

Per workload, on the mesh the class made and with the host rules of host/SfM.h: the HIP-event times of the phases of one
sfmba_mesh_clean call (SFMBA_MESH_CLEAN_TIMING; median over --reps calls after --warmup, the capacities given so that a call is ONE
call), its end-to-end time, the time of one smoothing pass (smooth_ms over the 2 x iterations passes: the degree count and the final
positions are inside it), the bytes each phase must move (this tool's own arithmetic from the counts, stated in the code) and the rate
that gives, the components, what the default rule removes, and the share of boundary edges and the Euler characteristic before and
after.  Beside them the end-to-end time of the two-call form (filter, then smooth, the mesh crossing the host twice) and of
sfmba_mesh_components alone.  Every repetition is compared byte for byte with the first, the one-call form with the two-call form and
with the class's clean mesh.  These are first measurements; nothing is gated on them.
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dense_bench import measure  # noqa: E402

PHASES = ("upload_ms", "check_ms", "components_ms", "filter_ms", "quantise_ms", "smooth_ms", "normals_ms", "download_ms")
KERNELS = ("check_ms", "components_ms", "filter_ms", "quantise_ms", "smooth_ms", "normals_ms")


def must_move(nv, nt, kv, kt, iterations):
    """Bytes each phase cannot avoid, from the counts alone (V, T of the input; v, t kept): every array read or written once per kernel
    that needs it, atomics counted as a read and a write of their word, no reuse assumed across kernels.
      components   init 4 V; hook reads 12 T and touches parent at least twice per triangle (16 T); flatten 8 V; count 12 T + 4 T + 8 T;
                   summary 8 V
      filter       keep 12 T + 8 T (label, count) + 4 T + 12 T (flags); two scans 8 (T + V); emit 12 T + 4 T + 12 t and 27 v + 12 V
      one pass     scatter: 12 t indices, 36 t positions, 9 x 16 t for the int64 atomics; move: v (12 + 12 + 24 + 24 + 4)
      normals      scatter as a pass's (12 + 36 + 144) t; final v (24 + 12)"""
    comp = 4 * nv + 28 * nt + 8 * nv + 24 * nt + 8 * nv
    filt = 36 * nt + 8 * (nt + nv) + 16 * nt + 12 * kt + 27 * kv + 12 * nv
    one_pass = 192 * kt + 76 * kv
    normals = 192 * kt + 36 * kv
    return dict(components=comp, filter=filt, one_pass=one_pass, smooth=2 * iterations * one_pass + 12 * kt + 4 * 3 * kt + 24 * kv, normals=normals)


def workload(capi, name, images, args):
    import mesh_clean_pipeline_run as run
    import mesh_oracle as mo
    inp = dict(images=images)
    cls = run.run_class_clean(inp)
    quantum, min_triangles = run.host_rules(inp, cls)
    xyz, bgr, tri = cls["mesh_xyz"], cls["mesh_bgr"], cls["mesh_tri"]
    nv, nt, kv, kt = len(xyz), len(tri), len(cls["clean_xyz"]), len(cls["clean_tri"])
    iterations, lam, mu = 10, 0.5, -0.53
    same = lambda a, b: all((a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    call = lambda: capi.mesh_clean(xyz, bgr, tri, cls["origin"], quantum, min_triangles, False, iterations, lam, mu, vcap=kv, tcap=kt)
    clean, med, wall, wall_min = measure(call, "mesh_clean", PHASES, same, args.reps, args.warmup)
    for k in ("xyz", "bgr", "normal", "tri"):
        assert clean[k].tobytes() == cls["clean_" + k].tobytes(), k
    two, alone = [], []
    for _ in range(max(args.reps // 2, 1)):
        t0 = time.perf_counter()
        f = capi.mesh_filter(xyz, bgr, tri, min_triangles, False, vcap=kv, tcap=kt)
        s = capi.mesh_smooth(f["xyz"], f["tri"], cls["origin"], quantum, iterations, lam, mu)
        two.append(1e3 * (time.perf_counter() - t0))
        assert s["xyz"].tobytes() == clean["xyz"].tobytes() and s["normal"].tobytes() == clean["normal"].tobytes() and f["tri"].tobytes() == clean["tri"].tobytes()
        t0 = time.perf_counter()
        comp = capi.mesh_components(nv, tri)
        alone.append(1e3 * (time.perf_counter() - t0))
    before, after = mo.topology(tri), mo.topology(clean["tri"])
    kernel_ms = sum(med[k] for k in KERNELS)
    need = must_move(nv, nt, kv, kt, iterations)
    top = max(KERNELS, key=lambda k: med[k])
    out = dict(workload=name, views=len(images), vertices=nv, triangles=nt, components=comp["n_components"],
               largest_triangles=int(comp["comp_triangles"].max()) if nv else 0, min_triangles=min_triangles, iterations=iterations,
               vertices_removed=nv - kv, triangles_removed=nt - kt, boundary_share_before=round(before[2] / max(before[3], 1), 4),
               boundary_share_after=round(after[2] / max(after[3], 1), 4), euler_before=before[1], euler_after=after[1], reps=args.reps)
    for k in PHASES:
        out[k.replace("_ms", "_us")] = round(1e3 * med[k], 1)
    out.update(kernels_us=round(1e3 * kernel_ms, 1), one_pass_us=round(1e3 * med["smooth_ms"] / (2 * iterations), 2), dominant=top.replace("_ms", ""),
               dominant_share=round(med[top] / kernel_ms, 3), call_ms=round(wall, 3), call_ms_min=round(wall_min, 3),
               two_calls_ms=round(float(np.median(two)), 3), components_call_ms=round(float(np.median(alone)), 3), accumulation="int64 atomics (scatter)")
    for k, ms in (("components", med["components_ms"]), ("filter", med["filter_ms"]), ("smooth", med["smooth_ms"]), ("normals", med["normals_ms"])):
        out[k + "_must_move_MB"] = round(need[k] / 1e6, 2)
        out[k + "_GB_per_s"] = float("%.4g" % (need[k] / (ms * 1e-3) / 1e9)) if ms > 0 else None
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="corner,crazyhorse")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_MESH_CLEAN_TIMING"] = "1"
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
