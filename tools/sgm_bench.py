"""Semi-global matching measurement (sfmba_depth_sweep_sgm beside the unchanged sfmba_depth_sweep): one JSON line per workload.

  a        one 1024 x 768 job with 2 sources at D = 64, r = 3 (tools/dense_bench.py's workload a)
  b        the four 640 x 480 corner views of tests/sfm_scene.py in one call (its workload b)
  quality  sfmtoy -D --mesh 256 with and without --sgm on the corner views and on the seven Crazy Horse photographs at 512 x 384
           (tests/golden/crazyhorse_half): dense points and the share of boundary edges of the mesh; and, on the corner views through
           the class, every dense point against the true surface point of its own pixel after the best similarity

a, b: HIP-event times of the phases of both calls in the same run (SFMBA_DEPTH_TIMING; median over --reps calls after --warmup, the two
calls alternating): the sweep kernel, the kernel that stores the cost volume in its place, the aggregation as a whole and per direction,
the selection and the finish.  The aggregation's bytes are counted here -- with E = pixels * D entries: every direction reads the volume
(E bytes); the first writes the sums (2 E), each later one reads and writes them (4 E): (3 + 5 (n_paths - 1)) E -- and set against its
time.  Every repetition is compared byte for byte with the first.  First measurements; nothing is gated on them.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SWEEP = dict(n_planes=64, radius=3, min_std=2, min_sources=1)
SGM = dict(p1=8, p2=64, n_paths=8, invalid_cost=127, uniqueness=5)
SFMTOY = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")


def captured(call):
    """(result, what the library wrote to stderr)"""
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            res = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return res, f.read().decode()


def phases(text, tag):
    """{name: ms} of the timing lines of one call; the eight per-direction times as path_ms [8]"""
    out = {}
    for line in re.findall(r"\[sfmba " + tag + r"\] (.*)", text):
        tok = line.split()
        if "path_ms" in tok:
            at = tok.index("path_ms")
            out["path_ms"] = [float(v) for v in tok[at + 1:at + 9]]
            tok = tok[:at]
        out.update({k: float(v) for k, v in zip(tok[::2], tok[1::2])})
    if not out:
        raise RuntimeError("no timing line from the library: %r" % text)
    return out


def timing(capi, name, images, K, P, jobs, args):
    same = lambda a, b: all(x[i].tobytes() == y[i].tobytes() for x, y in zip(a, b) for i in range(3))
    plain = lambda: capi.depth_sweep(images, K, P, jobs, min_score=0.6, **SWEEP)
    sgm = lambda: capi.depth_sweep_sgm(images, K, P, jobs, **dict(SWEEP, **SGM))
    rows, first = dict(plain=[], sgm=[]), {}
    for rep in range(args.warmup + args.reps):
        for kind, call, tag in (("plain", plain, "depth_sweep"), ("sgm", sgm, "depth_sweep_sgm")):
            res, text = captured(call)
            assert same(first.setdefault(kind, res), res), "two calls differ"
            if rep >= args.warmup:
                rows[kind].append(phases(text, tag))
    med = lambda kind, k: float(np.median([r[k] for r in rows[kind]]))
    paths = np.median([r["path_ms"] for r in rows["sgm"]], axis=0)
    entries = sum(images[j[0]].size for j in jobs) * SWEEP["n_planes"]
    agg_bytes = (3 + 5 * (SGM["n_paths"] - 1)) * entries
    agg_ms = med("sgm", "aggregate_ms")
    out = dict(workload=name, jobs=len(jobs), sizes=sorted({images[j[0]].shape[::-1] for j in jobs}), reps=args.reps, **SWEEP, **SGM,
               sweep_us=round(1e3 * med("plain", "sweep_ms"), 1), cost_store_us=round(1e3 * med("sgm", "sweep_ms"), 1),
               aggregate_us=round(1e3 * agg_ms, 1), per_direction_us=[round(1e3 * float(v), 1) for v in paths],
               select_us=round(1e3 * med("sgm", "select_ms"), 1), finish_us=round(1e3 * med("sgm", "finish_ms"), 1),
               volume_entries=entries, aggregate_bytes=agg_bytes, aggregate_TB_per_s=float("%.4g" % (agg_bytes / (agg_ms * 1e-3) / 1e12)),
               aggregate_over_sweep=float("%.3g" % (agg_ms / med("plain", "sweep_ms"))),
               accepted_plain=[int((r[0] > 0).sum()) for r in first["plain"]], accepted_sgm=[int((r[0] > 0).sum()) for r in first["sgm"]])
    print(json.dumps(out), flush=True)


def boundary_share(tri):
    e = np.sort(np.asarray(tri, np.int64).reshape(-1, 3)[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    _, n = np.unique(e[:, 0] * (int(e.max()) + 1) + e[:, 1], return_counts=True)
    return round(float((n == 1).sum()) / max(len(n), 1), 4)


def ply_counts(prefix):
    """(dense points, mesh triangles, share of boundary edges) of the files one sfmtoy run wrote"""
    head = lambda path: open(path, "rb").read().split(b"end_header")[0].decode()
    count = lambda text, what: int(re.search(r"element " + what + r" (\d+)", text).group(1))
    points = count(head(prefix + "_dense.ply"), "vertex")
    text = head(prefix + "_mesh.ply")
    nv, nf = count(text, "vertex"), count(text, "face")
    rows = open(prefix + "_mesh.ply").read().split("end_header")[1].split("\n")[1 + nv:1 + nv + nf]
    tri = np.array([[int(v) for v in r.split()[1:4]] for r in rows])
    return points, nf, boundary_share(tri)


def sfmtoy_quality(name, directory, tmp):
    out = dict(workload="quality", scene=name, mesh_resolution=256, sgm="%(p1)d,%(p2)d paths %(n_paths)d uniqueness %(uniqueness)d" % SGM)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SFMBA_")}
    env["SFMBA_DETERMINISTIC"] = "1"
    for kind, extra in (("plain", []), ("sgm", ["--sgm"])):
        prefix = os.path.join(tmp, name + "_" + kind)
        subprocess.run([SFMTOY, "-d", "4", "-D", "--mesh", "256", "-o", prefix] + extra + [directory], env=env, check=True, timeout=300)
        out["dense_points_" + kind], out["mesh_triangles_" + kind], out["boundary_share_" + kind] = ply_counts(prefix)
    return out


def corner_distance(images, scene):
    """every dense point of the class against the true surface point of its own pixel, after the similarity that best maps the one
    set on the other (tests/test_gpu_depth_pipeline.py prints the same figure for the plain sweep)"""
    import depth_cases as dc
    import sfm_scene
    import sgm_pipeline_run as run
    out = {}
    Kinv = np.linalg.inv(scene["K"])
    h, w = images.shape[1:]
    for kind, sgm in (("plain", [0, 8, 64, 8, 127, 5]), ("sgm", [1] + [SGM[k] for k in ("p1", "p2", "n_paths", "invalid_cost", "uniqueness")])):
        cls = run.run_class_sgm(dict(images=images), sgm)
        est = cls["dense_xyz"].astype(np.float64)
        truth, hit = np.zeros((len(est), 3)), np.zeros(len(est), bool)
        for v in range(len(images)):
            sel = cls["dense_view"] == v
            pix = cls["dense_pixel"][sel]
            z = dc.corner_depth(scene, v).reshape(-1)[pix]
            rays = np.stack([pix % w, pix // w, np.ones(len(pix))], axis=1) @ (scene["R"][v].T @ Kinv).T
            truth[sel] = scene["centres"][v] + np.where(np.isfinite(z), z, 0.0)[:, None] * rays
            hit[sel] = np.isfinite(z)
        s, R, t = sfm_scene.align_similarity(est[hit][::50], truth[hit][::50])
        err = np.linalg.norm(s * est[hit] @ R.T + t - truth[hit], axis=1)
        out["surface_" + kind] = dict(points=len(est), within_0_02=round(float((err <= 0.02).mean()), 4), median=float("%.4g" % np.median(err)),
                                      p95=float("%.4g" % np.percentile(err, 95)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b,quality")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["SFMBA_DEPTH_TIMING"] = "1"
    os.environ.setdefault("SFMBA_DETERMINISTIC", "1")
    from sfm_toy_library_amd import capi
    import depth_cases as dc
    import sfm_scene
    assert capi.device_count() >= 1
    todo = args.workloads.split(",")
    if "a" in todo:
        images, K, P = dc.scene((1024, 768), 2, focal=2500.0, scale=250.0)
        timing(capi, "a", images, K, P, [(0, [1, 2], dc.Z_NEAR, dc.Z_FAR)], args)
    scene = sfm_scene.make_corner(seed=0) if ("b" in todo or "quality" in todo) else None
    if "b" in todo:
        P = np.concatenate([scene["R"], scene["t"][:, :, None]], axis=2).astype(np.float32)
        jobs = [(0, [1, 2], 8.5, 12.0), (1, [0, 2], 8.5, 12.0), (2, [1, 3], 8.5, 12.0), (3, [2, 1], 8.5, 12.0)]
        timing(capi, "b", scene["images"], scene["K"].astype(np.float32), P, jobs, args)
    if "quality" in todo:
        del os.environ["SFMBA_DEPTH_TIMING"]
        with tempfile.TemporaryDirectory() as tmp:
            directory = os.path.join(tmp, "corner")
            os.mkdir(directory)
            for i, im in enumerate(scene["images"]):
                sfm_scene.write_pnm(os.path.join(directory, "view%02d.pgm" % i), im)
            out = sfmtoy_quality("corner", directory, tmp)
            out.update(corner_distance(np.stack(scene["images"]), scene))
            print(json.dumps(out), flush=True)
            print(json.dumps(sfmtoy_quality("crazyhorse", os.path.join(ROOT, "tests", "golden", "crazyhorse_half"), tmp)), flush=True)


if __name__ == "__main__":
    main()
