"""SfM::meshDenseCloud and sfmtoy --mesh through the whole pipeline on the MI355X (-m gpu), on the four rendered 640 x 480 corner
views of tests/test_gpu_sfm_pipeline.py.

Every run is a fresh process (tests/mesh_pipeline_run.py, sfmtoy) with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0 as its only
SFMBA_* variables; a child that fails or overruns its time stops the module.

  mesh          meshDenseCloud equals, byte for byte, the sfmba_tsdf_mesh call made from Python through the C ABI with the class's
                images, poses, depth maps and grid
  grid          the grid the class chose equals the restatement of its rule (the top of host/SfM.h), fed the class's own dense cloud
  bookkeeping   getDenseCloud() and the depth maps are unchanged by the call; without a densify the call refuses and keeps nothing
  PLY           <prefix>_mesh.ply holds exactly the mesh
  sfmtoy        with -D --mesh 256 it writes the class's file, and the other three files equal those of a run without --mesh;
                --mesh without -D is a usage error
  reported      vertices, triangles, the share of boundary edges and the median distance of the vertices to the true planes
                (profiles/tsdf_mesh.txt holds them); NOT gated: nobody has measured them before"""
import os
import subprocess
import sys

import numpy as np
import pytest

import sfm_scene

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SFMTOY = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")
CHILD_TIMEOUT = 120
FAILED = []


def child(cmd, what):
    """One fresh deterministic process; nothing more is started on the device after one went wrong."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SFMBA_")}
    env.update(SFMBA_DETERMINISTIC="1", SFMBA_SHIM_CACHE="0")
    if FAILED:
        pytest.fail("not started: an earlier child process failed (%s)" % FAILED[0])
    try:
        done = subprocess.run(cmd, env=env, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    except subprocess.TimeoutExpired:
        FAILED.append("%s overran %d s" % (what, CHILD_TIMEOUT))
        pytest.fail("%s overran its %d s" % (what, CHILD_TIMEOUT))
    if done.returncode != 0:
        FAILED.append("%s ended with %d" % (what, done.returncode))
        pytest.fail("%s ended with %d:\n%s" % (what, done.returncode, done.stderr.decode()[-2000:]))
    return done


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mesh_pipeline")
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    src = str(tmp / "in.npz")
    np.savez(src, images=gray)
    prefix = str(tmp / "class")
    script = os.path.join(HERE, "mesh_pipeline_run.py")
    child([sys.executable, script, "class", src, str(tmp / "class.npz"), prefix], "class")
    child([sys.executable, script, "capi", src, str(tmp / "class.npz"), str(tmp / "capi.npz")], "capi")
    return dict(np.load(str(tmp / "class.npz"))), dict(np.load(str(tmp / "capi.npz"))), prefix, gray, tmp


def distance_to_the_corner(cls, X):
    """The distance of mesh points X (the reconstruction's frame) to the scene's two half planes, in scene units (a pixel of the views
    is 1 / 250 of one).  The reconstruction is the scene up to a similarity, and the camera centres (1.5 units apart, 10 from the
    surface) fix it too loosely to judge a surface: as tests/test_gpu_depth_pipeline.py does for the dense points, every vertex that
    view 0 sees is paired with the true surface point of the pixel it projects to there, and the similarity that best maps the one
    set on the other is applied to all vertices."""
    import depth_cases as dc
    scene = sfm_scene.make_corner(seed=0)
    P0 = cls["poses"].reshape(-1, 3, 4).astype(np.float64)[0]
    K = cls["K"].reshape(3, 3).astype(np.float64)
    w, h = scene["size"]
    cam = X.astype(np.float64) @ P0[:, :3].T + P0[:, 3]
    u = np.rint(K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2]).astype(np.int64)
    v = np.rint(K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]).astype(np.int64)
    seen = (cam[:, 2] > 0) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
    z = dc.corner_depth(scene, 0)[np.where(seen, v, 0), np.where(seen, u, 0)]
    seen &= np.isfinite(z)
    rays = np.stack([u, v, np.ones(len(u))], axis=1) @ (scene["R"][0].T @ np.linalg.inv(scene["K"])).T
    truth = scene["centres"][0] + np.where(seen, z, 0.0)[:, None] * rays
    s, R, t = sfm_scene.align_similarity(X[seen][::20].astype(np.float64), truth[seen][::20])
    Xs = s * X.astype(np.float64) @ R.T + t
    best = np.full(len(Xs), np.inf)
    for o, u, v, nrm in sfm_scene._plane_frames():
        a = (Xs - o) @ u
        d_plane = np.abs((Xs - o) @ nrm)
        d_edge = np.sqrt(d_plane ** 2 + a ** 2)                       # beyond the edge (a < 0): the distance to the edge line
        best = np.minimum(best, np.where(a >= 0, d_plane, d_edge))
    return best


def test_mesh_equals_the_c_abi_call(runs):
    import mesh_oracle as mo
    cls, capi = runs[0], runs[1]
    assert len(cls["mesh_xyz"]) > 1000 and len(cls["mesh_tri"]) > 1000
    for k in ("mesh_xyz", "mesh_bgr", "mesh_tri"):
        assert cls[k].dtype == capi[k].dtype and cls[k].shape == capi[k].shape and cls[k].tobytes() == capi[k].tobytes(), k
    closed, euler, boundary, n_edges = mo.topology(cls["mesh_tri"])
    d = distance_to_the_corner(cls, cls["mesh_xyz"])
    print("mesh_pipeline corner: grid %s at voxel %.6g, trunc %.6g: %d vertices, %d triangles, %d of %d edges on a boundary (%.4f), "
          "characteristic %d, distance to the true planes median %.5f / 90th percentile %.5f scene units (a pixel is 0.004)"
          % (cls["dims"].tolist(), float(cls["voxel"]), float(cls["trunc"]), len(cls["mesh_xyz"]), len(cls["mesh_tri"]), boundary, n_edges,
             boundary / max(n_edges, 1), euler, np.median(d), np.percentile(d, 90)))


def test_the_grid_equals_its_restatement(runs):
    cls = runs[0]
    cloud = cls["dense_xyz"]
    lo, hi, side = [], [], []
    for a in range(3):
        c = np.sort(cloud[:, a][np.isfinite(cloud[:, a])])
        n = len(c)
        lo.append(c[n // 100]); hi.append(c[(99 * n) // 100])
        side.append(float(hi[-1]) - float(lo[-1]))
    voxel = np.float32(max(side) / float(256 - 1))
    trunc = np.float32(4.0) * voxel
    pad = float(trunc) + float(voxel)
    origin = np.array([np.float32(float(lo[a]) - pad) for a in range(3)], np.float32)
    dims = [min(int(np.floor((side[a] + (pad + pad)) / float(voxel))) + 2, 1024) for a in range(3)]
    assert np.float32(cls["voxel"]).tobytes() == voxel.tobytes() and np.float32(cls["trunc"]).tobytes() == np.float32(trunc).tobytes()
    assert cls["origin"].astype(np.float32).tobytes() == origin.tobytes() and cls["dims"].tolist() == dims
    assert max(dims) in (266, 267)                                   # 255 voxels along the longest side (one rounding either way), 5 of padding at either end, + 2


def test_the_dense_cloud_and_the_depth_maps_are_unchanged(runs):
    cls, _, _, gray, tmp = runs
    assert int(cls["unchanged"]) == 1 and cls["has_map"].sum() == 4 and len(cls["dense_xyz"]) > 100000
    # without a densify the call refuses and keeps nothing (no device involved)
    small = str(tmp / "small.npz")
    np.savez(small, images=gray[:2, :8, :8])
    child([sys.executable, os.path.join(HERE, "mesh_pipeline_run.py"), "refuse", small, str(tmp / "refuse.npz")], "refuse")
    assert int(np.load(str(tmp / "refuse.npz"))["code"]) == 21                              # 20 + ERROR, nothing kept


def test_the_ply_file_holds_exactly_the_mesh(runs):
    cls, _, prefix = runs[:3]
    lines = open(prefix + "_mesh.ply").read().split("\n")
    head = lines.index("end_header          ")
    nv, nt = len(cls["mesh_xyz"]), len(cls["mesh_tri"])
    assert lines[:head] == ["ply                 ", "format ascii 1.0    ", "element vertex %d" % nv, "property float x    ", "property float y    ",
                            "property float z    ", "property uchar red  ", "property uchar green", "property uchar blue ", "element face %d" % nt,
                            "property list uchar int vertex_indices"]
    rows = lines[head + 1:-1]
    assert lines[-1] == "" and len(rows) == nv + nt and all(r.endswith(" ") for r in rows[:nv])
    got = np.array([r.split() for r in rows[:nv]])
    assert np.array_equal(got[:, 3:].astype(int), cls["mesh_bgr"][:, ::-1])                      # R G B
    assert np.array_equal(got[:, :3], np.array([["%g" % v for v in p] for p in cls["mesh_xyz"]]))   # the stream's default: 6 significant digits
    faces = np.array([r.split() for r in rows[nv:]]).astype(int)
    assert (faces[:, 0] == 3).all() and np.array_equal(faces[:, 1:], cls["mesh_tri"])


def test_sfmtoy_mesh_switch(runs):
    cls, _, prefix, gray, tmp = runs
    directory = tmp / "pgm"
    directory.mkdir()
    for i, im in enumerate(gray):
        sfm_scene.write_pnm(str(directory / ("view%02d.pgm" % i)), im)
    dense, meshed = str(tmp / "dense"), str(tmp / "meshed")
    child([SFMTOY, "-d", "4", "-D", "-o", dense, str(directory)], "sfmtoy -D")
    child([SFMTOY, "-d", "4", "-D", "--mesh", "256", "-o", meshed, str(directory)], "sfmtoy -D --mesh 256")
    assert not os.path.exists(dense + "_mesh.ply")
    assert open(meshed + "_mesh.ply", "rb").read() == open(prefix + "_mesh.ply", "rb").read()
    for suffix in ("_points.ply", "_cameras.ply", "_dense.ply"):
        a, b = (open(p + suffix, "rb").read() for p in (dense, meshed))
        assert len(a) > 300 and a == b, suffix
    assert not os.path.exists(meshed + "_dense_merged.ply")
    # --mesh without -D is a usage error: nothing runs
    done = subprocess.run([SFMTOY, "--mesh", "256", str(directory)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
    assert done.returncode == 2 and b"--mesh needs -D" in done.stderr
    done = subprocess.run([SFMTOY, "-D", "--mesh", "1", str(directory)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
    assert done.returncode == 2 and b"cannot be used" in done.stderr
