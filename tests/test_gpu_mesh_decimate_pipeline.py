"""SfM::decimateMesh, textureMesh after it and sfmtoy --mesh-decimate through the whole pipeline on the MI355X (-m gpu), on the four
rendered 640 x 480 corner views of tests/test_gpu_sfm_pipeline.py.

Every run is a fresh process (tests/decimate_pipeline_run.py, sfmtoy) with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0 as its only
SFMBA_* variables; a child that fails or overruns its time stops the module.

  decimated     decimateMesh equals, byte for byte, the sfmba_mesh_decimate and sfmba_mesh_smooth (0 iterations) calls made from Python
                through the C ABI with the class's mesh and the host rules (the top of host/SfM.h): origin = the grid's, quantum =
                voxel / 1024, cell = round(cellVoxels * 1024); on the mesh, and on the clean mesh after a cleanMesh, which clears it
  bookkeeping   getMesh(), getCleanMesh(), the dense cloud and the depth maps are unchanged; without a meshDenseCloud the call refuses
                and keeps nothing
  texture       textureMesh after decimateMesh equals sfmba_mesh_texture on the decimated mesh; before it, on the mesh, today's bytes
  sfmtoy        with -D --mesh 256 --mesh-decimate it writes the class's file, and the other files equal those of a run without the
                flag; --mesh-decimate without --mesh is a usage error
  reported      triangles before and after, the share of triangles with a view and the atlas size before and after; NOT gated"""
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
SCRIPT = os.path.join(HERE, "decimate_pipeline_run.py")
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
    tmp = tmp_path_factory.mktemp("mesh_decimate_pipeline")
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    src = str(tmp / "in.npz")
    np.savez(src, images=gray)
    prefix = str(tmp / "class")
    child([sys.executable, SCRIPT, "class", src, str(tmp / "class.npz"), prefix], "class")
    child([sys.executable, SCRIPT, "capi", src, str(tmp / "class.npz"), str(tmp / "capi.npz")], "capi")
    return dict(np.load(str(tmp / "class.npz"))), dict(np.load(str(tmp / "capi.npz"))), prefix, gray, tmp


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_decimated_mesh_equals_the_c_abi_calls(runs):
    cls, capi = runs[0], runs[1]
    for name, source in (("decimated", "mesh"), ("decimated_clean", "clean")):
        assert len(cls[source + "_tri"]) > 1000 and 0 < len(cls[name + "_tri"]) < len(cls[source + "_tri"]), name
        for k in ("_xyz", "_bgr", "_normal", "_tri"):
            assert same(cls[name + k], capi[name + k]), name + k
        n = np.linalg.norm(cls[name + "_normal"].astype(np.float64), axis=1)
        assert np.allclose(n[n > 0], 1.0, atol=1e-6) and (n > 0).any()
        print("mesh_decimate_pipeline corner, %s: %d -> %d vertices, %d -> %d triangles at the default cell of 2 voxels; stats %s"
              % (source, len(cls[source + "_xyz"]), len(cls[name + "_xyz"]), len(cls[source + "_tri"]), len(cls[name + "_tri"]), capi[name + "_stats"].tolist()))
    assert not same(cls["decimated_xyz"], cls["decimated_clean_xyz"])


def test_the_meshes_the_dense_cloud_and_the_depth_maps_are_unchanged(runs):
    cls, _, _, gray, tmp = runs
    assert int(cls["unchanged"]) == 1
    assert not cls["mesh_normal"].any() and cls["clean_normal"].any()                         # getMesh() still has no normals; getCleanMesh() its own
    # without a meshDenseCloud the call refuses and keeps nothing (no device involved)
    small = str(tmp / "small.npz")
    np.savez(small, images=gray[:2, :8, :8])
    child([sys.executable, SCRIPT, "refuse", small, str(tmp / "refuse.npz")], "refuse")
    assert int(np.load(str(tmp / "refuse.npz"))["code"]) == 61                              # 60 + ERROR, nothing kept


def test_texture_takes_the_decimated_mesh_and_is_as_before_without_it(runs):
    cls, capi = runs[0], runs[1]
    for name in ("raw", "coarse"):
        assert int(cls[name + "_same_source"]) == 1
        for k in ("_atlas", "_uv", "_view"):
            assert same(cls[name + k], capi[name + k]), name + k
        assert int(cls[name + "_textured"]) == int(capi[name + "_textured"])
    nt0, nt1 = len(cls["mesh_tri"]), len(cls["decimated_tri"])
    print("mesh_decimate_pipeline corner, texture: triangles with a view %d of %d (%.3f) -> %d of %d (%.3f); atlas %d x %d -> %d x %d"
          % (int(cls["raw_textured"]), nt0, int(cls["raw_textured"]) / nt0, int(cls["coarse_textured"]), nt1, int(cls["coarse_textured"]) / nt1,
             cls["raw_atlas"].shape[1], cls["raw_atlas"].shape[0], cls["coarse_atlas"].shape[1], cls["coarse_atlas"].shape[0]))


def test_the_ply_file_holds_exactly_the_decimated_mesh(runs):
    cls, _, prefix = runs[:3]
    lines = open(prefix + "_mesh_decimated.ply").read().split("\n")
    head = lines.index("end_header          ")
    nv, nt = len(cls["decimated_xyz"]), len(cls["decimated_tri"])
    assert lines[:head] == ["ply                 ", "format ascii 1.0    ", "element vertex %d" % nv, "property float x    ", "property float y    ",
                            "property float z    ", "property float nx   ", "property float ny   ", "property float nz   ", "property uchar red  ",
                            "property uchar green", "property uchar blue ", "element face %d" % nt, "property list uchar int vertex_indices"]
    rows = lines[head + 1:-1]
    assert lines[-1] == "" and len(rows) == nv + nt and all(r.endswith(" ") for r in rows[:nv])
    got = np.array([r.split() for r in rows[:nv]])
    assert np.array_equal(got[:, 6:].astype(int), cls["decimated_bgr"][:, ::-1])                 # R G B
    want = np.concatenate([cls["decimated_xyz"], cls["decimated_normal"]], axis=1)
    assert np.array_equal(got[:, :6], np.array([["%g" % v for v in p] for p in want]))           # the stream's default: 6 significant digits
    faces = np.array([r.split() for r in rows[nv:]]).astype(int)
    assert (faces[:, 0] == 3).all() and np.array_equal(faces[:, 1:], cls["decimated_tri"])


def test_sfmtoy_mesh_decimate_switch(runs):
    cls, _, prefix, gray, tmp = runs
    directory = tmp / "pgm"
    directory.mkdir()
    for i, im in enumerate(gray):
        sfm_scene.write_pnm(str(directory / ("view%02d.pgm" % i)), im)
    meshed, coarse = str(tmp / "meshed"), str(tmp / "coarse")
    child([SFMTOY, "-d", "4", "-D", "--mesh", "256", "-o", meshed, str(directory)], "sfmtoy -D --mesh 256")
    child([SFMTOY, "-d", "4", "-D", "--mesh", "256", "--mesh-decimate", "-o", coarse, str(directory)], "sfmtoy -D --mesh 256 --mesh-decimate")
    assert not os.path.exists(meshed + "_mesh_decimated.ply")
    assert open(coarse + "_mesh_decimated.ply", "rb").read() == open(prefix + "_mesh_decimated.ply", "rb").read()
    for suffix in ("_points.ply", "_cameras.ply", "_dense.ply", "_mesh.ply"):
        a, b = (open(p + suffix, "rb").read() for p in (meshed, coarse))
        assert len(a) > 300 and a == b, suffix
    # --mesh-decimate without --mesh, the mean without it and a cell out of range are usage errors: nothing runs
    for args, text in ((["-D", "--mesh-decimate"], b"--mesh-decimate needs --mesh"), (["-D", "--mesh", "256", "--mesh-decimate-mean"], b"needs --mesh-decimate"),
                       (["-D", "--mesh", "256", "--mesh-decimate", "0.01"], b"cannot be used"),
                       (["-D", "--mesh", "256", "--mesh-decimate=2000"], b"cannot be used")):
        done = subprocess.run([SFMTOY] + args + [str(directory)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
        assert done.returncode == 2 and text in done.stderr, args
