"""SfM::cleanMesh and sfmtoy --mesh-clean through the whole pipeline on the MI355X (-m gpu), on the four rendered 640 x 480 corner
views of tests/test_gpu_sfm_pipeline.py.

Every run is a fresh process (tests/mesh_clean_pipeline_run.py, sfmtoy) with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0 as its only
SFMBA_* variables; a child that fails or overruns its time stops the module.

  clean mesh    cleanMesh equals, byte for byte, the sfmba_mesh_clean call made from Python through the C ABI with the class's mesh and
                the host rules (the top of host/SfM.h): origin = the grid's, quantum = voxel / 1024, a thousandth of the triangles
  bookkeeping   getMesh(), the dense cloud and the depth maps are unchanged by the call; without a meshDenseCloud the call refuses and
                keeps nothing
  PLY           <prefix>_mesh_clean.ply holds exactly the clean mesh, normals included
  sfmtoy        with -D --mesh 256 --mesh-clean it writes the class's file, and the other files equal those of a run without the flag;
                --mesh-clean without --mesh is a usage error
  reported      components, triangles and vertices removed, the share of boundary edges and the Euler characteristic before and after
                (profiles/mesh_clean.txt holds them); NOT gated: nobody has measured them before"""
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
SCRIPT = os.path.join(HERE, "mesh_clean_pipeline_run.py")
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
    tmp = tmp_path_factory.mktemp("mesh_clean_pipeline")
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    src = str(tmp / "in.npz")
    np.savez(src, images=gray)
    prefix = str(tmp / "class")
    child([sys.executable, SCRIPT, "class", src, str(tmp / "class.npz"), prefix], "class")
    child([sys.executable, SCRIPT, "capi", src, str(tmp / "class.npz"), str(tmp / "capi.npz")], "capi")
    return dict(np.load(str(tmp / "class.npz"))), dict(np.load(str(tmp / "capi.npz"))), prefix, gray, tmp


def test_clean_mesh_equals_the_c_abi_call(runs):
    import mesh_oracle as mo
    cls, capi = runs[0], runs[1]
    assert len(cls["mesh_tri"]) > 1000 and 1000 < len(cls["clean_tri"]) <= len(cls["mesh_tri"])
    for k in ("clean_xyz", "clean_bgr", "clean_normal", "clean_tri"):
        assert cls[k].dtype == capi[k].dtype and cls[k].shape == capi[k].shape and cls[k].tobytes() == capi[k].tobytes(), k
    n = np.linalg.norm(cls["clean_normal"].astype(np.float64), axis=1)
    assert np.allclose(n[n > 0], 1.0, atol=1e-6)
    before, after = mo.topology(cls["mesh_tri"]), mo.topology(cls["clean_tri"])
    print("mesh_clean_pipeline corner: %d components (the largest has %d triangles); %d -> %d vertices, %d -> %d triangles at the default "
          "rule (a component needs %d triangles); edges on a boundary %d of %d (%.4f) -> %d of %d (%.4f); characteristic %d -> %d"
          % (int(capi["n_components"]), int(capi["comp_triangles"].max()), len(cls["mesh_xyz"]), len(cls["clean_xyz"]), len(cls["mesh_tri"]),
             len(cls["clean_tri"]), max(1, len(cls["mesh_tri"]) // 1000), before[2], before[3], before[2] / max(before[3], 1), after[2], after[3],
             after[2] / max(after[3], 1), before[1], after[1]))


def test_the_mesh_the_dense_cloud_and_the_depth_maps_are_unchanged(runs):
    cls, _, _, gray, tmp = runs
    assert int(cls["unchanged"]) == 1
    # without a meshDenseCloud the call refuses and keeps nothing (no device involved)
    small = str(tmp / "small.npz")
    np.savez(small, images=gray[:2, :8, :8])
    child([sys.executable, SCRIPT, "refuse", small, str(tmp / "refuse.npz")], "refuse")
    assert int(np.load(str(tmp / "refuse.npz"))["code"]) == 31                              # 30 + ERROR, nothing kept


def test_the_ply_file_holds_exactly_the_clean_mesh(runs):
    cls, _, prefix = runs[:3]
    lines = open(prefix + "_mesh_clean.ply").read().split("\n")
    head = lines.index("end_header          ")
    nv, nt = len(cls["clean_xyz"]), len(cls["clean_tri"])
    assert lines[:head] == ["ply                 ", "format ascii 1.0    ", "element vertex %d" % nv, "property float x    ", "property float y    ",
                            "property float z    ", "property float nx   ", "property float ny   ", "property float nz   ", "property uchar red  ",
                            "property uchar green", "property uchar blue ", "element face %d" % nt, "property list uchar int vertex_indices"]
    rows = lines[head + 1:-1]
    assert lines[-1] == "" and len(rows) == nv + nt and all(r.endswith(" ") for r in rows[:nv])
    got = np.array([r.split() for r in rows[:nv]])
    assert np.array_equal(got[:, 6:].astype(int), cls["clean_bgr"][:, ::-1])                     # R G B
    want = np.concatenate([cls["clean_xyz"], cls["clean_normal"]], axis=1)
    assert np.array_equal(got[:, :6], np.array([["%g" % v for v in p] for p in want]))           # the stream's default: 6 significant digits
    faces = np.array([r.split() for r in rows[nv:]]).astype(int)
    assert (faces[:, 0] == 3).all() and np.array_equal(faces[:, 1:], cls["clean_tri"])


def test_sfmtoy_mesh_clean_switch(runs):
    cls, _, prefix, gray, tmp = runs
    directory = tmp / "pgm"
    directory.mkdir()
    for i, im in enumerate(gray):
        sfm_scene.write_pnm(str(directory / ("view%02d.pgm" % i)), im)
    meshed, cleaned = str(tmp / "meshed"), str(tmp / "cleaned")
    child([SFMTOY, "-d", "4", "-D", "--mesh", "256", "-o", meshed, str(directory)], "sfmtoy -D --mesh 256")
    child([SFMTOY, "-d", "4", "-D", "--mesh", "256", "--mesh-clean", "-o", cleaned, str(directory)], "sfmtoy -D --mesh 256 --mesh-clean")
    assert not os.path.exists(meshed + "_mesh_clean.ply")
    assert open(cleaned + "_mesh_clean.ply", "rb").read() == open(prefix + "_mesh_clean.ply", "rb").read()
    for suffix in ("_points.ply", "_cameras.ply", "_dense.ply", "_mesh.ply"):
        a, b = (open(p + suffix, "rb").read() for p in (meshed, cleaned))
        assert len(a) > 300 and a == b, suffix
    assert open(cleaned + "_mesh.ply", "rb").read() == open(prefix + "_mesh.ply", "rb").read()
    # --mesh-clean without --mesh, and its options without it, are usage errors: nothing runs
    for args, text in ((["-D", "--mesh-clean"], b"--mesh-clean needs --mesh"), (["-D", "--mesh", "256", "--mesh-smooth", "3"], b"need --mesh-clean"),
                       (["-D", "--mesh", "256", "--mesh-clean", "--mesh-smooth", "101"], b"cannot be used"),
                       (["-D", "--mesh", "256", "--mesh-clean", "--mesh-min-component", "-1"], b"cannot be used")):
        done = subprocess.run([SFMTOY] + args + [str(directory)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
        assert done.returncode == 2 and text in done.stderr, args
