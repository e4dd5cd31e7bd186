"""SfM::meshDenseCloud with MeshParams::fillIterations and sfmtoy --mesh-fill through the whole pipeline on the MI355X (-m gpu), on the
four rendered 640 x 480 corner views of tests/test_gpu_mesh_pipeline.py, at resolution 64.

Every run is a fresh process (tests/tsdf_fill_pipeline_run.py, sfmtoy) with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0 as its only
SFMBA_* variables; a child that fails or overruns its time stops the module.

  filled mesh   meshDenseCloud with fillIterations = 3 equals, byte for byte, the sfmba_tsdf_mesh_fill call made from Python through the
                C ABI with the class's images, poses, depth maps and grid; filled.size() == vertices.size() and equals vfilled
  off           with fillIterations = 0 the mesh equals the sfmba_tsdf_mesh call byte for byte and filled is empty
  bookkeeping   the depth maps, the dense cloud and the grid rule are unchanged; cleanMesh afterwards returns OKAY; without a densify
                the call refuses
  sfmtoy        -D --mesh 64 --mesh-fill 3 writes the class's <prefix>_mesh.ply and leaves every other file byte-identical to the run
                without the flag; --mesh-fill without --mesh is a usage error
  reported      the share of boundary edges before and after; NOT gated"""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_oracle as mo
import sfm_scene

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SFMTOY = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")
SCRIPT = os.path.join(HERE, "tsdf_fill_pipeline_run.py")
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
    tmp = tmp_path_factory.mktemp("tsdf_fill_pipeline")
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    src = str(tmp / "in.npz")
    np.savez(src, images=gray, resolution=64, fill_iterations=3, fill_min_neighbours=2)
    prefix = str(tmp / "class")
    child([sys.executable, SCRIPT, "class", src, str(tmp / "class.npz"), prefix], "class")
    child([sys.executable, SCRIPT, "capi", src, str(tmp / "class.npz"), str(tmp / "capi.npz")], "capi")
    return dict(np.load(str(tmp / "class.npz"))), dict(np.load(str(tmp / "capi.npz"))), prefix, gray, tmp


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_filled_mesh_equals_the_c_abi_call(runs):
    cls, capi = runs[0], runs[1]
    assert len(cls["mesh_xyz"]) > 1000 and len(cls["mesh_tri"]) > 1000
    for k in ("mesh_xyz", "mesh_bgr", "mesh_tri", "mesh_filled"):
        assert same_bits(cls[k], capi[k]), k
    assert int(cls["filled_size"]) == len(cls["mesh_xyz"]) and cls["mesh_filled"].any() and set(np.unique(cls["mesh_filled"]).tolist()) <= {0, 1}
    assert len(cls["mesh_tri"]) > len(cls["mesh0_tri"])
    share = []
    for tri in (cls["mesh0_tri"], cls["mesh_tri"]):
        closed, euler, boundary, n_edges = mo.topology(tri)
        share.append(boundary / max(n_edges, 1))
    filled_tri = int(cls["mesh_filled"][cls["mesh_tri"]].any(axis=1).sum())
    print("tsdf_fill_pipeline corner: grid %s, 3 passes, k 2: %d -> %d vertices (%d made by the fill), %d -> %d triangles (%d with a filled vertex), "
          "boundary-edge share %.4f -> %.4f"
          % (cls["dims"].tolist(), len(cls["mesh0_xyz"]), len(cls["mesh_xyz"]), int(cls["mesh_filled"].sum()), len(cls["mesh0_tri"]),
             len(cls["mesh_tri"]), filled_tri, share[0], share[1]))


def test_without_the_fill_the_mesh_is_the_one_of_sfmba_tsdf_mesh(runs):
    cls, capi = runs[0], runs[1]
    assert len(cls["mesh0_tri"]) > 1000 and int(cls["filled0_size"]) == 0
    for k in ("mesh0_xyz", "mesh0_bgr", "mesh0_tri"):
        assert same_bits(cls[k], capi[k]), k


def test_the_bookkeeping_is_unchanged_and_the_clean_up_runs(runs):
    cls, _, _, gray, tmp = runs
    assert int(cls["unchanged"]) == 1 and cls["has_map"].sum() == 4 and len(cls["dense_xyz"]) > 100000
    for k in ("origin", "voxel", "trunc", "dims"):                                          # the grid rule does not know about the fill
        assert same_bits(np.asarray(cls[k]), np.asarray(cls[k + "0"])), k
    assert max(cls["dims"].tolist()) in (74, 75)                                            # 63 voxels, 5 of padding at either end, + 2
    assert int(cls["clean_code"]) == 0                                                      # OKAY
    # without a densify the call with the fill refuses and keeps nothing, as the one without it does (no device involved)
    small = str(tmp / "small.npz")
    np.savez(small, images=gray[:2, :8, :8], fill_iterations=3, fill_min_neighbours=2)
    child([sys.executable, SCRIPT, "refuse", small, str(tmp / "refuse.npz")], "refuse")
    assert int(np.load(str(tmp / "refuse.npz"))["code"]) == 41                              # 40 + ERROR, nothing kept


def test_sfmtoy_mesh_fill_switch(runs):
    cls, _, prefix, gray, tmp = runs
    directory = tmp / "pgm"
    directory.mkdir()
    for i, im in enumerate(gray):
        sfm_scene.write_pnm(str(directory / ("view%02d.pgm" % i)), im)
    plain, filled = str(tmp / "plain"), str(tmp / "filled")
    child([SFMTOY, "-d", "4", "-D", "--mesh", "64", "-o", plain, str(directory)], "sfmtoy -D --mesh 64")
    child([SFMTOY, "-d", "4", "-D", "--mesh", "64", "--mesh-fill", "3", "-o", filled, str(directory)], "sfmtoy -D --mesh 64 --mesh-fill 3")
    assert open(filled + "_mesh.ply", "rb").read() == open(prefix + "_mesh.ply", "rb").read()
    assert open(filled + "_mesh.ply", "rb").read() != open(plain + "_mesh.ply", "rb").read()
    for suffix in ("_points.ply", "_cameras.ply", "_dense.ply"):
        a, b = (open(p + suffix, "rb").read() for p in (plain, filled))
        assert len(a) > 300 and a == b, suffix
    assert sorted(os.path.basename(p) for p in os.listdir(str(tmp)) if os.path.basename(p).startswith("filled")) == \
        ["filled_cameras.ply", "filled_dense.ply", "filled_mesh.ply", "filled_points.ply"]
    # the flags are valid only with --mesh, as the other mesh flags are: nothing runs
    for args, text in ((["-D", "--mesh-fill", "3"], b"--mesh-fill needs --mesh"), (["-D", "--mesh", "64", "--mesh-fill-neighbours", "2"], b"--mesh-fill-neighbours needs --mesh-fill"),
                       (["-D", "--mesh", "64", "--mesh-fill", "255"], b"cannot be used"), (["-D", "--mesh", "64", "--mesh-fill", "3", "--mesh-fill-neighbours", "0"], b"cannot be used")):
        done = subprocess.run([SFMTOY] + args + [str(directory)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
        assert done.returncode == 2 and text in done.stderr, args
