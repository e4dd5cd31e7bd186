"""DenseParams::sgm and sfmtoy --sgm through the whole pipeline on the MI355X (-m gpu), on the four rendered 640 x 480 corner views of
tests/test_gpu_sfm_pipeline.py.

Every run is a fresh process (tests/sgm_pipeline_run.py, tests/depth_pipeline_run.py, sfmtoy) with SFMBA_DETERMINISTIC=1 and
SFMBA_SHIM_CACHE=0 as its only SFMBA_* variables; a child that fails or overruns its time stops the module.

  sgm set      densify's depth maps and dense cloud equal, byte for byte, sfmba_depth_sweep_sgm + sfmba_depth_fuse called from Python
               with the class's jobs and the same (non-default) parameters; meshDenseCloud runs on those maps
  sgm unset    the maps, the cloud and the three PLY files are those of the path that never heard of the switch: the driver that
               calls densify() without parameters, and sfmba_depth_sweep + sfmba_depth_fuse called directly
  sfmtoy       -D --sgm writes the class's _dense.ply; without --sgm all its files equal those of the driver without parameters
  reported     dense points with and without; not gated"""
import os
import subprocess
import sys

import numpy as np
import pytest

import sfm_scene
import sgm_pipeline_run as run

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SFMTOY = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")
CHILD_TIMEOUT = 120
FAILED = []
CLOUD = ("depth", "dense_xyz", "dense_bgr", "dense_view", "dense_pixel")


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


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sgm_pipeline")
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    src = str(tmp / "in.npz")
    np.savez(src, images=gray)
    new, old = os.path.join(HERE, "sgm_pipeline_run.py"), os.path.join(HERE, "depth_pipeline_run.py")
    child([sys.executable, old, "class", src, str(tmp / "plain.npz"), str(tmp / "plain")], "densify()")
    child([sys.executable, new, "class", "off", src, str(tmp / "off.npz"), str(tmp / "off")], "densify(sgm unset)")
    child([sys.executable, new, "class", run.sgm_text(), src, str(tmp / "on.npz"), str(tmp / "on")], "densify(sgm set)")
    child([sys.executable, new, "capi", src, str(tmp / "on.npz"), str(tmp / "capi.npz")], "capi")
    load = lambda name: dict(np.load(str(tmp / name)))
    return dict(plain=load("plain.npz"), off=load("off.npz"), on=load("on.npz"), capi=load("capi.npz"), tmp=tmp, gray=gray, src=src, script=new)


def test_densify_with_sgm_equals_the_c_abi_call(runs):
    on, capi = runs["on"], runs["capi"]
    assert int(on["code"]) == 0 and len(on["job_ref"]) == 4 and on["has_map"].all()
    for k in CLOUD:
        assert same(on[k], capi["sgm_" + k]), k
    assert not same(on["depth"], capi["depth"])                  # ... and that is another map than the plain sweep's
    print("sgm_pipeline corner: dense points %d without, %d with sgm %s; mesh triangles at resolution %d: %d without, %d with"
          % (len(runs["off"]["dense_xyz"]), len(on["dense_xyz"]), run.sgm_text(), run.MESH_RESOLUTION, int(runs["off"]["n_triangles"]),
             int(on["n_triangles"])))


def test_mesh_runs_on_the_sgm_maps(runs):
    assert int(runs["on"]["n_triangles"]) > 1000


def test_sgm_unset_is_the_path_that_never_heard_of_it(runs):
    plain, off, capi, tmp = runs["plain"], runs["off"], runs["capi"], runs["tmp"]
    for k in CLOUD + ("poses", "K", "xyz", "job_ref", "job_src", "z_near", "z_far"):
        assert same(off[k], plain[k]), k
    for k in CLOUD:
        assert same(off[k], capi[k]), k                          # sfmba_depth_sweep + sfmba_depth_fuse called directly
    for suffix in ("_points.ply", "_cameras.ply", "_dense.ply"):
        a, b = (open(str(tmp / (p + suffix)), "rb").read() for p in ("plain", "off"))
        assert len(a) > 300 and a == b, suffix
    for k in ("poses", "K", "job_ref", "job_src", "z_near", "z_far"):           # the switch changes nothing before the sweep
        assert same(runs["on"][k], plain[k]), k


def test_sfmtoy_sgm_switch(runs):
    tmp, gray = runs["tmp"], runs["gray"]
    directory = tmp / "pgm"
    directory.mkdir()
    for i, im in enumerate(gray):
        sfm_scene.write_pnm(str(directory / ("view%02d.pgm" % i)), im)
    s = run.SGM_SET
    # sfmtoy has no switch for invalid_cost: the class once more with its default
    text = "1,%d,%d,%d,127,%d" % (s["p1"], s["p2"], s["n_paths"], s["uniqueness"])
    child([sys.executable, runs["script"], "class", text, runs["src"], str(tmp / "toy.npz"), str(tmp / "toyclass")], "densify(sgm set, invalid_cost 127)")
    child([SFMTOY, "-d", "4", "-D", "-o", str(tmp / "toyplain"), str(directory)], "sfmtoy -D")
    child([SFMTOY, "-d", "4", "-D", "--sgm", "%d,%d" % (s["p1"], s["p2"]), "--sgm-paths", str(s["n_paths"]), "--sgm-uniqueness", str(s["uniqueness"]),
           "-o", str(tmp / "toysgm"), str(directory)], "sfmtoy -D --sgm")
    read = lambda name: open(str(tmp / name), "rb").read()
    assert len(read("toysgm_dense.ply")) > 300 and read("toysgm_dense.ply") == read("toyclass_dense.ply")
    assert read("toysgm_dense.ply") != read("toyplain_dense.ply")
    for suffix in ("_points.ply", "_cameras.ply", "_dense.ply"):
        assert read("toyplain" + suffix) == read("plain" + suffix), suffix
    for suffix in ("_points.ply", "_cameras.ply"):
        assert read("toysgm" + suffix) == read("plain" + suffix), suffix
