"""SfM::textureMesh and sfmtoy --texture through the whole pipeline on the MI355X (-m gpu), on the four rendered 640 x 480 corner
views of tests/test_gpu_sfm_pipeline.py.

Every run is a fresh process (tests/texture_pipeline_run.py, sfmtoy) with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0 as its only
SFMBA_* variables; a child that fails or overruns its time stops the module.

  textured mesh  textureMesh equals, byte for byte, the sfmba_mesh_texture call made from Python through the C ABI with the class's
                 mesh and the host rules (the top of host/SfM.h): occl_tol = 2 voxels, min_area = 256, a square atlas, S = 6
  which mesh     the clean mesh after cleanMesh and the raw one without
  bookkeeping    the mesh, the clean mesh, the dense cloud and the depth maps are unchanged by the calls; without a meshDenseCloud the
                 call refuses and keeps nothing
  PNG, OBJ       the PNG read back through sfmba_png_decode is the atlas; the OBJ has nv v lines, 3 nt vt lines and nt faces, and its vt
                 values reproduce uv
  sfmtoy         with -D --mesh 256 --texture it writes the class's three files, and the other files equal those of a run without the
                 flag; --texture without --mesh is a usage error
  reported       the share of textured triangles and of adjacent pairs with different views; NOT gated: nobody has measured them before"""
import os
import subprocess
import sys

import numpy as np
import pytest

import sfm_scene
import texture_oracle as to

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SFMTOY = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")
SCRIPT = os.path.join(HERE, "texture_pipeline_run.py")
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
    tmp = tmp_path_factory.mktemp("texture_pipeline")
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    src = str(tmp / "in.npz")
    np.savez(src, images=gray)
    (tmp / "class").mkdir()
    prefix = str(tmp / "class" / "out")
    child([sys.executable, SCRIPT, "class", src, str(tmp / "class.npz"), prefix], "class")
    child([sys.executable, SCRIPT, "capi", src, str(tmp / "class.npz"), str(tmp / "capi.npz")], "capi")
    return dict(np.load(str(tmp / "class.npz"))), dict(np.load(str(tmp / "capi.npz"))), prefix, gray, tmp


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_textured_mesh_equals_the_c_abi_call_on_either_mesh(runs):
    cls, capi = runs[0], runs[1]
    assert len(cls["mesh_tri"]) > 1000 and 1000 < len(cls["clean_tri"]) <= len(cls["mesh_tri"])
    assert not same(cls["mesh_xyz"], cls["clean_xyz"])                                       # two different meshes ...
    for name, mesh in (("raw", "mesh"), ("cleaned", "clean")):
        assert int(cls[name + "_same_source"]) == 1 and len(cls[name + "_view"]) == len(cls[mesh + "_tri"]), name   # ... each textured as itself
        for k in ("_atlas", "_uv", "_view"):
            assert same(cls[name + k], capi[name + k]), (name, k)
        assert int(cls[name + "_textured"]) == int(capi[name + "_textured"]) == int((cls[name + "_view"] >= 0).sum())
        H, W = cls[name + "_atlas"].shape[:2]
        assert (W, H) == to.atlas_size(len(cls[mesh + "_tri"]), 6, to.default_blocks_per_row(len(cls[mesh + "_tri"])))
        pairs, changes = to.view_changes(cls[mesh + "_tri"], cls[name + "_view"])
        print("texture_pipeline corner, %s mesh: %d triangles, %.4f textured, %d adjacent pairs, %.4f with different views, atlas %d x %d"
              % (mesh, len(cls[mesh + "_tri"]), int(cls[name + "_textured"]) / float(len(cls[mesh + "_tri"])), pairs, changes / float(max(pairs, 1)), W, H))
        assert int(cls[name + "_textured"]) > 0


def test_nothing_else_is_changed(runs):
    cls, _, _, gray, tmp = runs
    assert int(cls["unchanged"]) == 1
    # without a meshDenseCloud the call refuses and keeps nothing (no device involved)
    small = str(tmp / "small.npz")
    np.savez(small, images=gray[:2, :8, :8])
    child([sys.executable, SCRIPT, "refuse", small, str(tmp / "refuse.npz")], "refuse")
    assert int(np.load(str(tmp / "refuse.npz"))["code"]) == 51                              # 50 + ERROR, nothing kept


def test_the_png_read_back_is_the_atlas(runs):
    cls, capi = runs[0], runs[1]
    for name in ("raw", "cleaned"):
        assert same(capi[name + "_png"], cls[name + "_atlas"]), name                         # the reader gives B, G, R; the file holds R, G, B
    data = open(runs[2] + "_textured.png", "rb").read()
    H, W = cls["raw_atlas"].shape[:2]
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[16:29] == W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, 2, 0, 0, 0])
    assert data[37:41] == b"IDAT" and data[41:43] == b"\x78\x01" and data[43] in (0, 1)      # a stored block first
    stream = H * (1 + 3 * W)
    assert len(data) == 8 + 25 + 12 + (2 + 5 * -(-stream // 65535) + stream + 4) + 12         # no compression at all


def test_the_obj_holds_exactly_the_textured_mesh(runs):
    cls, _, prefix = runs[:3]
    for suffix, name, mesh in (("", "raw", "mesh"), ("_clean", "cleaned", "clean")):
        lines = open(prefix + suffix + "_textured.obj").read().split("\n")
        base = os.path.basename(prefix) + suffix
        assert lines[0] == "mtllib %s_textured.mtl" % base and lines[1] == "usemtl atlas" and lines[-1] == ""
        v = [l for l in lines if l.startswith("v ")]
        vt = [l for l in lines if l.startswith("vt ")]
        f = [l for l in lines if l.startswith("f ")]
        nv, nt = len(cls[mesh + "_xyz"]), len(cls[mesh + "_tri"])
        assert (len(v), len(vt), len(f)) == (nv, 3 * nt, nt) and len(lines) == 3 + nv + 4 * nt
        assert v == ["v %.9g %.9g %.9g" % tuple(float(c) for c in p) for p in cls[mesh + "_xyz"]]
        H, W = cls[name + "_atlas"].shape[:2]
        uv = cls[name + "_uv"].astype(np.float64).reshape(-1, 2)
        assert vt == ["vt %.9g %.9g" % (p[0] / W, 1.0 - p[1] / H) for p in uv]
        got = np.array([l.split()[1:] for l in vt], np.float64)
        assert np.allclose(got[:, 0] * W, uv[:, 0], atol=1e-4) and np.allclose((1.0 - got[:, 1]) * H, uv[:, 1], atol=1e-4)
        tri = cls[mesh + "_tri"]
        assert f == ["f %d/%d %d/%d %d/%d" % (t[0] + 1, 3 * i + 1, t[1] + 1, 3 * i + 2, t[2] + 1, 3 * i + 3) for i, t in enumerate(tri.tolist())]
        mtl = open(prefix + suffix + "_textured.mtl").read()
        assert "newmtl atlas\n" in mtl and mtl.endswith("map_Kd %s_textured.png\n" % base)


def test_sfmtoy_texture_switch(runs):
    cls, _, prefix, gray, tmp = runs
    directory = tmp / "pgm"
    directory.mkdir()
    for i, im in enumerate(gray):
        sfm_scene.write_pnm(str(directory / ("view%02d.pgm" % i)), im)
    for d in ("plain", "toy", "toyclean"):
        (tmp / d).mkdir()
    plain, toy, toyclean = (str(tmp / d / os.path.basename(prefix)) for d in ("plain", "toy", "toyclean"))
    child([SFMTOY, "-d", "4", "-D", "--mesh", "256", "-o", plain, str(directory)], "sfmtoy -D --mesh 256")
    child([SFMTOY, "-d", "4", "-D", "--mesh", "256", "--texture", "-o", toy, str(directory)], "sfmtoy -D --mesh 256 --texture")
    child([SFMTOY, "-d", "4", "-D", "--mesh", "256", "--mesh-clean", "--texture=6", "-o", toyclean + "_clean", str(directory)],
          "sfmtoy -D --mesh 256 --mesh-clean --texture=6")
    assert not any(os.path.exists(plain + "_textured" + e) for e in (".obj", ".mtl", ".png"))
    for e in (".obj", ".mtl", ".png"):
        assert open(toy + "_textured" + e, "rb").read() == open(prefix + "_textured" + e, "rb").read(), e
        assert open(toyclean + "_clean_textured" + e, "rb").read() == open(prefix + "_clean_textured" + e, "rb").read(), e
    for suffix in ("_points.ply", "_cameras.ply", "_dense.ply", "_mesh.ply"):
        a, b = (open(p + suffix, "rb").read() for p in (plain, toy))
        assert len(a) > 300 and a == b, suffix
    assert sorted(os.listdir(str(tmp / "toy"))) == sorted(os.listdir(str(tmp / "plain")) + [os.path.basename(prefix) + "_textured" + e for e in (".obj", ".mtl", ".png")])
    # --texture without --mesh, and a patch out of range, are usage errors: nothing runs
    for args, text in ((["-D", "--texture"], b"--texture needs --mesh"), (["-D", "--mesh", "256", "--texture", "2"], b"cannot be used"),
                       (["-D", "--mesh", "256", "--texture=65"], b"cannot be used")):
        done = subprocess.run([SFMTOY] + args + [str(directory)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
        assert done.returncode == 2 and text in done.stderr, args
