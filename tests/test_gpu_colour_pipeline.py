"""TextureParams' levelling fields and sfmtoy --texture-level through the whole pipeline on the MI355X (-m gpu), on the four rendered
640 x 480 corner views of tests/test_gpu_sfm_pipeline.py.

Every run is a fresh process (tests/texture_pipeline_run.py, sfmtoy) with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0 as its only
SFMBA_* variables; a child that fails or overruns its time stops the module.

  the class      sfmtoy --texture-level goes through SfM::textureMesh with the levelling fields set.  Held against the
                 sfmba_mesh_texture_adjust call made from Python through the C ABI with the class's mesh and the host rules (the top of
                 host/SfM.h), at the switch's defaults (16 passes, weight 16, radius 1) and at values given on the command line together
                 with --texture-smooth: the PNG read back equals the call's atlas byte for byte; the OBJ's vt lines are the call's uv; the
                 INFO line carries the call's statistics
  the default    TextureParams' defaults make the plain call: no levelling line, and the PNG is sfmba_mesh_texture's atlas
  sfmtoy         the other output files are byte-identical with and without the option; the option without --texture, the radius without
                 the option and values out of range are usage errors
  quality        the plane under two exposures (tests/colour_cases.py) meets on the device the floor measured on the restatement"""
import os
import subprocess
import sys

import numpy as np
import pytest

import colour_cases as cc
import colour_oracle as co
import sfm_scene
import texture_pipeline_run as tpr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SFMTOY = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")
SCRIPT = os.path.join(HERE, "texture_pipeline_run.py")
CHILD_TIMEOUT = 120
FAILED = []
RUNS = (("plain", [], None), ("level", ["--texture-level"], ((0, 256, 0), (1, 16, 16))),
        ("given", ["--texture-smooth", "--texture-level=8,4", "--texture-level-radius", "2"], ((4, 256, 100), (2, 4, 8))))


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
    tmp = tmp_path_factory.mktemp("colour_pipeline")
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    src = str(tmp / "in.npz")
    np.savez(src, images=gray)
    child([sys.executable, SCRIPT, "class", src, str(tmp / "class.npz")], "class")
    directory = tmp / "pgm"
    directory.mkdir()
    for i, im in enumerate(gray):
        sfm_scene.write_pnm(str(directory / ("view%02d.pgm" % i)), im)
    out = {}
    for name, extra, _ in RUNS:
        (tmp / name).mkdir()
        prefix = str(tmp / name / "out")
        done = child([SFMTOY, "-d", "2", "-D", "--mesh", "256", "--texture"] + extra + ["-o", prefix, str(directory)], "sfmtoy " + " ".join(extra))
        out[name] = (prefix, (done.stdout + done.stderr).decode())
    return dict(np.load(str(tmp / "class.npz"))), out, gray, tmp, str(directory)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def capi_adjust(capi, cls, gray, smooth, level):
    maps = [m if has else None for m, has in zip(cls["depth"], cls["has_map"])]
    occl_tol, area, B = tpr.host_rules(cls, len(cls["mesh_tri"]))
    return capi.mesh_texture_adjust(cls["mesh_xyz"], cls["mesh_bgr"], cls["mesh_tri"], list(gray), cls["K"], cls["poses"], maps, occl_tol, area, 6, B, 4,
                                    *smooth, *level)


@pytest.mark.parametrize("name,smooth,level", [(n, p[0], p[1]) for n, _, p in RUNS if p])
def test_sfmtoy_texture_level_writes_what_the_c_abi_call_gives(runs, name, smooth, level):
    from sfm_toy_library_amd import capi
    cls, out, gray = runs[:3]
    prefix, text = out[name]
    want = capi_adjust(capi, cls, gray, smooth, level)
    infos, decoded = capi.png_decode([open(prefix + "_textured.png", "rb").read()])
    assert infos[0]["status"] == 0 and same(decoded[0], want["atlas"])
    H, W = want["atlas"].shape[:2]
    uv = want["uv"].astype(np.float64).reshape(-1, 2)
    assert [l for l in open(prefix + "_textured.obj").read().split("\n") if l.startswith("vt ")] == ["vt %.9g %.9g" % (p[0] / W, 1.0 - p[1] / H) for p in uv]
    st = want["level_stats"]
    line = [l for l in text.split("\n") if "levelled colours" in l]
    print("colour_pipeline corner, %s: %s" % (name, dict(zip(co.STATS, st.tolist()))))
    assert len(line) == 1 and ("%d nodes (%d blind), %d seam vertices; summed spread at the seams %d -> %d" % tuple(st[:5])) in line[0]
    assert ("in %d passes; largest offset %d; %d texels clamped" % (st[7], st[5], st[6])) in line[0]
    assert ("smoothed view labels" in text) == (smooth != (0, 256, 0))
    assert st[2] > 0 and st[4] < st[3]                                                      # the option does something on this scene
    off = capi_adjust(capi, cls, gray, smooth, level[:2] + (0,))
    assert same(off["view"], want["view"]) and same(off["uv"], want["uv"]) and not same(off["atlas"], want["atlas"])


def test_the_defaults_make_the_plain_call(runs):
    from sfm_toy_library_amd import capi
    cls, out, gray = runs[:3]
    maps = [m if has else None for m, has in zip(cls["depth"], cls["has_map"])]
    occl_tol, area, B = tpr.host_rules(cls, len(cls["mesh_tri"]))
    plain = capi.mesh_texture(cls["mesh_xyz"], cls["mesh_bgr"], cls["mesh_tri"], list(gray), cls["K"], cls["poses"], maps, occl_tol, area, 6, B)
    for k in ("atlas", "uv", "view"):
        assert same(cls["raw_" + k], plain[k]), k                                         # TextureParams() through the class: today's result
    assert "levelled colours" not in out["plain"][1] and "smoothed view labels" not in out["plain"][1]
    infos, decoded = capi.png_decode([open(out["plain"][0] + "_textured.png", "rb").read()])
    assert same(decoded[0], plain["atlas"])
    off = capi_adjust(capi, cls, gray, (0, 256, 0), (1, 16, 0))
    assert same(off["atlas"], plain["atlas"]) and same(off["view"], plain["view"]) and off["level_stats"][5] == off["level_stats"][6] == 0


def test_the_other_files_do_not_change(runs):
    out, tmp = runs[1], runs[3]
    for suffix in ("_points.ply", "_cameras.ply", "_dense.ply", "_mesh.ply", "_textured.mtl", "_textured.obj"):
        a, b = (open(out[n][0] + suffix, "rb").read() for n in ("plain", "level"))
        assert len(a) > 30 and a == b, suffix
    for name in ("level", "given"):
        assert sorted(os.listdir(str(tmp / name))) == sorted(os.listdir(str(tmp / "plain")))
        assert open(out[name][0] + "_textured.png", "rb").read() != open(out["plain"][0] + "_textured.png", "rb").read()


def test_usage_errors(runs):
    directory = runs[4]
    for args, text in ((["-D", "--mesh", "256", "--texture-level"], b"--texture-level needs --texture"),
                       (["-D", "--mesh", "256", "--texture", "--texture-level-radius", "1"], b"--texture-level-radius needs --texture-level"),
                       (["-D", "--mesh", "256", "--texture", "--texture-level=0"], b"cannot be used"),
                       (["-D", "--mesh", "256", "--texture", "--texture-level=1025"], b"cannot be used"),
                       (["-D", "--mesh", "256", "--texture", "--texture-level", "16,257"], b"cannot be used"),
                       (["-D", "--mesh", "256", "--texture", "--texture-level=16,0"], b"cannot be used"),
                       (["-D", "--mesh", "256", "--texture", "--texture-level=16,"], b"cannot be used"),
                       (["-D", "--mesh", "256", "--texture", "--texture-level", "--texture-level-radius", "3"], b"cannot be used")):
        done = subprocess.run([SFMTOY] + args + [directory], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
        assert done.returncode == 2 and text in done.stderr, args


def test_quality_on_the_plane_under_two_exposures():
    """The quality scene of tests/colour_cases.py through the combined call at the defaults.  CONDITION and GATE as
    tests/test_colour_oracle_cpu.py states them: the spread falls to a quarter at most, to twice the ratio measured on the restatement
    (0.024304) at most, and no texel clamps.  The statistics and the atlas equal the restatement's exactly."""
    from sfm_toy_library_amd import capi
    s, p = cc.quality_scene(), cc.QUALITY_PARAMS
    got = capi.mesh_texture_adjust(s["xyz"], s["bgr"], s["tri"], s["images"], s["K"], s["P"], s["depth_maps"], s["occl_tol"], s["min_area"], s["patch"],
                                   s["blocks_per_row"], p["k"], p["rings"], p["penalty"], p["max_passes"], p["radius"], p["weight"], p["passes"])
    st = got["level_stats"]
    print("quality scene on the device: %s; ratio %.6f" % (dict(zip(co.STATS, st.tolist())), st[4] / st[3]))
    assert 4 * st[4] <= st[3] and st[6] == 0
    assert 1000000 * st[4] <= 2 * cc.QUALITY_RATIO_MEASURED_PPM * st[3]
    want = cc.quality_want()
    assert same(st, want["level_stats"]) and same(got["atlas"], want["atlas"])
