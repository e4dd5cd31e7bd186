"""TextureParams' smoothing fields and sfmtoy --texture-smooth through the whole pipeline on the MI355X (-m gpu), on the four rendered
640 x 480 corner views of tests/test_gpu_sfm_pipeline.py.

Every run is a fresh process (tests/texture_pipeline_run.py, sfmtoy) with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0 as its only
SFMBA_* variables; a child that fails or overruns its time stops the module.

  the class      sfmtoy --texture-smooth goes through SfM::textureMesh with the smoothing fields set.  Held against the
                 sfmba_mesh_texture_smooth call made from Python through the C ABI with the class's mesh and the host rules (the top of
                 host/SfM.h), at the switch's defaults (4, 256, 100 passes) and at values given on the command line: the PNG read back
                 equals the call's atlas byte for byte; the OBJ's vt lines are the call's uv printed as the class prints them; the INFO
                 line carries the call's seam counts, moves and passes.  TexturedMesh::view and the other statistics are NOT read back
                 here (sfmtoy writes neither): the labels are held through the atlas they produce
  the default    TextureParams' defaults make the plain call: the class's textured mesh equals sfmba_mesh_texture_smooth with rings 0 and
                 passes 0 and sfmba_mesh_texture alike
  sfmtoy         the other output files are byte-identical with and without the option; the option without --texture, the passes without
                 the option and values out of range are usage errors
  reported       the corner scene's eight statistics at the default area floor and at min_area 0"""
import os
import subprocess
import sys

import numpy as np
import pytest

import sfm_scene
import texture_pipeline_run as tpr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SFMTOY = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")
SCRIPT = os.path.join(HERE, "texture_pipeline_run.py")
CHILD_TIMEOUT = 120
FAILED = []
STATS = ("energy_start", "energy_end", "diff_rank0", "diff_start", "diff_end", "frontier", "moves", "n_passes")


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
    tmp = tmp_path_factory.mktemp("label_pipeline")
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    src = str(tmp / "in.npz")
    np.savez(src, images=gray)
    child([sys.executable, SCRIPT, "class", src, str(tmp / "class.npz")], "class")
    directory = tmp / "pgm"
    directory.mkdir()
    for i, im in enumerate(gray):
        sfm_scene.write_pnm(str(directory / ("view%02d.pgm" % i)), im)
    out = {}
    for name, extra in (("plain", []), ("smooth", ["--texture-smooth"]), ("given", ["--texture-smooth=2,1000", "--texture-smooth-passes", "3"])):
        (tmp / name).mkdir()
        prefix = str(tmp / name / "out")
        done = child([SFMTOY, "-d", "2", "-D", "--mesh", "256", "--texture"] + extra + ["-o", prefix, str(directory)], "sfmtoy " + " ".join(extra))
        out[name] = (prefix, (done.stdout + done.stderr).decode())
    return dict(np.load(str(tmp / "class.npz"))), out, gray, tmp, str(directory)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def capi_smooth(capi, cls, gray, rings, penalty, passes, min_area=None):
    maps = [m if has else None for m, has in zip(cls["depth"], cls["has_map"])]
    occl_tol, area, B = tpr.host_rules(cls, len(cls["mesh_tri"]))
    return capi.mesh_texture_smooth(cls["mesh_xyz"], cls["mesh_bgr"], cls["mesh_tri"], list(gray), cls["K"], cls["poses"], maps, occl_tol,
                                    area if min_area is None else min_area, 6, B, 4, rings, penalty, passes)


def obj_vt(path):
    return [l for l in open(path).read().split("\n") if l.startswith("vt ")]


@pytest.mark.parametrize("name,params", [("smooth", (4, 256, 100)), ("given", (2, 1000, 3))])
def test_sfmtoy_texture_smooth_writes_what_the_c_abi_call_gives(runs, name, params):
    from sfm_toy_library_amd import capi
    cls, out, gray = runs[:3]
    prefix, text = out[name]
    want = capi_smooth(capi, cls, gray, *params)
    infos, decoded = capi.png_decode([open(prefix + "_textured.png", "rb").read()])
    assert infos[0]["status"] == 0 and same(decoded[0], want["atlas"])
    H, W = want["atlas"].shape[:2]
    uv = want["uv"].astype(np.float64).reshape(-1, 2)
    assert obj_vt(prefix + "_textured.obj") == ["vt %.9g %.9g" % (p[0] / W, 1.0 - p[1] / H) for p in uv]
    st = want["stats"]
    line = [l for l in text.split("\n") if "smoothed view labels" in l]
    print("label_pipeline corner, %s: %s" % (name, dict(zip(STATS, st.tolist()))))
    assert len(line) == 1 and ("%d plain, %d after the diffusion, %d at the end" % (st[2], st[3], st[4])) in line[0]
    assert ("%d moves in %d passes" % (st[6], st[7])) in line[0]
    plain = capi_smooth(capi, cls, gray, 0, 256, 0)
    assert not same(want["view"], plain["view"]) and (name != "smooth" or st[4] < st[2])     # the option does something on this scene


def test_the_defaults_make_the_plain_call(runs):
    from sfm_toy_library_amd import capi
    cls, out, gray = runs[:3]
    maps = [m if has else None for m, has in zip(cls["depth"], cls["has_map"])]
    occl_tol, area, B = tpr.host_rules(cls, len(cls["mesh_tri"]))
    plain = capi.mesh_texture(cls["mesh_xyz"], cls["mesh_bgr"], cls["mesh_tri"], list(gray), cls["K"], cls["poses"], maps, occl_tol, area, 6, B)
    off = capi_smooth(capi, cls, gray, 0, 256, 0)
    for k in ("atlas", "uv", "view"):
        assert same(cls["raw_" + k], plain[k]) and same(off[k], plain[k]), k
    assert "smoothed view labels" not in out["plain"][1]
    infos, decoded = capi.png_decode([open(out["plain"][0] + "_textured.png", "rb").read()])
    assert same(decoded[0], plain["atlas"])


def test_the_other_files_do_not_change(runs):
    out, tmp = runs[1], runs[3]
    for name in ("smooth", "given"):
        for suffix in ("_points.ply", "_cameras.ply", "_dense.ply", "_mesh.ply", "_textured.mtl"):
            a, b = (open(out[n][0] + suffix, "rb").read() for n in ("plain", name))
            assert len(a) > 30 and a == b, (name, suffix)
        assert sorted(os.listdir(str(tmp / name))) == sorted(os.listdir(str(tmp / "plain")))
        assert open(out[name][0] + "_textured.png", "rb").read() != open(out["plain"][0] + "_textured.png", "rb").read()


def test_usage_errors(runs):
    directory = runs[4]
    for args, text in ((["-D", "--mesh", "256", "--texture-smooth"], b"--texture-smooth needs --texture"),
                       (["-D", "--mesh", "256", "--texture", "--texture-smooth-passes", "5"], b"--texture-smooth-passes needs --texture-smooth"),
                       (["-D", "--mesh", "256", "--texture", "--texture-smooth=9,256"], b"cannot be used"),
                       (["-D", "--mesh", "256", "--texture", "--texture-smooth", "4,65536"], b"cannot be used"),
                       (["-D", "--mesh", "256", "--texture", "--texture-smooth=4"], b"cannot be used"),
                       (["-D", "--mesh", "256", "--texture", "--texture-smooth", "--texture-smooth-passes", "10001"], b"cannot be used")):
        done = subprocess.run([SFMTOY] + args + [directory], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
        assert done.returncode == 2 and text in done.stderr, args


def test_the_corner_scene_statistics(runs):
    """Reported, not gated: how far the share of adjacent pairs with different views falls on the corner mesh."""
    from sfm_toy_library_amd import capi
    cls, _, gray = runs[:3]
    for min_area in (0, None):
        st = capi_smooth(capi, cls, gray, 4, 256, 100, min_area)["stats"]
        pairs = capi.mesh_adjacency(cls["mesh_tri"])["n_pairs"]
        print("label_pipeline corner, min_area %s: %d pairs; different views %.4f plain, %.4f after the diffusion, %.4f at the end; frontier %.4f; %s"
              % ("0" if min_area == 0 else "default", pairs, st[2] / pairs, st[3] / pairs, st[4] / pairs, st[5] / pairs, dict(zip(STATS, st.tolist()))))
        assert st[1] <= st[0]
