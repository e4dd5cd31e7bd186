"""sfmtoylib::SfM end to end on the MI355X (-m gpu): one call of the class (sfmba_shim_run_sfm) against the restatement of its control
flow over the per-stage drivers (tests/sfm_loop.py) and against the planted truth of the synthetic scenes of tests/sfm_scene.py.

Every run is a fresh process (tests/sfm_loop.py as a program) with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0 as its only SFMBA_*
variables, so every adjustBundle is a deterministic rebuild; a child that fails or overruns its time stops the module.

Bars:
  discrete      the order of added views, the done / good sets, the PnP verdicts, the cloud size after every view and the final cloud's
                views CSR are EQUAL between the class and the restatement.
  continuous    poses, points and K are expected byte-equal; the bar is max(10 x the largest difference between TWO runs of the
                restatement, 4 float ulps of the value), measured per run and printed -- never chosen in advance.
  truth         camera centres after a similarity alignment, relative rotation angles and the RMS reprojection error of the final cloud in
                the final cameras: each at most 2 x what the restated loop reaches on the same input (the factor covers the seed-dependence
                of which hypotheses win, nothing else).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sfm_loop
import sfm_scene

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 120
FAILED = []


def run_child(mode, pairs, ply=None):
    """tests/sfm_loop.py MODE in a fresh process over (input.npz, output.npz) pairs; the outputs as dicts."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SFMBA_")}
    env.update(SFMBA_DETERMINISTIC="1", SFMBA_SHIM_CACHE="0")
    cmd = [sys.executable, os.path.join(HERE, "sfm_loop.py"), mode] + (["--ply", ply] if ply else [])
    for a, b in pairs:
        cmd += [a, b]
    if FAILED:                                                     # nothing more is started on the device after a child went wrong
        pytest.fail("not started: an earlier child process failed (%s)" % FAILED[0])
    try:
        done = subprocess.run(cmd, env=env, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    except subprocess.TimeoutExpired:
        FAILED.append("%s overran %d s" % (mode, CHILD_TIMEOUT))
        pytest.fail("tests/sfm_loop.py %s overran its %d s" % (mode, CHILD_TIMEOUT))
    if done.returncode != 0:
        FAILED.append("%s ended with %d" % (mode, done.returncode))
        pytest.fail("tests/sfm_loop.py %s ended with %d:\n%s" % (mode, done.returncode, done.stderr.decode()[-2000:]))
    return [dict(np.load(b)) for _, b in pairs]


def save_input(path, inp):
    np.savez(path, **inp)
    return path


def three_runs(tmp, name, inp, ply=None):
    """(the class, the restatement, the restatement again) on one input; the class writes its PLY files to `ply` if given."""
    src = save_input(os.path.join(tmp, name + "_in.npz"), inp)
    cls = run_child("class", [(src, os.path.join(tmp, name + "_class.npz"))], ply=ply)[0]
    a = run_child("loop", [(src, os.path.join(tmp, name + "_loop_a.npz"))])[0]
    b = run_child("loop", [(src, os.path.join(tmp, name + "_loop_b.npz"))])[0]
    return cls, a, b


DISCRETE = ("code", "added_view", "added_posed", "added_cloud", "done", "good", "view_ptr", "view_idx", "feat_idx")
CONTINUOUS = ("poses", "xyz", "K")


def check_against_restatement(name, cls, a, b):
    for k in DISCRETE:
        assert np.array_equal(a[k], b[k]), ("the restatement differs from itself", name, k)
        assert np.array_equal(cls[k], a[k]), (name, k, cls[k], a[k])
    for k in CONTINUOUS:
        x, y, z = (r[k].astype(np.float64) for r in (cls, a, b))
        noise = float(np.abs(y - z).max()) if y.size else 0.0
        bar = np.maximum(10.0 * noise, 4.0 * np.spacing(np.abs(a[k]).astype(np.float32)).astype(np.float64))
        gap = np.abs(x - y)
        print("sfm_pipeline %-6s %-5s restatement run-to-run %.3e  class vs restatement %.3e  (largest bar %.3e, byte-equal %s)"
              % (name, k, noise, float(gap.max()) if gap.size else 0.0, float(bar.max()) if bar.size else 0.0, cls[k].tobytes() == a[k].tobytes()))
        assert np.all(gap <= bar), (name, k, float(gap.max()))


def centres_and_rotations(poses):
    P = poses.reshape(-1, 3, 4).astype(np.float64)
    return np.array([-p[:, :3].T @ p[:, 3] for p in P]), P[:, :, :3]


def truth_figures(res, scene, kp_ptr, kp_xy):
    """(largest camera-centre distance after a similarity alignment, largest relative-rotation angle in degrees, RMS reprojection px)
    over the good views."""
    good = np.flatnonzero(res["good"])
    C_est, R_est = centres_and_rotations(res["poses"])
    s, R, t = sfm_scene.align_similarity(C_est[good], scene["centres"][good])
    centre = float(np.linalg.norm((s * C_est[good] @ R.T + t) - scene["centres"][good], axis=1).max())
    g0 = good[0]
    angle = max(sfm_scene.rotation_angle_deg(R_est[g] @ R_est[g0].T, scene["R"][g] @ scene["R"][g0].T) for g in good)
    K = res["K"].reshape(3, 3).astype(np.float64)
    pt = np.repeat(np.arange(len(res["xyz"])), np.diff(res["view_ptr"]))
    P = res["poses"].reshape(-1, 3, 4).astype(np.float64)[res["view_idx"]]
    X = res["xyz"].astype(np.float64)[pt]
    pc = np.einsum("nij,nj->ni", P[:, :, :3], X) + P[:, :, 3]
    uv = pc[:, :2] / pc[:, 2:3] * np.array([K[0, 0], K[1, 1]]) + K[:2, 2]
    obs = kp_xy[kp_ptr[res["view_idx"]] + res["feat_idx"]].astype(np.float64)
    rms = float(np.sqrt(((uv - obs) ** 2).sum(axis=1).mean()))
    return centre, angle, rms


# ---- "box": from features -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("box"))
    scene = sfm_scene.make_box(seed=0)
    inp = sfm_loop.features_input(scene["views"], *scene["size"])
    return scene, inp, three_runs(tmp, "box", inp)


def test_box_class_equals_the_restated_loop(box):
    _, _, (cls, a, b) = box
    assert cls["code"] == 0 and a["code"] == 0
    check_against_restatement("box", cls, a, b)


def test_box_against_the_planted_truth(box):
    scene, inp, (cls, a, _) = box
    n = len(scene["views"])
    seen = np.zeros(len(scene["X"]), int)
    for v in scene["views"]:
        seen[v["track"][v["track"] >= 0]] += 1
    for name, res in (("restatement", a), ("class", cls)):
        assert res["good"].all() and res["done"].all() and len(res["good"]) == n, (name, res["good"])           # a condition
        assert len(res["xyz"]) >= 0.5 * (seen >= 2).sum(), (name, len(res["xyz"]), int((seen >= 2).sum()))        # a condition
    want = truth_figures(a, scene, inp["kp_ptr"], inp["kp_xy"])
    got = truth_figures(cls, scene, inp["kp_ptr"], inp["kp_xy"])
    print("sfm_pipeline box truth: cloud %d of %d points seen twice; centres %.4e (restatement %.4e) units, rotations %.4e (%.4e) deg, rms %.4f (%.4f) px"
          % (len(cls["xyz"]), int((seen >= 2).sum()), got[0], want[0], got[1], want[1], got[2], want[2]))
    for g, w in zip(got, want):
        assert g <= 2.0 * w


# ---- "corner": from pixels ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corner(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("corner"))
    scene = sfm_scene.make_corner(seed=0)
    inp = dict(images=np.stack(scene["images"]))
    prefix = os.path.join(tmp, "corner")
    return scene, inp, three_runs(tmp, "corner", inp, ply=prefix), prefix


def test_corner_from_pixels_equals_the_restated_loop(corner):
    scene, inp, (cls, a, b), _ = corner
    assert cls["code"] == 0 and a["code"] == 0
    check_against_restatement("corner", cls, a, b)
    assert cls["good"].sum() >= 3
    feats = sfm_loop.extract_features(inp["images"])
    want = truth_figures(a, scene, feats["kp_ptr"], feats["kp_xy"])[2]
    got = truth_figures(cls, scene, feats["kp_ptr"], feats["kp_xy"])[2]
    print("sfm_pipeline corner: good %s, cloud %d, rms %.4f (restatement %.4f) px" % (cls["good"].astype(int), len(cls["xyz"]), got, want))
    assert got <= 2.0 * want


# ---- edges ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    """Five runs of the class in ONE fresh process: two images (which also writes its PLY files), zero images, one image, a view of
    clutter, downscale 0.5."""
    tmp = str(tmp_path_factory.mktemp("edges"))
    scene = sfm_scene.make_box(seed=0)
    cols, rows = scene["size"]
    inputs = {
        "two": sfm_loop.features_input(scene["views"][:2], cols, rows),
        "zero": sfm_loop.features_input([], cols, rows),
        "one": sfm_loop.features_input(scene["views"][:1], cols, rows),
        "clutter": sfm_loop.features_input(sfm_scene.clutter_view(scene, 3)["views"], cols, rows),
        "half": dict(sfm_loop.features_input(scene["views"][:2], cols, rows), downscale=0.5),
    }
    pairs = [(save_input(os.path.join(tmp, k + "_in.npz"), v), os.path.join(tmp, k + "_out.npz")) for k, v in inputs.items()]
    prefix = os.path.join(tmp, "two")
    outs = run_child("class", pairs, ply=prefix)
    return scene, inputs, dict(zip(inputs, outs)), prefix


def test_no_image_and_one_image_are_errors(edges):
    _, _, out, _ = edges
    assert out["zero"]["code"] == 1 and out["one"]["code"] == 1


def test_downscale_is_refused(edges):
    _, _, out, _ = edges
    assert out["half"]["code"] == 1 and out["two"]["code"] == 0


def test_two_images_end_after_the_baseline(edges):
    _, _, out, _ = edges
    r = out["two"]
    assert r["code"] == 0 and r["good"].all() and r["done"].all() and len(r["added_view"]) == 0 and len(r["xyz"]) > 100
    assert np.array_equal(np.unique(r["view_idx"]), [0, 1]) and np.all(np.diff(r["view_ptr"]) == 2)


def test_a_view_of_clutter_ends_done_and_not_good(edges):
    _, _, out, _ = edges
    r = out["clutter"]
    assert r["code"] == 0 and r["done"].all()
    assert np.array_equal(r["good"], [True, True, True, False, True, True])
    assert 3 in r["added_view"] and not r["added_posed"][list(r["added_view"]).index(3)]
    assert 3 not in r["view_idx"] and len(r["xyz"]) > 100


def exporter_ply_equals(prefix, tmp_path, res, kp_ptr, kp_xy, bgr):
    """<prefix>_points.ply / _cameras.ply against what SfMExport (sfmba_shim_save_ply) writes for the containers of `res`, the key
    points and the B, G, R images bgr [v, h, w, 3].  Two rows of gray 128 go behind every image: the exporter rounds a feature to the
    nearest pixel without a bounds check, and a feature on the last row must not read past the buffer."""
    lib = C.CDLL(sfm_loop.SHIM)
    lp, ip, fp, bp = sfm_loop.lp, sfm_loop.ip, sfm_loop.fp, sfm_loop.bp
    n, h, w = bgr.shape[:3]
    assert n == len(res["poses"])
    padded = np.full((n, h + 2, w, 3), 128, np.uint8)
    padded[:, :h] = bgr
    mine = str(tmp_path / "export")
    arrs = [np.ascontiguousarray(x) for x in (res["poses"], res["xyz"], res["view_ptr"], res["view_idx"], res["feat_idx"], kp_ptr, kp_xy)]
    rc = lib.sfmba_shim_save_ply(mine.encode(), C.c_int(n), arrs[0].ctypes.data_as(fp), C.c_int(len(res["xyz"])), arrs[1].ctypes.data_as(fp),
                                 arrs[2].ctypes.data_as(lp), arrs[3].ctypes.data_as(ip), arrs[4].ctypes.data_as(ip), arrs[5].ctypes.data_as(lp),
                                 arrs[6].ctypes.data_as(fp), C.c_int(h + 2), C.c_int(w), padded.ctypes.data_as(bp))
    assert rc == 0
    for suffix in ("_points.ply", "_cameras.ply"):
        a, b = open(prefix + suffix, "rb").read(), open(mine + suffix, "rb").read()
        assert len(a) > 300 and a == b, suffix
    return open(prefix + "_points.ply", "rb").read()


def vertex_colours(points_ply):
    rows = points_ply.split(b"end_header")[1].split(b"\n")[1:]
    return np.array([[int(x) for x in r.split()[3:6]] for r in rows if r.strip()])


def test_ply_files_after_setFeatures_are_the_exporters_in_gray_128(edges, tmp_path):
    scene, inputs, out, prefix = edges
    r, inp = out["two"], inputs["two"]
    cols, rows = scene["size"]
    ply = exporter_ply_equals(prefix, tmp_path, r, inp["kp_ptr"], inp["kp_xy"], np.full((len(r["poses"]), rows, cols, 3), 128, np.uint8))
    assert np.all(vertex_colours(ply) == 128)


def test_ply_files_of_gray_images_carry_the_pixel_in_all_three_channels(corner, tmp_path):
    _, inp, (cls, _, _), prefix = corner
    feats = sfm_loop.extract_features(inp["images"])
    ply = exporter_ply_equals(prefix, tmp_path, cls, feats["kp_ptr"], feats["kp_xy"], np.repeat(inp["images"][..., None], 3, axis=3))
    rgb = vertex_colours(ply)
    assert len(rgb) == len(cls["xyz"]) and np.all(rgb[:, 0] == rgb[:, 1]) and np.all(rgb[:, 1] == rgb[:, 2]) and len(np.unique(rgb[:, 0])) > 20


def test_ply_files_of_colour_images_carry_b_g_r_as_the_exporter_reads_them(corner, tmp_path_factory, tmp_path):
    """The corner views once more as colour images whose blue channel is inverted (a B / R swap or a gray conversion would show): one
    run of the class in a fresh process, its PLY files against the exporter on the same B, G, R bytes."""
    _, inp, _, _ = corner
    img = inp["images"]
    bgr = np.stack([255 - img, img, img], axis=3)
    tmp = str(tmp_path_factory.mktemp("colour"))
    prefix = os.path.join(tmp, "colour")
    src = save_input(os.path.join(tmp, "in.npz"), dict(images=bgr))
    res = run_child("class", [(src, os.path.join(tmp, "out.npz"))], ply=prefix)[0]
    assert res["code"] == 0 and res["good"].sum() >= 3 and len(res["xyz"]) > 100
    feats = sfm_loop.extract_features(bgr)
    ply = exporter_ply_equals(prefix, tmp_path, res, feats["kp_ptr"], feats["kp_xy"], bgr)
    rgb = vertex_colours(ply)                                       # written red, green, blue
    assert np.all(rgb[:, 0] == rgb[:, 1]) and np.all(rgb[:, 2] == 255 - rgb[:, 0]) and len(np.unique(rgb[:, 0])) > 20
