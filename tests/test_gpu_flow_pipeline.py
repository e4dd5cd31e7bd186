"""Matching by optical flow through the whole pipeline on the MI355X (-m gpu): sfmtoylib::SfM with setMatcherType(MATCHER_FLOW) on the
four rendered 640 x 480 corner views of tests/test_gpu_sfm_pipeline.py, read as a short frame sequence: the cameras stand 3 degrees
apart, and the largest displacement of a surface point between consecutive views, computed from the planted geometry, stays under
20 px (it is asserted below).

Every run is a fresh process (tests/flow_pipeline_run.py, tests/sfm_loop.py, sfmtoy) with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0
as its only SFMBA_* variables; a child that fails or overruns its time stops the module.

  matrix       SfMFeatureMatching::createFlowMatchMatrix equals, byte for byte, ONE sfmba_flow_track and ONE sfmba_flow_match call with
               the class's parameters; with window 1 the entries beyond it are empty and the others are those of window 0
  class        runSfM with MATCHER_FLOW equals, byte for byte in poses, cloud and K (and in every discrete result), the restated loop
               of tests/sfm_loop.py fed that matrix
  sfmtoy       sfmtoy -M flow on the same images as PGM files writes the class's two PLY files; without -M it writes the files of the
               class with the descriptor matcher
  refusal      MATCHER_FLOW after setFeatures returns ERROR (tests/test_flow_oracle_cpu.py holds the same without a device)
  reported     the number of registered views, the cloud size and the RMS reprojection error are printed; they are not gated"""
import ctypes
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
KEYS = ("code", "added_view", "added_posed", "added_cloud", "done", "good", "view_ptr", "view_idx", "feat_idx", "poses", "xyz", "K")
MATRIX = ("sizes", "query", "train", "distance")


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


def rms_reprojection(res, kp_ptr, kp_xy):
    """RMS reprojection error in px of the final cloud in the final cameras."""
    K = res["K"].reshape(3, 3).astype(np.float64)
    pt = np.repeat(np.arange(len(res["xyz"])), np.diff(res["view_ptr"]))
    P = res["poses"].reshape(-1, 3, 4).astype(np.float64)[res["view_idx"]]
    pc = np.einsum("nij,nj->ni", P[:, :, :3], res["xyz"].astype(np.float64)[pt]) + P[:, :, 3]
    uv = pc[:, :2] / pc[:, 2:3] * np.array([K[0, 0], K[1, 1]]) + K[:2, 2]
    obs = kp_xy[kp_ptr[res["view_idx"]] + res["feat_idx"]].astype(np.float64)
    return float(np.sqrt(((uv - obs) ** 2).sum(axis=1).mean()))


@pytest.fixture(scope="module")
def scene():
    return sfm_scene.make_corner(seed=0)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, scene):
    tmp = tmp_path_factory.mktemp("flow_pipeline")
    gray = np.stack(scene["images"])
    src = str(tmp / "in.npz")
    np.savez(src, images=gray, window=np.int32(0))
    prefix = str(tmp / "class")
    script = os.path.join(HERE, "flow_pipeline_run.py")
    child([sys.executable, script, "class", src, str(tmp / "class.npz"), prefix], "class")
    child([sys.executable, script, "loop", src, str(tmp / "loop.npz")], "loop")
    return dict(np.load(str(tmp / "class.npz"))), dict(np.load(str(tmp / "loop.npz"))), prefix, gray, tmp


def test_consecutive_views_move_less_than_20_px(scene):
    """Points of the two planes (a point is a u + b v with a in 0 .. 2, |b| <= 1.2: more than the images show) seen in two consecutive views."""
    a, b = (g.reshape(-1) for g in np.meshgrid(np.linspace(0.0, 2.0, 41), np.linspace(-1.2, 1.2, 25)))
    w, h = scene["size"]
    worst = 0.0
    for _, u, v, _ in sfm_scene._plane_frames():
        X = a[:, None] * u + b[:, None] * v
        uv = [sfm_scene.project(scene["K"], R, t, X)[0] for R, t in zip(scene["R"], scene["t"])]
        inside = [(p[:, 0] >= 0) & (p[:, 0] <= w - 1) & (p[:, 1] >= 0) & (p[:, 1] <= h - 1) for p in uv]
        for k in range(len(uv) - 1):
            both = inside[k] & inside[k + 1]
            assert both.sum() > 100
            worst = max(worst, float(np.linalg.norm(uv[k + 1][both] - uv[k][both], axis=1).max()))
    print("largest consecutive displacement %.2f px" % worst)
    assert worst < 20.0


def test_the_match_matrix_equals_the_two_c_abi_calls(runs):
    _, loop, _, _, _ = runs
    for k in MATRIX:
        a, b = loop["shim_" + k], loop["capi_" + k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    sizes = loop["shim_sizes"]
    assert (sizes[np.tril_indices(len(sizes))] == 0).all()
    print("flow_pipeline corner: key points per view %s, status 1 per pair %s, matches\n%s"
          % (np.diff(loop["kp_ptr"]).tolist(), loop["tracked_ok"].tolist(), sizes))


def test_a_pair_window_leaves_the_entries_beyond_it_empty(runs):
    _, loop, _, gray, tmp = runs
    src = str(tmp / "in_w1.npz")
    np.savez(src, images=gray, window=np.int32(1))
    child([sys.executable, os.path.join(HERE, "flow_pipeline_run.py"), "matrix", src, str(tmp / "matrix_w1.npz")], "matrix with window 1")
    w1 = dict(np.load(str(tmp / "matrix_w1.npz")))
    for k in MATRIX:
        assert w1["shim_" + k].tobytes() == w1["capi_" + k].tobytes(), k
    n = len(w1["shim_sizes"])
    full, at_full, at_w1 = loop["shim_sizes"], 0, 0
    for i in range(n):
        for j in range(n):
            if j - i == 1:                                       # an entry inside the window is the entry of the full matrix
                s = int(full[i, j])
                assert w1["shim_sizes"][i, j] == s
                for k in MATRIX[1:]:
                    assert w1["shim_" + k][at_w1:at_w1 + s].tobytes() == loop["shim_" + k][at_full:at_full + s].tobytes(), (i, j, k)
                at_w1 += s
            else:
                assert w1["shim_sizes"][i, j] == 0, (i, j)
            at_full += int(full[i, j])


def test_the_class_with_the_flow_matcher_equals_the_restated_loop(runs):
    cls, loop, _, _, _ = runs
    for k in KEYS:
        assert cls[k].shape == loop[k].shape and cls[k].tobytes() == loop[k].tobytes(), k
    assert int(cls["code"]) == 0 and cls["done"].all()
    print("flow_pipeline corner: good %s, cloud %d, rms %.4f px" % (cls["good"].astype(int), len(cls["xyz"]),
                                                                   rms_reprojection(cls, loop["kp_ptr"], loop["kp_xy"])))


def test_sfmtoy_with_and_without_the_flow_matcher(runs):
    cls, _, prefix, gray, tmp = runs
    directory = tmp / "pgm"
    directory.mkdir()
    for i, im in enumerate(gray):
        sfm_scene.write_pnm(str(directory / ("view%02d.pgm" % i)), im)
    assert int(cls["code"]) == 0
    mine = str(tmp / "sfmtoy_flow")
    child([SFMTOY, "-d", "4", "-M", "flow", "-o", mine, str(directory)], "sfmtoy -M flow")
    for suffix in ("_points.ply", "_cameras.ply"):
        a, b = open(prefix + suffix, "rb").read(), open(mine + suffix, "rb").read()
        assert len(a) > 300 and a == b, suffix
    # without -M: the files of the class with the descriptor matcher, which this change leaves as it was
    src, want = str(tmp / "in_plain.npz"), str(tmp / "plain")
    np.savez(src, images=gray)
    child([sys.executable, os.path.join(HERE, "sfm_loop.py"), "class", "--ply", want, src, str(tmp / "plain.npz")], "class with descriptors")
    for args, name in ((["-d", "4"], "sfmtoy_plain"), (["-d", "4", "-M", "descriptors", "-w", "3"], "sfmtoy_named")):
        mine = str(tmp / name)
        child([SFMTOY] + args + ["-o", mine, str(directory)], name)
        for suffix in ("_points.ply", "_cameras.ply"):
            a, b = open(want + suffix, "rb").read(), open(mine + suffix, "rb").read()
            assert len(a) > 300 and a == b, (name, suffix)


def test_the_flow_matcher_after_set_features_returns_error():
    shim = ctypes.CDLL(os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so"))
    assert shim.sfmba_shim_flow_refusal(0) == 1 and shim.sfmba_shim_flow_refusal(1) == 1
