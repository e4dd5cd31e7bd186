"""Float descriptors from the project's own extractor through the whole pipeline on the MI355X (-m gpu): sfmtoylib::SfM with
setFeatureType(FEATURES_SURF) on the four rendered 640 x 480 corner views of tests/test_gpu_sfm_pipeline.py (as B, G, R images with
three equal channels, so the gray conversion gives back the rendering).

Every run is a fresh process (tests/surf_pipeline_run.py, sfmtoy) with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0 as its only
SFMBA_* variables; a child that fails or overruns its time stops the module.

  class        the class with FEATURES_SURF and an explicit merge distance returns OKAY
  features     it equals, byte for byte in poses, cloud and K (and in every discrete result), the same class fed through setFeatures
               with the output of sfmba_surf_extract and the same merge distance
  sfmtoy       sfmtoy -f surf -m <that value> on the same images as PPM files writes the class's two PLY files
  reported     the number of registered views, the cloud size and the RMS reprojection error are printed (profiles/surf_extract.txt
               holds them beside ORB's stored figures for this scene); they are not gated"""
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
MERGE_DISTANCE = 0.25          # on the scale of unit-length descriptors (distances 0 .. 2); given explicitly, as the class asks
FAILED = []
KEYS = ("code", "added_view", "added_posed", "added_cloud", "done", "good", "view_ptr", "view_idx", "feat_idx", "poses", "xyz", "K")


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
    tmp = tmp_path_factory.mktemp("surf_pipeline")
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    bgr = np.ascontiguousarray(np.stack([gray, gray, gray], axis=3))
    src = str(tmp / "in.npz")
    np.savez(src, images=bgr, merge_distance=np.float32(MERGE_DISTANCE))
    prefix = str(tmp / "class")
    script = os.path.join(HERE, "surf_pipeline_run.py")
    child([sys.executable, script, "class", src, str(tmp / "class.npz"), prefix], "class")
    child([sys.executable, script, "features", src, str(tmp / "features.npz")], "features")
    return dict(np.load(str(tmp / "class.npz"))), dict(np.load(str(tmp / "features.npz"))), prefix, bgr, tmp


def rms_reprojection(res, kp_ptr, kp_xy):
    """RMS reprojection error in px of the final cloud in the final cameras."""
    K = res["K"].reshape(3, 3).astype(np.float64)
    pt = np.repeat(np.arange(len(res["xyz"])), np.diff(res["view_ptr"]))
    P = res["poses"].reshape(-1, 3, 4).astype(np.float64)[res["view_idx"]]
    pc = np.einsum("nij,nj->ni", P[:, :, :3], res["xyz"].astype(np.float64)[pt]) + P[:, :, 3]
    uv = pc[:, :2] / pc[:, 2:3] * np.array([K[0, 0], K[1, 1]]) + K[:2, 2]
    obs = kp_xy[kp_ptr[res["view_idx"]] + res["feat_idx"]].astype(np.float64)
    return float(np.sqrt(((uv - obs) ** 2).sum(axis=1).mean()))


def test_the_class_with_surf_features_returns_okay(runs):
    cls, feats, _, _, _ = runs
    assert int(cls["code"]) == 0 and cls["done"].all()
    print("surf_pipeline corner: key points per view %s, good %s, cloud %d, rms %.4f px (merge distance %.2f)"
          % (np.diff(feats["kp_ptr"]).tolist(), cls["good"].astype(int), len(cls["xyz"]), rms_reprojection(cls, feats["kp_ptr"], feats["kp_xy"]),
             MERGE_DISTANCE))


def test_the_class_equals_set_features_with_the_extractors_output(runs):
    cls, feats, _, _, _ = runs
    assert int(feats["code"]) == 0
    for k in KEYS:
        assert cls[k].shape == feats[k].shape and cls[k].tobytes() == feats[k].tobytes(), k


def test_sfmtoy_with_surf_writes_the_ply_files_of_the_class(runs):
    cls, _, prefix, bgr, tmp = runs
    directory = tmp / "ppm"
    directory.mkdir()
    for i, im in enumerate(bgr):
        sfm_scene.write_pnm(str(directory / ("view%02d.ppm" % i)), im[:, :, ::-1])       # a PPM file stores R, G, B
    mine = str(tmp / "sfmtoy")
    child([SFMTOY, "-d", "4", "-f", "surf", "-m", repr(MERGE_DISTANCE), "-o", mine, str(directory)], "sfmtoy")
    for suffix in ("_points.ply", "_cameras.ply"):
        a, b = open(prefix + suffix, "rb").read(), open(mine + suffix, "rb").read()
        assert len(a) > 300 and a == b, suffix
