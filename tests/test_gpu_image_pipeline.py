"""sfmtoylib::SfM from a DIRECTORY on the MI355X (-m gpu): setImagesDirectory (PNM and JPEG files, the downscale factor applied at load
time) followed by runSfM, against the class started from the same pixels through setImages and against the restatement of its loop
(tests/sfm_loop.py) fed the pixels the device produced.  Every run is a fresh process with SFMBA_DETERMINISTIC=1 and
SFMBA_SHIM_CACHE=0 as its only SFMBA_* variables, as in tests/test_gpu_sfm_pipeline.py; a child that fails or overruns its time
stops the module.  The bar is equality byte for byte in every output.

  corner, factor 1      the four rendered 640 x 480 views written as PPM: the outputs of setImages on the same B, G, R bytes
  corner, factor 0.5    the class equals the restated loop fed the device-resized pixels
  Crazy Horse           the seven 512 x 384 photographs of tests/golden/crazyhorse_half at factor 1: runSfM ends; the class equals the
                        restated loop fed the decoded pixels; sfmtoy as a fresh child writes the same two PLY files.  How many views
                        register, the cloud size and the RMS reprojection error are printed (tools/image_io_bench.py writes them
                        to profiles/image_io.txt); nothing is asserted about them beyond the code being the same in class and
                        restatement.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import image_io_loop
import jpeg_cases as jc
import sfm_loop
import sfm_scene

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SFMTOY = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")
CHILD_TIMEOUT = 180
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
    if done.returncode < 0 or done.returncode > 2:
        FAILED.append("%s ended with %d" % (what, done.returncode))
        pytest.fail("%s ended with %d:\n%s" % (what, done.returncode, done.stderr.decode()[-2000:]))
    return done


def run_program(script, args, out):
    done = child([sys.executable, os.path.join(HERE, script)] + args + [out], script + " " + args[0])
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    return dict(np.load(out))


def assert_equal_runs(name, a, b):
    for k in KEYS:
        if k not in a or k not in b:
            continue                                                   # an ERROR of the restatement carries the code alone
        same = a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        gap = float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()) if a[k].shape == b[k].shape and a[k].size else 0.0
        print("image_pipeline %-10s %-11s byte-equal %s (largest difference %.3e)" % (name, k, same, gap))
    assert int(a["code"]) == int(b["code"]), name
    if int(a["code"]) != 0:
        return
    for k in KEYS:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)


# ---- the rendered corner views -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corner_dir(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("corner_ppm")
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    bgr = np.stack([255 - gray, gray, gray], axis=3)                    # the blue channel inverted: a B / R swap would show
    for i, im in enumerate(bgr):
        with open(tmp / ("view%02d.ppm" % i), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + im[:, :, ::-1].tobytes())
    return str(tmp), bgr


def test_corner_directory_at_factor_one_equals_set_images(corner_dir, tmp_path):
    directory, bgr = corner_dir
    from_dir = run_program("image_io_loop.py", ["class", directory, "1.0"], str(tmp_path / "dir.npz"))
    src = str(tmp_path / "in.npz")
    np.savez(src, images=bgr)
    from_images = run_program("sfm_loop.py", ["class", src], str(tmp_path / "images.npz"))
    assert int(from_dir["code"]) == 0 and from_dir["good"].sum() >= 3
    assert_equal_runs("corner x1", from_dir, from_images)


def test_corner_directory_at_one_half_equals_the_restated_loop(corner_dir, tmp_path):
    directory, bgr = corner_dir
    cls = run_program("image_io_loop.py", ["class", directory, "0.5"], str(tmp_path / "class.npz"))
    px = run_program("image_io_loop.py", ["pixels", directory, "0.5"], str(tmp_path / "pixels.npz"))
    assert bool(px["ok"]) and px["images"].shape == (4, 240, 320, 3)
    import jpeg_oracle as jo
    assert np.array_equal(px["images"][0], jo.resize(bgr[0], 0.5))
    src = str(tmp_path / "in.npz")
    np.savez(src, images=px["images"])
    loop = run_program("sfm_loop.py", ["loop", src], str(tmp_path / "loop.npz"))
    # the halved views still register (first run on an MI355X: code 0), so ERROR / ERROR, which assert_equal_runs accepts for the
    # photographs, is not accepted here: every pose, point and index below is compared
    assert int(cls["code"]) == 0 and int(loop["code"]) == 0
    assert (cls["K"][2], cls["K"][5]) == (160.0, 120.0)                # the centre comes from the RESIZED image 0 (the focal length is adjusted)
    print("image_pipeline corner x0.5: good %s, cloud %d" % (cls["good"].astype(int), len(cls["xyz"])))
    assert_equal_runs("corner x0.5", cls, loop)


# ---- the photographs ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crazyhorse(tmp_path_factory):
    """The class from the directory (writing its PLY files), the decoded pixels, the restated loop on them."""
    tmp = str(tmp_path_factory.mktemp("crazyhorse"))
    directory = os.path.join(tmp, "photos")                           # the photographs alone: the fixture directory also holds a .json
    os.makedirs(directory)
    for n in jc.photo_names():
        shutil.copy(os.path.join(jc.PHOTOS, n), directory)
    prefix = os.path.join(tmp, "class")
    cls = run_program("image_io_loop.py", ["class", "--ply", prefix, directory, "1.0"], os.path.join(tmp, "class.npz"))
    px = run_program("image_io_loop.py", ["pixels", directory, "1.0"], os.path.join(tmp, "pixels.npz"))
    src = os.path.join(tmp, "in.npz")
    np.savez(src, images=px["images"])
    loop = run_program("sfm_loop.py", ["loop", src], os.path.join(tmp, "loop.npz"))
    return directory, prefix, cls, px, loop


def test_crazyhorse_pixels_are_libjpegs(crazyhorse):
    _, _, _, px, _ = crazyhorse
    assert bool(px["ok"]) and px["images"].shape == (7, 384, 512, 3)
    hashes = jc.photo_hashes()
    for n, im in zip(jc.photo_names(), px["images"]):
        assert jc.sha256(im) == hashes[n], n


def test_crazyhorse_class_equals_the_restated_loop(crazyhorse):
    _, _, cls, px, loop = crazyhorse
    assert int(cls["code"]) in (0, 1)                                   # runSfM ended
    if int(cls["code"]) == 0:
        feats = sfm_loop.extract_features(px["images"])
        views, cloud, rms = image_io_loop.figures(cls, feats)
        print("image_pipeline crazyhorse_half: code 0, %d of 7 views registered (good %s), cloud %d points, rms %.4f px, K centre (%g, %g)"
              % (views, cls["good"].astype(int), cloud, rms, cls["K"][2], cls["K"][5]))
    else:
        print("image_pipeline crazyhorse_half: code 1 (runSfM reported ERROR)")
    assert_equal_runs("crazyhorse", cls, loop)


def test_sfmtoy_writes_the_ply_files_of_the_class(crazyhorse, tmp_path):
    directory, prefix, cls, _, _ = crazyhorse
    mine = str(tmp_path / "toy")
    done = child([SFMTOY, "-d", "4", "-s", "1", "-v", "3", "-o", mine, directory], "sfmtoy")
    assert done.returncode == (0 if int(cls["code"]) == 0 else 1), done.stderr.decode()[-2000:]
    for suffix in ("_points.ply", "_cameras.ply"):
        if int(cls["code"]) == 0:
            a, b = open(prefix + suffix, "rb").read(), open(mine + suffix, "rb").read()
            assert len(a) > 300 and a == b, suffix
        else:
            assert not os.path.exists(mine + suffix)
