"""SfM::mergeDenseCloud and sfmtoy --voxel through the whole pipeline on the MI355X (-m gpu), on the four rendered 640 x 480 corner
views of tests/test_gpu_sfm_pipeline.py.

Every run is a fresh process (tests/cloud_pipeline_run.py, sfmtoy) with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0 as its only
SFMBA_* variables; a child that fails or overruns its time stops the module.

  merged cloud  mergeDenseCloud equals, byte for byte, computeNormals + the gather + sfmba_cloud_merge made from Python through the
                C ABI with the class's depth maps, dense cloud and voxel
  auto voxel    the voxel the class chose equals the restatement of its rule, fed the class's own job ranges and K
  bookkeeping   sum(count) + n_skipped == dense points; getDenseCloud() is unchanged by the call
  PLY           <prefix>_dense_merged.ply holds exactly the merged cloud
  sfmtoy        with -D --voxel 0 it writes the class's merged file, and the other three files equal those of a run without --voxel
  reported      the de-duplication ratio at the auto voxel and the share of merged points with a non-zero normal
                (profiles/cloud_merge.txt holds them); NOT gated: nobody has measured them before"""
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
    tmp = tmp_path_factory.mktemp("cloud_pipeline")
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    src = str(tmp / "in.npz")
    np.savez(src, images=gray)
    prefix = str(tmp / "class")
    script = os.path.join(HERE, "cloud_pipeline_run.py")
    child([sys.executable, script, "class", src, str(tmp / "class.npz"), prefix], "class")
    child([sys.executable, script, "capi", src, str(tmp / "class.npz"), str(tmp / "capi.npz")], "capi")
    return dict(np.load(str(tmp / "class.npz"))), dict(np.load(str(tmp / "capi.npz"))), prefix, gray, tmp


def test_merge_equals_the_two_c_abi_calls(runs):
    cls, capi = runs[0], runs[1]
    assert len(cls["merged_xyz"]) > 1000
    for k in ("merged_xyz", "merged_bgr", "merged_normal", "merged_count", "merged_first"):
        assert cls[k].dtype == capi[k].dtype and cls[k].shape == capi[k].shape and cls[k].tobytes() == capi[k].tobytes(), k
    assert int(cls["n_skipped"]) == int(capi["n_skipped"])
    has_normal = (cls["merged_normal"] != 0).any(axis=1)
    print("cloud_pipeline corner: %d dense points -> %d merged at the auto voxel %.6g (ratio %.3f; counts 1 / 2 / 3 / 4+: %s), "
          "merged points with a non-zero normal %.4f, depth pixels with a normal %.4f"
          % (len(cls["dense_xyz"]), len(cls["merged_xyz"]), float(cls["voxel_used"]), len(cls["dense_xyz"]) / len(cls["merged_xyz"]),
             np.bincount(np.minimum(cls["merged_count"], 4), minlength=5)[1:].tolist(), has_normal.mean(), float(capi["normals_with_a_value"])))


def test_auto_voxel_equals_its_restatement(runs):
    cls = runs[0]
    g = sorted(float(np.sqrt(np.float64(zn) * np.float64(zf))) for zn, zf in zip(cls["z_near"], cls["z_far"]))
    assert len(g) == 4
    want = np.float32(g[len(g) // 2] / float(cls["K"][0]))
    assert np.float32(cls["voxel_used"]).tobytes() == want.tobytes() and want > 0


def test_counts_add_up_and_the_dense_cloud_is_unchanged(runs):
    cls = runs[0]
    assert int(cls["merged_count"].sum()) + int(cls["n_skipped"]) == len(cls["dense_xyz"])
    assert int(cls["dense_unchanged"]) == 1
    assert len(set(cls["merged_first"].tolist())) == len(cls["merged_first"])
    assert cls["merged_first"].min() >= 0 and cls["merged_first"].max() < len(cls["dense_xyz"])


def ply_rows(path, properties):
    lines = open(path).read().split("\n")
    head = lines.index("end_header          ")
    assert lines[:2] == ["ply                 ", "format ascii 1.0    "] and lines[-1] == ""
    assert [l.split()[2] for l in lines[:head] if l.startswith("property ")] == properties
    assert all(len(l) == 20 for l in lines[:head] if l.startswith("property "))
    n = int([l for l in lines[:head] if l.startswith("element vertex ")][0].split()[2])
    rows = lines[head + 1:-1]
    assert len(rows) == n and all(r.endswith(" ") for r in rows)
    return rows


def test_the_ply_file_holds_exactly_the_merged_cloud(runs):
    cls, _, prefix = runs[:3]
    rows = ply_rows(prefix + "_dense_merged.ply", ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"])
    assert len(rows) == len(cls["merged_xyz"])
    got = np.array([r.split() for r in rows])
    assert np.array_equal(got[:, 6:].astype(int), cls["merged_bgr"][:, ::-1])                   # R G B
    want = np.array([["%g" % v for v in list(p) + list(n)] for p, n in zip(cls["merged_xyz"], cls["merged_normal"])])
    assert np.array_equal(got[:, :6], want)                                                     # the stream's default: 6 significant digits


def test_sfmtoy_voxel_switch(runs):
    cls, _, prefix, gray, tmp = runs
    directory = tmp / "pgm"
    directory.mkdir()
    for i, im in enumerate(gray):
        sfm_scene.write_pnm(str(directory / ("view%02d.pgm" % i)), im)
    dense, merged = str(tmp / "dense"), str(tmp / "merged")
    child([SFMTOY, "-d", "4", "-D", "-o", dense, str(directory)], "sfmtoy -D")
    child([SFMTOY, "-d", "4", "-D", "--voxel", "0", "-o", merged, str(directory)], "sfmtoy -D --voxel 0")
    assert not os.path.exists(dense + "_dense_merged.ply")
    assert open(merged + "_dense_merged.ply", "rb").read() == open(prefix + "_dense_merged.ply", "rb").read()
    for suffix in ("_points.ply", "_cameras.ply", "_dense.ply"):
        a, b, c = (open(p + suffix, "rb").read() for p in (dense, merged, prefix))
        assert len(a) > 300 and a == b == c, suffix
    # --voxel without -D is a usage error: nothing runs
    done = subprocess.run([SFMTOY, "--voxel", "0", str(directory)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
    assert done.returncode == 2 and b"--voxel needs -D" in done.stderr
