"""Float descriptors through the whole pipeline on the MI355X (-m gpu): sfmtoylib::SfM::runSfM after setFeatures with CV_32F
descriptors (sfmba_shim_run_sfm_f32), and the merge distance of SfMAssociation::mergeNewPointCloud (sfmba_shim_merge_ex).

The runs are fresh processes with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0 as their only SFMBA_* variables, as in
tests/test_gpu_sfm_pipeline.py; a child that fails or overruns its time stops the module.

Box scene as floats: the 32-byte descriptors of tests/sfm_scene.py's box expanded to 256 floats of 0.0 / 1.0.  The squared L2
distance of such rows IS their Hamming distance, and where the two matchers keep the same (query, train) lists with every kept
Hamming distance below 20 (asserted from the two oracles before the device is asked), nothing downstream can tell the runs apart:
the float run with merge distance 20 equals the byte run byte for byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import match_l2_oracle as lo
import match_oracle as mo
import sfm_loop
import sfm_scene

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHIM = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
CHILD_TIMEOUT = 120
FAILED = []
FIELDS = ("code", "poses", "K", "done", "good", "added_view", "added_posed", "added_cloud", "xyz", "view_ptr", "view_idx", "feat_idx")


def run_child(script, args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SFMBA_")}
    env.update(SFMBA_DETERMINISTIC="1", SFMBA_SHIM_CACHE="0")
    if FAILED:                                                     # nothing more is started on the device after a child went wrong
        pytest.fail("not started: an earlier child process failed (%s)" % FAILED[0])
    cmd = [sys.executable, os.path.join(HERE, script)] + args
    try:
        done = subprocess.run(cmd, env=env, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    except subprocess.TimeoutExpired:
        FAILED.append("%s overran %d s" % (script, CHILD_TIMEOUT))
        pytest.fail("tests/%s overran its %d s" % (script, CHILD_TIMEOUT))
    if done.returncode != 0:
        FAILED.append("%s ended with %d" % (script, done.returncode))
        pytest.fail("tests/%s ended with %d:\n%s" % (script, done.returncode, done.stderr.decode()[-2000:]))
    return dict(np.load(args[-1]))


def test_box_scene_as_floats_equals_the_byte_run(tmp_path):
    scene = sfm_scene.make_box(seed=0)
    byte_descs = [v["desc"] for v in scene["views"]]
    float_descs = [np.unpackbits(d, axis=1).astype(np.float32) for d in byte_descs]
    assert len(byte_descs) == 6 and float_descs[0].shape[1] == 256
    # the precondition, from the two oracles: the same (query, train) lists, every kept Hamming distance below 20
    ham = mo.match_features(byte_descs, knn=mo.knn_keys)
    l2 = lo.match_features(float_descs)
    assert len(ham) == len(l2) == 15
    largest = 0.0
    for (pair_h, list_h), (pair_f, list_f) in zip(ham, l2):
        assert pair_h == pair_f and len(list_h) > 100
        assert [(q, t) for q, t, _ in list_h] == [(q, t) for q, t, _ in list_f], pair_h
        assert [int(np.sqrt(np.float32(d)).view(np.uint32)) for _, _, d in list_h] == [b for _, _, b in list_f], pair_h
        largest = max(largest, max(d for _, _, d in list_h))
    print("match_l2_pipeline box: 15 of 15 pairs identical under both matchers, largest kept Hamming distance %g" % largest)
    assert largest < 20
    # the two runs
    inp = sfm_loop.features_input(scene["views"], *scene["size"])
    src_b, src_f = str(tmp_path / "bytes_in.npz"), str(tmp_path / "floats_in.npz")
    np.savez(src_b, **inp)
    np.savez(src_f, kp_ptr=inp["kp_ptr"], kp_xy=inp["kp_xy"], desc=np.concatenate(float_descs), cols=inp["cols"], rows=inp["rows"], merge_distance=20.0)
    by = run_child("sfm_loop.py", ["class", src_b, str(tmp_path / "bytes_out.npz")])
    fl = run_child("match_l2_run.py", [src_f, str(tmp_path / "floats_out.npz")])
    assert by["code"] == 0 and by["good"].all() and by["done"].all() and len(by["good"]) == 6
    assert fl["code"] == 0 and fl["good"].all() and fl["done"].all() and len(fl["good"]) == 6      # OKAY with all 6 views good
    assert len(fl["xyz"]) > 100
    for k in FIELDS:
        assert by[k].dtype == fl[k].dtype and by[k].shape == fl[k].shape and by[k].tobytes() == fl[k].tobytes(), k


def run_merge(max_distance):
    """A cloud of 3 points, 3 new points: one close to point 0 whose confirming match has distance 150, one close to point 1 whose
    confirming match has distance 10, one far from everything.  max_distance None: sfmba_shim_merge (the unchanged driver)."""
    L = C.CDLL(SHIM)
    lp, ip, fp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    A = lambda a, tp: a.ctypes.data_as(tp)
    ex = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    evp = np.array([0, 1, 2, 3], np.int64); evi = np.array([0, 0, 0], np.int32); efi = np.array([5, 6, 7], np.int32)
    nw = np.array([[0.001, 0, 0], [1.001, 0, 0], [9, 9, 9]], np.float32)
    nvp = np.array([0, 1, 2, 3], np.int64); nvi = np.array([1, 1, 1], np.int32); nfi = np.array([15, 16, 17], np.int32)
    pl = np.array([0], np.int32); pr = np.array([1], np.int32); pp = np.array([0, 2], np.int64)
    q = np.array([5, 6], np.int32); t = np.array([15, 16], np.int32); d = np.array([150.0, 10.0], np.float32)
    out_n = C.c_int(0)
    oxyz = np.zeros((8, 3), np.float32); ovp = np.zeros(9, np.int64); ovi = np.zeros(32, np.int32); ofi = np.zeros(32, np.int32)
    counts = np.zeros(2, np.int64); mp = np.zeros((16, 4), np.int32); nm = C.c_int64(0)
    args = [C.c_int(2), C.c_int(3), A(ex, fp), A(evp, lp), A(evi, ip), A(efi, ip), C.c_int(3), A(nw, fp), A(nvp, lp), A(nvi, ip), A(nfi, ip),
            C.c_int(1), A(pl, ip), A(pr, ip), A(pp, lp), A(q, ip), A(t, ip), A(d, fp), C.c_int(8), C.c_int64(32), C.byref(out_n), A(oxyz, fp),
            A(ovp, lp), A(ovi, ip), A(ofi, ip), A(counts, lp), C.c_int64(16), A(mp, ip), C.byref(nm)]
    rc = L.sfmba_shim_merge(*args) if max_distance is None else L.sfmba_shim_merge_ex(*args, C.c_float(max_distance))
    assert rc == 0
    n = out_n.value
    cloud = [(oxyz[i].tolist(), {int(v): int(f) for v, f in zip(ovi[ovp[i]:ovp[i + 1]], ofi[ovp[i]:ovp[i + 1]])}) for i in range(n)]
    return cloud, int(counts[0]), int(counts[1]), [tuple(r) for r in mp[:nm.value].tolist()]


def test_merge_distance():
    far = ([9.0, 9.0, 9.0], {1: 17})
    cloud, new, merged, pairs = run_merge(200.0)                  # the match of distance 150 confirms: the point is merged
    assert cloud == [([0.0, 0.0, 0.0], {0: 5, 1: 15}), ([1.0, 0.0, 0.0], {0: 6, 1: 16}), ([2.0, 0.0, 0.0], {0: 7}), far]
    assert (new, merged) == (1, 2) and pairs == [(0, 1, 5, 15), (0, 1, 6, 16)]
    for limit in (20.0, None):                                    # 20, and the unchanged driver: neither merged nor appended
        cloud, new, merged, pairs = run_merge(limit)
        assert cloud == [([0.0, 0.0, 0.0], {0: 5}), ([1.0, 0.0, 0.0], {0: 6, 1: 16}), ([2.0, 0.0, 0.0], {0: 7}), far]
        assert (new, merged) == (1, 1) and pairs == [(0, 1, 6, 16)]
    cloud, new, merged, _ = run_merge(150.0)                      # a strict <: 150 does not confirm at 150
    assert (new, merged) == (1, 1) and cloud[0][1] == {0: 5}
