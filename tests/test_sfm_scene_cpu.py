"""The synthetic scenes of tests/sfm_scene.py checked on their own (no GPU): the "box" recipe gives every pair of views enough right
matches and is not one homography, the similarity alignment recovers planted similarities, libsfmba_shim.so exports the entry points
of the orchestrator, and SfM::setImagesDirectory reads what write_pnm wrote and refuses what it must."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import match_oracle as mo
import sfm_scene

SHIM = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sfm-toy-library_amd", "host", "libsfmba_shim.so")


@pytest.fixture(scope="module")
def box():
    return sfm_scene.make_box(seed=0)


def test_box_is_the_recipe(box):
    assert len(box["views"]) == 6 and box["size"] == (1024, 768) and len(box["X"]) == 900
    assert np.allclose(np.linalg.norm(box["centres"], axis=1), 10.0)
    z = np.array([0.0, 0.0, 1.0])
    for v, (R, c) in enumerate(zip(box["R"], box["centres"])):
        assert np.allclose(R.T @ z, -c / 10.0)                     # looks at the origin
        assert np.isclose(np.degrees(np.arctan2(c[0], -c[2])), 4.0 * v)
    for v in box["views"]:
        assert (v["track"] < 0).sum() == 100 and v["desc"].shape == (len(v["xy"]), 32)
        assert (v["xy"] >= 0).all() and (v["xy"][:, 0] < 1024).all() and (v["xy"][:, 1] < 768).all()
    again = sfm_scene.make_box(seed=0)
    assert all(a["xy"].tobytes() == b["xy"].tobytes() and a["desc"].tobytes() == b["desc"].tobytes() for a, b in zip(box["views"], again["views"]))


def test_every_pair_of_box_shares_100_right_matches(box):
    descs = [v["desc"] for v in box["views"]]
    for (l, r), lst in mo.match_features(descs, knn=mo.knn_keys):
        q, t = np.array([m[0] for m in lst], int), np.array([m[1] for m in lst], int)
        right = sfm_scene.right_matches(box, l, r, q, t)
        assert right.sum() >= 100, ((l, r), int(right.sum()))
        assert right.mean() > 0.95


def test_box_is_not_one_homography(box):
    """The parallax of the depth range at the widest baseline: a point at the near face against one at the far face on the same ray
    of view 0, seen from view 5."""
    K = box["K"]
    near, far = np.array([[0.0, 0.0, -1.5]]), np.array([[0.0, 0.0, 1.5]])
    a, _ = sfm_scene.project(K, box["R"][5], box["t"][5], near)
    b, _ = sfm_scene.project(K, box["R"][5], box["t"][5], far)
    assert np.linalg.norm(a - b) > 10.0


def test_similarity_alignment_recovers_planted_similarities():
    rng = np.random.default_rng(0)
    import triangulate_cases as tc
    for k in range(5):
        src = rng.normal(0, 3.0, (6 + k, 3))
        s, R, t = rng.uniform(0.1, 10.0), tc.rotvec_to_matrix(rng.normal(0, 1.0, 3)), rng.normal(0, 5.0, 3)
        s2, R2, t2 = sfm_scene.align_similarity(src, s * src @ R.T + t)
        assert abs(s2 - s) <= 1e-12 * s and np.abs(R2 - R).max() <= 1e-12 and np.abs(t2 - t).max() <= 1e-12 * max(1.0, np.abs(t).max())


def test_shim_exports_the_new_symbols():
    names = subprocess.run(["nm", "-D", "--defined-only", SHIM], stdout=subprocess.PIPE, check=True).stdout.decode()
    for sym in ("sfmba_shim_triangulate_views_batch", "sfmba_shim_run_sfm", "sfmba_shim_read_images_directory"):
        assert (" T " + sym + "\n") in names, sym
    for member in ("triangulateViewsBatch", "SfM6runSfMEv", "SfM18setImagesDirectory", "SfM11setFeatures", "SfM9setImages",
                   "SfM24saveCloudAndCamerasToPLY"):
        assert member in names, member


def read_directory(path, cap_images=8, cap=1 << 20):
    lib = C.CDLL(SHIM)
    w, h = np.zeros(cap_images, np.int32), np.zeros(cap_images, np.int32)
    ch = C.c_int(0)
    px = np.zeros(cap, np.uint8)
    n = lib.sfmba_shim_read_images_directory(str(path).encode(), C.c_int(cap_images), C.c_int64(cap), w.ctypes.data_as(C.POINTER(C.c_int32)),
                                             h.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ch), px.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return n, w, h, ch.value, px


def test_pgm_and_ppm_round_trip_in_file_name_order(tmp_path):
    rng = np.random.default_rng(1)
    gray = [rng.integers(0, 256, (5, 7), dtype=np.uint8), rng.integers(0, 256, (5, 7), dtype=np.uint8)]
    d = tmp_path / "gray"
    d.mkdir()
    sfm_scene.write_pnm(d / "b.pgm", gray[1])
    sfm_scene.write_pnm(d / "a.PGM", gray[0])
    (d / "notes.txt").write_text("not an image")
    n, w, h, ch, px = read_directory(d)
    assert n == 2 and ch == 1 and list(w[:2]) == [7, 7] and list(h[:2]) == [5, 5]
    assert px[:35].tobytes() == gray[0].tobytes() and px[35:70].tobytes() == gray[1].tobytes()          # "a.PGM" < "b.pgm"
    colour = rng.integers(0, 256, (4, 3, 3), dtype=np.uint8)     # written R, G, B; held B, G, R
    d = tmp_path / "colour"
    d.mkdir()
    with open(d / "c.ppm", "wb") as f:
        f.write(b"P6\n# a comment\n3 4\n255\n" + colour.tobytes())
    n, w, h, ch, px = read_directory(d)
    assert n == 1 and ch == 3 and (w[0], h[0]) == (3, 4)
    assert px[:36].tobytes() == colour[:, :, ::-1].tobytes()


def test_what_is_not_binary_8_bit_is_refused(tmp_path):
    img = np.arange(12, dtype=np.uint8).reshape(3, 4)
    cases = {"p2": dict(magic="P2"), "deep": dict(maxval=65535), "ok": {}}
    for name, kw in cases.items():
        d = tmp_path / name
        d.mkdir()
        sfm_scene.write_pnm(d / "x.pgm", img, **kw)
        assert read_directory(d)[0] == (1 if name == "ok" else -1), name
    d = tmp_path / "short"
    d.mkdir()
    (d / "x.pgm").write_bytes(b"P5\n4 3\n255\n" + img.tobytes()[:-1])
    assert read_directory(d)[0] == -1
    d = tmp_path / "mixed"
    d.mkdir()
    sfm_scene.write_pnm(d / "a.pgm", img)
    sfm_scene.write_pnm(d / "b.ppm", np.zeros((3, 4, 3), np.uint8))
    assert read_directory(d)[0] == -1
    d = tmp_path / "empty"
    d.mkdir()
    assert read_directory(d)[0] == -1 and read_directory(tmp_path / "missing")[0] == -1
