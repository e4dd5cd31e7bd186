"""The CPU restatement of sfmba_depth_normals / sfmba_cloud_merge (tests/cloud_oracle.py; the contract is in include/sfmba.h), held
against itself and against csrc/cloud_math.h compiled for the host -- no GPU.

  * the two statements of the merge (a dict loop with Python integers; a stable numpy sort with reduceat) and of the normals (a pixel
    loop; shifted copies with masks) agree bit for bit on every case of tests/cloud_cases.py;
  * the cases exercise what they claim;
  * tools/micro/cloud_math_host.hip -- the header the kernels run, compiled for the host -- agrees bit for bit with the restatement in
    q, the key, the normal quanta, the finalised xyz / bgr / normal and every intermediate of the pixel normal;
  * a tilted analytic plane gives the analytic normal;
  * the new symbols are declared, exported and bound, by the library and by the shim."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cloud_cases as cc
import cloud_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(cc.CASES))
def test_two_statements_of_the_merge_agree(name):
    c, want = cc.case(name), cc.oracle(name)
    got = co.merge_loop(c["xyz"], c["bgr"], c["normal"], c["voxel"], c["min_count"])
    assert got["n_skipped"] == want["n_skipped"]
    for f in co.MERGE_FIELDS:
        assert same_bits(got[f], want[f]), (name, f)
    assert (np.diff(want["key"].astype(np.int64)) > 0).all()                   # ascending key order (keys stay below 2^63)
    assert int(want["count"].sum()) + int((want["voxel_of"] < 0).sum()) == len(c["xyz"])  # -1: the skipped and the dropped


def test_the_merge_without_attributes():
    c = cc.case("runs_straddle")
    both = cc.oracle("runs_straddle")
    for with_bgr, with_normal in ((False, False), (True, False), (False, True)):
        got = co.merge_loop(c["xyz"], c["bgr"] if with_bgr else None, c["normal"] if with_normal else None, c["voxel"], 1)
        want = cc.oracle("runs_straddle", with_bgr, with_normal)
        for f in co.MERGE_FIELDS:
            assert same_bits(got[f], want[f]), f
        assert (want["bgr"] is None) == (not with_bgr) and (want["normal"] is None) == (not with_normal)
        assert same_bits(want["xyz"], both["xyz"]) and same_bits(want["count"], both["count"])


def test_merge_cases_exercise_what_they_claim():
    o = cc.oracle("one_voxel_5000")
    assert o["count"].tolist() == [5000] and o["first"].tolist() == [0] and (o["voxel_of"] == 0).all()
    o = cc.oracle("distinct_5000")
    assert len(o["count"]) == 5000 and (o["count"] == 1).all() and sorted(o["voxel_of"].tolist()) == list(range(5000))
    o = cc.oracle("runs_straddle")
    assert sorted(set(o["count"].tolist())) == list(cc.RUN_LENGTHS)
    starts = np.concatenate([[0], np.cumsum(o["count"])])
    long_runs = [(int(a), int(b)) for a, b in zip(starts[:-1], starts[1:]) if b - a >= 63]
    assert any(a // 64 != (b - 1) // 64 for a, b in long_runs) and any(a // 256 != (b - 1) // 256 for a, b in long_runs)
    assert {int(s) % 64 for s in starts} >= {0, 1, 2, 3}
    for name, n in (("n_32767", 32767), ("n_32768", 32768), ("n_32769", 32769)):
        o = cc.oracle(name)
        assert len(cc.case(name)["xyz"]) == n and o["n_skipped"] == 0 and {1, 2, 3} <= set(o["count"].tolist())
    c, o = cc.case("edges"), cc.oracle("edges")
    q, valid, key = co.quantise_array(c["xyz"], c["voxel"])
    i = q >> 10
    assert valid.all() and i[0].tolist() == [-1, 0, 0] and i[1].tolist() == [-1, -2, 0]
    assert i[2].tolist() == [1, 2, -3] and i[3].tolist() == [0, 2, -3]                      # on the face, and one float below it
    assert q[4].tolist() == [8, 1024, 0] and i[4].tolist() == [0, 1, 0]                     # halves go up: -0.5 + 0.5 = 0
    assert q[5].tolist() == [0, 0, 0]
    c, o = cc.case("q_limits"), cc.oracle("q_limits")
    q, valid, key = co.quantise_array(c["xyz"], c["voxel"])
    assert valid.tolist() == [True, False, True, True, False, False, True, True] and o["n_skipped"] == 3
    assert q[0, 0] == -2 ** 30 and q[2, 0] == 2 ** 30 - 64 and int(key[6]) == 0
    assert int(key[3]) == ((2 ** 20) << 42) | (0 << 21) | (2 ** 21 - 1)
    assert cc.oracle("nonfinite")["n_skipped"] == 5 and (cc.oracle("nonfinite")["voxel_of"][[3, 7, 11, 12, 20]] == -1).all()
    o = cc.oracle("subnormal_voxel")
    assert o["n_skipped"] == 30 and len(o["count"]) == 0 and (o["voxel_of"] == -1).all()
    assert (cc.case("subnormal_voxel")["xyz"] != 0).all() and 0 < float(cc.case("subnormal_voxel")["voxel"]) < np.finfo(np.float32).tiny
    o2, o3, none = cc.oracle("min_count_2"), cc.oracle("min_count_3"), cc.oracle("min_count_none_left")
    assert sorted(o2["count"].tolist()) == [2, 2, 2, 3, 3, 5, 40] and sorted(o3["count"].tolist()) == [3, 3, 5, 40]
    assert (o2["voxel_of"] < 0).sum() == 5 and (o3["voxel_of"] < 0).sum() == 11 and o2["n_skipped"] == 0
    assert len(none["count"]) == 0 and (none["voxel_of"] == -1).all()
    o = cc.oracle("opposite_normals")
    assert o["normal"][0].tolist() == [0.0, 0.0, 0.0] and o["count"].tolist() == [2, 2]
    assert np.allclose(o["normal"][1], [0.6, 0.0, 0.8], atol=1e-4)
    o = cc.oracle("nan_normal")                                                             # voxel 0: (0 + 0, 0 + 0, 1 + 1) -> (0, 0, 1)
    assert o["normal"][0].tolist() == [0.0, 0.0, 1.0] and o["normal"][1].tolist() == [0.0, 0.0, 0.0]
    assert np.allclose(o["normal"][2], np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0), atol=1e-6)     # +-inf and 100 all clamp to 2^20
    assert not np.isnan(o["normal"]).any()


def test_sums_stay_inside_their_bounds():
    # the worst case the contract admits: 2^31 - 1 members with |q| = 2^30, |m| = 2^20, colour 255
    c = 2 ** 31 - 1
    assert c * 2 ** 30 < 2 ** 61 and c * 2 ** 20 < 2 ** 51 < 2 ** 53 and c * 255 < 2 ** 39 and 2 * c * 255 + c < 2 ** 41
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    for text in ("|Sq_a| < 2^61", "|Sm_a| < 2^51", "< 2^39", "2 S + c < 2^41"):
        assert text in header


@pytest.mark.parametrize("name", list(cc.NORMAL_CASES))
def test_two_statements_of_the_normals_agree(name):
    c, want = cc.normals_case(name), cc.normals_oracle(name)
    got = co.normals_loop(c["K"], c["P"], c["depth"], c["max_rel_step"])
    assert same_bits(got["has"], want["has"]) and same_bits(got["flipped"], want["flipped"]), name
    assert same_bits(got["normal"], want["normal"]), name
    assert not want["normal"][~want["has"]].any()
    n = np.linalg.norm(want["normal"][want["has"]].astype(np.float64), axis=-1)
    assert np.allclose(n, 1.0, atol=1e-6)


def test_normal_cases_exercise_what_they_claim():
    for name in ("size_1x1", "size_7x1", "size_1x7"):
        assert (cc.normals_case(name)["depth"] > 0).all() and not cc.normals_oracle(name)["has"].any(), name
    assert cc.normals_oracle("size_33x17")["has"].all()
    o = cc.normals_oracle("size_70x45")
    assert 0.5 < o["has"].mean() < 0.9
    c, o = cc.normals_case("one_sided"), cc.normals_oracle("one_sided")
    d = c["depth"]
    assert o["has"][4, 3] and o["has"][4, 5] and o["has"][3, 4] and o["has"][5, 4]          # beside the four holes: one-sided differences
    assert d[4, 2] == 0 and d[4, 6] == 0 and d[2, 4] == 0 and d[6, 4] == 0
    assert not o["has"][0, 0] and d[0, 0] > 0                                               # alone
    assert not o["has"][3, 3] and d[3, 3] > 0                                               # no neighbour within the step
    assert o["has"][3, 4] and o["has"][4, 3]                                                # ... and its neighbours do without it
    assert o["has"][2, 2] and o["has"][6, 6]                                                # block corners: one-sided both ways
    assert cc.normals_oracle("step_exact")["has"][1, 1] and not cc.normals_oracle("step_below")["has"][1, 1]
    # the flip fires only where rounding decides the sign (cloud_cases._flip says why); on every ordinary map it never does ...
    for name in cc.NORMAL_CASES:
        assert name == "flip" or not cc.normals_oracle(name)["flipped"].any(), name
    o = cc.normals_oracle("flip")
    assert 0.02 < o["flipped"].mean() < 0.98 and o["has"].mean() > 0.5
    # ... and every normal faces its camera: n_cam . p0 < 0
    c, o = cc.normals_case("size_70x45"), cc.normals_oracle("size_70x45")
    R = c["P"][:, :3].astype(np.float64)
    n_cam = o["normal"].astype(np.float64) @ R.T
    h, w = c["depth"].shape
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    rays = np.stack([(xs - c["K"][0, 2]) / c["K"][0, 0], (ys - c["K"][1, 2]) / c["K"][1, 1], np.ones((h, w))], -1)
    assert ((n_cam * rays).sum(-1)[o["has"]] < 0).all()
    c, o = cc.normals_case("odd_values"), cc.normals_oracle("odd_values")
    # NaN and negative depths have no normal; an INFINITE depth is > 0 and every neighbour passes |zn - inf| <= step inf, so the
    # contract gives it the normal of its neighbours' differences: the device must do the same, and no NaN may come out
    assert not o["has"][2, 3] and not o["has"][6, 7] and not np.isnan(o["normal"]).any()
    assert o["has"].sum() > 60
    assert cc.normals_oracle("step_zero")["has"].all()                                      # equal depths pass a step of 0


def test_tilted_plane_gives_the_analytic_normal():
    """The restatement against the analytic normal of a plane n . X = d seen by a rotated camera.  The only errors are the float32
    depth map (2^-24 relative, against a depth change of about z / f per pixel: an angle of about f 2^-24 / 1 = 4e-6 at f = 60) and
    the float32 output.  MEASURED ONCE on this restatement: the largest deviation over the map is 6.6e-6 (radians; the norm of the
    difference of unit vectors).  The bound asserted is ten times that, 6.6e-5."""
    w, h = 40, 30
    K, P = cc.camera(w, h, deg=35.0)
    n_cam = np.array([0.35, -0.25, -1.0])
    n_cam /= np.linalg.norm(n_cam)
    depth = cc.plane_depth(K, w, h, n_cam, -5.0)
    assert (depth > 2).all()
    o = co.normals_shifted(K, P, depth, 0.5)
    assert o["has"].all() and not o["flipped"].any()
    want = P[:, :3].astype(np.float64).T @ n_cam                                            # faces the camera: n_cam . p0 = d < 0
    err = np.linalg.norm(o["normal"].astype(np.float64) - want, axis=-1).max()
    print("largest deviation from the analytic normal: %.3e" % err)
    assert err <= 6.6e-5


# ---- csrc/cloud_math.h on the host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("cloud") / "cloud_math_host")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tools", "micro", "cloud_math_host.hip")])
    return exe


def hx(v):
    return float(v).hex()


def run(host_exe, mode, tmp_path, text):
    path = tmp_path / (mode + ".txt")
    path.write_text(text)
    return subprocess.check_output([host_exe, mode, str(path)]).decode().splitlines()


def bits32(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0]


def bits64(v):
    return struct.pack("<d", float(v))


def test_host_quantise_matches(host_exe, tmp_path):
    rng = np.random.default_rng(71)
    rows = []
    for name in ("edges", "q_limits", "nonfinite", "subnormal_voxel"):
        c = cc.case(name)
        rows += [(p, c["voxel"]) for p in c["xyz"]]
    for _ in range(4000):
        voxel = np.float32(10.0 ** rng.uniform(-4, 2))
        scale = voxel * 10.0 ** rng.uniform(0, 6.5)
        rows.append(((rng.normal(size=3) * scale).astype(np.float32), voxel))
    for k in range(300):                                                                    # exact halves and voxel faces at voxel 2^-3
        rows.append((np.asarray([(k - 150 + 0.5) / 8192.0, (k - 150) / 8.0, -(k + 0.5) / 8192.0], np.float32), np.float32(0.125)))
    out = run(host_exe, "quantise", tmp_path, "".join(" ".join(hx(v) for v in list(p) + [voxel]) + "\n" for p, voxel in rows))
    assert len(out) == len(rows)
    n_skipped = 0
    for i, ((p, voxel), line) in enumerate(zip(rows, out)):
        t = line.split()
        q = [co.quantise(float(x), float(voxel)) for x in p]
        assert int(t[0]) == int(None not in q), i
        assert [int(x) for x in t[1:4]] == [0 if v is None else v for v in q], i
        assert int(t[4], 16) == (co.SKIPPED if None in q else co.key_of(q)), i
        qa, valid, key = co.quantise_array(p[None], voxel)
        assert bool(valid[0]) == (None not in q) and int(key[0]) == int(t[4], 16), i
        n_skipped += None in q
    assert 50 < n_skipped < len(rows) // 2


def test_host_normal_quanta_match(host_exe, tmp_path):
    rng = np.random.default_rng(72)
    vals = [0.0, -0.0, 1.0, -1.0, 0.5 / 16384, -0.5 / 16384, 1.5 / 16384, 64.0, -64.0, 64.0001, 1e30, -1e30, np.inf, -np.inf, np.nan, 3e38]
    vals += list(rng.normal(size=3000).astype(np.float32)) + list((rng.integers(-40000, 40000, size=500) + 0.5) / 16384.0)
    vals = [np.float32(v) for v in vals]
    out = run(host_exe, "nquant", tmp_path, "".join(hx(v) + "\n" for v in vals))
    want = [co.normal_quantum(float(v)) for v in vals]
    assert [int(x) for x in out] == want
    assert want == co.normal_quanta_array(np.asarray(vals, np.float32)).tolist()
    assert max(want) == 2 ** 20 and min(want) == -2 ** 20 and want[14] == 0 and want[4] == 1 and want[5] == 0


def test_host_finalise_matches(host_exe, tmp_path):
    rng = np.random.default_rng(73)
    rows = []
    for _ in range(3000):
        c = int(rng.choice([1, 2, 3, 7, 100, 5000, 2 ** 31 - 1]))
        big = int(rng.integers(0, 3))
        Sq = [int(rng.integers(-c * 2 ** 30, c * 2 ** 30 + 1)) if big else int(rng.integers(-c * 4096, c * 4096 + 1)) for _ in range(3)]
        Sb = [int(rng.integers(0, 255 * c + 1)) for _ in range(3)]
        Sm = [int(rng.integers(-c * 2 ** 20, c * 2 ** 20 + 1)) if rng.random() < 0.8 else 0 for _ in range(3)]
        rows.append((c, Sq, Sb, Sm, np.float32(10.0 ** rng.uniform(-3, 1))))
    rows.append((2, [3, -3, 1], [255, 0, 1], [0, 0, 0], np.float32(0.1)))                   # L == 0; colour halves go up: 1 / 2 -> 1
    text = "".join(" ".join([str(c)] + [str(v) for v in Sq + Sb + Sm] + [hx(voxel)]) + "\n" for c, Sq, Sb, Sm, voxel in rows)
    out = run(host_exe, "final", tmp_path, text)
    assert len(out) == len(rows)
    for i, ((c, Sq, Sb, Sm, voxel), line) in enumerate(zip(rows, out)):
        t = line.split()
        assert t[:3] == [bits32(co.final_coord(s, c, float(voxel))) for s in Sq], i
        assert [int(x) for x in t[3:6]] == [co.final_colour(s, c) for s in Sb], i
        assert t[6:9] == [bits32(v) for v in co.final_normal(Sm)], i
    assert out[-1].split()[3:] == ["128", "0", "1", "00000000", "00000000", "00000000"]
    assert any(abs(s) > 2 ** 53 for r in rows for s in r[1])                                # sums that a double cannot hold exactly


@pytest.mark.parametrize("name", list(cc.NORMAL_CASES))
def test_host_pixel_normal_matches(host_exe, tmp_path, name):
    c = cc.normals_case(name)
    want = co.normals_loop(c["K"], c["P"], c["depth"], c["max_rel_step"])
    h, w = c["depth"].shape
    K, P = c["K"], c["P"]
    head = [str(w), str(h)] + [hx(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2])] + [hx(v) for v in P.reshape(-1)] + [hx(c["max_rel_step"])]
    out = run(host_exe, "normal", tmp_path, " ".join(head) + "\n" + " ".join(hx(v) for v in c["depth"].reshape(-1)) + "\n")
    assert len(out) == h * w
    for i, line in enumerate(out):
        v, u = divmod(i, w)
        t = line.split()
        assert int(t[0]) == int(want["has"][v, u]), (u, v)
        assert t[1:4] == [bits32(x) for x in want["normal"][v, u]], (u, v)
        got, ref = [float.fromhex(x) for x in t[4:17]], want["mid"][v, u]
        for k, (a, b) in enumerate(zip(got, ref)):
            assert (np.isnan(a) and np.isnan(b)) or bits64(a) == bits64(b) or (a == 0.0 and b == 0.0), (u, v, k)


def test_symbols_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    lib = os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "libsfmba_hip.so")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    from sfm_toy_library_amd import capi
    for name in ("sfmba_depth_normals", "sfmba_cloud_merge"):
        assert "SFMBA_API int %s(" % name in header
        assert " T %s\n" % name in exported
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    assert callable(capi.depth_normals) and callable(capi.cloud_merge)
    assert capi.lib().sfmba_abi_version() == 6
    shim = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    exported = subprocess.check_output(["nm", "-D", "-C", "--defined-only", shim]).decode()
    for name in ("sfmtoylib::SfMDenseUtilities::computeNormals(", "sfmtoylib::SfMDenseUtilities::mergeCloud(", "sfmtoylib::SfM::mergeDenseCloud(",
                 "sfmtoylib::SfM::saveMergedDenseCloudToPLY(", "sfmba_shim_run_sfm_merged"):
        assert name in exported, name
    for text in ("sfmba_cloud_merge",):                                                     # the three notes point to the new call
        assert text in open(os.path.join(ROOT, "README.md")).read()
        assert text in open(os.path.join(ROOT, "sfm-toy-library_amd", "host", "SfMDenseUtilities.h")).read()
