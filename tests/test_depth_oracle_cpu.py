"""The CPU restatement of the dense-stereo contract (tests/depth_oracle.py; include/sfmba.h, sfmba_depth_sweep / sfmba_depth_fuse),
held against itself and against csrc/depth_math.h compiled for the host -- no GPU.

  * the two formulations of the sweep (shifted-copy window sums + a lane's running winner; integral images + an argmax over the
    cost volume) agree bit for bit on every case of tests/depth_cases.py;
  * tools/micro/depth_math_host.hip -- the header the kernels run, compiled for the host -- agrees bit for bit with the
    restatement on A, b, u', v', su, sv, J, the sums, the score, delta and the outputs, on some thousands of inputs that include
    coordinates exactly on 0 and ws - 1, q_2 on both sides of 0 and a quotient exactly on a half of 1/16 px;
  * the int32 bounds of the window sums at r = 4;
  * the new symbols are declared, exported and bound;
  * the quality floors of the contract on the rendered corner scene (the device is held equal to the restatement, so it inherits
    them)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import depth_cases as dc
import depth_oracle as do
import sfm_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("depth", "score", "plane")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(dc.CASES))
def test_two_formulations_agree(name):
    c, want = dc.case(name), dc.oracle(name)
    got = do.sweep_direct(c["images"], c["K"], c["P"], c["jobs"][0], **c["params"])
    for f in FIELDS + ("cost", "delta", "part"):
        assert same_bits(got[f], want[f]), (name, f)


def test_cases_exercise_what_they_claim():
    for name in ("size_1x1_r1", "size_4x4_r2", "size_8x8_r4", "blind", "const_ref"):
        o = dc.oracle(name)
        assert not o["depth"].any() and not o["score"].any() and (o["plane"] == -1).all(), name
    assert not dc.oracle("const_ref")["part"].any() and dc.oracle("blind")["part"].any()
    # D = 2 puts its two planes at z = 8 and 12.5 with the surface at 10: few windows match, some do
    assert dc.oracle("size_15x16_r1_d2")["accepted"].any()
    for name in ("size_16x16_r4_d3", "size_17x33_r1_d64_s4", "size_48x31_r4_d64_s4", "size_48x31_r3_d64", "const_src"):
        o = dc.oracle(name)
        assert o["accepted"].sum() >= 0.5 * o["part"].sum() > 0, name
    assert not dc.oracle("size_15x16_r1_d2")["delta"].any()                   # D = 2: no refinement possible
    assert dc.oracle("size_48x31_r3_d64")["delta"].any()
    o = dc.oracle("behind")                                                     # q_2 <= 0 for source 1 over the left half: source 2 alone there
    assert o["accepted"].any()
    o, one = dc.oracle("min_sources_2"), None
    c = dc.case("min_sources_2")
    one = do.sweep_integral(c["images"], c["K"], c["P"], c["jobs"][0], **dict(c["params"], min_sources=1))
    assert 0 < (o["plane"] >= 0).sum() < (one["plane"] >= 0).sum()
    o = dc.oracle("tie")                                                        # all planes cost the same: the lowest k, delta = 0
    assert o["part"].any() and (o["plane"][o["part"]] == 0).all() and not o["delta"].any()
    assert (o["cost"][o["part"]] == 1.0).all() and o["accepted"][o["part"]].all()          # min_score lies exactly on C_k*


def test_window_sums_fit_int32_at_radius_4():
    n = 81
    I, J = np.full(n, 255, np.int64), np.full(n, 4080, np.int64)
    assert (16 * 16 * 255 + 8) >> 4 == 4080
    bounds = dict(SI=I.sum(), SII=(I * I).sum(), SJ=J.sum(), SJJ=(J * J).sum(), SIJ=(I * J).sum())
    assert bounds == dict(SI=20655, SII=5267025, SJ=330480, SJJ=1348358400, SIJ=84272400)
    assert max(bounds.values()) < 2 ** 31
    assert n * bounds["SJJ"] > 2 ** 31                                          # ... and the variances need int64
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    for v in bounds.values():
        assert str(v) in header


# ---- csrc/depth_math.h on the host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("depth") / "depth_math_host")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tools", "micro", "depth_math_host.hip")])
    return exe


def hx(v):
    return float(v).hex()


def run(host_exe, mode, tmp_path, text):
    path = tmp_path / (mode + ".txt")
    path.write_text(text)
    return subprocess.check_output([host_exe, mode, str(path)]).decode().splitlines()


def bits64(v):
    return struct.pack("<d", float(v))


def random_pose(rng, spread=1.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    return np.concatenate([R, rng.normal(scale=spread, size=(3, 1))], axis=1).astype(np.float32).reshape(12)


def test_host_warp_matches(host_exe, tmp_path):
    rng = np.random.default_rng(11)
    rows = []
    for _ in range(1000):
        k4 = np.asarray([rng.uniform(100, 3000), rng.uniform(100, 3000), rng.uniform(0, 1000), rng.uniform(0, 1000)], np.float32)
        rows.append((k4, random_pose(rng), random_pose(rng)))
    out = run(host_exe, "warp", tmp_path, "".join(" ".join(hx(v) for v in np.concatenate(r)) + "\n" for r in rows))
    assert len(out) == len(rows)
    for (k4, pr, ps), line in zip(rows, out):
        A, b = do.warp([float(v) for v in k4], [float(v) for v in pr], [float(v) for v in ps])
        got = [float.fromhex(t) for t in line.split()]
        assert [bits64(v) for v in got] == [bits64(v) for v in A + b]


def test_host_project_matches(host_exe, tmp_path):
    rng = np.random.default_rng(12)
    eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    rows = []
    # planted: coordinates exactly on 0 and ws - 1 (valid), one step outside (not valid)
    for u, v in ((0, 0), (39, 29), (39, 0), (0, 29), (40, 5), (5, 30)):
        rows.append((eye, [0.0, 0.0, 0.0], 0.1, u, v, 40, 30))
    # ... a quotient exactly on a half of 1/16 px: u' = u + 1/32, 16 u' + 0.5 = 16 u + 1 exactly; and just below it
    half = list(eye); half[2] = 1.0 / 32
    below = list(eye); below[2] = np.nextafter(1.0 / 32, 0.0)
    for u in range(0, 39, 3):
        rows.append((half, [0.0, 0.0, 0.0], 0.1, u, 7, 40, 30))
        rows.append((below, [0.0, 0.0, 0.0], 0.1, u, 7, 40, 30))
    # ... q_2 on both sides of 0 and exactly 0: q_2 = 1 + w b_2 with w = 0.5
    for b2 in (-2.0, np.nextafter(-2.0, 0.0), np.nextafter(-2.0, -3.0), -1.0, -3.0):
        rows.append((eye, [0.0, 0.0, b2], 0.5, 10, 10, 40, 30))
    n_planted = len(rows)
    for _ in range(4000):
        A = (np.asarray(eye) + rng.normal(scale=[0.02, 0.02, 8.0, 0.02, 0.02, 8.0, 1e-4, 1e-4, 1.0], size=9)).tolist()
        b = rng.normal(scale=[40.0, 40.0, 1.0], size=3).tolist()
        rows.append((A, b, float(rng.uniform(0.05, 0.5)), int(rng.integers(0, 48)), int(rng.integers(0, 31)), 48, 31))
    text = "".join(" ".join([hx(v) for v in A] + [hx(v) for v in b] + [hx(w), str(u), str(v), str(ws), str(hs)]) + "\n" for A, b, w, u, v, ws, hs in rows)
    out = run(host_exe, "project", tmp_path, text)
    assert len(out) == len(rows)
    n_valid = n_neg = 0
    for i, ((A, b, w, u, v, ws, hs), line) in enumerate(zip(rows, out)):
        valid, up, vp = do.project(A, b, np.float64(u), np.float64(v), w, ws, hs)
        t = line.split()
        assert int(t[0]) == int(valid), i
        gu, gv = float.fromhex(t[1]), float.fromhex(t[2])
        assert (np.isnan(gu) and np.isnan(up)) or bits64(gu) == bits64(up), i
        assert (np.isnan(gv) and np.isnan(vp)) or bits64(gv) == bits64(vp), i
        if valid:
            assert (int(t[3]), int(t[4])) == (int(do.fix(up)), int(do.fix(vp))), i
            n_valid += 1
        n_neg += not (((A[6] * u + A[7] * v) + A[8]) + w * b[2] > 0.0)
    assert n_valid > 1000 and n_neg > 100
    planted = [l.split() for l in out[:n_planted]]
    assert [int(t[0]) for t in planted[:6]] == [1, 1, 1, 1, 0, 0]
    assert (int(planted[1][3]), int(planted[1][4])) == (16 * 39, 16 * 29)
    for j, u in enumerate(range(0, 39, 3)):
        assert int(planted[6 + 2 * j][3]) == 16 * u + 1                         # the half goes up
        # one ulp below the half the sum 16 u' + 0.5 itself may round up to the integer: the contract's own arithmetic decides
        assert int(planted[7 + 2 * j][3]) == int(np.floor(16.0 * (u + below[2]) + 0.5))
    # q_2 = 0 (u' infinite), 2^-53 (positive, but u' far outside the image), -2^-52, 0.5 (u' = 20: valid), -0.5
    assert [int(t[0]) for t in planted[-5:]] == [0, 0, 0, 1, 0]


def test_host_unproject_matches(host_exe, tmp_path):
    rng = np.random.default_rng(13)
    rows = []
    for _ in range(2000):
        k4 = [float(np.float32(v)) for v in (rng.uniform(150, 400), rng.uniform(150, 400), 24.0, 15.5)]
        p, ps = random_pose(rng, 0.3), random_pose(rng, 0.3)
        if rng.random() < 0.7:
            ps = p.copy()
            ps[[3, 7, 11]] += rng.normal(scale=0.05, size=3).astype(np.float32)
        z = float(np.float32(rng.uniform(0.5, 12.0)))
        zs = float(np.float32(z * (1 + rng.normal(scale=0.01))))
        rows.append((k4, [float(v) for v in p], int(rng.integers(0, 48)), int(rng.integers(0, 31)), z, [float(v) for v in ps], 48, 31, zs,
                     float(np.float32(rng.choice([0.0, 0.005, 0.02])))))
    text = "".join(" ".join([hx(v) for v in k4 + p] + [str(u), str(v), hx(z)] + [hx(x) for x in ps] + [str(ws), str(hs), hx(zs), hx(tol)]) + "\n"
                   for k4, p, u, v, z, ps, ws, hs, zs, tol in rows)
    out = run(host_exe, "unproject", tmp_path, text)
    assert len(out) == len(rows)
    n_in = n_agree = 0
    for i, ((k4, p, u, v, z, ps, ws, hs, zs, tol), line) in enumerate(zip(rows, out)):
        X = do.unproject(k4, p, np.float64(u), np.float64(v), np.float64(z))
        inside, px, py, qz = do.reproject(k4, ps, X, ws, hs)
        t = line.split()
        assert [bits64(float.fromhex(x)) for x in t[:3]] == [bits64(x) for x in X], i
        assert int(t[3]) == int(inside) and bits64(float.fromhex(t[6])) == bits64(qz), i
        if inside:
            assert (int(t[4]), int(t[5])) == (int(px), int(py)), i
        agrees = bool(zs > 0.0 and abs(zs - qz) <= tol * qz)
        assert int(t[7]) == int(agrees), i
        n_in += bool(inside)
        n_agree += agrees
    assert n_in > 300 and n_agree > 100


def sweep_file(c):
    p = c["params"]
    lines = ["%d %d %d %d %d" % (len(c["images"]), p["n_planes"], p["radius"], p["min_std"], p["min_sources"]),
             " ".join([hx(np.float32(p["min_score"]))] + [hx(v) for v in np.asarray(c["K"], np.float32).reshape(9)])]
    for im, P in zip(c["images"], np.asarray(c["P"], np.float32).reshape(-1, 12)):
        lines.append("%d %d " % (im.shape[1], im.shape[0]) + " ".join(hx(v) for v in P))
        lines.append(" ".join(str(int(v)) for v in im.reshape(-1)))
    ref, srcs, zn, zf = c["jobs"][0]
    lines.append("%d %d %s %s %s" % (ref, len(srcs), " ".join(str(s) for s in srcs), hx(np.float32(zn)), hx(np.float32(zf))))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("name", ["size_17x33_r2_d3", "size_16x16_r4_d3", "behind", "const_src", "min_sources_2", "tie", "small_d12"])
def test_host_sweep_matches(host_exe, tmp_path, name):
    c = dc._case((23, 18), 2, 2, 12, src_size=(20, 21)) if name == "small_d12" else dc.case(name)
    want = do.sweep_integral(c["images"], c["K"], c["P"], c["jobs"][0], debug=True, **c["params"])
    out = run(host_exe, "sweep", tmp_path, sweep_file(c))
    h, w = want["depth"].shape
    n_src = len(c["jobs"][0][1])
    for s in range(n_src):
        t = out[s].split()
        assert t[:2] == ["A", str(s)]
        assert [bits64(float.fromhex(x)) for x in t[2:]] == [bits64(x) for x in want["AB"][s][0] + want["AB"][s][1]]
    t = out[n_src].split()
    assert t[0] == "W" and [bits64(float.fromhex(x)) for x in t[1:]] == [bits64(want["wf"]), bits64(want["step"])]
    n_s = n_o = 0
    for line in out[n_src + 1:]:
        t = line.split()
        x, y = int(t[1]), int(t[2])
        if t[0] == "S":
            k, s = int(t[3]), int(t[4])
            d = want["planes"][k][s]
            assert want["part"][y, x]
            assert int(t[5]) == int(d["all_valid"][y, x]) and int(t[6]) == int(d["counts"][y, x]) and int(t[7]) == int(d["J"][y, x]), line
            if d["all_valid"][y, x]:
                assert (int(t[8]), int(t[9]), int(t[10])) == (int(d["SJ"][y, x]), int(d["SJJ"][y, x]), int(d["SIJ"][y, x])), line
            assert bits64(float.fromhex(t[11])) == bits64(d["score"][y, x]), line
            n_s += 1
        else:
            assert t[0] == "O"
            assert int(t[3]) == int(want["part"][y, x]) and (int(t[4]), int(t[5])) == (int(want["SI"][y, x]), int(want["SII"][y, x])), line
            assert int(t[6]) == int(want["plane"][y, x]), line
            assert int(t[7], 16) == int(want["depth"].view(np.uint32)[y, x]) and int(t[8], 16) == int(want["score"].view(np.uint32)[y, x]), line
            assert bits64(float.fromhex(t[9])) == bits64(want["delta"][y, x]) and bits64(float.fromhex(t[10])) == bits64(want["cost"][y, x]), line
            n_o += 1
    assert n_o == h * w and n_s == int(want["part"].sum()) * c["params"]["n_planes"] * n_src
    if name == "small_d12":
        assert n_s > 4000 and want["delta"].any()


# ---- the public layers ------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build_hip()
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    lib = os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "libsfmba_hip.so")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    from sfm_toy_library_amd import capi
    for name in ("sfmba_depth_sweep", "sfmba_depth_fuse"):
        assert "SFMBA_API int %s(" % name in header
        assert " T %s\n" % name in exported
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    assert callable(capi.depth_sweep) and callable(capi.depth_fuse)
    assert capi.lib().sfmba_abi_version() == 6


def test_fuse_restatement_properties():
    images, K, P, maps = dc.fuse_scene()
    checks = [[1, 2], [0], [0]]
    all_ = do.fuse(images, K, P, maps, checks, rel_tol=0.01, min_consistent=0)
    assert all_["pt_ptr"].tolist() == np.concatenate([[0], np.cumsum([(m > 0).sum() for m in maps])]).tolist()     # 0: every depth is kept
    one = do.fuse(images, K, P, maps, checks, rel_tol=0.01, min_consistent=1)
    two = do.fuse(images, K, P, maps, checks, rel_tol=0.01, min_consistent=2)
    assert 0 < two["pt_ptr"][-1] < one["pt_ptr"][-1] < all_["pt_ptr"][-1]
    assert two["pt_ptr"][1] == two["pt_ptr"][-1]                                # only image 0 has two check images
    # the kept points lie on the planted plane z = 0 (a plane step at this baseline is about 0.1 world units)
    assert np.median(np.abs(one["xyz"][:, 2])) < 0.1
    # stable order and the pixel's own colour
    key = one["src_image"].astype(np.int64) * 10 ** 6 + one["src_pixel"]
    assert (np.diff(key) > 0).all()
    i, q = int(one["src_image"][5]), int(one["src_pixel"][5])
    assert one["bgr"][5].tolist() == [int(images[i].reshape(-1)[q])] * 3


# ---- quality floors ---------------------------------------------------------------------------------------------------------
def test_quality_floors_on_the_corner_scene():
    """Prototype figures for this configuration (numpy `@` products for A and b): accepted / textured 0.999, right within one
    plane step 0.958, nothing accepted on the background.  The floors are those less a margin."""
    sc = sfm_scene.make_corner(size=(320, 240), focal=1250, texture_scale=125)
    zt = dc.corner_depth(sc, 1)
    fin = np.isfinite(zt)
    zn, zf = zt[fin].min() / 1.05, zt[fin].max() * 1.05
    P = np.concatenate([sc["R"], sc["t"][:, :, None]], axis=2).astype(np.float32)
    o = do.sweep_integral(sc["images"], sc["K"].astype(np.float32), P, (1, [0, 2], zn, zf), n_planes=32, radius=3, min_std=2, min_score=0.6)
    acc = o["depth"] > 0
    with np.errstate(all="ignore"):
        err = np.abs(1.0 / np.where(acc, o["depth"], 1).astype(np.float64) - 1.0 / np.where(fin, zt, 1.0))
    right = acc & fin & (err <= o["step"])
    accepted, correct = acc.sum() / o["part"].sum(), right.sum() / acc.sum()
    print("corner 320x240 r3 D32: textured %.3f accepted/textured %.4f right/accepted %.4f background accepted %d"
          % (o["part"].mean(), accepted, correct, (acc & ~fin).sum()))
    assert not (acc & ~o["part"]).any()
    assert accepted >= 0.97
    assert correct >= 0.90
    assert not (acc & ~fin).any()


def test_sfmtoy_usage_names_the_dense_switch_and_the_shim_has_the_drivers():
    import __graft_entry__ as ge
    ge.build_host()
    exe = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")
    ok = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert ok.returncode == 0 and "-D, --dense" in ok.stdout and "_dense.ply" in ok.stdout
    # the switch takes no value and gets past the argument check: the missing directory is then an ordinary failure, before any device
    for args in (["-D"], ["--dense", "-d", "4"]):
        done = subprocess.run([exe] + args + ["/nonexistent-directory"], capture_output=True, text=True)
        assert done.returncode == 1, (args, done.returncode, done.stderr)
    so_ = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    syms = subprocess.check_output(["nm", "-C", so_]).decode()
    for name in ("sfmba_shim_run_sfm_dense", "sfmba_shim_densify_refusal"):
        assert " T %s\n" % name in syms, name
    assert "sfmtoylib::SfM::densify(" in syms and "sfmtoylib::SfMDenseUtilities::computeDepthMaps(" in syms
    assert "sfmtoylib::SfMDenseUtilities::fuseDepthMaps(" in syms and "sfmtoylib::SfM::saveDenseCloudToPLY(" in syms


def test_densify_refuses_without_pixels_or_without_a_run():
    import ctypes
    import __graft_entry__ as ge
    ge.build_host()
    shim = ctypes.CDLL(os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so"))
    for what in (0, 1, 2):                   # after setFeatures; images without a run; a fresh object: ERROR, nothing kept, no device touched
        assert shim.sfmba_shim_densify_refusal(what) == 1, what


def test_host_rules_restatement_on_a_planted_cloud():
    """depth_oracle.dense_jobs on a cloud whose depths are known: the percentiles, the 1.25 margins, the m < 8 rule, the source order."""
    R = np.eye(3)
    poses = np.array([np.concatenate([R, np.array([[-x], [0.0], [0.0]])], axis=1).reshape(12) for x in (0.0, 1.0, 3.0, 3.5)], np.float32)
    z = np.arange(1, 101, dtype=np.float64)                                     # 100 points at depth 1..100 seen by views 0 and 1
    xyz = np.stack([np.zeros(100), np.zeros(100), z], axis=1).astype(np.float32)
    view_ptr = np.arange(0, 201, 2)
    view_idx = np.tile([0, 1], 100)
    view_idx[:14] = np.tile([2, 3], 7)                                          # ... the first 7 by views 2 and 3 instead: m = 7 < 8
    jobs = do.dense_jobs(poses, xyz, view_ptr, view_idx, np.ones(4, bool))
    assert [j[0] for j in jobs] == [0, 1]
    assert jobs[0][1] == [1, 2] and jobs[1][1] == [0, 2]                        # nearest centres first; 2 (at 3.0) before 3 (at 3.5)
    m = 93                                                                      # depths 8..100
    assert jobs[0][2] == float(np.float32((8 + (5 * m) // 100) / 1.25)) and jobs[0][3] == float(np.float32((8 + (95 * m) // 100) * 1.25))
    assert do.dense_jobs(poses, xyz, view_ptr, view_idx, np.array([1, 0, 0, 0], bool)) == []      # no other good view: no job
