"""CPU-side checks of the float-descriptor extractor's contract (include/sfmba.h, sfmba_surf_extract): no GPU needed.

  formulations    the vectorised (integral image) and the plain (direct pixel sums, Python integers, exact rationals) statement of the
                  detector, the orientation and the descriptor of tests/surf_oracle.py agree bit for bit
  tables          the weight literals of the header and of csrc/surf_math.h equal their formulas
  host program    tools/micro/surf_math_host.hip (csrc/surf_math.h, the arithmetic the kernels run, compiled for the host) equals the
                  oracle on every image of the GPU test: H bits, moments, bins, the 64 sums, descriptor bits, key point fields
  bounds          every |v| < 4.8e14, every n2 < 2^52, every descriptor has |norm - 1| <= 64 * 2^-24
  blobs           a blob centred on a grid position is found there: sigma 6 at L = 27, sigma 9 at L = 51
  equivariance    two crops of one texture at offsets that differ by multiples of 2^(n_octaves - 1): every key point whose 27 filters
                  and whole descriptor window lie inside both crops appears in both with the same H bits and descriptor bits
  sanity          on the 300 x 300 texture, 3 octaves, threshold 20, 300 features: after the 0.8 ratio test at least 30 matches are
                  kept and at least half of them are right (within 3 max(1, L / 9) px), for a roll by (8, 4) and a 20 degree rotation.
                  Measured: roll 271 kept, 269 right; 20 degrees 174 kept, 172 right
  symbols         the libraries export sfmba_surf_extract, the new members and the new shim drivers; the old entry points stay
  program         sfmtoy names -f and -m in its usage text and refuses unusable values with exit status 2"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import match_l2_oracle as ml
import surf_cases as sc
import surf_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits64(a):
    return np.asarray(a, np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def img60():
    return sc.noise(60, 60, 50)


def test_box_formulations_agree(img60):
    I, P = so.integral(img60), so.padded(img60)
    rng = np.random.default_rng(1)
    for _ in range(300):
        y0, x0 = int(rng.integers(-70, 70)), int(rng.integers(-70, 80))
        bh, bw = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        assert int(so.box(I, y0, x0, bh, bw)) == so.box_plain(P, y0, x0, bh, bw), (y0, x0, bh, bw)
    assert int(so.box(I, 0, 0, 50, 60)) == int(img60.astype(np.int64).sum()) and int(so.box(I, -9, -9, 5, 5)) == 0


def test_detector_formulations_agree(img60):
    h, w = img60.shape
    I, P = so.integral(img60), so.padded(img60)
    found = 0
    for o in (0, 1):
        R = so.response_maps(I, o)
        for m in (1, 2):
            ys, xs, H = so.candidates(R, o, m, w, h, 0.5)
            plain = so.candidates_plain(P, o, m, w, h, 0.5)
            assert [(int(y), int(x)) for y, x in zip(ys, xs)] == [(y, x) for y, x, _ in plain], (o, m)
            assert bits64(H).tolist() == bits64([v for _, _, v in plain]).tolist(), (o, m)
            found += len(ys)
    assert found >= 5
    # the sign of the trace, at a few positions of both signs
    ys, xs = np.array([20, 25, 30, 22]), np.array([20, 31, 28, 40])
    lap = so.hessian(I, ys, xs, 15)[1]
    assert [int(v) for v in lap] == [so.hessian_plain(P, int(y), int(x), 15)[1] for y, x in zip(ys, xs)]
    # equal neighbours drop each other: a response map with a 2 x 2 plateau has no candidate
    R = np.zeros((4, 60, 60))
    R[1, 30:32, 30:32] = 50.0
    assert len(so.candidates(R, 0, 1, 60, 60, 1.0)[0]) == 0
    R[1, 30, 30] = 51.0
    assert [int(v[0]) for v in so.candidates(R, 0, 1, 60, 60, 1.0)[:2]] == [30, 30]


def test_orientation_and_descriptor_formulations_agree(img60):
    I, P = so.integral(img60), so.padded(img60)
    ys, xs = np.array([25, 12, 30, 44, 25]), np.array([30, 14, 50, 8, 30])          # three of them with a window that leaves the image
    ls = np.array([5, 7, 9, 17, 65])
    mx, my = so.moments(I, ys, xs, ls)
    bn = so.oo.bins(mx, my)
    v = so.sums(I, ys, xs, ls, bn)
    d = so.normalise(v)
    assert len(set(bn.tolist())) > 1
    for k in range(len(ys)):
        assert (int(mx[k]), int(my[k]), int(bn[k])) == so.orientation_plain(P, int(ys[k]), int(xs[k]), int(ls[k]))
        plain = so.sums_plain(P, int(ys[k]), int(xs[k]), int(ls[k]), int(bn[k]))
        assert [int(c) for c in v[k]] == plain
        assert bits32(d[k]).tolist() == bits32(so.normalise_plain(plain)).tolist()
    # the shift keeps 23 bits of the largest sum; zero sums give zero descriptors
    big = np.zeros((2, 64), np.int64)
    big[0, 3], big[0, 4] = -(2 ** 40 + 12345), 2 ** 39
    t, n2 = so.shifted(big)
    assert t[0, 3] == (-(2 ** 40 + 12345)) >> 18 and t[0, 4] == 2 ** 21 and n2[1] == 0
    assert not so.normalise(big)[1].any() and bits32(so.normalise(big)[0]).tolist() == bits32(so.normalise_plain([int(c) for c in big[0]])).tolist()


def test_table_literals():
    wg = [v for row in so.WG for v in row]
    wd = [v for row in so.WD for v in row]
    assert wg[0] == 65536 and wg[35] == 1200 and wd[0] == 4003 and wd[99] == 1 and len(wg) == 36 and len(wd) == 100
    for path in (os.path.join(ROOT, "include", "sfmba.h"), os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "surf_math.h")):
        text = open(path).read()
        for lit in (wg, wd):
            pat = r"[\s,*/\\]+".join(re.escape(str(v)) for v in lit)
            assert re.search(r"(?<![\d-])" + pat + r"(?!\d)", text), (path, lit[:3])
    assert [so.layer_size(o, i) for o in range(4) for i in range(4)] == [9, 15, 21, 27, 15, 27, 39, 51, 27, 51, 75, 99, 51, 99, 147, 195]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("surf") / "surf_math_host")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tools", "micro", "surf_math_host.hip")])
    return exe


@pytest.mark.parametrize("name", list(sc.CASES))
def test_device_arithmetic_on_the_host_against_the_oracle(host_exe, tmp_path, name):
    """csrc/surf_math.h compiled for the host and run serially over the whole contract equals the oracle on every image the GPU test
    uses: candidates, position, octave, layer, laplacian, H bits, bin, moments, the 64 sums, the 64 descriptor bits, the float fields."""
    img, p, want = sc.image(name), sc.params(name), sc.oracle(name)
    h, w = img.shape[:2]
    path = tmp_path / "image.bin"
    with open(path, "wb") as f:
        f.write(("%d %d %d %d %d %r %d\n" % (w, h, 1 if img.ndim == 2 else 3, p["n_features"], p["n_octaves"],
                                             float(np.float32(p["hessian_threshold"])), p["upright"])).encode())
        f.write(img.tobytes())
    lines = subprocess.check_output([host_exe, str(path)]).decode().splitlines()
    assert [int(v) for v in lines[0].split()[1:]] == want["candidates"].ravel().tolist()
    assert len(lines) - 1 == len(want["kp"])
    for i, line in enumerate(lines[1:]):
        t = line.split()
        k = want["kp"][i]
        assert [int(v) for v in t[0:5]] == [int(k["x"]), int(k["y"]), k["octave"], k["layer"], k["laplacian"]], (name, i)
        assert int(t[5], 16) == int(bits64(want["H"][i])), (name, i)
        assert [int(v) for v in t[6:9]] == [want["bin"][i]] + want["moments"][i].tolist(), (name, i)
        assert [int(v) for v in t[9:73]] == want["sums"][i].tolist(), (name, i)
        assert [int(v, 16) for v in t[73:137]] == bits32(want["desc"][i]).tolist(), (name, i)
        assert [np.float32(v) for v in t[137:142]] == [k["x"], k["y"], k["size"], k["angle"], k["response"]], (name, i)


def test_cases_cover_what_they_claim():
    for name in ("noise_1x1", "none_23x40", "none_40x23", "uniform_60x60"):
        assert len(sc.oracle(name)["kp"]) == 0
    assert len(sc.oracle("noise_24x24")["kp"]) == 1 and len(sc.oracle("noise_25x31")["kp"]) >= 1
    assert sc.oracle("noise_40x40")["candidates"][1:].sum() == 0 and sc.oracle("noise_40x40")["candidates"][0].sum() > 0
    assert sc.oracle("octaves_2_100x90")["candidates"][1].sum() > 0
    assert np.array_equal(sc.oracle("octaves_4_100x90")["candidates"][:2], sc.oracle("octaves_2_100x90")["candidates"])
    assert sc.oracle("blob_300x300")["candidates"][3].sum() > 0 and sc.oracle("texture_300x300")["candidates"][2].sum() > 0
    up, ori = sc.oracle("upright_100x90"), sc.oracle("octaves_3_100x90")
    assert not up["bin"].any() and not up["moments"].any() and ori["bin"].any() and np.array_equal(up["H"], ori["H"])
    # the cut lies inside a group of equal H, and the kept ones are the first in (octave, layer, y, x)
    ties = sc.oracle("ties_150x120")
    full = so.extract(sc.image("ties_150x120"), **dict(sc.params("ties_150x120"), n_features=1000))
    n = len(ties["kp"])
    assert n == 10 and full["H"][n - 1] == full["H"][n] and np.array_equal(full["kp"][:n], ties["kp"])
    keys = [(k["octave"], k["layer"], k["y"], k["x"]) for k in full["kp"][full["H"] == full["H"][n]]]
    assert keys == sorted(keys) and len(keys) > 2
    assert sc.oracle("noise_130x257")["candidates"].sum() > 300                          # the cut applies


def test_bounds_and_norms():
    for name in sc.CASES:
        r = sc.oracle(name)
        if len(r["kp"]) == 0:
            continue
        assert np.abs(r["sums"]).max() < 4.8e14, name
        t, n2 = so.shifted(r["sums"])
        assert n2.max() < 2 ** 52 and np.abs(t).max() < 2 ** 23, name
        norm = np.sqrt((r["desc"].astype(np.float64) ** 2).sum(axis=1))
        assert np.abs(norm[n2 > 0] - 1.0).max() <= 64 * 2.0 ** -24, name


@pytest.mark.parametrize("sigma,L", [(6.0, 27), (9.0, 51)])
def test_blob_on_the_grid_is_found_at_its_centre(sigma, L):
    r = so.extract(sc.blob(200, 200, 100, 100, sigma), n_features=300, n_octaves=3, hessian_threshold=2.0)
    k = r["kp"][0]                                                                   # the strongest
    assert (k["x"], k["y"], k["size"], k["laplacian"]) == (100.0, 100.0, float(L), -1), k


def test_shift_equivariance_is_exact():
    T = sc.to_u8(sc.texture())
    n_oct, step = 3, 4
    (ay, ax), (by, bx), side = (0, 0), (3 * step, 5 * step), 240
    A = so.extract(T[ay:ay + side, ax:ax + side], n_features=100000, n_octaves=n_oct, hessian_threshold=20.0)
    B = so.extract(T[by:by + side, bx:bx + side], n_features=100000, n_octaves=n_oct, hessian_threshold=20.0)
    index = {(int(k["x"]) + bx, int(k["y"]) + by, int(k["octave"]), int(k["layer"])): i for i, k in enumerate(B["kp"])}
    checked = 0
    for i, k in enumerate(A["kp"]):
        o, m = int(k["octave"]), int(k["layer"])
        l = int(k["size"]) // 3
        reach = max(2 ** o + (so.layer_size(o, m + 1) - 1) // 2, int(math.ceil(0.4 * l * 19 * math.sqrt(2.0) / 2)) + (4 * l + 5) // 10,
                    (4 * l * 5 + 5) // 10 + 2 * ((4 * l + 5) // 10))                  # filters, descriptor window, orientation disc
        x, y = int(k["x"]) + ax, int(k["y"]) + ay
        inside = all(cx + reach <= x and x + reach <= cx + side - 1 and cy + reach <= y and y + reach <= cy + side - 1
                     for cy, cx in ((ay, ax), (by, bx)))
        if not inside:
            continue
        j = index.get((x, y, o, m))
        assert j is not None, (x, y, o, m)
        assert bits64(A["H"][i]) == bits64(B["H"][j]) and np.array_equal(bits32(A["desc"][i]), bits32(B["desc"][j])), (x, y, o, m)
        checked += 1
    assert checked >= 50


def _matches(a, b):
    m = ml.match_pair(a["desc"], b["desc"], ratio=ml.RATIO_F32)
    return np.array([e[0] for e in m], np.int64), np.array([e[1] for e in m], np.int64)


@pytest.mark.parametrize("change", ["roll", "rot20"])
def test_descriptors_match_across_a_change(change):
    from scipy.ndimage import map_coordinates
    T = sc.texture()
    p = dict(n_features=300, n_octaves=3, hessian_threshold=20.0)
    a = sc.oracle("texture_300x300")
    if change == "roll":
        b = so.extract(sc.to_u8(np.roll(T, (8, 4), axis=(0, 1))), **p)
        to_b = lambda x, y: ((x + 4) % 300, (y + 8) % 300)
    else:
        th, c = np.deg2rad(20.0), 149.5
        yy, xx = np.mgrid[0:300, 0:300].astype(np.float64)
        sx = c + np.cos(th) * (xx - c) + np.sin(th) * (yy - c)               # source position of every destination pixel
        sy = c - np.sin(th) * (xx - c) + np.cos(th) * (yy - c)
        b = so.extract(sc.to_u8(map_coordinates(T, [sy, sx], order=1, mode="reflect")), **p)
        to_b = lambda x, y: (c + np.cos(th) * (x - c) - np.sin(th) * (y - c), c + np.sin(th) * (x - c) + np.cos(th) * (y - c))
    q, j = _matches(a, b)
    tx, ty = to_b(a["kp"]["x"][q].astype(np.float64), a["kp"]["y"][q].astype(np.float64))
    err = np.hypot(tx - b["kp"]["x"][j], ty - b["kp"]["y"][j])
    right = int((err <= 3.0 * np.maximum(1.0, a["kp"]["size"][q] / 9.0)).sum())
    print("%s: %d kept, %d right" % (change, len(q), right))
    assert len(q) >= 30 and 2 * right >= len(q)


def test_libraries_export_the_symbols():
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    lib = os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "libsfmba_hip.so")
    so_ = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    assert " T sfmba_surf_extract\n" in subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    from sfm_toy_library_amd import capi
    assert "sfmba_surf_extract" in open(capi.__file__).read()
    syms = subprocess.check_output(["nm", "-C", so_]).decode()
    for name in ("sfmba_shim_extract_features_surf", "sfmba_shim_extract_features_surf_batch", "sfmba_shim_run_sfm_typed",
                 "sfmba_shim_extract_features", "sfmba_shim_extract_features_batch", "sfmba_shim_run_sfm", "sfmba_shim_run_sfm_f32"):
        assert " T %s\n" % name in syms, name
    assert " T sfmtoylib::SfM2DFeatureUtilities::extractFeatures(cv::Mat const&)\n" in syms                        # the reference's signature stays
    assert " T sfmtoylib::SfM2DFeatureUtilities::extractFeatures(cv::Mat const&, sfmtoylib::FeatureType)\n" in syms
    assert "std::vector<sfmtoylib::Features, std::allocator<sfmtoylib::Features> >&, sfmtoylib::FeatureType)\n" in syms
    hdr = open(os.path.join(ROOT, "sfm-toy-library_amd", "host", "SfM.h")).read()
    assert "setFeatureType" in hdr and "CONFIRMS EVERY MATCH" in hdr
    assert "SFMBA_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "sfmba.h")).read()


def test_sfmtoy_takes_the_extractor_and_the_merge_distance():
    import __graft_entry__ as ge
    ge.build_host()
    exe = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")
    ok = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert ok.returncode == 0 and "--features orb|surf" in ok.stdout and "--merge-distance" in ok.stdout
    for bad in (["-f", "sift"], ["--features=SURF"], ["-f"], ["-m", "abc"], ["-m", "-1"], ["--merge-distance=nan"], ["-m", "inf"], ["-m"]):
        done = subprocess.run([exe] + bad + ["/nonexistent-directory"], capture_output=True, text=True)
        assert done.returncode == 2 and "usage:" in done.stderr, (bad, done.returncode)
    # usable values get past the argument check: the missing directory is then an ordinary failure (no device is touched before it)
    for good in (["-f", "surf", "-m", "0.25"], ["--features=orb", "--merge-distance=20"], ["-m", "0"]):
        done = subprocess.run([exe, "-d", "4"] + good + ["/nonexistent-directory"], capture_output=True, text=True)
        assert done.returncode == 1, (good, done.returncode, done.stderr)
