"""CPU-side checks of the feature extractor's contract (include/sfmba.h, sfmba_orb_extract): no GPU needed.

  formulations    the vectorised and the plain per-pixel statement of every stage of tests/orb_oracle.py agree exactly on 40 x 40 noise
  resample        the fixed-point resampling equals a fractions.Fraction evaluation of the same formula
  pattern         256 pairs within radius^2 169, rotated points within |13|; the 60 literals of the header are numpy's cos / sin rounded
  quotas          (5000, 1.2, 8) -> 1086 905 754 628 524 436 364 303
  host program    tools/micro/orb_math_host.hip (csrc/orb_math.h, the arithmetic the kernels run, compiled for the host) equals the
                  oracle bit for bit on every image of the GPU test
  matching        the descriptors do their job: oracle features of renderings of one scene at 640 x 480, 1000 features, identity
                  against three warps, matched by match_oracle with the (double)0.8f ratio; a kept match is right when it lies
                  within 3 px of the true correspondence.  Floors: 100 right ones and half of the kept ones.  Measured:
                      shift (15, -9)          754 kept, 730 right (96.8 %)
                      17 degrees              403 kept, 357 right (88.6 %)
                      40 degrees x 1.3        364 kept, 304 right (83.5 %)
  symbols         the libraries export sfmba_orb_extract and the two shim drivers"""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import match_oracle as mo
import orb_cases as oc
import orb_oracle as oo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def img40():
    return np.random.default_rng(40).integers(0, 256, (40, 40), dtype=np.uint8)


def test_gray_formulations_agree():
    img = np.random.default_rng(41).integers(0, 256, (40, 40, 3), dtype=np.uint8)
    assert np.array_equal(oo.gray(img), oo.gray_plain(img))
    assert np.array_equal(oo.gray(np.full((2, 2, 3), 255, np.uint8)), np.full((2, 2), 255))       # the weights sum to 2^14


def test_resample_formulations_agree_and_equal_fractions(img40):
    for wl, hl in ((33, 33), (40, 37), (21, 29), (1, 1), (40, 40)):
        a = oo.resample_level(img40, wl, hl)
        assert np.array_equal(a, oo.resample_plain(img40, wl, hl))
        # the same formula in exact rational arithmetic: f is the rounded 11-bit fraction of the source coordinate (d + 1/2) n / m - 1/2
        for y in range(hl):
            cy = Fraction((2 * y + 1) * 40 - hl, 2 * hl)
            y0 = cy.numerator // cy.denominator
            fy = int((cy - y0) * 2048 + Fraction(1, 2))                      # floor(t 2048 + 1/2)
            y1 = min(y0 + 1, 39)
            for x in range(wl):
                cx = Fraction((2 * x + 1) * 40 - wl, 2 * wl)
                x0 = cx.numerator // cx.denominator
                fx = int((cx - x0) * 2048 + Fraction(1, 2))
                x1 = min(x0 + 1, 39)
                top = int(img40[y0, x0]) * (2048 - fx) + int(img40[y0, x1]) * fx
                bot = int(img40[y1, x0]) * (2048 - fx) + int(img40[y1, x1]) * fx
                v = Fraction(top * (2048 - fy) + bot * fy, 1 << 22) + Fraction(1, 2)
                assert a[y, x] == v.numerator // v.denominator, (wl, hl, x, y)
    assert np.array_equal(oo.resample_level(img40, 40, 40), img40)               # the identity resampling changes nothing


def test_score_formulations_agree(img40):
    for thr in (1, 20, 60, 254):
        S = oo.score_map(img40, thr)
        assert not S[:3].any() and not S[-3:].any() and not S[:, :3].any() and not S[:, -3:].any()
        for y in range(3, 37):
            for x in range(3, 37):
                assert S[y, x] == oo.score_plain(img40, x, y, thr), (thr, x, y)
    assert oo.score_map(img40, 20).max() > 20


def test_candidate_formulations_agree(img40):
    S = oo.score_map(img40, 20)
    for edge in (4, 8):
        ys, xs = oo.candidates(S, edge)
        py, px = oo.candidates_plain(S, edge)
        assert len(ys) > 0 and np.array_equal(ys, py) and np.array_equal(xs, px)
    flat = np.zeros((40, 40), np.int64)
    flat[10:12, 10:12] = 50                                                       # equal neighbours drop each other
    assert len(oo.candidates(flat, 4)[0]) == 0 and len(oo.candidates_plain(flat, 4)[0]) == 0
    assert len(oo.candidates(S)[0]) == 0                                          # 40 <= 62: no admissible pixel at the contract's border


def test_harris_orientation_smooth_descriptor_formulations_agree(img40):
    ys, xs = np.array([16, 17, 20, 23, 23]), np.array([16, 22, 19, 16, 23])
    R = oo.harris(img40, ys, xs)
    m10, m01 = oo.moments(img40, ys, xs)
    bn = oo.bins(m10, m01)
    B = oo.smooth(img40)
    D = oo.describe(B, ys, xs, bn)
    for i, (y, x) in enumerate(zip(ys.tolist(), xs.tolist())):
        assert R[i] == oo.harris_plain(img40, x, y)
        assert (m10[i], m01[i], bn[i]) == oo.orientation_plain(img40, x, y)
        assert np.array_equal(D[i], oo.describe_plain(img40, x, y, int(bn[i])))
    for y in range(3, 37):
        for x in range(3, 37):
            assert B[y, x] == oo.smooth_plain(img40, x, y)
    assert np.array_equal(oo.smooth(np.full((9, 9), 200, np.uint8))[3:6, 3:6], np.full((3, 3), 200))   # the taps sum to 256
    # ties between bins go to the lowest one; the order of selection is (R descending, y, x)
    assert oo.bins(np.array([0]), np.array([0]))[0] == 0
    keep = oo.select(np.array([5, 9, 5, 9]), np.array([3, 2, 1, 2]), np.array([0, 7, 9, 4]), 3)
    assert keep.tolist() == [3, 1, 2]


def test_pattern_and_literals():
    base = oo.base_pattern()
    assert len(base) == 256
    for x0, y0, x1, y1 in base:
        assert x0 * x0 + y0 * y0 <= 169 and x1 * x1 + y1 * y1 <= 169 and (x0, y0) != (x1, y1)
    T = oo.pattern_table().astype(int)
    assert T.shape == (30, 256, 4) and np.abs(T).max() <= 13
    assert max((T[..., 0] ** 2 + T[..., 1] ** 2).max(), (T[..., 2] ** 2 + T[..., 3] ** 2).max()) <= 173
    assert np.array_equal(T[0], np.array(base))                                   # bin 0 is the identity
    k = np.arange(30)
    cos = np.floor(16384 * np.cos(2 * np.pi * k / 30) + 0.5).astype(int).tolist()
    sin = np.floor(16384 * np.sin(2 * np.pi * k / 30) + 0.5).astype(int).tolist()
    assert cos == oo.COS and sin == oo.SIN
    for path in (os.path.join(ROOT, "include", "sfmba.h"), os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "orb_math.h")):
        text = open(path).read()
        for lit in (cos, sin):
            pat = r"[\s,*\\]+".join(re.escape(str(v)) for v in lit)
            assert re.search(r"(?<![\d-])" + pat + r"(?!\d)", text), (path, lit[:3])


def test_quotas():
    q = oo.quotas(5000, 1.2, 8)
    assert q == [1086, 905, 754, 628, 524, 436, 364, 303] and sum(q) == 5000
    assert oo.quotas(500, 1.2, 1) == [500] and oo.quotas(1, 1.2, 8) == [0] * 7 + [1]
    assert all(sum(oo.quotas(n, s, l)) >= n for n in (1, 7, 100, 5000) for s in (1.2, 2.0, 1.05) for l in (1, 2, 8, 12))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("orb") / "orb_math_host")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tools", "micro", "orb_math_host.hip")])
    return exe


@pytest.mark.parametrize("name", list(oc.CASES))
def test_device_arithmetic_on_the_host_against_the_oracle(host_exe, tmp_path, name):
    """csrc/orb_math.h compiled for the host and run serially over the whole contract: level coordinates, octave, R, bin, the 32
    descriptor bytes and the six key point fields equal the oracle's on every image the GPU test uses."""
    img, p, want = oc.image(name), oc.params(name), oc.oracle(name)
    h, w = img.shape[:2]
    path = tmp_path / "image.bin"
    with open(path, "wb") as f:
        f.write(("%d %d %d %d %r %d %d\n" % (w, h, 1 if img.ndim == 2 else 3, p["n_features"], float(np.float32(p["scale_factor"])),
                                             p["n_levels"], p["fast_threshold"])).encode())
        f.write(img.tobytes())
    lines = subprocess.check_output([host_exe, str(path)]).decode().splitlines()
    assert [int(v) for v in lines[0].split()[1:]] == want["candidates"].tolist()
    assert len(lines) - 1 == len(want["kp"])
    for i, line in enumerate(lines[1:]):
        t = line.split()
        k = want["kp"][i]
        assert [int(t[0]), int(t[1])] == want["level_xy"][i].tolist() and int(t[2]) == k["octave"], (name, i)
        assert int(t[3]) == want["harris"][i] and int(t[4]) == want["bin"][i], (name, i)
        assert bytes.fromhex(t[5]) == want["desc"][i].tobytes(), (name, i)
        assert [np.float32(v) for v in t[6:11]] == [k["x"], k["y"], k["size"], k["angle"], k["response"]], (name, i)


def test_cases_cover_what_they_claim():
    assert len(oc.oracle("one_pixel_63x63")["kp"]) == 1
    assert len(oc.oracle("none_62x200")["kp"]) == 0 and len(oc.oracle("none_200x62")["kp"]) == 0 and len(oc.oracle("uniform_100x100")["kp"]) == 0
    assert oc.oracle("noise_256x256")["candidates"][0] > 10 * oo.quotas(500, 1.2, 8)[0]        # dense in corners: the quota cuts
    assert len(oc.oracle("render_1024x768")["kp"]) > 3000


@pytest.mark.parametrize("view", ["shift", "rot17", "rot40"])
def test_descriptors_match_across_warps(view):
    from sfm_toy_library_amd import synthetic as sy
    W, H = 640, 480
    a = oc.oracle("render_640x480")
    b = oc.oracle("render_640x480_rot17") if view == "rot17" else oo.extract(oc.render(W, H, view), **oc.params("render_640x480"))
    m = mo.match_pair(a["desc"], b["desc"], ratio=mo.RATIO_F32, knn=mo.knn_keys)
    q, j = np.array([e[0] for e in m]), np.array([e[1] for e in m])
    pa = np.stack([a["kp"]["x"][q], a["kp"]["y"][q]], axis=1).astype(np.float64)
    pb = np.stack([b["kp"]["x"][j], b["kp"]["y"][j]], axis=1).astype(np.float64)
    true = sy.orb_scene_to_view(sy.orb_view_to_scene(pa, W, H, *oc.VIEWS["identity"]), W, H, *oc.VIEWS[view])
    right = int((np.hypot(*(true - pb).T) <= 3.0).sum())
    print("%s: %d kept, %d right (%.1f %%)" % (view, len(m), right, 100.0 * right / max(len(m), 1)))
    assert right >= 100 and 2 * right >= len(m)


def test_libraries_export_the_symbols():
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    lib = os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "libsfmba_hip.so")
    so = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    assert " T sfmba_orb_extract\n" in subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    syms = subprocess.check_output(["nm", "-C", so]).decode()
    assert " T sfmba_shim_extract_features\n" in syms and " T sfmba_shim_extract_features_batch\n" in syms
    assert " T sfmtoylib::SfM2DFeatureUtilities::extractFeatures(cv::Mat const&)\n" in syms
    assert " T sfmtoylib::SfMFeatureExtraction::extractFeatures(std::vector<cv::Mat, std::allocator<cv::Mat> > const&, " in syms
    hdr = open(os.path.join(ROOT, "sfm-toy-library_amd", "host", "SfM2DFeatureUtilities.h")).read()
    assert "stays on the reference's OpenCV path" not in hdr
