"""The CPU restatement of the optical-flow contract (tests/flow_oracle.py; include/sfmba.h, sfmba_flow_track / sfmba_flow_match), held
against itself and against csrc/flow_math.h compiled for the host -- no GPU.

  * the two formulations of the tracker (per-pixel loops with b = sum (T - J) g; shifted copies with b = sum T g - sum J g) and of
    the matcher (a sort per query with a serial set; a vectorised 2-NN with a per-train minimum) agree bit for bit on every case of
    tests/flow_cases.py;
  * tools/micro/flow_math_host.hip -- the header the kernels run, compiled for the host -- agrees bit for bit with the restatement
    on the pyramid, the template, G, the trackable flag, the iterations, every per-level dq, next, status, err and the matches;
  * the cases exercise what they claim (the clamp on both sides, a level-0 trackable point that leaves dst, min_eig exactly on a
    point's value, untrackable 1 x 1 levels, ...);
  * the int32 bounds a lane of the kernel relies on;
  * the new symbols are declared, exported and bound, and both calls refuse what the contract says (the checks come before the device
    is opened);
  * the quality floors of the contract on the multi-scale texture (the device is held equal to the restatement, so it inherits them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flow_cases as fc
import flow_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SFMBA_ERR_INVALID_ARG = 1


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_tracks(got, want):
    (gp, gl), (wp, wl) = got, want
    assert len(gp) == len(wp) and len(gl) == len(wl)
    for p, (g, w) in enumerate(zip(gp, wp)):
        for f, (a, b) in enumerate(zip(g, w)):
            assert same_bits(a, b), (p, ("next", "status", "err", "G", "state")[f])
    for i, (g, w) in enumerate(zip(gl, wl)):
        assert (g is None) == (w is None), i
        for l, (a, b) in enumerate(zip(g or [], w or [])):
            assert same_bits(a, b), (i, l)
    return True


# ---- the restatement against itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.TRACK_CASES))
def test_two_formulations_of_the_tracker_agree(name):
    c = fc.case(name)
    assert same_tracks(fo.track_loops(c["images"], c["pairs"], c["points"], **c["params"]), fc.oracle(name))


@pytest.mark.parametrize("name", list(fc.MATCH_CASES))
def test_two_formulations_of_the_matcher_agree(name):
    c = fc.match_case(name)
    got = fo.match_serial(c["keypoints"], c["pairs"], c["tracked"], **c["params"])
    for a, b in zip(got, fc.match_oracle(name)):
        assert same_bits(a, b), name


def test_track_cases_exercise_what_they_claim():
    for name in ("size_1x1", "size_1x7", "constant_src"):
        out, _ = fc.oracle(name)
        first = out[0]
        assert not first[1].any() and not first[2].any() and not first[4][:, :, 0].any(), name     # nothing trackable: status 0, err 0
        assert same_bits(first[0], np.asarray(fc.case(name)["points"][0], np.float32)), name       # ... and next = the point itself
    out, levels = fc.oracle("levels_8_on_5x3")
    assert [a.shape for a in levels[0]] == [(3, 5), (2, 3), (1, 2)] + [(1, 1)] * 5
    assert not out[0][4][:, 3:, 0].any() and out[0][4][:, 0, 0].any()                              # 1 x 1 levels (and 1 x 2) are untrackable
    out, _ = fc.oracle("edges")
    nxt, status, err, G, state = out[0]
    assert status[:4].all() or state[:4, 0, 0].all()                                                # the corners are trackable at level 0
    assert not status[10:13].any() and same_bits(nxt[11], np.asarray([3e38, 3e38], np.float32))     # far outside: saturated centres
    assert status[13] == 1
    out, _ = fc.oracle("leaves_dst")
    assert out[0][4][0, 0, 0] == 1 and out[0][1][0] == 0 and out[0][2][0] > 0                       # trackable at level 0, outside dst, err still formed
    assert out[0][1][1] == 1 and out[1][1][0] == 1
    on, above = fc.oracle("min_eig_on")[0][0], fc.oracle("min_eig_above")[0][0]
    Gxx, Gyy, Gxy = (int(v) for v in on[3][0, 0])
    assert (Gxx, Gyy, Gxy) == (9 * 8 * 64 * 64, 81 * 32 * 32, 0) and fo.lam_of(Gxx, Gyy, Gxy) == 81.0 * 1024.0
    assert on[4][0, 0, 0] == 1 and on[1][0] == 1 and above[4][0, 0, 0] == 0 and above[1][0] == 0
    out, _ = fc.oracle("max_iters_1")
    assert (out[0][4][:, :, 1] <= 1).all() and out[0][4][:, :, 1].any()
    out, _ = fc.oracle("max_iters_64")
    assert (out[0][4][:, 0, 1] == 64).any()                                                         # a two-cycle runs to the limit: accepted
    out, _ = fc.oracle("src_is_dst")
    st = out[0][4]
    assert not st[:, :, 2:].any() and (st[:, :, 1] == st[:, :, 0]).all() and st[:, 0, 0].any()      # dq = 0 in one iteration per trackable level
    assert not out[0][2].any()
    assert [len(p[0]) for p in fc.oracle("counts")[0]] == [0, 1, 63, 64, 65]
    c = fc.case("bgr")
    assert c["images"][0].ndim == 3 and (c["images"][0][..., 0] != c["images"][0][..., 2]).any()
    for name in ("size_33x17_r4_l3", "size_70x45_r10_l4", "size_64x48_r7_defaults"):
        o = fc.oracle(name)[0][0]
        assert o[1].sum() >= 0.5 * len(o[1]) and o[4][:, :, 3].any(), name


def test_match_cases_exercise_what_they_claim():
    rows = lambda name: [tuple(int(v) for v in r) for r in zip(*fc.match_oracle(name)[1:3])]
    assert rows("on_radius") == [(0, 0)] and fc.match_oracle("on_radius")[3].tolist() == [2.0]
    assert rows("one_two_three_in_range") == [(0, 0), (1, 3), (2, 5)]       # three, two and one in range; none; a tie of two
    assert rows("tie_dropped") == [] and rows("tie_lower_j") == [(0, 0)]
    assert rows("coincident") == [(1, 2)]
    assert rows("three_on_one") == [(0, 1), (1, 0)]
    assert rows("err_on_max") == [(1, 1)]
    assert rows("status_0") == [(1, 1)]
    assert rows("empty_train") == [(0, 0)] and fc.match_oracle("empty_train")[0].tolist() == [0, 0, 1]
    assert fc.match_oracle("empty_queries")[0].tolist() == [0, 0, 1, 1]
    for name in ("kp_255", "kp_256", "kp_257", "kp_600"):
        assert 50 < len(fc.match_oracle(name)[1]) < 300, name


def test_lane_partials_fit_int32():
    # a lane owns at most ceil(441 / 64) = 7 window pixels; |gx|, |gy|, |D| <= 4080
    assert -(-441 // 64) == 7 and 7 * 4080 * 4080 < 2 ** 31 and 441 * 4080 * 4080 == 7341062400 < 2 ** 33
    assert "7341062400" in open(os.path.join(ROOT, "include", "sfmba.h")).read()
    assert (16 * 16 * 255 + 8) >> 4 == 4080 and (256 * 255 + 128) >> 8 == 255
    # a saturated centre plus the largest displacement plus the window stays inside int32
    assert fo.CENTRE_LIMIT + 64 * 160 * 255 + 16 * 11 < 2 ** 31


# ---- csrc/flow_math.h on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("flow") / "flow_math_host")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tools", "micro", "flow_math_host.hip")])
    return exe


def run(host_exe, mode, tmp_path, text):
    path = tmp_path / (mode + ".txt")
    path.write_text(text)
    return subprocess.check_output([host_exe, mode, str(path)]).decode().splitlines()


def image_text(img):
    g = fo.gray(img)
    return "%d %d\n%s\n" % (g.shape[1], g.shape[0], " ".join(str(int(v)) for v in g.reshape(-1)))


def bits32(v):
    return "%08x" % int(np.asarray(v, np.float32).view(np.uint32))


def test_host_pyramid_matches(host_exe, tmp_path):
    rng = np.random.default_rng(1)
    for k, (w, h, L) in enumerate(((1, 1, 3), (1, 7, 4), (2, 2, 2), (5, 3, 8), (33, 17, 4), (70, 45, 5))):
        img = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
        if k == 4:
            img[:] = 255                                                             # the rounding at the top of the range
        out = run(host_exe, "pyramid", tmp_path, "%d %d %d\n%s\n" % (w, h, L, " ".join(str(int(v)) for v in img.reshape(-1))))
        want = fo.pyramid(img, L)
        assert len(out) == L
        for l, line in enumerate(out):
            t = line.split()
            assert t[0] == "V" and [int(v) for v in t[1:4]] == [l, want[l].shape[1], want[l].shape[0]]
            assert [int(v) for v in t[4:]] == want[l].reshape(-1).tolist(), (w, h, l)


def test_host_template_matches(host_exe, tmp_path):
    img = fc.texture(40, 30, seed=3)
    rows = [(0, 0, 1), (16 * 39, 16 * 29, 4), (-200, 1000, 3), (317, 211, 10), (-(1 << 28), 1 << 28, 2), (16 * 39 + 1, -1, 1), (100, 100, 7)]
    out = run(host_exe, "template", tmp_path, image_text(img) + "".join("%d %d %d\n" % r for r in rows))
    assert len(out) == len(rows)
    I = fo.gray(img)
    for (cx, cy, r), line in zip(rows, out):
        assert [int(v) for v in line.split()] == fo.sample_block(I, cx, cy, r + 1).reshape(-1).tolist(), (cx, cy, r)


@pytest.mark.parametrize("name", list(fc.TRACK_CASES))
def test_host_track_matches(host_exe, tmp_path, name):
    c, (want, _) = fc.case(name), fc.oracle(name)
    prm = c["params"]
    head = "%d %d %d %d %s\n" % (len(c["images"]), prm["n_levels"], prm["radius"], prm["max_iters"], float(np.float32(prm["min_eig"])).hex())
    head += "".join(image_text(im) for im in c["images"])
    for p, ((s, d), pts) in enumerate(zip(c["pairs"], c["points"])):
        pts = np.asarray(pts, np.float32).reshape(-1, 2)
        text = head + "%d %d %d\n" % (s, d, len(pts)) + "".join("%s %s\n" % (float(x).hex(), float(y).hex()) for x, y in pts)
        out = run(host_exe, "track", tmp_path, text)
        L = prm["n_levels"]
        assert len(out) == len(pts) * (1 + L)
        nxt, status, err, G, state = want[p]
        for q in range(len(pts)):
            assert out[q * (1 + L)].split() == ["P", bits32(nxt[q, 0]), bits32(nxt[q, 1]), str(int(status[q])), bits32(err[q])], (name, p, q)
            for l in range(L):
                got = [int(v) for v in out[q * (1 + L) + 1 + l].split()[1:]]
                assert got == [l] + G[q, l].tolist() + state[q, l].tolist(), (name, p, q, l)


@pytest.mark.parametrize("name", list(fc.MATCH_CASES))
def test_host_match_matches(host_exe, tmp_path, name):
    c = fc.match_case(name)
    prm = c["params"]
    ptr, qi, ti, di = fc.match_oracle(name)
    for p, ((_, d), t) in enumerate(zip(c["pairs"], c["tracked"])):
        kp = c["keypoints"][d]
        text = "%d %d %s %s %s\n" % (len(kp), len(t[0]), float(np.float32(prm["max_err"])).hex(), float(np.float32(prm["radius"])).hex(),
                                     float(prm["ratio"]).hex())
        text += "".join("%s %s\n" % (float(x).hex(), float(y).hex()) for x, y in kp)
        text += "".join("%s %s %d %s\n" % (float(x).hex(), float(y).hex(), s, float(e).hex()) for (x, y), s, e in zip(*t))
        out = [line.split() for line in run(host_exe, "match", tmp_path, text)]
        a, b = int(ptr[p]), int(ptr[p + 1])
        assert out == [["M", str(int(q)), str(int(j)), bits32(dd)] for q, j, dd in zip(qi[a:b], ti[a:b], di[a:b])], (name, p)


# ---- the public layers ------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build_hip()
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    lib = os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "libsfmba_hip.so")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    from sfm_toy_library_amd import capi
    for name in ("sfmba_flow_track", "sfmba_flow_match"):
        assert "SFMBA_API int %s(" % name in header
        assert " T %s\n" % name in exported
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    assert callable(capi.flow_track) and callable(capi.flow_match)
    assert capi.lib().sfmba_abi_version() == 6


def test_track_refuses_what_the_contract_says():
    import __graft_entry__ as ge
    ge.build_hip()
    from sfm_toy_library_amd import capi
    im = [fc.texture(12, 9, seed=1), fc.texture(12, 9, seed=2)]
    good = dict(pair_src=[0, 1], pair_dst=[1, 1], pt_ptr=[0, 1, 3], pts=[(1, 1), (2, 2), (3, 3)])

    def refused(images=im, **over):
        rc, nxt, status, err = fc.raw_track(capi, images, **dict(good, **over))
        untouched = (nxt == 7.0).all() and (status == 9).all() and (err == 7.0).all()        # nothing written
        return rc == SFMBA_ERR_INVALID_ARG and untouched

    nan, inf = float("nan"), float("inf")
    for over in (dict(n_levels=0), dict(n_levels=9), dict(radius=0), dict(radius=11), dict(max_iters=0), dict(max_iters=65),
                 dict(min_eig=-0.5), dict(min_eig=nan), dict(min_eig=inf),
                 dict(pair_src=[2, 1]), dict(pair_src=[-1, 1]), dict(pair_dst=[1, 2]), dict(pair_dst=[1, -1]),
                 dict(pt_ptr=[1, 1, 3]), dict(pt_ptr=[0, 2, 1]), dict(pt_ptr=[0, 1, 1 << 31]),
                 dict(pts=[(1, 1), (nan, 2), (3, 3)]), dict(pts=[(1, 1), (2, 2), (3, inf)]), dict(pts=[(-inf, 1), (2, 2), (3, 3)]),
                 dict(channels=2), dict(channels=0), dict(img_ptr=[0, 108, 215]), dict(img_ptr=[1, 109, 217])):
        assert refused(**over), over
    assert "flow_track" in (capi.lib().sfmba_last_error() or b"").decode() or "img_ptr" in (capi.lib().sfmba_last_error() or b"").decode()
    rc, *_ = fc.raw_track(capi, im, **dict(good, min_eig=nan))
    assert rc == SFMBA_ERR_INVALID_ARG and "min_eig" in capi.lib().sfmba_last_error().decode()      # the message comes through


def test_match_refuses_what_the_contract_says():
    import __graft_entry__ as ge
    ge.build_hip()
    from sfm_toy_library_amd import capi
    good = dict(kp_ptr=[0, 1, 3], kp=[(1, 1), (2, 2), (3, 3)], pair_dst=[1, 0], pt_ptr=[0, 2, 3], nxt=[(2, 2), (3, 3), (1, 1)],
                status=[1, 1, 1], err=[0, 0, 0])

    def refused(**over):
        rc, ptr, q, t, d, total = fc.raw_match(capi, **dict(good, **over))
        untouched = (ptr == -7).all() and (q == -7).all() and (t == -7).all() and (d == -7.0).all() and total == -7
        return rc == SFMBA_ERR_INVALID_ARG and untouched

    nan, inf = float("nan"), float("inf")
    for over in (dict(max_err=nan), dict(max_err=inf), dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf),
                 dict(ratio=0.0), dict(ratio=-0.7), dict(ratio=nan), dict(ratio=inf), dict(pair_dst=[2, 0]), dict(pair_dst=[1, -1]),
                 dict(pt_ptr=[1, 2, 3]), dict(pt_ptr=[0, 3, 2]), dict(pt_ptr=[0, 2, 1 << 31]), dict(kp_ptr=[1, 1, 3]), dict(kp_ptr=[0, 4, 3]),
                 dict(kp_ptr=[0, 1 << 22, (1 << 22) + 2]), dict(cap=-1)):
        assert refused(**over), over
    rc, *_ = fc.raw_match(capi, **dict(good, ratio=nan))
    assert rc == SFMBA_ERR_INVALID_ARG and "ratio" in capi.lib().sfmba_last_error().decode()


def test_sfmtoy_usage_names_the_matcher_switch_and_the_shim_has_the_drivers():
    import __graft_entry__ as ge
    ge.build_host()
    exe = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")
    ok = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert ok.returncode == 0 and "-M, --matcher" in ok.stdout and "-w, --flow-window" in ok.stdout
    for args in (["-M", "bogus"], ["-w", "-1"], ["-w", "1.5"], ["--matcher"]):              # a usage error, before anything is read
        done = subprocess.run([exe] + args + ["/nonexistent-directory"], capture_output=True, text=True)
        assert done.returncode == 2, (args, done.returncode, done.stderr)
    # good values get past the argument check: the missing directory is then an ordinary failure, before any device
    for args in (["-M", "flow"], ["--matcher=flow", "-w", "2"], ["-M", "descriptors", "--flow-window=0"]):
        done = subprocess.run([exe] + args + ["/nonexistent-directory"], capture_output=True, text=True)
        assert done.returncode == 1, (args, done.returncode, done.stderr)
    so_ = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    syms = subprocess.check_output(["nm", "-C", so_]).decode()
    for name in ("sfmba_shim_flow_match_matrix", "sfmba_shim_run_sfm_matcher", "sfmba_shim_flow_refusal"):
        assert " T %s\n" % name in syms, name
    assert "sfmtoylib::SfMFeatureMatching::createFlowMatchMatrix(" in syms


def test_the_flow_matcher_refuses_without_pixels():
    import __graft_entry__ as ge
    ge.build_host()
    shim = C.CDLL(os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so"))
    for what in (0, 1):                      # MATCHER_FLOW after setFeatures; a negative pair window: ERROR, no device touched
        assert shim.sfmba_shim_flow_refusal(what) == 1, what


# ---- quality floors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(3.3, -2.6), (11.5, 7.25)])
def test_quality_floors_on_the_multi_scale_texture(shift):
    """Prototype figures for this configuration (200 x 160, 60 points at least 25 px from the border, L = 3, r = 7, max_iters 20,
    min_eig 1): 60 of 60 within 0.05 px at (3.3, -2.6) and 60 of 60 exact at (11.5, 7.25).  The floor is 57 of 60 within 0.125 px with
    status 1 and err < 12."""
    images, pts = fc.floor_scene(shift)
    (nxt, status, err, G, state), = fo.track_vec(images, [(0, 1)], [pts], n_levels=3, radius=7, max_iters=20, min_eig=1.0)[0]
    off = np.abs(nxt.astype(np.float64) - (pts.astype(np.float64) + np.asarray(shift)))
    good = (off.max(axis=1) <= 0.125) & (status == 1) & (err < 12)
    print("shift %s: %d of %d within 0.125 px with status 1 and err < 12; worst good %.4f px, median err %.3f, iterations at level 0: max %d"
          % (shift, good.sum(), len(pts), off.max(axis=1)[good].max(), float(np.median(err)), state[:, 0, 1].max()))
    assert len(pts) == 60 and good.sum() >= 57


def test_an_identical_pair_gives_zero_flow_in_one_iteration_per_level():
    images, pts = fc.floor_scene((0.0, 0.0))
    assert same_bits(images[0], images[1])
    (nxt, status, err, G, state), = fo.track_vec(images, [(0, 1)], [pts], n_levels=3, radius=7, max_iters=20, min_eig=1.0)[0]
    assert state[:, :, 0].all() and (state[:, :, 1] == 1).all() and not state[:, :, 2:].any()
    assert same_bits(nxt, pts) and status.all() and not err.any()
