"""The contract of sfmba_depth_cost_volume / sfmba_sgm_aggregate / sfmba_depth_sweep_sgm without a GPU (include/sfmba.h,
tests/sgm_oracle.py):

  * every stage of the restatement is stated twice and the two statements agree on every named case (tests/sgm_cases.py);
  * tools/micro/sgm_math_host.hip -- the header the kernels run, compiled for the host with the address and undefined-behaviour
    sanitizers as a program of its own -- agrees with the restatement on every intermediate: q, c, each L_r, m, S, k*, best, second,
    den, delta, depth, score;
  * identities of the restatement: no penalties, a transposed volume, a constant volume;
  * the bounds the header states;
  * quality floors on the corner scene with a band without texture."""
import os
import subprocess

import numpy as np
import pytest

import depth_cases as dc
import depth_oracle as do
import sfm_scene
import sgm_cases as sc
import sgm_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def planes_of(D):
    return do.planes(dc.Z_NEAR, dc.Z_FAR, D)


# ---- the two statements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_two_statements_agree(name):
    c = sc.case(name)
    prm = (c["p1"], c["p2"], c["n_paths"], c["invalid_cost"])
    a, b = so.aggregate_loop(c["vol"], *prm), so.aggregate_lines(c["vol"], *prm)
    assert len(a["L"]) == c["n_paths"]
    for r in range(c["n_paths"]):
        assert same_bits(a["L"][r], b["L"][r]) and same_bits(a["m"][r], b["m"][r]), (name, r)
    assert same_bits(a["sums"], b["sums"]) and same_bits(b["sums"], sc.oracle(name)["sums"])
    s1, s2 = so.select_loop(a["sums"]), so.select(a["sums"])
    for x, y, f in zip(s1, s2, ("plane", "best", "second")):
        assert same_bits(x, y) and same_bits(y, sc.oracle(name)[f]), (name, f)
    wf, step = planes_of(c["vol"].shape[2])
    for u in (0, 5, 100):
        f1, f2 = so.finish_loop(c["vol"], a["sums"], *s1, wf, step, u), so.finish(c["vol"], a["sums"], *s2, wf, step, u)
        for k in f1:
            assert same_bits(f1[k], f2[k]), (name, u, k)


def test_cases_exercise_what_they_claim():
    L_max = lambda n: max(int(L.max()) for L in so.aggregate_lines(*[sc.case(n)[k] for k in ("vol", "p1", "p2", "n_paths", "invalid_cost")])["L"])
    assert L_max("ramp_equal_1023") == L_max("ramp_zero_1023") == 254 + 1023 and L_max("ramp_equal_200") == 254 + 200
    assert 9000 < int(sc.oracle("ramp_equal_1023")["sums"].max()) <= 8 * 1277 == 10216  # S comes close to its bound
    assert (sc.oracle("all_254")["plane"] == 0).all() and (sc.oracle("all_sentinel")["plane"] == 0).all()
    assert (sc.oracle("all_sentinel")["sums"] == 8 * 127).all()
    for name in ("two_minima_d65", "two_minima_d256"):                                    # equal minima: the lower plane
        assert (sc.oracle(name)["plane"] == 1).all()
    assert (sc.oracle("edge_low")["plane"] == 0).all()
    assert (sc.oracle("edge_high_d65")["plane"] == 64).all() and (sc.oracle("edge_high_d256")["plane"] == 255).all()
    assert (sc.oracle("second_absent_d3")["second"] == so.NO_SECOND).all() and (sc.oracle("second_absent_d3")["plane"] == 1).all()
    assert (sc.oracle("second_absent_d2")["second"] == so.NO_SECOND).all() and len(np.unique(sc.oracle("second_absent_d2")["plane"])) == 2
    o = sc.oracle("70x45_d64_p4")
    assert len(np.unique(o["plane"])) > 20 and (o["second"] != so.NO_SECOND).all()
    assert (sc.case("invalid_cost_254")["vol"] == so.SENTINEL).any() and (sc.case("invalid_cost_0")["vol"] == so.SENTINEL).any()
    sizes = {c()["vol"].shape[:2][::-1] for c in sc.CASES.values()}
    assert {(1, 1), (1, 7), (7, 1), (2, 2), (17, 33), (33, 17), (70, 45)} <= sizes
    assert {2, 3, 63, 64, 65, 129, 256} <= {sc.case(n)["vol"].shape[2] for n in sc.CASES}
    assert {(0, 0), (0, 1023)} <= {(sc.case(n)["p1"], sc.case(n)["p2"]) for n in sc.CASES}
    assert any(sc.case(n)["p1"] == sc.case(n)["p2"] > 0 for n in sc.CASES) and {4, 8} == {sc.case(n)["n_paths"] for n in sc.CASES}
    c, sgm, u, agg = sc.uniqueness_case()
    assert 1 <= u <= 99


def test_every_pixel_lies_on_one_line_of_every_direction():
    for w, h in ((1, 1), (1, 7), (7, 1), (5, 3), (3, 5)):
        c = np.arange(h * w * 2, dtype=np.int64).reshape(h, w, 2)
        for dx, dy in so.DIRECTIONS:
            L, M = so.path_loop(c, dx, dy, 0, 0)
            first = M == -1
            ys, xs = np.mgrid[0:h, 0:w]
            assert (first == ~((xs - dx >= 0) & (xs - dx < w) & (ys - dy >= 0) & (ys - dy < h))).all()
            assert (L[first] == c[first]).all()


# ---- the volume -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.VOLUME_SCENES)
def test_volume_two_statements_and_the_sweep(name):
    c, o = dc.case(name), dc.oracle(name)
    p = sc.sweep_params(c)
    vol, wf, step = sc.volume_oracle(name)
    direct, _, _ = so.cost_volume_direct(c["images"], c["K"], c["P"], c["jobs"][0], **p)
    assert same_bits(vol, direct)
    assert (vol[~o["part"]] == so.SENTINEL).all()
    # per pixel against depth_oracle.sweep: a plane was valid iff the volume holds a cost; the winner's cost is the smallest
    # entry, at the lowest plane unless two fp64 costs share a byte; and the entry is the quantised score (a float32 of C_k*)
    has = (vol != so.SENTINEL).any(2)
    assert (has == (o["plane"] >= 0)).all()
    k = np.clip(o["plane"].astype(np.int64), 0, None)
    q = np.take_along_axis(vol.astype(np.int64), k[..., None], 2)[..., 0]
    low = np.where(vol == so.SENTINEL, 999, vol.astype(np.int64)).min(2)
    assert (q[has] == low[has]).all()
    assert (q[has] == so.quantise(o["cost"])[has]).all()
    assert (np.abs((1.0 - q[has] / 127.0) - o["score"][has].astype(np.float64)) <= 0.5 / 127.0 + 1e-6).all()
    assert (wf, step) == (o["wf"], o["step"])


def test_quantise_ends_and_halves():
    C = np.array([1.0, -1.0, 0.0, 1.0 - 1.0 / 127.0, 1.0 - 0.51 / 127.0, 1.0 - 0.49 / 127.0, 1.0 + 2.0 ** -52, -1.0 - 2.0 ** -52])
    assert so.quantise(C).tolist() == [0, 254, 127, 1, 1, 0, 0, 254]


# ---- csrc/sgm_math.h on the host, under the sanitizers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("sgm") / "sgm_math_host")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tools", "micro", "sgm_math_host.hip")])
    return exe


def run(host_exe, mode, tmp_path, text):
    path = tmp_path / (mode + ".txt")
    path.write_text(text)
    done = subprocess.run([host_exe, mode, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert done.returncode == 0 and not done.stderr, done.stderr.decode()[-2000:]        # a sanitizer report goes to stderr
    return done.stdout.decode().splitlines()


def bits64(v):
    return np.float64(v).view(np.uint64)


def test_host_quantise_and_delta(host_exe, tmp_path):
    rng = np.random.default_rng(0)
    C = np.concatenate([rng.uniform(-1.0, 1.0, 4000), 1.0 - (np.arange(0, 254) + 0.5) / 127.0, [1.0, -1.0, 0.0, 1.0 + 2.0 ** -52, -1.0 - 2.0 ** -52]])
    C = np.concatenate([C, np.nextafter(C, 2.0), np.nextafter(C, -2.0)])
    out = run(host_exe, "quantise", tmp_path, "\n".join(float(v).hex() for v in C) + "\n")
    assert [int(t) for t in out] == so.quantise(C).tolist()
    assert set(so.quantise(C).tolist()) == set(range(255))
    trip = rng.integers(0, 10217, size=(3000, 3))
    trip = np.concatenate([trip, [[5, 5, 5], [0, 0, 0], [10216, 0, 10216], [7, 7, 9], [9, 7, 7], [3, 5, 3]]])      # den = 0 and den < 0 among them
    out = run(host_exe, "delta", tmp_path, "\n".join("%d %d %d" % tuple(t) for t in trip) + "\n")
    for t, line in zip(trip, out):
        sm, s0, sp = (int(v) for v in t)
        den = (sm - 2 * s0) + sp
        delta = (0.5 * float(sm - sp)) / float(den) if den > 0 else 0.0
        got = line.split()
        assert int(got[0]) == den and bits64(float.fromhex(got[1])) == bits64(delta), (t, line)


HOST_CASES = ["1x1_d2_p8", "1x7_d64_p8", "7x1_d3_p4", "2x2_d63_p8", "2x2_d2_p4", "17x33_d3_p4_zero", "all_254", "all_sentinel", "invalid_cost_0",
              "invalid_cost_254", "ramp_equal_1023", "ramp_zero_1023", "ramp_equal_200", "two_minima_d65", "edge_low", "edge_high_d65",
              "edge_high_d256", "second_absent_d3", "second_absent_d2", "7x1_d256_p8"]


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_volume_matches_every_intermediate(host_exe, tmp_path, name):
    c = sc.case(name)
    vol = c["vol"]
    h, w, D = vol.shape
    wf, step = planes_of(D)
    u = 5
    want = so.aggregate_lines(vol, c["p1"], c["p2"], c["n_paths"], c["invalid_cost"])
    plane, best, second = so.select(want["sums"])
    fin = so.finish(vol, want["sums"], plane, best, second, wf, step, u)
    text = "%d %d %d %d %d %d %d %d %s %s\n" % (w, h, D, c["p1"], c["p2"], c["n_paths"], c["invalid_cost"], u, float(wf).hex(), float(step).hex())
    out = run(host_exe, "volume", tmp_path, text + " ".join(str(int(v)) for v in vol.reshape(-1)) + "\n")
    seen = dict(C=0, L=0, S=0, O=0)
    for line in out:
        t = line.split()
        seen[t[0]] += 1
        if t[0] == "C":
            x, y = int(t[1]), int(t[2])
            assert [int(v) for v in t[3:]] == want["c"][y, x].tolist(), line[:80]
        elif t[0] == "L":
            r, x, y = int(t[1]), int(t[2]), int(t[3])
            assert int(t[4]) == int(want["m"][r][y, x]) and [int(v) for v in t[5:]] == want["L"][r][y, x].tolist(), line[:80]
        elif t[0] == "S":
            x, y = int(t[1]), int(t[2])
            assert [int(v) for v in t[3:]] == want["sums"][y, x].tolist(), line[:80]
        else:
            x, y = int(t[1]), int(t[2])
            assert (int(t[3]), int(t[4]), int(t[5])) == (int(plane[y, x]), int(best[y, x]), int(second[y, x])), line
            assert int(t[6]) == int(fin["den"][y, x]) and bits64(float.fromhex(t[7])) == bits64(fin["delta"][y, x]), line
            assert int(t[8], 16) == int(fin["depth"].view(np.uint32)[y, x]) and int(t[9], 16) == int(fin["score"].view(np.uint32)[y, x]), line
            assert int(t[10]) == int(fin["accepted"][y, x]) and int(t[11]) == int(fin["q"][y, x]), line
    assert seen == dict(C=h * w, L=h * w * c["n_paths"], S=h * w, O=h * w)


# ---- identities -----------------------------------------------------------------------------------------------------------------
def test_without_penalties_the_sums_are_the_costs():
    for name in ("17x33_d65_p8", "invalid_cost_254", "70x45_d3_p8"):
        c = sc.case(name)
        for n_paths in (4, 8):
            a = so.sgm_aggregate(c["vol"], 0, 0, n_paths, c["invalid_cost"])
            cost = so.costs(c["vol"], c["invalid_cost"])
            assert (a["sums"] == n_paths * cost).all()
            assert (a["plane"] == cost.argmin(2)).all() and (a["best"] == n_paths * cost.min(2)).all()


def test_transposing_the_volume_transposes_the_result_of_four_paths():
    for name in ("17x33_d65_p8", "70x45_d64_p4", "33x17_d64_p8_wide"):
        c = sc.case(name)
        a = so.sgm_aggregate(c["vol"], c["p1"], c["p2"], 4, c["invalid_cost"])
        b = so.sgm_aggregate(np.ascontiguousarray(c["vol"].transpose(1, 0, 2)), c["p1"], c["p2"], 4, c["invalid_cost"])
        assert same_bits(a["sums"], np.ascontiguousarray(b["sums"].transpose(1, 0, 2)))
        for f in ("plane", "best", "second"):
            assert same_bits(a[f], np.ascontiguousarray(b[f].T)), f


def test_a_constant_volume_gives_the_far_plane_and_no_acceptance():
    for value in (0, 77, 254, 255):
        vol = np.full((6, 9, 12), value, np.uint8)
        a = so.sgm_aggregate(vol, 8, 64, 8, 127)
        assert (a["plane"] == 0).all() and (a["second"] == a["best"]).all()
        wf, step = planes_of(12)
        for u in (1, 5, 100):
            f = so.finish(vol, a["sums"], a["plane"], a["best"], a["second"], wf, step, u)
            assert f["accepted"].any() == (value == 0) and (value == 0 or not f["depth"].any())     # all sums 0: 0 >= 0 holds
        assert so.finish(vol, a["sums"], a["plane"], a["best"], a["second"], wf, step, 0)["accepted"].all()


def test_bounds_the_header_states():
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    for text in ("254 + p2 <= 1277", "8 * 1277 = 10216", "0 <= p1 <= p2 <= 1023"):
        assert text in header, text
    assert 100 * 10216 < 2 ** 31 and 10216 * 256 + 255 < 2 ** 22 and 8 * (254 + 1023) < 2 ** 16


def test_symbols_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build_hip()
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    lib = os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "libsfmba_hip.so")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    from sfm_toy_library_amd import capi
    for name in ("sfmba_depth_cost_volume", "sfmba_sgm_aggregate", "sfmba_depth_sweep_sgm"):
        assert "SFMBA_API int %s(" % name in header
        assert " T %s\n" % name in exported
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    assert callable(capi.depth_cost_volume) and callable(capi.sgm_aggregate) and callable(capi.depth_sweep_sgm)
    assert capi.lib().sfmba_abi_version() == 6


def test_sfmtoy_usage_names_the_sgm_switches_and_the_shim_has_the_driver():
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    exe = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")
    ok = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert ok.returncode == 0 and all(s in ok.stdout for s in ("--sgm [P1,P2]", "--sgm-paths 4|8", "--sgm-uniqueness U"))
    for args in (["--sgm"], ["-D", "--sgm", "9,8"], ["-D", "--sgm=1,1024"], ["-D", "--sgm-paths", "8"], ["-D", "--sgm", "--sgm-paths", "6"],
                 ["-D", "--sgm", "--sgm-uniqueness", "101"], ["-D", "--sgm", "1,2", "3,4", "/another-directory"]):
        done = subprocess.run([exe] + args + ["/nonexistent-directory"], capture_output=True, text=True)
        assert done.returncode == 2, (args, done.returncode)
    # a good command line gets past the argument check: the missing directory is then an ordinary failure, before any device
    # ... and a directory whose name is a number is a directory: only digits around a comma are taken for --sgm's value
    for args in (["-D", "--sgm"], ["-D", "--sgm", "3,40", "--sgm-paths", "4", "--sgm-uniqueness", "0"], ["-D", "--sgm=0,0"], ["-D", "--sgm", "2024"]):
        done = subprocess.run([exe] + args + (["/nonexistent-directory"] if args[-1] != "2024" else []), capture_output=True, text=True)
        assert done.returncode == 1, (args, done.returncode, done.stderr)
    so_ = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    assert " T sfmba_shim_run_sfm_dense_sgm\n" in subprocess.check_output(["nm", "-C", so_]).decode()


# ---- quality floors ---------------------------------------------------------------------------------------------------------
BAND = (slice(100, 140), slice(40, 280))                     # rows, columns of the reference view: 40 x 240 of 240 x 320


def banded_corner():
    """The 320 x 240 corner scene of tests/test_depth_oracle_cpu.py's floor test with a flat grey band painted ON THE WALLS where
    view 1 sees BAND: every view shows it where its own pixel's surface point falls into the band of view 1."""
    scene = sfm_scene.make_corner(size=(320, 240), focal=1250, texture_scale=125)
    band = np.zeros((240, 320), bool)
    band[BAND] = True
    K, Kinv = scene["K"], np.linalg.inv(scene["K"])
    images = [im.copy() for im in scene["images"]]
    ys, xs = np.mgrid[0:240, 0:320]
    pix = np.stack([xs, ys, np.ones_like(xs)], -1).reshape(-1, 3).astype(np.float64)
    for v in (0, 1, 2):
        z = dc.corner_depth(scene, v).reshape(-1)
        fin = np.isfinite(z)
        Xw = ((pix @ Kinv.T) * np.where(fin, z, 1.0)[:, None] - scene["t"][v]) @ scene["R"][v]
        q = (Xw @ scene["R"][1].T + scene["t"][1]) @ K.T
        u, w_ = np.rint(q[:, 0] / q[:, 2]).astype(int), np.rint(q[:, 1] / q[:, 2]).astype(int)
        inside = fin & (u >= 0) & (u < 320) & (w_ >= 0) & (w_ < 240)
        grey = np.zeros(240 * 320, bool)
        grey[inside] = band[w_[inside], u[inside]]
        images[v][grey.reshape(240, 320)] = 128
    return scene, images, band


def test_quality_floors_on_the_corner_scene_with_a_flat_band():
    """Measured on this configuration (r 3, D 32, 8 paths, p1 8, p2 64, invalid_cost 127, uniqueness 5), the band being the 34 x 234
    pixels whose whole window is grey:

        plain sweep   band accepted 0 (by construction)      textured accepted 0.9989, right within one step 0.9536
        SGM           band accepted 0.0370, right 1.0000     textured accepted 0.9997, right within one step 0.9870
                      k* within one step of the truth (accepted or not): band 0.5109, textured 0.9748

    The floors are those less 0.03, the margin the sweep's own floors took.  THE BAND GETS A PLANE EVERYWHERE BUT FEW OF ITS PIXELS ARE
    ACCEPTED WITH THE DEFAULTS: every path crosses the band with a constant cost of invalid_cost = 127, so the sums there stand on
    8 * 127 and a 5 % uniqueness needs most of the 8 paths to agree on the plane, which on a slanted wall they do only near the band's
    border.  Not asserted, for the record: uniqueness 0 accepts all of the band with 0.640 right, uniqueness 2 accepts 0.400 with
    0.929 right, invalid_cost 0 accepts 0.724 with 0.811 right."""
    scene, images, band = banded_corner()
    zt = dc.corner_depth(scene, 1)
    fin = np.isfinite(zt)
    zn, zf = zt[fin].min() / 1.05, zt[fin].max() * 1.05
    P = np.concatenate([scene["R"], scene["t"][:, :, None]], axis=2).astype(np.float32)
    K = scene["K"].astype(np.float32)
    job = (1, [0, 2], zn, zf)
    o = do.sweep_integral(images, K, P, job, n_planes=32, radius=3, min_std=2, min_score=0.6)
    depth, score, plane = so.sweep_sgm(images, K, P, [job], n_planes=32, radius=3, min_std=2, min_sources=1, **so.DEFAULTS)[0]
    inner = np.zeros_like(band)
    inner[BAND[0].start + 3:BAND[0].stop - 3, BAND[1].start + 3:BAND[1].stop - 3] = True       # the whole window is grey
    assert inner.sum() == 34 * 234 and inner.sum() < 0.2 * band.size and not (inner & o["part"]).any()
    assert not ((o["depth"] > 0) & inner).any()                  # the plain sweep accepts nothing in the band, by construction
    textured = o["part"] & ~band

    def shares(d, region):
        acc = (d > 0) & region
        with np.errstate(all="ignore"):
            err = np.abs(1.0 / np.where(acc, d, 1).astype(np.float64) - 1.0 / np.where(fin, zt, 1.0))
        return acc.sum() / region.sum(), (acc & fin & (err <= o["step"])).sum() / max(acc.sum(), 1)

    band_acc, band_right = shares(depth, inner)
    tex_acc, tex_right = shares(depth, textured)
    plain_acc, plain_right = shares(o["depth"], textured)
    with np.errstate(all="ignore"):
        near = fin & (np.abs((o["wf"] + plane.astype(np.float64) * o["step"]) - 1.0 / np.where(fin, zt, 1.0)) <= o["step"])
    print("banded corner 320x240 r3 D32: plain textured accepted %.4f right %.4f; sgm band accepted %.4f right %.4f, textured accepted %.4f "
          "right %.4f; k* within one step: band %.4f textured %.4f"
          % (plain_acc, plain_right, band_acc, band_right, tex_acc, tex_right, (near & inner).sum() / inner.sum(), (near & textured).sum() / textured.sum()))
    assert (plane >= 0).all() and not (score[inner] != 0).any()  # a plane everywhere; the band's score says "from the neighbours"
    assert band_acc >= 0.0370 - 0.03
    assert band_right >= 1.0 - 0.03
    assert tex_acc >= 0.9997 - 0.03
    assert tex_right >= 0.9870 - 0.03
    assert tex_right >= plain_right - 0.03
