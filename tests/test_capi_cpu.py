"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol
include/sfmba.h declares, agrees with the ctypes struct mirrors, and refuses to run without a GPU
(no compute calls here; the parity tests proper are the -m gpu tests)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build_hip()
    from sfm_toy_library_amd import capi as c
    return c


def test_library_exports_every_declared_symbol(capi):
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    declared = re.findall(r"SFMBA_API[^;(]*?(sfmba_\w+)\(", header)
    assert sorted(set(declared)) == sorted(capi.SYMBOLS)
    L = capi.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert L.sfmba_abi_version() == 6


def test_default_options_match_reference_values(capi, sfm, oracle):
    o = capi.default_options()
    ref = sfm.SfmbaOptions.defaults()
    orc = sfm.SfmbaOptions()
    oracle.lib().sfmba_oracle_options_default(C.byref(orc))
    for name, _ in sfm.SfmbaOptions._fields_:
        assert getattr(o, name) == getattr(ref, name) == getattr(orc, name), name
    assert o.max_iters == 500 and o.max_seconds == 10.0        # BA.cpp:174,176


def test_struct_sizes_match_header(capi, sfm):
    # natural C layout of the header structs on x86-64
    assert C.sizeof(sfm.SfmbaIteration) == 4 * 4 + 6 * 8
    assert C.sizeof(sfm.SfmbaSummary) == 7 * 4 + 4 + 4 * 8 + 128 + 4 + 4      # ... message, cholesky_fallbacks (ABI v4) + tail padding
    assert C.sizeof(sfm.SfmbaOptions) == 8 + 10 * 8 + 4 * 4 + 8 + 3 * 4 + 7 * 4     # ... pcg_max_iters, verbose, pcg_anchored, 7 switches (ABI v4)
    # the header and the mirror agree on the field lists (names, in order)
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    body = header[header.index("typedef struct sfmba_options {"):header.index("} sfmba_options;")]
    names = re.findall(r"^\s+(?:int|double)\s+(\w+);", body, flags=re.M)
    assert names == [n for n, _ in sfm.SfmbaOptions._fields_]
    body = header[header.index("typedef struct sfmba_summary {"):header.index("} sfmba_summary;")]
    names = re.findall(r"^\s+(?:int|double|char)\s+(\w+)(?:\[\d+\])?;", body, flags=re.M)
    assert names == [n for n, _ in sfm.SfmbaSummary._fields_]


def test_no_cpu_fallback_without_device(capi, sfm):
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    prob = sfm.make_problem("tiny")
    with pytest.raises(capi.SfmbaError, match="no HIP device"):
        capi.Problem(prob)
    with pytest.raises(capi.SfmbaError, match="no HIP device"):
        capi.solve(prob)
    with pytest.raises(capi.SfmbaError, match="no HIP device"):
        capi.dense_spd_solve(np.eye(3), np.ones(3))
    with pytest.raises(capi.SfmbaError, match="no HIP device"):
        capi.device_warmup(0, 1000)
    with pytest.raises(capi.SfmbaError, match="no HIP device"):
        capi.dense_pcg_probe(np.eye(7), np.ones(7), max_iters=5)


def test_dense_pcg_probe_refuses_bad_arguments(capi):
    """Refused before the device is looked at: an iteration cap outside 1 .. 1000 (no call may spin through 4 d batches), a tolerance that is
    not positive, unknown flags, the segmented coarse space without vectors."""
    A, b = np.eye(7), np.ones(7)
    for bad in (0, -1, 1001):
        with pytest.raises(capi.SfmbaError, match="max_iters must lie in 1 .. 1000"):
            capi.dense_pcg_probe(A, b, max_iters=bad)
    with pytest.raises(capi.SfmbaError, match="max_iters must lie in 1 .. 1000"):
        capi.dense_pcg_probe(A, np.ones((3, 7)), max_iters=[5, 0, 5])
    for kw in (dict(tol=0.0), dict(tol=float("nan")), dict(flags=16), dict(flags=-1)):
        with pytest.raises(capi.SfmbaError, match="bad arguments"):
            capi.dense_pcg_probe(A, b, max_iters=5, **kw)
    with pytest.raises(capi.SfmbaError, match="needs Wt"):
        capi.dense_pcg_probe(A, b, flags=capi.PCG_PROBE_SEGMENTS, max_iters=5)
    with pytest.raises(ValueError):
        capi.dense_pcg_probe(A, np.ones(6), max_iters=5)


def test_dist_cg_probe_refuses_bad_arguments(capi):
    """Refused before the device is looked at: a world outside 1 .. 16, a dimension that is not 6 ncam + 1, an iteration cap outside 1 .. 1000,
    unknown flags, a negative surplus, a tolerance that is not positive."""
    A, b = np.eye(7), np.ones(7)
    for bad in (0, -1, 17):
        with pytest.raises(capi.SfmbaError, match="world must lie in 1 .. 16"):
            capi.dist_cg_probe(A, bad, b, max_iters=5)
    for n in (6, 8, 12):
        with pytest.raises(capi.SfmbaError, match="bad arguments"):
            capi.dist_cg_probe(np.eye(n), 2, np.ones(n), max_iters=5)
    for bad in (0, -1, 1001):
        with pytest.raises(capi.SfmbaError, match="max_iters must lie in 1 .. 1000"):
            capi.dist_cg_probe(A, 2, b, max_iters=bad)
    with pytest.raises(capi.SfmbaError, match="max_iters must lie in 1 .. 1000"):
        capi.dist_cg_probe(A, 2, np.ones((3, 7)), max_iters=[5, 0, 5])
    for kw in (dict(flags=4), dict(flags=-1), dict(surplus=-1), dict(tol=0.0), dict(tol=float("nan"))):
        with pytest.raises(capi.SfmbaError, match="bad arguments"):
            capi.dist_cg_probe(A, 2, b, max_iters=5, **kw)
    with pytest.raises(ValueError):
        capi.dist_cg_probe(A, 2, np.ones(6), max_iters=5)
    if capi.device_count() == 0:
        with pytest.raises(capi.SfmbaError, match="no HIP device"):
            capi.dist_cg_probe(A, 2, b, max_iters=5)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "sfm-toy-library_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp", ".hpp")) or fn == "Makefile":
                text = open(os.path.join(dirpath, fn), errors="replace").read()
                assert "oracle_py" not in text and "libsfmba_oracle" not in text and "sfmba_oracle_" not in text, fn


def test_problem_dump_roundtrip(sfm, tmp_path):
    prob = sfm.make_problem("tiny")
    path = tmp_path / "p.sfmba"
    sfm.save_problem(path, prob)
    back = sfm.load_problem(path)
    for a in ("cam6", "pt3", "obs_cam", "obs_pt", "obs_xy"):
        assert np.array_equal(getattr(prob, a), getattr(back, a))
    assert back.focal == prob.focal


def test_synthetic_generator_is_deterministic_and_matches_spec(sfm):
    a, b = sfm.make_problem("cfg2"), sfm.make_problem("cfg2")
    assert np.array_equal(a.obs_xy, b.obs_xy) and np.array_equal(a.cam6, b.cam6)
    assert (a.n_cam, a.n_pt, a.n_obs) == (20, 5000, 30000)
    assert np.array_equal(a.cam6[0], [0, 0, 0, 0, 0, 5.0])                     # identity first camera
    assert np.array_equal(a.obs_xy.astype(np.float32).astype(np.float64), a.obs_xy)   # Point2f-representable
    assert np.all(np.diff(a.obs_pt) >= 0)                                      # point-major
    same_pt = np.diff(a.obs_pt) == 0
    assert np.all(np.diff(a.obs_cam)[same_pt] > 0)                             # ascending view inside a point
    s0, s1 = a.shard_points(0, 2), a.shard_points(1, 2)
    assert s0.n_obs + s1.n_obs == a.n_obs and s0.n_pt + s1.n_pt == a.n_pt


def test_cpp_shim_exports_reference_symbol(capi):
    """The shim library carries sfmtoylib::SfMBundleAdjustmentUtils::adjustBundle with the reference's mangled signature."""
    import subprocess
    import __graft_entry__ as ge
    ge.build_host()
    so = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
    assert os.path.exists(so)
    syms = subprocess.check_output(["nm", "-C", so]).decode()
    assert "sfmtoylib::SfMBundleAdjustmentUtils::adjustBundle(" in syms
    assert "std::vector<cv::Matx<float, 3, 4>" in syms
    C.CDLL(so)   # loads (and resolves libsfmba_hip.so through its rpath)
