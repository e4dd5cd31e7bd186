"""CPU-side checks of the float matcher's contract (include/sfmba.h, sfmba_match_features_l2): no GPU needed.

  routes        the numpy restatement (tests/match_l2_oracle.py, route A) and csrc/match_l2_math.h compiled for the host
                (tools/micro/match_l2_math_host.hip, route B: the code the kernel runs) agree BIT FOR BIT on the case table of
                tests/match_l2_cases.py and on 120 000 random row pairs of the six kinds of rows
  top-2         the lexsort form, the insertion form and the fast key form agree
  ABI           the header declares the symbol and still says ABI 6; the built library exports it
  shim          createFeatureMatchMatrix refuses mixed CV_8U / CV_32F descriptors before any device call
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import match_l2_cases as cases
import match_l2_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-toy-library_amd", "csrc")
SHIM = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("match_l2") / "match_l2_math_host")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tools", "micro", "match_l2_math_host.hip")])
    return exe


def host_rows(exe, tmp_path, a, b):
    """(s, s from the two-query step, dist, keep) of row i of a against row i of b, as the host program writes them."""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    n, dims = a.shape
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([n, dims], np.int32).tobytes()); f.write(a.tobytes()); f.write(b.tobytes())
    subprocess.check_call([exe, "rows", str(src), str(dst)])
    raw = dst.read_bytes()
    assert len(raw) == 13 * n
    f32 = np.frombuffer(raw[:12 * n], np.float32).reshape(3, n)
    return f32[0], f32[1], f32[2], np.frombuffer(raw[12 * n:], np.uint8).astype(bool)


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x, np.float32).view(np.uint32), np.ascontiguousarray(y, np.float32).view(np.uint32))


def check_routes(exe, tmp_path, a, b):
    want = lo.row_sq(a, b)
    s, s2, d, keep = host_rows(exe, tmp_path, a, b)
    assert not np.isnan(want).any() and not np.isnan(s).any()
    assert same_bits(s, want) and same_bits(s2, want)
    assert same_bits(d, lo.dist(want))
    dn = np.roll(lo.dist(want), -1)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(keep, lo.dist(want).astype(np.float64) < lo.RATIO_F32 * dn.astype(np.float64))
    return want


def test_case_table_covers_every_value_twice_and_every_edge_with_an_odd_dims():
    for values, col in ((cases.QUERY_ROWS, 0), (cases.TRAIN_ROWS, 1), (cases.DIMS, 2)):
        for v in values:
            assert sum(1 for c in cases.CASES if c[col] == v) >= 2, (col, v)
    assert {c[2] for c in cases.CASES} == set(cases.DIMS)
    for col, values in ((0, cases.QUERY_ROWS), (1, cases.TRAIN_ROWS)):
        for v in values:
            assert any(c[col] == v and c[2] % 2 == 1 for c in cases.CASES), (col, v)
    # the unit's own edges, from its restated cut rule: the LDS stage at the table's dims, and the two-kernel threshold
    assert [lo.stage_rows(d) for d in (1, 32, 33, 64, 65, 128, 129, 512)] == [256, 256, 128, 128, 80, 64, 48, 16]
    assert lo.padded_dims(64) == 64 and lo.padded_dims(65) == 96
    assert lo.plan([cases.SLICED[0]], [cases.SLICED[1]]) == [(2, 3)]


def test_routes_agree_on_the_case_table(host_exe, tmp_path):
    seen_inf = seen_subnormal = False
    for index, (nq, nt, dims) in enumerate(cases.CASES):
        q, t = cases.case_rows(index)
        if nq == 0 or nt == 0:
            continue
        n = max(nq, nt)
        a, b = q[np.arange(n) % nq], t[np.arange(n) % nt]
        s = check_routes(host_exe, tmp_path, a, b)
        seen_inf |= bool(np.isinf(s).any())
        seen_subnormal |= bool(((s > 0) & (s < np.finfo(np.float32).tiny)).any())
    assert seen_inf and seen_subnormal


@pytest.mark.parametrize("kind", lo.KINDS)
def test_routes_agree_on_random_rows(host_exe, tmp_path, kind):
    rng = np.random.default_rng(lo.KINDS.index(kind))
    total = 0
    for dims, n in ((1, 6000), (3, 5000), (37, 4000), (64, 2500), (128, 1500), (256, 1000)):       # 20 000 row pairs per kind
        a, b = lo.rows_of(kind, rng, n, dims), lo.rows_of(kind, rng, n, dims)
        near = rng.random(n) < 0.3                                                                 # near matches: where a GEMM form cancels
        b[near] = a[near] * np.float32(1.0 + 2.0 ** -12) if kind != "sift" else a[near]
        s = check_routes(host_exe, tmp_path, a, b)
        total += n
        if kind == "huge" and dims >= 3:
            assert np.isinf(s).any()
        if kind == "tiny":
            assert ((s > 0) & (s < np.finfo(np.float32).tiny)).any()
    assert total * len(lo.KINDS) >= 100000


def test_integer_shortcut_equals_the_chain():
    rng = np.random.default_rng(5)
    for dims in (1, 31, 128, 256):
        q, t = lo.rows_of("sift", rng, 40, dims), lo.rows_of("sift", rng, 50, dims)
        assert lo.small_integers(q, t)
        assert same_bits(lo.sq_distances(q, t), lo.sq_distances_chain(q, t))
    bits01 = rng.integers(0, 2, (30, 256)).astype(np.float32)
    bits01[3, :7] = -0.0
    assert lo.small_integers(bits01, bits01) and same_bits(lo.sq_distances(bits01, bits01), lo.sq_distances_chain(bits01, bits01))
    assert not lo.small_integers(lo.rows_of("sift", rng, 4, 258), lo.rows_of("sift", rng, 4, 258) + 255)
    assert not lo.small_integers(lo.rows_of("uniform", rng, 4, 8), lo.rows_of("sift", rng, 4, 8))


def test_top2_forms_agree():
    rng = np.random.default_rng(9)
    for kind, nq, nt, dims in (("sift", 40, 90, 16), ("uniform", 33, 70, 5), ("huge", 20, 30, 4), ("tiny", 20, 30, 3), ("mixed", 25, 41, 7),
                               ("uniform", 5, 1, 4), ("uniform", 5, 2, 4), ("uniform", 0, 4, 4), ("uniform", 4, 0, 4)):
        q, t = lo.rows_of(kind, rng, nq, dims), lo.rows_of(kind, rng, nt, dims)
        if nt > 4:
            t[3] = t[1]; t[nt - 1] = t[1]                    # ties: the lower index stays ahead
            q[0] = t[1]
        forms = [f(q, t) for f in (lo.knn_lexsort, lo.knn_insertion, lo.knn_keys)]
        for other in forms[1:]:
            for x, y in zip(forms[0], other):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), kind
        if nt > 4 and nq:
            assert forms[0][0][0] == 1 and forms[0][2][0] == 3
        lists = [lo.match_pair(q, t, knn=f) for f in (lo.knn_lexsort, lo.knn_insertion, lo.knn_keys)]
        assert lists[0] == lists[1] == lists[2]
    # +inf orders last, and a finite best against an infinite second is kept; a best of +inf is dropped
    q = np.array([[0.0, 0.0]], np.float32)
    t = np.array([[3e19, 0.0], [3.0, 4.0], [-3e19, 1.0]], np.float32)
    assert lo.match_pair(q, t, knn=lo.knn_insertion) == [(0, 1, int(np.float32(5.0).view(np.uint32)))]
    assert lo.match_pair(q, t[[0, 2]], knn=lo.knn_insertion) == []


def test_header_declares_the_symbol_and_abi_6():
    hdr = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    assert "#define SFMBA_ABI_VERSION 6" in hdr
    assert "SFMBA_API int sfmba_match_features_l2(int device, int n_images, const int64_t* img_ptr, const float* desc, int dims," in hdr
    from sfm_toy_library_amd import capi
    assert "sfmba_match_features_l2" in capi.SYMBOLS


def test_built_library_exports_the_symbol():
    lib = C.CDLL(os.path.join(CSRC, "libsfmba_hip.so"))
    assert hasattr(lib, "sfmba_match_features_l2") and hasattr(lib, "sfmba_match_features")
    assert lib.sfmba_abi_version() == 6


def test_shim_refuses_mixed_descriptor_types_without_a_device():
    """A child process in which no GPU is visible: the refusal must come before any device call, so it comes all the same."""
    code = ("import ctypes as C, numpy as np\n"
            "L = C.CDLL(%r)\n"
            "L.sfmba_shim_feature_match_matrix_mixed.restype = C.c_int64\n"
            "rows = np.array([5, 0, 4, 3], np.int32)\n"
            "def run(kinds):\n"
            "    k = np.array(kinds, np.uint8)\n"
            "    return L.sfmba_shim_feature_match_matrix_mixed(4, rows.ctypes.data_as(C.POINTER(C.c_int32)), k.ctypes.data_as(C.POINTER(C.c_ubyte)))\n"
            "print(run([0, 0, 1, 0]), run([1, 1, 0, 1]))\n" % SHIM)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    done = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    assert done.stdout.decode().split() == ["-1", "-1"]
    err = done.stderr.decode()
    assert err.count("descriptor types differ") == 2 and "sfmba rc=" not in err          # refused by the shim, not by a failed device call
