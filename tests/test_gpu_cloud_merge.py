"""The voxel merge and the depth normals on the MI355X (-m gpu) against the CPU restatement of their contract (tests/cloud_oracle.py;
include/sfmba.h, sfmba_cloud_merge / sfmba_depth_normals).  Every comparison is EXACT: the bit patterns of xyz and normal, the
colours, counts, first, voxel_of, the number of skipped points.  The shapes are those of tests/cloud_cases.py -- the smallest at
which the kernels can still go wrong -- and the restatement's answer for each is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import cloud_cases as cc
import cloud_oracle as co

pytestmark = pytest.mark.gpu
SFMBA_ERR_INVALID_ARG, SFMBA_ERR_CAPACITY = 1, 5
FIELDS = ("xyz", "bgr", "normal", "count", "first", "voxel_of")


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_merged(got, want, what=""):
    assert got["n_skipped"] == want["n_skipped"], (what, "n_skipped", got["n_skipped"], want["n_skipped"])
    assert len(got["count"]) == len(want["count"]), (what, "total", len(got["count"]), len(want["count"]))
    for f in FIELDS:
        assert same_bits(got[f], want[f]), (what, f)


def merge(capi, c, with_bgr=True, with_normal=True, **over):
    kw = dict(voxel=c["voxel"], min_count=c["min_count"])
    kw.update(over)
    return capi.cloud_merge(c["xyz"], c["bgr"] if with_bgr else None, c["normal"] if with_normal else None, **kw)


# ---- merge --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.CASES))
def test_cases_exact(capi, name):
    assert_merged(merge(capi, cc.case(name)), cc.oracle(name), name)


def test_no_points(capi):
    got = capi.cloud_merge(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.float32), voxel=0.5)
    assert got["n_skipped"] == 0 and all(len(got[f]) == 0 for f in FIELDS)
    got = capi.cloud_merge(np.zeros((0, 3), np.float32), voxel=0.5)
    assert got["bgr"] is None and got["normal"] is None and len(got["xyz"]) == 0


@pytest.mark.parametrize("with_bgr,with_normal", [(False, False), (True, False), (False, True)])
def test_attributes_may_be_null(capi, with_bgr, with_normal):
    for name in ("runs_straddle", "min_count_2"):
        got = merge(capi, cc.case(name), with_bgr, with_normal)
        assert_merged(got, cc.oracle(name, with_bgr, with_normal), name)
        assert (got["bgr"] is None) == (not with_bgr) and (got["normal"] is None) == (not with_normal)


def test_voxel_of_may_be_null(capi):
    got = merge(capi, cc.case("min_count_2"), want_voxel_of=False)
    want = cc.oracle("min_count_2")
    assert got["voxel_of"] is None
    for f in FIELDS[:-1]:
        assert same_bits(got[f], want[f]), f


@pytest.mark.parametrize("min_count", [1, 2, 3])
def test_min_count_and_voxel_of(capi, min_count):
    c = cc.case("min_count_2")
    want = co.merge_sorted(c["xyz"], c["bgr"], c["normal"], c["voxel"], min_count)
    got = merge(capi, c, min_count=min_count)
    assert_merged(got, want, min_count)
    kept = got["voxel_of"] >= 0
    assert (np.bincount(got["voxel_of"][kept], minlength=len(got["count"])) == got["count"]).all()
    assert (got["count"] >= min_count).all() and kept.sum() == got["count"].sum()
    assert (got["voxel_of"][got["first"]] == np.arange(len(got["first"]))).all()


def test_a_permutation_gives_the_same_voxels(capi):
    c = cc.case("n_32769")
    base = merge(capi, c)
    perm = np.random.default_rng(91).permutation(len(c["xyz"]))
    got = capi.cloud_merge(c["xyz"][perm], c["bgr"][perm], c["normal"][perm], voxel=c["voxel"], min_count=c["min_count"])
    for f in ("xyz", "bgr", "normal", "count"):
        assert same_bits(got[f], base[f]), f
    assert same_bits(got["voxel_of"], base["voxel_of"][perm])                   # voxel_of follows the permutation
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(len(perm))
    members = [[] for _ in base["count"]]
    for i, v in enumerate(base["voxel_of"]):
        members[v].append(inverse[i])
    assert got["first"].tolist() == [min(m) for m in members]                   # ... and first is the lowest NEW index of the same members


def test_a_doubled_cloud_doubles_the_counts(capi):
    c = cc.case("runs_straddle")
    base = merge(capi, c)
    two = capi.cloud_merge(np.concatenate([c["xyz"]] * 2), np.concatenate([c["bgr"]] * 2), np.concatenate([c["normal"]] * 2), voxel=c["voxel"])
    for f in ("xyz", "bgr", "normal", "first"):
        assert same_bits(two[f], base[f]), f
    assert same_bits(two["count"], 2 * base["count"]) and same_bits(two["voxel_of"], np.concatenate([base["voxel_of"]] * 2))


def raw_merge(capi, c, cap, voxel=None, min_count=None, n=None, null=(), fill=0x5a):
    """the bare call with recognisable output buffers: (rc, total, n_skipped, outputs)"""
    fp, bp, ip = C.POINTER(C.c_float), C.POINTER(C.c_ubyte), C.POINTER(C.c_int32)
    xyz, bgr, nrm = (np.ascontiguousarray(c[k]) for k in ("xyz", "bgr", "normal"))
    rows = max(int(cap), 1)
    out = dict(xyz=np.full((rows, 3), 7.5, np.float32), bgr=np.full((rows, 3), fill, np.uint8), normal=np.full((rows, 3), 7.5, np.float32),
               count=np.full(rows, fill, np.int32), first=np.full(rows, fill, np.int32), voxel_of=np.full(max(len(xyz), 1), fill, np.int32))
    total, skipped = C.c_int64(-7), C.c_int64(-7)

    def ptr(name, arr, t):
        return None if name in null else arr.ctypes.data_as(t)

    rc = capi.lib().sfmba_cloud_merge(C.c_int(0), C.c_int64(len(xyz) if n is None else n), ptr("xyz", xyz, fp), ptr("bgr", bgr, bp),
                                      ptr("normal", nrm, fp), C.c_float(c["voxel"] if voxel is None else voxel),
                                      C.c_int(c["min_count"] if min_count is None else min_count), ptr("xyz_out", out["xyz"], fp),
                                      ptr("bgr_out", out["bgr"], bp), ptr("normal_out", out["normal"], fp), ptr("count", out["count"], ip),
                                      ptr("first", out["first"], ip), ptr("voxel_of", out["voxel_of"], ip), C.c_int64(cap),
                                      None if "total" in null else C.byref(total), None if "n_skipped" in null else C.byref(skipped))
    return rc, total.value, skipped.value, out


def untouched(out, fill=0x5a, but=()):
    return all(k in but or (v == (np.float32(7.5) if v.dtype == np.float32 else fill)).all() for k, v in out.items())


def test_capacity_protocol(capi):
    c, want = cc.case("nonfinite"), cc.oracle("nonfinite")
    m = len(want["count"])
    assert m > 3
    for cap in (0, m - 1):
        rc, total, skipped, out = raw_merge(capi, c, cap)
        assert rc == SFMBA_ERR_CAPACITY and total == m and skipped == want["n_skipped"] == 5
        assert same_bits(out["voxel_of"], want["voxel_of"]) and untouched(out, but=("voxel_of",))           # nothing else written
    rc, total, skipped, out = raw_merge(capi, c, m)
    assert rc == 0 and total == m and skipped == 5
    for f in FIELDS:
        assert same_bits(out[f][:m] if f != "voxel_of" else out[f], want[f]), f
    rc, total, skipped, out = raw_merge(capi, c, m + 3)
    assert rc == 0 and total == m and all((out[f][m:] == (7.5 if f in ("xyz", "normal") else 0x5a)).all() for f in FIELDS[:-1])


def test_refuses_what_the_contract_says(capi):
    c = cc.case("nonfinite")
    for kw in (dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(min_count=0), dict(min_count=-3),
               dict(n=-1), dict(n=2 ** 31), dict(null=("xyz",)), dict(null=("total",)), dict(null=("n_skipped",)), dict(null=("xyz_out",)),
               dict(null=("count",)), dict(null=("first",)), dict(null=("bgr_out",)), dict(null=("normal_out",))):
        rc, total, skipped, out = raw_merge(capi, c, 64, **kw)
        assert rc == SFMBA_ERR_INVALID_ARG, kw
        assert untouched(out) and total == -7 and skipped == -7, kw                         # nothing written
    # the output of an input that is NULL may be NULL
    rc, total, _, out = raw_merge(capi, c, 64, null=("bgr", "bgr_out", "normal", "normal_out", "voxel_of"))
    assert rc == 0 and total == len(cc.oracle("nonfinite")["count"]) and untouched(out, but=("xyz", "count", "first"))
    assert same_bits(out["xyz"][:total], cc.oracle("nonfinite")["xyz"])
    with pytest.raises(capi.SfmbaError, match="voxel"):                                     # the message comes through sfmba_last_error
        capi.cloud_merge(c["xyz"], voxel=0.0)


# ---- normals ------------------------------------------------------------------------------------------------------------------
def normals_of(capi, c, **over):
    kw = dict(max_rel_step=c["max_rel_step"])
    kw.update(over)
    return capi.depth_normals(c["K"], c["P"][None], [c["depth"]], **kw)[0]


@pytest.mark.parametrize("name", list(cc.NORMAL_CASES))
def test_normal_cases_exact(capi, name):
    got, want = normals_of(capi, cc.normals_case(name)), cc.normals_oracle(name)
    bad = np.argwhere(got.view(np.uint32) != want["normal"].view(np.uint32))
    assert len(bad) == 0, (name, len(bad), bad[:5].tolist())
    if name in ("size_1x1", "size_7x1", "size_1x7"):
        assert not got.any()
    if name == "step_exact":
        assert got[1, 1].any()
    if name == "step_below":
        assert not got[1, 1].any()
    if name == "flip":
        assert want["flipped"].any() and not want["flipped"].all()


def test_a_batch_equals_single_calls_and_a_map_may_be_missing(capi):
    names = ("size_33x17", "size_70x45", "one_sided")
    cases = [cc.normals_case(n) for n in names]
    K = cases[0]["K"]
    P = np.stack([cc.camera(8, 8, deg=20.0 * i)[1] for i in range(5)])
    maps = [cases[0]["depth"], None, cases[1]["depth"], cases[2]["depth"], None]
    got = capi.depth_normals(K, P, maps, max_rel_step=0.05)
    assert got[1] is None and got[4] is None
    for i in (0, 2, 3):
        one = capi.depth_normals(K, P[i:i + 1], [maps[i]], max_rel_step=0.05)[0]
        assert same_bits(got[i], one), i
        assert same_bits(one, co.normals_shifted(K, P[i], maps[i], 0.05)["normal"]), i
    assert capi.depth_normals(K, P[:2], [None, None]) == [None, None]


def test_normals_refuse_what_the_contract_says(capi):
    c = cc.normals_case("size_33x17")
    h, w = c["depth"].shape
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def raw(K=c["K"], P=c["P"], step=0.05, width=w, height=h, null_out=False):
        K, P = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(P, np.float32)
        out = np.full((h, w, 3), 7.5, np.float32)
        wd, ht = np.asarray([width], np.int32), np.asarray([height], np.int32)
        dptr, optr = (fp * 1)(c["depth"].ctypes.data_as(fp)), (fp * 1)(None if null_out else out.ctypes.data_as(fp))
        rc = capi.lib().sfmba_depth_normals(C.c_int(0), C.c_int(1), wd.ctypes.data_as(ip), ht.ctypes.data_as(ip), K.ctypes.data_as(fp),
                                            P.ctypes.data_as(fp), dptr, C.c_float(step), optr)
        return rc, bool((out == np.float32(7.5)).all())

    assert raw() == (0, False)
    bad_K, nan_K, bad_P = c["K"].copy(), c["K"].copy(), c["P"].copy()
    bad_K[0, 0], nan_K[1, 2], bad_P[1, 3] = 0.0, np.nan, np.inf
    for kw in (dict(step=-0.01), dict(step=float("nan")), dict(step=float("inf")), dict(K=bad_K), dict(K=nan_K), dict(P=bad_P), dict(width=0),
               dict(height=16385), dict(null_out=True)):
        assert raw(**kw) == (SFMBA_ERR_INVALID_ARG, True), kw
