"""TSDF integration and marching tetrahedra on the MI355X (-m gpu) against the CPU restatement of their contract (tests/mesh_oracle.py;
include/sfmba.h, sfmba_tsdf_integrate / sfmba_tsdf_extract / sfmba_tsdf_mesh).  Every comparison is EXACT: the bit patterns of xyz, the
bytes of the colours, keys, triangles and of the four grid arrays.  The shapes are those of tests/mesh_cases.py -- the smallest at which
the kernels can still go wrong -- and the restatement's answer for each is computed once and shared."""
import numpy as np
import pytest

import mesh_cases as mc
import mesh_oracle as mo
import mesh_refusals as mr

pytestmark = pytest.mark.gpu
SFMBA_OK, SFMBA_ERR_INVALID_ARG, SFMBA_ERR_CAPACITY = 0, 1, 5
GRID_FIELDS = ("sum", "weight", "csum", "cweight")


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


def assert_mesh(got, want, what=""):
    assert (len(got["xyz"]), len(got["tri"])) == (len(want["xyz"]), len(want["tri"])), (what, "totals")
    for f in mo.MESH_FIELDS:
        assert same_bits(got[f], want[f]), (what, f)


def extract(capi, c, colour=True, **over):
    kw = dict(min_weight=c["min_weight"])
    kw.update(over)
    return capi.tsdf_extract(c["origin"], c["voxel"], c["S"], c["W"], c["CS"] if colour else None, c["CW"] if colour else None, **kw)


def views(c, colour=True):
    return (c["images"] if colour else None, c["K"], c["P"], c["depth_maps"], c["origin"], c["voxel"], c["dims"], c["trunc"])


# ---- extraction -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.CASES))
def test_extraction_cases_exact(capi, name):
    assert_mesh(extract(capi, mc.case(name)), mc.mesh(name), name)


@pytest.mark.parametrize("name", mc.NO_CELL)
def test_no_cell_gives_an_empty_mesh(capi, name):
    got = extract(capi, mc.case(name))
    assert got["xyz"].shape == (0, 3) and got["tri"].shape == (0, 3) and len(got["vkey"]) == 0


@pytest.mark.parametrize("name", list(mc.CLOSED))
def test_planted_solids_are_closed_on_the_device(capi, name):
    got = extract(capi, mc.case(name))
    closed, euler, boundary, n_edges = mo.topology(got["tri"])
    assert closed and boundary == 0 and euler == mc.CLOSED[name]
    assert mo.signed_volume(got["xyz"], got["tri"]) > 0


def test_colours_and_keys_may_be_null(capi):
    for name in ("sphere_14", "undefined_corner", "all_256"):
        c = mc.case(name)
        got = extract(capi, c, colour=False)
        assert got["bgr"] is None
        assert_mesh(got, mc.mesh(name, False), name)
        got = extract(capi, c, want_vkey=False)
        assert got["vkey"] is None
        for f in ("xyz", "bgr", "tri"):
            assert same_bits(got[f], mc.mesh(name)[f]), (name, f)


def test_min_weight_decides(capi):
    c = mc.case("min_weight_w")
    assert len(extract(capi, c, min_weight=3)["tri"]) == len(mc.mesh("min_weight_w")["tri"]) > 0
    assert len(extract(capi, c, min_weight=4)["tri"]) == 0
    assert len(extract(capi, c, min_weight=65535)["tri"]) == 0


def test_capacity_protocol(capi):
    c, want = mc.case("sphere_14"), mc.mesh("sphere_14")
    nv, nt = len(want["xyz"]), len(want["tri"])
    for vcap, tcap in ((nv - 1, nt), (nv, nt - 1), (0, 0)):
        a = mr.valid("sfmba_tsdf_extract")
        nz, ny, nx = c["S"].shape
        a.update(origin=c["origin"], voxel=float(c["voxel"]), nx=nx, ny=ny, nz=nz, sum=c["S"], weight=c["W"], csum=c["CS"], cweight=c["CW"],
                 vcap=vcap, tcap=tcap, xyz=mr._filled((nv, 3), np.float32), bgr=mr._filled((nv, 3), np.uint8), vkey=mr._filled(nv, np.int32),
                 tri=mr._filled((nt, 3), np.int32))
        rc, _ = mr.invoke(capi.lib(), "sfmba_tsdf_extract", a)
        assert rc == SFMBA_ERR_CAPACITY and (int(a["n_vertices"][0]), int(a["n_triangles"][0])) == (nv, nt), (vcap, tcap)
        for f in ("xyz", "bgr", "vkey", "tri"):
            assert (a[f].view(np.uint8) == mr.FILL).all(), (vcap, tcap, f)                  # the fill bytes are untouched
    # a capacity given through the binding is retried once with the reported sizes
    assert_mesh(extract(capi, c, vcap=nv - 1, tcap=3), want)
    assert_mesh(extract(capi, c, vcap=nv, tcap=nt), want)


# ---- integration ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.INTEGRATION_CASES))
def test_integration_cases_exact(capi, name):
    got, want = capi.tsdf_integrate(*views(mc.integration_case(name))), mc.grid(name)
    for f in GRID_FIELDS:
        assert same_bits(got[f], want[f]), (name, f)


@pytest.mark.parametrize("name", ["five_images_bgr", "one_image_gray", "behind_and_outside"])
def test_pixels_may_be_null(capi, name):
    c = mc.integration_case(name)
    got, want = capi.tsdf_integrate(*views(c, colour=False)), mc.grid(name, False)
    assert got["csum"] is None and got["cweight"] is None
    assert same_bits(got["sum"], want["sum"]) and same_bits(got["weight"], want["weight"])
    got = capi.tsdf_integrate(*views(c), colour=False)                                      # pixels given, csum and cweight NULL
    assert got["csum"] is None and same_bits(got["sum"], want["sum"]) and same_bits(got["weight"], want["weight"])
    a = mr.valid("sfmba_tsdf_integrate")                                                    # pixels NULL: csum and cweight stay untouched
    a.update(pixels=None, img_ptr=None)
    rc, _ = mr.invoke(capi.lib(), "sfmba_tsdf_integrate", a)
    assert rc == SFMBA_OK and (a["csum"].view(np.uint8) == mr.FILL).all() and (a["cweight"].view(np.uint8) == mr.FILL).all()
    assert not (a["sum"].view(np.uint8) == mr.FILL).all()


def test_a_permutation_of_the_images_gives_the_same_bytes(capi):
    a = capi.tsdf_integrate(*views(mc.integration_case("five_images_bgr")))
    b = capi.tsdf_integrate(*views(mc.integration_case("five_images_permuted")))
    for f in GRID_FIELDS:
        assert same_bits(a[f], b[f]), f
    assert_mesh(capi.tsdf_mesh(*views(mc.integration_case("five_images_permuted"))), mc.grid_mesh("five_images_bgr"))


def test_bgr_equals_its_gray_rule_per_channel(capi):
    c = mc.integration_case("five_images_bgr")
    bgr = capi.tsdf_integrate(*views(c))
    for ch in range(3):
        gray = capi.tsdf_integrate(*views(mc.gray_of(c, ch)))
        assert same_bits(gray["sum"], bgr["sum"]) and same_bits(gray["cweight"], bgr["cweight"])
        for k in range(3):
            assert same_bits(gray["csum"][..., k], np.ascontiguousarray(bgr["csum"][..., ch])), (ch, k)


def test_no_image_and_no_map(capi):
    c = mc.integration_case("one_image_gray")
    for got in (capi.tsdf_integrate([], c["K"], np.zeros((0, 3, 4), np.float32), [], c["origin"], c["voxel"], c["dims"], c["trunc"]),
                capi.tsdf_integrate(c["images"], c["K"], c["P"], [None], c["origin"], c["voxel"], c["dims"], c["trunc"])):
        assert got["sum"].shape == c["dims"][::-1] and not any(got[f].any() for f in GRID_FIELDS)
    got = capi.tsdf_mesh(c["images"], c["K"], c["P"], [None], c["origin"], c["voxel"], c["dims"], c["trunc"])
    assert len(got["xyz"]) == 0 and len(got["tri"]) == 0


# ---- together -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["six_view_sphere", "two_views_holes", "five_images_bgr"])
@pytest.mark.parametrize("colour", [True, False])
def test_mesh_equals_integrate_then_extract(capi, name, colour):
    c = mc.integration_case(name)
    g = capi.tsdf_integrate(*views(c, colour))
    two = capi.tsdf_extract(c["origin"], c["voxel"], g["sum"], g["weight"], g["csum"], g["cweight"], min_weight=1)
    one = capi.tsdf_mesh(*views(c, colour), min_weight=1)
    assert_mesh(one, two, name)
    assert_mesh(one, mc.grid_mesh(name, colour), name)
    assert (one["bgr"] is None) == (not colour)
    if name == "five_images_bgr":
        assert_mesh(capi.tsdf_mesh(*views(c, colour), min_weight=2), mc.grid_mesh(name, colour, 2), name)


def test_six_view_sphere_quality_on_the_device(capi):
    """The bounds of tests/test_mesh_oracle_cpu.py (twice the distances measured on the restatement), on the device's vertices."""
    m = capi.tsdf_mesh(*views(mc.integration_case("six_view_sphere")))
    d = np.abs(np.linalg.norm(m["xyz"].astype(np.float64), axis=1) - 1.0)
    assert np.median(d) <= 2 * 0.011404 and d.max() <= 2 * 0.100485


def test_mesh_capacity_protocol(capi):
    c, want = mc.integration_case("two_views_holes"), mc.grid_mesh("two_views_holes")
    assert_mesh(capi.tsdf_mesh(*views(c), vcap=len(want["xyz"]) - 1, tcap=len(want["tri"])), want)
    assert_mesh(capi.tsdf_mesh(*views(c), vcap=len(want["xyz"]), tcap=len(want["tri"]) - 1), want)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing(capi):
    calls = mr.refusal_calls(capi, device_cases=True)
    assert len(calls) > 90
    for name, call in calls:
        rc, untouched = call()
        assert rc == SFMBA_ERR_INVALID_ARG and untouched, name
    msg = capi.lib().sfmba_last_error().decode()
    assert "tsdf" in msg or msg == "bad argument", msg


@pytest.mark.parametrize("entry", ["sfmba_tsdf_integrate", "sfmba_tsdf_extract", "sfmba_tsdf_mesh"])
def test_the_valid_call_of_the_refusal_table_succeeds(capi, entry):
    rc, untouched = mr.valid_call(capi, entry)
    assert rc == SFMBA_OK and not untouched
