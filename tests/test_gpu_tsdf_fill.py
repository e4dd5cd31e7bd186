"""Hole filling on the MI355X (-m gpu) against the CPU restatement of its contract (tests/tsdf_fill_oracle.py; include/sfmba.h,
sfmba_tsdf_fill / sfmba_tsdf_mesh_fill).  Every comparison is EXACT: the bytes of sum, weight, csum, cweight and state, n_filled, and
for the combined call the bytes of the mesh and of vfilled.  The shapes are those of tests/tsdf_fill_cases.py (the largest grid is
65 x 4 x 3) and the 32^3 and smaller spheres of tests/mesh_cases.py; the restatement's answer for each is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import mesh_cases as mc
import mesh_oracle as mo
import tsdf_fill_cases as fc
import tsdf_fill_oracle as fo

pytestmark = pytest.mark.gpu
SFMBA_OK, SFMBA_ERR_INVALID_ARG, SFMBA_ERR_CAPACITY = 0, 1, 5
FILL = 0xA5


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


def views(c, colour=True):
    return (c["images"] if colour else None, c["K"], c["P"], c["depth_maps"], c["origin"], c["voxel"], c["dims"], c["trunc"])


def device_fill(capi, c, **over):
    kw = dict(min_weight=c["min_weight"], iterations=c["iterations"], min_neighbours=c["min_neighbours"], want_state=c["want_state"])
    kw.update(over)
    return capi.tsdf_fill(c["S"], c["W"], c["CS"], c["CW"], **kw)


# ---- the fill -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_fill_cases_exact(capi, name):
    c, want = fc.case(name), fc.expected(name)
    got = device_fill(capi, c)
    for f in ("sum", "weight", "csum", "cweight"):
        assert same_bits(got[f], want[f]), (name, f)
    if c["want_state"]:
        assert same_bits(got["state"], want["state"]), name
    else:
        assert got["state"] is None
    assert got["n_filled"] == want["n_filled"], name


def test_iterations_0_returns_the_input_bits(capi):
    c = fc.case("iterations_0")
    got = device_fill(capi, c)
    assert same_bits(got["sum"], c["S"]) and same_bits(got["weight"], c["W"]) and same_bits(got["csum"], c["CS"]) and same_bits(got["cweight"], c["CW"])
    assert got["n_filled"] == 0 and set(np.unique(got["state"]).tolist()) <= {0, 255}


# ---- together -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["six_view_sphere", "two_views_holes", "five_images_bgr"])
@pytest.mark.parametrize("passes", [0, 1, 3])
def test_mesh_fill_equals_integrate_fill_extract(capi, name, passes):
    c = mc.integration_case(name)
    for colour in (True, False):
        g = capi.tsdf_integrate(*views(c, colour))
        f = capi.tsdf_fill(g["sum"], g["weight"], g["csum"], g["cweight"], min_weight=1, iterations=passes, min_neighbours=2)
        w = mc.grid(name, colour)
        assert fo.same(f, fo.fill_numpy(w["sum"], w["weight"], w["csum"], w["cweight"], 1, passes, 2)) is None, (name, colour)
        three = capi.tsdf_extract(c["origin"], c["voxel"], f["sum"], f["weight"], f["csum"], f["cweight"], min_weight=1)
        one = capi.tsdf_mesh_fill(*views(c, colour), min_weight=1, fill_iterations=passes, min_neighbours=2)
        assert_mesh(one, three, (name, colour, passes))
        assert (one["bgr"] is None) == (not colour)
        assert same_bits(one["vfilled"], fo.vfilled(one["vkey"], f["state"])), (name, colour, passes)
        if passes == 0:
            assert_mesh(one, capi.tsdf_mesh(*views(c, colour), min_weight=1), name)
            assert not one["vfilled"].any()
        elif name != "five_images_bgr":                                          # the spheres: the fill adds surface
            assert len(one["tri"]) > len(mc.grid_mesh(name, colour)["tri"]) and one["vfilled"].any()
    # the outputs that may be NULL
    bare = capi.tsdf_mesh_fill(*views(c), min_weight=1, fill_iterations=passes, min_neighbours=2, want_vkey=False, want_vfilled=False)
    assert bare["vkey"] is None and bare["vfilled"] is None and same_bits(bare["xyz"], one["xyz"]) and same_bits(bare["tri"], one["tri"])


def test_min_weight_2_fills_with_the_weight_of_its_block(capi):
    c = mc.integration_case("five_images_bgr")
    g = capi.tsdf_integrate(*views(c))
    f = capi.tsdf_fill(g["sum"], g["weight"], g["csum"], g["cweight"], min_weight=2, iterations=2, min_neighbours=1)
    w = mc.grid("five_images_bgr")
    assert fo.same(f, fo.fill_numpy(w["sum"], w["weight"], w["csum"], w["cweight"], 2, 2, 1)) is None
    three = capi.tsdf_extract(c["origin"], c["voxel"], f["sum"], f["weight"], f["csum"], f["cweight"], min_weight=2)
    assert_mesh(capi.tsdf_mesh_fill(*views(c), min_weight=2, fill_iterations=2, min_neighbours=1), three)


def test_the_six_view_sphere_closes_on_the_device(capi):
    """3 passes at min_neighbours 2: 0 boundary edges and characteristic 2 (tests/test_tsdf_fill_oracle_cpu.py has the restatement's)."""
    m = capi.tsdf_mesh_fill(*views(mc.integration_case("six_view_sphere")), min_weight=1, fill_iterations=3, min_neighbours=2)
    closed, euler, boundary, n_edges = mo.topology(m["tri"])
    assert closed and boundary == 0 and euler == 2 and mo.signed_volume(m["xyz"], m["tri"]) > 0
    d = np.abs(np.linalg.norm(m["xyz"].astype(np.float64), axis=1) - 1.0)
    assert np.median(d) <= 0.0228 and d.max() <= 0.2010
    m2 = capi.tsdf_mesh_fill(*views(mc.integration_case("six_view_sphere")), min_weight=1, fill_iterations=2, min_neighbours=2)
    assert not mo.topology(m2["tri"])[0]


# ---- raw calls: the capacity protocol and the refusals ------------------------------------------------------------------------------
def _filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def _untouched(*arrays):
    return all((a.view(np.uint8) == FILL).all() for a in arrays if a is not None)


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def raw_mesh_fill(capi, c, vcap, tcap, min_weight=1, passes=3, k=2, dims=None):
    """(rc, nv, nt, outputs): sfmba_tsdf_mesh_fill with pre-filled outputs of the given capacities"""
    v, keep = capi._tsdf_views(c["images"], c["K"], c["P"], c["depth_maps"])
    g, origin, _ = capi._tsdf_grid(c["origin"], c["voxel"], dims or c["dims"])
    out = dict(xyz=_filled((max(vcap, 1), 3), np.float32), bgr=_filled((max(vcap, 1), 3), np.uint8), vkey=_filled(max(vcap, 1), np.int32),
               vfilled=_filled(max(vcap, 1), np.uint8), tri=_filled((max(tcap, 1), 3), np.int32))
    nv, nt = C.c_int64(-7), C.c_int64(-7)
    rc = capi.lib().sfmba_tsdf_mesh_fill(C.c_int(0), *v, *g, C.c_float(c["trunc"]), C.c_int(min_weight), C.c_int(passes), C.c_int(k),
                                         _ptr(out["xyz"], C.c_float), _ptr(out["bgr"], C.c_ubyte), _ptr(out["vkey"], C.c_int32),
                                         _ptr(out["vfilled"], C.c_ubyte), C.c_int64(vcap), _ptr(out["tri"], C.c_int32), C.c_int64(tcap),
                                         C.byref(nv), C.byref(nt))
    return rc, int(nv.value), int(nt.value), out


def test_both_capacities_one_short(capi):
    c = mc.integration_case("two_views_holes")
    want = capi.tsdf_mesh_fill(*views(c), min_weight=1, fill_iterations=3, min_neighbours=2)
    NV, NT = len(want["xyz"]), len(want["tri"])
    for vcap, tcap in ((NV - 1, NT), (NV, NT - 1), (NV - 1, NT - 1), (0, 0)):
        rc, nv, nt, out = raw_mesh_fill(capi, c, vcap, tcap)
        assert rc == SFMBA_ERR_CAPACITY and (nv, nt) == (NV, NT), (vcap, tcap)
        assert _untouched(*out.values()), (vcap, tcap)
    rc, nv, nt, out = raw_mesh_fill(capi, c, NV, NT)
    assert rc == SFMBA_OK and (nv, nt) == (NV, NT)
    assert same_bits(out["xyz"], want["xyz"]) and same_bits(out["vfilled"], want["vfilled"]) and same_bits(out["tri"], want["tri"])
    # through the binding a short capacity is retried once with the reported sizes
    again = capi.tsdf_mesh_fill(*views(c), min_weight=1, fill_iterations=3, min_neighbours=2, vcap=NV - 1, tcap=3)
    assert_mesh(again, want)
    assert same_bits(again["vfilled"], want["vfilled"])


def raw_fill(capi, a):
    """(rc, untouched): sfmba_tsdf_fill with the arguments of dict a; every output array of a is pre-filled"""
    n_filled = a["n_filled"]
    rc = capi.lib().sfmba_tsdf_fill(C.c_int(0), C.c_int(a["nx"]), C.c_int(a["ny"]), C.c_int(a["nz"]), _ptr(a["sum"], C.c_int32),
                                    _ptr(a["weight"], C.c_int32), _ptr(a["csum"], C.c_int32), _ptr(a["cweight"], C.c_int32), C.c_int(a["min_weight"]),
                                    C.c_int(a["iterations"]), C.c_int(a["min_neighbours"]), _ptr(a["sum_out"], C.c_int32),
                                    _ptr(a["weight_out"], C.c_int32), _ptr(a["csum_out"], C.c_int32), _ptr(a["cweight_out"], C.c_int32),
                                    _ptr(a["state"], C.c_ubyte), _ptr(n_filled, C.c_int64))
    return rc, _untouched(a["sum_out"], a["weight_out"], a["csum_out"], a["cweight_out"], a["state"], n_filled)


def valid_fill():
    c = fc.case("k2_9")
    nz, ny, nx = c["S"].shape
    return dict(nx=nx, ny=ny, nz=nz, sum=c["S"].copy(), weight=c["W"].copy(), csum=c["CS"].copy(), cweight=c["CW"].copy(), min_weight=1, iterations=2,
                min_neighbours=2, sum_out=_filled(c["S"].shape, np.int32), weight_out=_filled(c["S"].shape, np.int32),
                csum_out=_filled(c["CS"].shape, np.int32), cweight_out=_filled(c["S"].shape, np.int32), state=_filled(c["S"].shape, np.uint8),
                n_filled=_filled(1, np.int64))


def _grid_edit(field, at, value):
    def edit(a):
        a[field][at] = value
    return edit


FILL_REFUSALS = {
    "nx 0": lambda a: a.update(nx=0),
    "ny 1025": lambda a: a.update(ny=1025),
    "nz -1": lambda a: a.update(nz=-1),
    "more than 2^26 vertices": lambda a: a.update(nx=1024, ny=1024, nz=65),
    "min_weight 0": lambda a: a.update(min_weight=0),
    "min_weight 65536": lambda a: a.update(min_weight=65536),
    "iterations -1": lambda a: a.update(iterations=-1),
    "iterations 255": lambda a: a.update(iterations=255),
    "min_neighbours 0": lambda a: a.update(min_neighbours=0),
    "min_neighbours 7": lambda a: a.update(min_neighbours=7),
    "NULL sum": lambda a: a.update(sum=None),
    "NULL weight": lambda a: a.update(weight=None),
    "NULL sum_out": lambda a: a.update(sum_out=None),
    "NULL weight_out": lambda a: a.update(weight_out=None),
    "NULL n_filled": lambda a: a.update(n_filled=None),
    "csum without cweight": lambda a: a.update(cweight=None),
    "cweight without csum": lambda a: a.update(csum=None),
    "NULL csum_out with colour": lambda a: a.update(csum_out=None),
    "NULL cweight_out with colour": lambda a: a.update(cweight_out=None),
    # the grid's contents, found on the device
    "a negative weight": _grid_edit("weight", (8, 8, 8), -1),
    "S above 1024 W": _grid_edit("sum", (0, 0, 0), 1024 * 5 + 1),
    "S below -1024 W": _grid_edit("sum", (4, 5, 6), -1024 * 5 - 1),
    "a negative cweight": _grid_edit("cweight", (3, 3, 3), -2),
    "a negative colour sum": _grid_edit("csum", (2, 2, 2, 1), -1),
    "a colour sum above 255 Wc": _grid_edit("csum", (1, 2, 3, 0), 255 * 5 + 1),
}


def test_the_valid_call_of_the_refusal_table_succeeds(capi):
    a = valid_fill()
    rc, untouched = raw_fill(capi, a)
    want = fc.run(dict(fc.case("k2_9"), iterations=2))
    assert rc == SFMBA_OK and not untouched and int(a["n_filled"][0]) == want["n_filled"] and same_bits(a["state"], want["state"])


@pytest.mark.parametrize("what", list(FILL_REFUSALS))
def test_every_refusal_of_the_fill_writes_nothing(capi, what):
    a = valid_fill()
    if what in ("S above 1024 W", "S below -1024 W"):                       # the vertex the edit touches has W <= 5 in this case
        assert a["weight"].max() <= 5
    FILL_REFUSALS[what](a)
    rc, untouched = raw_fill(capi, a)
    assert rc == SFMBA_ERR_INVALID_ARG and untouched, what
    msg = capi.lib().sfmba_last_error().decode()
    assert "tsdf_fill" in msg or msg == "bad argument", msg


@pytest.mark.parametrize("what, kw", [("fill_iterations -1", dict(passes=-1)), ("fill_iterations 255", dict(passes=255)),
                                      ("min_neighbours 0", dict(k=0)), ("min_neighbours 7", dict(k=7)), ("min_weight 0", dict(min_weight=0)),
                                      ("min_weight 65536", dict(min_weight=65536)), ("nx 1025", dict(dims=(1025, 4, 4))),
                                      ("more than 2^26 vertices", dict(dims=(1024, 1024, 65)))])
def test_every_refusal_of_the_combined_call_writes_nothing(capi, what, kw):
    rc, nv, nt, out = raw_mesh_fill(capi, mc.integration_case("five_images_bgr"), 64, 64, **kw)
    assert rc == SFMBA_ERR_INVALID_ARG and (nv, nt) == (-7, -7) and _untouched(*out.values()), what
