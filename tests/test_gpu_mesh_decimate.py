"""Mesh decimation on the MI355X (-m gpu) against the CPU restatement of its contract (tests/decimate_oracle.py; include/sfmba.h,
sfmba_mesh_decimate).  Every comparison is EXACT: the bit patterns of xyz, the bytes of the colours, the member counts, the
triangles, triangle_of, vertex_of, the totals and the four stats.  The shapes are those of tests/decimate_cases.py -- the smallest
at which the kernels can still go wrong -- and the restatement's answer for each is computed once and shared."""
import numpy as np
import pytest

import decimate_cases as dc
import decimate_oracle as do
import decimate_refusals as dr
import mesh_cases as mc

pytestmark = pytest.mark.gpu
SFMBA_OK, SFMBA_ERR_INVALID_ARG, SFMBA_ERR_CAPACITY = 0, 1, 5


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


def assert_fields(got, want, fields=dc.FIELDS, what=""):
    for f in fields:
        assert same_bits(got[f], want[f]), (what, f)
    if got.get("stats") is not None:
        assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


def decimated(capi, c, **kw):
    return capi.mesh_decimate(c["xyz"], c["bgr"], c["tri"], c["origin"], float(c["quantum"]), c["cell"], c["placement"], c["reg"], **kw)


# ---- every case, every output -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.CASES))
def test_cases_exact(capi, name):
    assert_fields(decimated(capi, dc.case(name)), dc.want(name), what=name)


@pytest.mark.parametrize("name", list(dc.REFUSED))
def test_a_coordinate_out_of_range_refuses_on_the_device(capi, name):
    assert dc.want(name) is None
    rc, untouched = dr.invoke(capi.lib(), dr.valid(name))
    assert rc == SFMBA_ERR_INVALID_ARG and untouched, name
    assert "coordinate" in capi.lib().sfmba_last_error().decode()


def test_outputs_may_be_null(capi):
    for name in ("member_runs", "small_cube", "no_colour"):
        c, want = dc.case(name), dc.want(name)
        for off in ("want_members", "want_triangle_of", "want_vertex_of", "want_stats"):
            got = decimated(capi, c, **{off: False})
            field = {"want_members": "members", "want_triangle_of": "triangle_of", "want_vertex_of": "vertex_of", "want_stats": "stats"}[off]
            assert got[field] is None
            assert_fields(got, want, [f for f in dc.FIELDS if f != field], (name, off))
        got = decimated(capi, c, want_members=False, want_triangle_of=False, want_vertex_of=False, want_stats=False)
        assert_fields(got, want, ("xyz", "bgr", "tri"), name)
        assert (got["bgr"] is None) == (c["bgr"] is None)
    # bgr NULL: bgr_out stays untouched
    a = dr.valid()
    a.update(bgr=None)
    rc, _ = dr.invoke(capi.lib(), a)
    assert rc == SFMBA_OK and (a["bgr_out"].view(np.uint8) == dr.FILL).all() and not (a["xyz_out"].view(np.uint8) == dr.FILL).all()


def test_the_device_mesh_of_the_six_view_sphere_decimates_as_the_restatement_says(capi):
    c = mc.integration_case("six_view_sphere")
    m = capi.tsdf_mesh(c["images"], c["K"], c["P"], c["depth_maps"], c["origin"], c["voxel"], c["dims"], c["trunc"])
    assert len(m["tri"]) > 10000
    quantum = float(np.float32(c["voxel"]) / np.float32(1024.0))
    for cell, placement in ((2048, 1), (2048, 0), (1024, 1), (4096, 1)):
        args = (m["xyz"], m["bgr"], m["tri"], c["origin"], quantum, cell, placement, 1024)
        want = do.decimate_np(*args)
        assert_fields(capi.mesh_decimate(*args), want, what=(cell, placement))
        print("six-view sphere, cell %d placement %d: %d -> %d triangles, stats %s" % (cell, placement, len(m["tri"]), len(want["tri"]), want["stats"]))
        assert 0 < len(want["tri"]) < len(m["tri"]) // 2


@pytest.mark.parametrize("cell", [256, 512])
def test_the_cube_floor_holds_on_device_output(capi, cell):
    """the quadric placement's mean distance to the surface is at most half the mean placement's, on what the device wrote"""
    _, _, R = dc.cube()
    d = {}
    for placement in (0, 1):
        c = dc.cube_case(cell, placement)
        got = decimated(capi, c)
        assert_fields(got, do.decimate_np(*dc.args(c)), what=(cell, placement))
        d[placement] = float(dc.cube_distance(got["xyz"], R).mean())
    print("cube, cell %d: mean distance quadric %.3g, cell mean %.3g" % (cell, d[1], d[0]))
    assert d[1] <= 0.5 * d[0]


# ---- the capacity protocol --------------------------------------------------------------------------------------------------------
def test_capacity_protocol(capi):
    want = dc.want("small_cube")
    nv, nt = len(want["xyz"]), len(want["tri"])
    for vcap, tcap in ((nv - 1, nt), (nv, nt - 1), (nv - 1, nt - 1), (0, 0)):
        a = dr.valid()
        a.update(vcap=vcap, tcap=tcap)
        rc, _ = dr.invoke(capi.lib(), a)
        assert rc == SFMBA_ERR_CAPACITY and (int(a["n_vertices_out"][0]), int(a["n_triangles_out"][0])) == (nv, nt), (vcap, tcap)
        for f in dr.ARRAYS_OUT:
            assert (a[f].view(np.uint8) == dr.FILL).all(), (vcap, tcap, f)                  # the fill bytes are untouched
    a = dr.valid()
    a.update(vcap=nv, tcap=nt)
    rc, _ = dr.invoke(capi.lib(), a)
    assert rc == SFMBA_OK and same_bits(a["tri_out"][:nt], want["tri"]) and (a["tri_out"][nt:].view(np.uint8) == dr.FILL).all()
    assert same_bits(a["xyz_out"][:nv], want["xyz"]) and (a["xyz_out"][nv:].view(np.uint8) == dr.FILL).all()
    assert [int(v) for v in a["stats"]] == want["stats"]
    # a capacity given through the binding is retried once with the reported sizes
    assert_fields(decimated(capi, dc.case("small_cube"), vcap=nv - 1, tcap=3), want)
    assert_fields(decimated(capi, dc.case("small_cube"), vcap=nv, tcap=nt), want)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing(capi):
    calls = dr.refusal_calls(capi, device_cases=True)
    assert len(calls) > 35
    for name, call in calls:
        rc, untouched = call()
        assert rc == SFMBA_ERR_INVALID_ARG and untouched, name


def test_the_valid_call_of_the_refusal_table_succeeds(capi):
    rc, untouched = dr.valid_call(capi)
    assert rc == SFMBA_OK and not untouched
    for what, spoil in dr.REG_IGNORED:                                                      # reg is read only with placement 1
        rc, untouched = dr.valid_call(capi, spoil)
        assert rc == SFMBA_OK and not untouched, what


# ---- a batch ----------------------------------------------------------------------------------------------------------------------
def test_two_calls_on_one_process_give_the_bits_of_each_alone(capi):
    """The arena hands a call the chunks of the call before it: nothing of one mesh may leak into the next."""
    for first, second in (("sphere_14", "member_runs"), ("member_runs", "sphere_14"), ("small_cube", "small_cube"), ("fan_65536", "clamps")):
        decimated(capi, dc.case(first))
        assert_fields(decimated(capi, dc.case(second)), dc.want(second), what=(first, second))
