"""Mesh cleaning on the MI355X (-m gpu) against the CPU restatement of its contract (tests/mesh_clean_oracle.py; include/sfmba.h,
sfmba_mesh_components / sfmba_mesh_filter / sfmba_mesh_smooth / sfmba_mesh_clean).  Every comparison is EXACT: labels, counts, totals,
the bit patterns of xyz and of the normals, the bytes of the colours, triangles and vertex_of.  The shapes are those of
tests/mesh_clean_cases.py -- the smallest at which the kernels can still go wrong -- and the restatement's answer for each is computed
once and shared."""
import numpy as np
import pytest

import mesh_cases as mc
import mesh_clean_cases as cc
import mesh_clean_oracle as co
import mesh_clean_refusals as mr

pytestmark = pytest.mark.gpu
SFMBA_OK, SFMBA_ERR_INVALID_ARG, SFMBA_ERR_CAPACITY = 0, 1, 5
CLEAN_FIELDS = ("xyz", "bgr", "normal", "tri", "vertex_of")


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


def assert_fields(got, want, fields, what=""):
    for f in fields:
        assert same_bits(got[f], want[f]), (what, f)


def components(capi, c, **kw):
    return capi.mesh_components(len(c["xyz"]), c["tri"], **kw)


def filtered(capi, c, **kw):
    return capi.mesh_filter(c["xyz"], c["bgr"], c["tri"], c["min_triangles"], c["keep_largest"], **kw)


def smoothed(capi, c, **kw):
    return capi.mesh_smooth(c["xyz"], c["tri"], c["origin"], float(c["quantum"]), c["iterations"], c["lam"], c["mu"], **kw)


def cleaned(capi, c, **kw):
    return capi.mesh_clean(c["xyz"], c["bgr"], c["tri"], c["origin"], float(c["quantum"]), c["min_triangles"], c["keep_largest"], c["iterations"],
                           c["lam"], c["mu"], **kw)


# ---- every case, every call -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.CASES))
def test_cases_exact(capi, name):
    c, want = cc.case(name), cc.want(name)
    got = components(capi, c)
    assert_fields(got, want["components"], ("label", "comp_triangles"), name)
    assert (got["n_components"], got["largest"]) == (want["components"]["n_components"], want["components"]["largest"]), name
    assert_fields(filtered(capi, c), want["filter"], ("xyz", "bgr", "tri", "vertex_of"), name)
    assert_fields(smoothed(capi, c), want["smooth"], ("xyz", "normal"), name)
    one = cleaned(capi, c)
    assert_fields(one, want["clean"], CLEAN_FIELDS, name)
    # the one call equals the two, byte for byte
    f = filtered(capi, c)
    s = capi.mesh_smooth(f["xyz"], f["tri"], c["origin"], float(c["quantum"]), c["iterations"], c["lam"], c["mu"])
    assert_fields(one, dict(xyz=s["xyz"], bgr=f["bgr"], normal=s["normal"], tri=f["tri"], vertex_of=f["vertex_of"]), CLEAN_FIELDS, name)


@pytest.mark.parametrize("name", list(cc.REFUSED))
def test_a_coordinate_out_of_range_refuses_on_the_device(capi, name):
    c = cc.case(name)
    assert cc.want(name)["smooth"] is None
    for entry in ("sfmba_mesh_smooth", "sfmba_mesh_clean"):
        a = mr.valid(entry, name)
        a.update(iterations=c["iterations"], min_triangles=1)
        rc, untouched = mr.invoke(capi.lib(), entry, a)
        assert rc == SFMBA_ERR_INVALID_ARG and untouched, (name, entry)
        assert "coordinate" in capi.lib().sfmba_last_error().decode()
    # the components and the filter do not look at coordinates
    assert_fields(filtered(capi, c), cc.want(name)["filter"], ("xyz", "bgr", "tri", "vertex_of"), name)
    # a bad coordinate on a vertex that the filter drops does not stop the one call
    if name == "nan_coordinate":
        d = dict(c)
        d["tri"] = c["tri"][~(c["tri"] == 40).any(axis=1)]                                  # vertex 40 holds the NaN
        want = co.clean(*cc.clean_args(d))
        assert want is not None and want["vertex_of"][40] == -1
        assert_fields(cleaned(capi, d), want, CLEAN_FIELDS, name)


def test_planted_solids_keep_their_topology_on_the_device(capi):
    import mesh_oracle as mo
    for name, euler in mc.CLOSED.items():
        got = cleaned(capi, cc.case(name))
        closed, e, boundary, _ = mo.topology(got["tri"])
        assert closed and e == euler and boundary == 0 and mo.signed_volume(got["xyz"], got["tri"]) > 0, name


def test_outputs_may_be_null(capi):
    for name in ("islands", "no_colour", "all_256"):
        c, want = cc.case(name), cc.want(name)
        got = components(capi, c, want_comp_triangles=False)
        assert got["comp_triangles"] is None and same_bits(got["label"], want["components"]["label"])
        got = filtered(capi, c, want_vertex_of=False)
        assert got["vertex_of"] is None
        assert_fields(got, want["filter"], ("xyz", "bgr", "tri"), name)
        got = smoothed(capi, c, want_normal=False)
        assert got["normal"] is None and same_bits(got["xyz"], want["smooth"]["xyz"])
        got = cleaned(capi, c, want_normal=False, want_vertex_of=False)
        assert got["normal"] is None and got["vertex_of"] is None
        assert_fields(got, want["clean"], ("xyz", "bgr", "tri"), name)
        assert (got["bgr"] is None) == (c["bgr"] is None)
    # bgr NULL: bgr_out stays untouched
    a = mr.valid("sfmba_mesh_clean")
    a.update(bgr=None)
    rc, _ = mr.invoke(capi.lib(), "sfmba_mesh_clean", a)
    assert rc == SFMBA_OK and (a["bgr_out"].view(np.uint8) == mr.FILL).all() and not (a["xyz_out"].view(np.uint8) == mr.FILL).all()


def test_the_device_mesh_of_the_six_view_sphere_cleans_as_the_restatement_says(capi):
    c = mc.integration_case("six_view_sphere")
    m = capi.tsdf_mesh(c["images"], c["K"], c["P"], c["depth_maps"], c["origin"], c["voxel"], c["dims"], c["trunc"])
    assert len(m["tri"]) > 10000
    quantum = float(np.float32(c["voxel"]) / np.float32(1024.0))
    min_triangles = max(1, len(m["tri"]) // 1000)
    args = (m["xyz"], m["bgr"], m["tri"], c["origin"], quantum, min_triangles, 0, 10, cc.LAM, cc.MU)
    want = co.clean(*args)
    assert_fields(capi.mesh_clean(*args), want, CLEAN_FIELDS)
    comp = co.components_np(len(m["xyz"]), m["tri"])
    got = capi.mesh_components(len(m["xyz"]), m["tri"])
    assert_fields(got, comp, ("label", "comp_triangles"))
    print("six-view sphere: %d components, %d of %d triangles kept at min_triangles %d" % (comp["n_components"], len(want["tri"]), len(m["tri"]), min_triangles))


# ---- the capacity protocol --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["sfmba_mesh_filter", "sfmba_mesh_clean"])
def test_capacity_protocol(capi, entry):
    want = cc.want("min_on_count")["clean"]
    nv, nt = len(want["xyz"]), len(want["tri"])
    for vcap, tcap in ((nv - 1, nt), (nv, nt - 1), (nv - 1, nt - 1), (0, 0)):
        a = mr.valid(entry)
        a.update(min_triangles=24, vcap=vcap, tcap=tcap)
        rc, _ = mr.invoke(capi.lib(), entry, a)
        assert rc == SFMBA_ERR_CAPACITY and (int(a["n_vertices_out"][0]), int(a["n_triangles_out"][0])) == (nv, nt), (vcap, tcap)
        for f in ("xyz_out", "bgr_out", "normal", "tri_out", "vertex_of"):
            assert (a[f].view(np.uint8) == mr.FILL).all(), (vcap, tcap, f)                  # the fill bytes are untouched
    a = mr.valid(entry)
    a.update(min_triangles=24, vcap=nv, tcap=nt)
    rc, _ = mr.invoke(capi.lib(), entry, a)
    assert rc == SFMBA_OK and same_bits(a["tri_out"][:nt], want["tri"]) and (a["tri_out"][nt:].view(np.uint8) == mr.FILL).all()
    # a capacity given through the binding is retried once with the reported sizes
    c = cc.case("min_on_count")
    assert_fields(cleaned(capi, c, vcap=nv - 1, tcap=3), want, CLEAN_FIELDS)
    assert_fields(filtered(capi, c, vcap=nv, tcap=nt), cc.want("min_on_count")["filter"], ("xyz", "bgr", "tri", "vertex_of"))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing(capi):
    calls = mr.refusal_calls(capi, device_cases=True)
    assert len(calls) > 110
    for name, call in calls:
        rc, untouched = call()
        assert rc == SFMBA_ERR_INVALID_ARG and untouched, name


@pytest.mark.parametrize("entry", list(mr.NAMES))
def test_the_valid_call_of_the_refusal_table_succeeds(capi, entry):
    rc, untouched = mr.valid_call(capi, entry)
    assert rc == SFMBA_OK and not untouched


# ---- a batch ----------------------------------------------------------------------------------------------------------------------
def test_two_calls_on_one_process_give_the_bits_of_each_alone(capi):
    """The arena hands a call the chunks of the call before it: nothing of one mesh may leak into the next."""
    for first, second in (("sphere_14", "islands"), ("islands", "sphere_14"), ("all_256", "all_256")):
        cleaned(capi, cc.case(first))
        assert_fields(cleaned(capi, cc.case(second)), cc.want(second)["clean"], CLEAN_FIELDS, (first, second))
        got = components(capi, cc.case(second))
        assert_fields(got, cc.want(second)["components"], ("label", "comp_triangles"), (first, second))
