"""Levelling the colours across seams on the MI355X (-m gpu) against the CPU restatement of its contract (tests/colour_oracle.py;
include/sfmba.h, "levelling the colours across seams").  Every comparison is EXACT: the nodes, their colours, the offsets, the eight
statistics, the bytes of the atlas, the count of clamped texels.  The shapes are those of tests/colour_cases.py -- the smallest at which
the kernels can still go wrong -- and the restatement's answer for each is computed once and shared."""
import numpy as np
import pytest

import colour_cases as cc
import colour_oracle as co
import colour_refusals as cr
import label_cases as lc
import mesh_cases as mc
import texture_oracle as to

pytestmark = pytest.mark.gpu
SFMBA_OK, SFMBA_ERR_INVALID_ARG = 0, 1
ALL, PLANTED = list(cc.CASES), list(cc.PLANTED)
COMBINED = ("sheet_65", "three_views_k8", "sheet_257")                     # scenes of tests/label_cases.py


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_nodes(got, want, what):
    assert got["n_nodes"] == want["n_nodes"], what
    for f in ("node_vertex", "node_view", "node_of", "seen", "F"):
        assert same_bits(got[f], want[f]), (what, f)


def mesh_args(c):
    return (c["xyz"], c["bgr"], c["tri"], c["images"], c["K"], c["P"])


@pytest.mark.parametrize("name", ALL)
def test_nodes_exact(capi, name):
    c, w = cc.case(name), cc.want(name)
    assert_nodes(capi.mesh_colour_nodes(*cc.node_args(c)), w["nodes"], name)


@pytest.mark.parametrize("name", ALL)
def test_level_exact_on_the_scenes(capi, name):
    c, w = cc.case(name), cc.want(name)
    nd = w["nodes"]
    g, stats = capi.mesh_colour_level(nd["node_vertex"], nd["seen"], nd["F"], nd["node_of"], c["weight"], c["passes"])
    print("%s: %s" % (name, dict(zip(co.STATS, stats.tolist()))))
    assert same_bits(stats, w["stats"]) and same_bits(g, w["g"])


@pytest.mark.parametrize("name", PLANTED)
def test_level_exact_on_planted_nodes(capi, name):
    c, w = cc.planted_case(name), cc.want_planted(name)
    g, stats = capi.mesh_colour_level(*cc.level_args(c))
    print("%s: %s" % (name, dict(zip(co.STATS, stats.tolist()))))
    assert same_bits(stats, w["stats"]) and same_bits(g, w["g"])


@pytest.mark.parametrize("name", ALL)
def test_levelled_raster_exact(capi, name):
    c, w = cc.case(name), cc.want(name)
    got = capi.mesh_texture_levelled(*mesh_args(c), c["view"], w["nodes"]["node_of"], w["g"], c["patch"], c["blocks_per_row"])
    assert same_bits(got["atlas"], w["tex"]["atlas"]) and same_bits(got["uv"], w["tex"]["uv"]), name
    assert (got["n_textured"], got["n_clamped"]) == (w["tex"]["n_textured"], w["tex"]["n_clamped"]), name


@pytest.mark.parametrize("name", ALL)
def test_with_offsets_of_zero_the_levelled_call_is_from_views(capi, name):
    c, w = cc.case(name), cc.want(name)
    plain = capi.mesh_texture_from_views(*mesh_args(c), c["view"], c["patch"], c["blocks_per_row"])
    got = capi.mesh_texture_levelled(*mesh_args(c), c["view"], w["nodes"]["node_of"], np.zeros_like(w["g"]), c["patch"], c["blocks_per_row"])
    assert same_bits(got["atlas"], plain["atlas"]) and same_bits(got["uv"], plain["uv"]) and got["n_textured"] == plain["n_textured"]
    assert got["n_clamped"] == 0


@pytest.mark.parametrize("name", ["grid_2_views", "gray", "patch_3", "patch_64", "fan_nine_views"])
@pytest.mark.parametrize("offset", [65280, -65280, 40000, -40000])
def test_planted_offsets_clamp_texels_and_the_count_is_the_recount(capi, name, offset):
    c, w = cc.case(name), cc.want(name)
    g = np.full_like(w["g"], offset)
    g[::3] //= 2                                                                         # not the same at every corner
    want = co.texture_levelled(*mesh_args(c), c["view"], w["nodes"]["node_of"], g, c["patch"], c["blocks_per_row"])
    got = capi.mesh_texture_levelled(*mesh_args(c), c["view"], w["nodes"]["node_of"], g, c["patch"], c["blocks_per_row"])
    assert want["n_clamped"] > 0 and got["n_clamped"] == want["n_clamped"]
    assert same_bits(got["atlas"], want["atlas"])
    assert (got["atlas"] == (255 if offset > 0 else 0)).any()


def _combined(c, p, level):
    return lc.texture_args(c) + tuple(p) + tuple(level)


@pytest.mark.parametrize("smoothing", [True, False])
@pytest.mark.parametrize("name", COMBINED)
def test_the_combined_call_equals_the_restatement_and_the_composition(capi, name, smoothing):
    c = lc.case(name)
    s = c["scene"]
    p = (c["k"], c["rings"], c["penalty"], c["max_passes"]) if smoothing else (c["k"], 0, c["penalty"], 0)
    level = (1, 16, 6)
    got = capi.mesh_texture_adjust(*_combined(c, p, level))
    want = co.texture_adjust(*_combined(c, p, level))
    for f in ("atlas", "uv", "view", "score", "stats", "level_stats"):
        assert same_bits(got[f], want[f]), (name, f)
    assert got["n_textured"] == want["n_textured"] and got["level_stats"][2] > 0
    # the composition of the separate calls
    tex = capi.mesh_texture_smooth(*lc.texture_args(c), *p)
    nd = capi.mesh_colour_nodes(s["xyz"], s["tri"], s["images"], s["K"], s["P"], tex["view"], level[0])
    g, stats = capi.mesh_colour_level(nd["node_vertex"], nd["seen"], nd["F"], nd["node_of"], level[1], level[2])
    lev = capi.mesh_texture_levelled(s["xyz"], s["bgr"], s["tri"], s["images"], s["K"], s["P"], tex["view"], nd["node_of"], g, s["patch"], s["blocks_per_row"])
    stats[6] = lev["n_clamped"]
    assert same_bits(tex["view"], got["view"]) and same_bits(tex["score"], got["score"]) and same_bits(tex["stats"], got["stats"])
    assert same_bits(lev["atlas"], got["atlas"]) and same_bits(lev["uv"], got["uv"]) and lev["n_textured"] == got["n_textured"]
    assert same_bits(stats, got["level_stats"])
    if not smoothing:
        plain = capi.mesh_texture(*lc.texture_args(c))
        assert same_bits(plain["view"], got["view"]) and same_bits(plain["score"], got["score"])


@pytest.mark.parametrize("name", COMBINED + ("nt_0", "nt_1", "no_images"))
def test_without_level_passes_the_combined_call_is_the_smooth_call(capi, name):
    c = lc.case(name)
    p = (c["k"], c["rings"], c["penalty"], c["max_passes"])
    smooth = capi.mesh_texture_smooth(*lc.texture_args(c), *p)
    got = capi.mesh_texture_adjust(*_combined(c, p, (1, 16, 0)))
    for f in ("atlas", "uv", "view", "score", "stats"):
        assert same_bits(got[f], smooth[f]), (name, f)
    assert got["n_textured"] == smooth["n_textured"]
    st = got["level_stats"]
    assert st[3] == st[4] and st[5] == st[6] == st[7] == 0


def test_a_permutation_of_the_triangles_gives_the_same_offsets(capi):
    a, b = cc.case("grid_4_views"), cc.case("grid_permuted")
    na, nb = capi.mesh_colour_nodes(*cc.node_args(a)), capi.mesh_colour_nodes(*cc.node_args(b))
    ga, _ = capi.mesh_colour_level(na["node_vertex"], na["seen"], na["F"], na["node_of"], a["weight"], a["passes"])
    gb, _ = capi.mesh_colour_level(nb["node_vertex"], nb["seen"], nb["F"], nb["node_of"], b["weight"], b["passes"])
    assert same_bits(na["node_vertex"], nb["node_vertex"]) and same_bits(na["node_view"], nb["node_view"]) and same_bits(na["F"], nb["F"])
    assert same_bits(ga, gb) and not same_bits(na["node_of"], nb["node_of"])


def test_the_device_mesh_of_the_six_view_sphere_levels_as_the_restatement_says(capi):
    c = mc.integration_case("six_view_sphere")
    m = capi.tsdf_mesh(c["images"], c["K"], c["P"], c["depth_maps"], c["origin"], c["voxel"], c["dims"], c["trunc"])
    assert len(m["tri"]) > 10000
    args = (m["xyz"], m["bgr"], m["tri"], c["images"], c["K"], c["P"], c["depth_maps"], 2.0 * float(c["voxel"]), 256, 3, None, 4, 4, 256, 100, 1, 16, 16)
    got, want = capi.mesh_texture_adjust(*args), co.texture_adjust(*args)
    print("six-view sphere: %s" % dict(zip(co.STATS, got["level_stats"].tolist())))
    for f in ("atlas", "uv", "view", "score", "stats", "level_stats"):
        assert same_bits(got[f], want[f]), f
    assert got["level_stats"][4] < got["level_stats"][3]


def test_every_refusal_writes_nothing(capi):
    calls = cr.refusal_calls(capi, device_cases=True)
    assert len(calls) > 160
    for name, call in calls:
        rc, untouched = call()
        assert rc == SFMBA_ERR_INVALID_ARG and untouched, name


@pytest.mark.parametrize("entry", list(cr.NAMES))
def test_the_valid_call_of_the_refusal_table_succeeds(capi, entry):
    rc, untouched = cr.valid_call(capi, entry)
    assert rc == SFMBA_OK and not untouched


def test_two_calls_on_one_process_give_the_bits_of_each_alone(capi):
    """The arena hands a call the chunks of the call before it, and the levelling's arrays are not zeroed: nothing of one call may leak
    into the next."""
    for first, second in (("six_view_sphere", "strip_21"), ("strip_10923", "blind_node"), ("fan_nine_views", "all_unlabelled")):
        a, b = cc.case(first), cc.case(second)
        capi.mesh_colour_nodes(*cc.node_args(a))
        assert_nodes(capi.mesh_colour_nodes(*cc.node_args(b)), cc.want(second)["nodes"], (first, second))
        nd = cc.want(second)["nodes"]
        g, stats = capi.mesh_colour_level(nd["node_vertex"], nd["seen"], nd["F"], nd["node_of"], b["weight"], b["passes"])
        assert same_bits(g, cc.want(second)["g"]) and same_bits(stats, cc.want(second)["stats"])
