"""Smoothing the view labels on the MI355X (-m gpu) against the CPU restatement of its contract (tests/label_oracle.py; include/sfmba.h,
"smoothing the view labels").  Every comparison is EXACT: the lists, the adjacency and its counts, the labels, the eight statistics, the
bytes of the atlas.  The shapes are those of tests/label_cases.py -- the smallest at which the kernels can still go wrong -- and the
restatement's answer for each is computed once and shared."""
import numpy as np
import pytest

import label_cases as lc
import label_oracle as lo
import label_refusals as lr
import texture_oracle as to

pytestmark = pytest.mark.gpu
SFMBA_OK, SFMBA_ERR_INVALID_ARG = 0, 1
# as tests/test_label_oracle_cpu.py measured them on the restatement; the gates are twice these
WALL_DIFF_END_MEASURED = 2501
WALL_AREA_GIVEN_UP_MEASURED = 0.064349
ALL = list(lc.CASES)
SCENES = list(lc.SCENES) + ["six_view_sphere"]


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_texture(got, want, what):
    for f in ("atlas", "uv", "view", "score"):
        assert same_bits(got[f], want[f]), (what, f)
    assert got["n_textured"] == want["n_textured"], what


@pytest.mark.parametrize("name", SCENES)
def test_candidates_exact(capi, name):
    c, w = lc.case(name), lc.want(name)
    cv, cs = capi.mesh_view_candidates(*lc.candidate_args(c))
    assert same_bits(cv, w["cand_view"]) and same_bits(cs, w["cand_score"])


@pytest.mark.parametrize("name", ALL)
def test_adjacency_exact(capi, name):
    c, w = lc.case(name), lc.want(name)
    got = capi.mesh_adjacency(c["tri"])
    assert same_bits(got["adj"], w["adj"])
    assert (got["n_pairs"], got["n_open_edges"], got["n_nonmanifold_edges"]) == (w["n_pairs"], w["n_open_edges"], w["n_nonmanifold_edges"])


@pytest.mark.parametrize("name", ALL)
def test_view_smooth_exact(capi, name):
    c, w = lc.case(name), lc.want(name)
    view, stats = capi.mesh_view_smooth(w["cand_view"], w["cand_score"], w["adj"], c["n_images"], c["rings"], c["penalty"], c["max_passes"])
    print("%s: %s" % (name, dict(zip(lo.STATS, stats.tolist()))))
    assert same_bits(stats, w["smooth"]["stats"]) and same_bits(view, w["smooth"]["view"])


@pytest.mark.parametrize("name", SCENES)
def test_the_combined_call_equals_the_restatement_and_the_composition(capi, name):
    c, want = lc.case(name), lc.want_texture(name)
    p = (c["k"], c["rings"], c["penalty"], c["max_passes"])
    got = capi.mesh_texture_smooth(*lc.texture_args(c), *p)
    assert_texture(got, want, name)
    assert same_bits(got["stats"], want["stats"])
    s = c["scene"]
    cv, cs = capi.mesh_view_candidates(*lc.candidate_args(c))
    adj = capi.mesh_adjacency(c["tri"])["adj"]
    view, stats = capi.mesh_view_smooth(cv, cs, adj, c["n_images"], *p[1:])
    tex = capi.mesh_texture_from_views(s["xyz"], s["bgr"], s["tri"], s["images"], s["K"], s["P"], view, s["patch"], s["blocks_per_row"])
    assert same_bits(view, got["view"]) and same_bits(stats, got["stats"])
    assert same_bits(tex["atlas"], got["atlas"]) and same_bits(tex["uv"], got["uv"]) and tex["n_textured"] == got["n_textured"]


@pytest.mark.parametrize("name", SCENES)
def test_without_rings_and_passes_the_combined_call_is_the_plain_call(capi, name):
    c = lc.case(name)
    plain = capi.mesh_texture(*lc.texture_args(c))
    got = capi.mesh_texture_smooth(*lc.texture_args(c), c["k"], 0, c["penalty"], 0)
    assert_texture(got, plain, name)
    assert got["stats"][0] == got["stats"][1] and got["stats"][2] == got["stats"][3] == got["stats"][4] and got["stats"][6] == got["stats"][7] == 0
    s = c["scene"]
    tex = capi.mesh_texture_from_views(s["xyz"], s["bgr"], s["tri"], s["images"], s["K"], s["P"], plain["view"], s["patch"], s["blocks_per_row"])
    assert same_bits(tex["atlas"], plain["atlas"]) and same_bits(tex["uv"], plain["uv"]) and tex["n_textured"] == plain["n_textured"]


def test_given_labels_of_another_choice_raster_as_the_restatement_says(capi):
    """labels that no rule would choose: the last candidate, and -1 for every third triangle"""
    c, w = lc.case("sheet_65"), lc.want("sheet_65")
    s = c["scene"]
    view = np.where(np.arange(len(c["tri"])) % 3 == 0, -1, w["cand_view"].max(axis=1)).astype(np.int32)
    got = capi.mesh_texture_from_views(s["xyz"], s["bgr"], s["tri"], s["images"], s["K"], s["P"], view, s["patch"], s["blocks_per_row"])
    B = to.default_blocks_per_row(len(c["tri"]))
    assert same_bits(got["atlas"], to.raster_np(s["xyz"], s["bgr"], s["tri"], s["images"], s["K"], s["P"], view, s["patch"], B))
    assert got["n_textured"] == int((view >= 0).sum())


def test_quality_on_the_wall(capi):
    """The noisy wall under five similar views (tests/label_cases.py), through the combined call.  CONDITION: the final count of pairs
    with different views is at most half the count under rank 0.  GATE: twice what the restatement measured (2501 pairs, 0.064349 of the
    area given up).  The statistics equal the restatement's exactly."""
    c, w = lc.wall(), lc.wall_want()
    p = lc.WALL_PARAMS
    got = capi.mesh_texture_smooth(c["xyz"], c["bgr"], c["tri"], c["images"], c["K"], c["P"], c["depth_maps"], c["occl_tol"], c["min_area"], c["patch"], None,
                                   p["k"], p["rings"], p["penalty"], p["max_passes"])
    st = got["stats"]
    given_up = lc.mean_area_given_up(w["cand_score"], w["cand_view"], got["view"])
    print("wall on the device: %s; mean area given up %.6f" % (dict(zip(lo.STATS, st.tolist())), given_up))
    assert 2 * st[4] <= st[2]
    assert st[4] <= 2 * WALL_DIFF_END_MEASURED and given_up <= 2.0 * WALL_AREA_GIVEN_UP_MEASURED
    assert same_bits(st, w["smooth"]["stats"]) and same_bits(got["view"], w["smooth"]["view"])


def test_every_refusal_writes_nothing(capi):
    calls = lr.refusal_calls(capi, device_cases=True)
    assert len(calls) > 160
    for name, call in calls:
        rc, untouched = call()
        assert rc == SFMBA_ERR_INVALID_ARG and untouched, name
    assert "index" in capi.lib().sfmba_last_error().decode()


@pytest.mark.parametrize("entry", list(lr.NAMES))
def test_the_valid_call_of_the_refusal_table_succeeds(capi, entry):
    rc, untouched = lr.valid_call(capi, entry)
    assert rc == SFMBA_OK and not untouched


def test_two_calls_on_one_process_give_the_bits_of_each_alone(capi):
    """The arena hands a call the chunks of the call before it: nothing of one call may leak into the next."""
    for first, second in (("sheet_257", "nt_1"), ("six_view_sphere", "sheet_63"), ("three_views_k8", "no_images")):
        a, b = lc.case(first), lc.case(second)
        capi.mesh_texture_smooth(*lc.texture_args(a), a["k"], a["rings"], a["penalty"], a["max_passes"])
        got = capi.mesh_texture_smooth(*lc.texture_args(b), b["k"], b["rings"], b["penalty"], b["max_passes"])
        assert_texture(got, lc.want_texture(second), (first, second))
        assert same_bits(got["stats"], lc.want_texture(second)["stats"])
